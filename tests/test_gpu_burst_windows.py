"""GPU tests (-m gpu) of the burst TX side: the TX split at the coded bytes (ria_gpu_encode_frames_batch,
ria_gpu_tx_coded_batch) and the device-side burst window builder of ria_amd.acquire, against the oracle's TX pieces (the
recipe of oracle/gen_golden.burst_buffer) and, through ria_gpu_rx_burst_batch, against the restatement."""
import numpy as np
import pytest

import burst_restatement as br
import pyoracle as po
from test_gpu_parity import bits, dev, engine
from test_gpu_rx_burst import assert_equal_to_restatement

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mod,rate", [("QAM16", "R1_2"), ("DQPSK", "R1_2"), ("QAM64", "R3_4")])
def test_tx_split_at_the_coded_bytes(oracle, mod, rate):
    """encode_frames is encodeFixedFrame (channel interleaved, MSB first), and tx_coded of it is tx bit for bit, with and
    without the peak scaling; tx_coded of burst-interleaved bytes is the oracle's modulator on them."""
    from ria_amd import capi
    e = engine(mod, rate)
    n = 5
    info = e.make_frames(99, 40, n)
    coded = e.encode_frames(info)
    h = info.cpu().numpy()
    want = np.stack([oracle.encode_fixed_frame(h[f], capi.RATE[rate], True, e.geo.bits_per_symbol) for f in range(n)])
    assert np.array_equal(coded.cpu().numpy(), want)
    for peak in (0.8, 0.0):
        assert np.array_equal(bits(e.tx_coded(coded, peak).cpu().numpy()), bits(e.tx(info, peak).cpu().numpy())), peak
    phys = e.burst_interleave(coded[:4].contiguous(), 4)
    assert np.array_equal(phys.cpu().numpy(), oracle.burst_interleave(want[:4]))
    x = e.tx_coded(phys, 0.0).cpu().numpy()
    for f in range(4):
        assert np.array_equal(bits(x[f]), bits(oracle.modulate(capi.MOD[mod], capi.RATE[rate], phys[f].cpu().numpy()))), f


def _cpu_window(O, infos, off, wl, seed, kind, snr, interleaved, marker, peak=0.5):
    """the builder's recipe from the oracle's pieces, for one window"""
    g = O.geom(po.QAM16, po.R1_2)
    coded = np.stack([O.encode_fixed_frame(i, po.R1_2, True, g.bits_per_symbol) for i in infos])
    phys = O.burst_interleave(coded) if interleaved else coded
    s = np.concatenate([O.modulate(po.QAM16, po.R1_2, p) for p in phys])
    if marker:
        s[:1152] = -s[:1152]
    s = s * (np.float32(peak) / np.abs(s).max())
    assert s.dtype == np.float32
    x = np.zeros(wl, np.float32)
    x[off:off + len(s)] = s
    return O.channel(kind, snr, int(seed), x)


@pytest.mark.parametrize("n_frames,interleaved", [(4, True), (3, False)])
def test_burst_window_builder_and_counters(oracle, n_frames, interleaved):
    """make_burst_windows on the device equals the recipe built from the oracle's pieces sample for sample (offsets and
    channel seeds from window_recipe, frame sequence numbers trial * n_frames + f), does not depend on the chunk, and
    rx_burst on its windows equals the restatement on every field; burst_tally counts exactly what those results hold."""
    from ria_amd.acquire import BURST_COUNTERS, BURST_STOPS, DETECT_THRESHOLD, SEARCH_LEN, burst_tally, make_burst_windows, window_recipe
    from ria_amd.sweep import SweepPoint
    e = engine("QAM16", "R1_2")
    pt, seed, start, n = SweepPoint(0, 22.0), 20261018, 7, 3
    win, sent, offs = make_burst_windows(e, seed, pt, 2, start, n, n_frames, interleaved=interleaved)
    fs = e.geo.frame_samples
    assert win.shape == (n, SEARCH_LEN + (n_frames + 1) * fs) and sent.shape == (n, n_frames, e.geo.info_bytes_per_frame)
    offs_r, seeds = window_recipe(seed, 2, np.arange(start, start + n))
    assert np.array_equal(offs, offs_r)
    assert np.array_equal(sent.cpu().numpy().reshape(n * n_frames, -1), e.make_frames(seed, start * n_frames, n * n_frames).cpu().numpy())
    X = win.cpu().numpy()
    H = sent.cpu().numpy()
    for k in range(n):
        want = _cpu_window(oracle, H[k], int(offs[k]), X.shape[1], seeds[k], 0, 22.0, interleaved, interleaved)
        assert np.array_equal(bits(X[k]), bits(want)), (k, float(np.abs(X[k] - want).max()))
    one, _, _ = make_burst_windows(e, seed, pt, 2, start + 1, 1, n_frames, interleaved=interleaved)
    assert np.array_equal(bits(one.cpu().numpy()[0]), bits(X[1]))
    out = e.rx_burst(win, SEARCH_LEN, group_size=max(2, n_frames), detect_threshold=DETECT_THRESHOLD, interleave=interleaved)
    rs = [br.burst_window(oracle, po.QAM16, po.R1_2, X[k], SEARCH_LEN, max(2, n_frames), interleave=interleaved) for k in range(n)]
    for k in range(n):
        assert_equal_to_restatement(f"window {k}", out, k, rs[k])
    row = dict(zip(BURST_COUNTERS, burst_tally(out, sent)))
    assert row["windows"] == n and row["accepted"] == sum(r["accepted"] for r in rs)
    for m in (1, 2):
        for s, name in enumerate(BURST_STOPS):
            assert row[f"mode{m}_{name}"] == sum(r["mode"] == m and r["stop"] == s for r in rs), (m, name)
    assert row["frames"] == sum(r["frames"] for r in rs) and row["frames_decoded"] == sum(r["frames_decoded"] for r in rs)
    ok = sum(bool(r["cw_ok"][f].all() and r["frame_valid"][f] and np.array_equal(r["info"][f], H[k][f]))
             for k, r in enumerate(rs) for f in range(min(n_frames, r["frames_decoded"])))
    assert row["frames_ok"] == ok
    assert row["mode2_none" if interleaved else "mode1_energy"] >= 1, row    # the workload does what it is built for
