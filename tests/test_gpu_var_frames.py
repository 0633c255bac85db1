"""GPU tests (-m gpu) of frames of any length: ria_gpu_tx_coded_var_batch against the oracle's modulator and
ria_gpu_demod_var_batch against the oracle's process() on spans shorter than a frame, bit for bit (snr_db, a display value, to
the tolerance of test_gpu_parity.py); the full-length cases against the fixed-frame calls bit for bit; argument checks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pyoracle as po
import control_restatement as R
from ria_amd.capi import RiaError
from test_gpu_parity import bits, dev, engine

pytestmark = pytest.mark.gpu

TX_HANDLES = {"dqpsk_r14": ("DQPSK", "R1_4"), "qam16_r12": ("QAM16", "R1_2"), "d8psk_r12": ("D8PSK", "R1_2"), "qam32_r34": ("QAM32", "R3_4")}
DEMOD_HANDLES = dict(TX_HANDLES, dbpsk_r12=("DBPSK", "R1_2"))
CODED_BYTES = (1, 80, 81, 82, 162, 323, 324)
SPANS = (3 * 1152, 9 * 1152 - 1, 9 * 1152, 9 * 1152 + 700, 15 * 1152, None)       # None: frame_samples
STATUS_BITS = ("cfo_hz", "fading_index", "noise_variance", "lts_phase_slope", "snr_linear", "corr_phase")


def ids(name):
    m, r = DEMOD_HANDLES[name]
    return getattr(po, m), getattr(po, r)


def coded_rows(nb, n=5):
    """n frames of nb distinct bytes each (a function of nb and the frame number)"""
    return ((np.arange(n)[:, None] * 101 + np.arange(nb)[None, :] * 37 + 13 * nb) % 256).astype(np.uint8)


@pytest.mark.parametrize("name", list(TX_HANDLES))
def test_tx_coded_var_equals_the_oracle_modulator(oracle, name):
    e = engine(*TX_HANDLES[name])
    mod, rate = ids(name)
    for nb in CODED_BYTES:
        coded = coded_rows(nb)
        n_out = e.var_frame_samples(nb)
        assert n_out == R.var_frame_samples(mod, rate, nb)
        ref = np.stack([oracle.modulate(mod, rate, c) for c in coded])
        assert ref.shape == (5, n_out)
        for peak in (0.0, 0.8):
            got = e.tx_coded_var(dev(coded), peak=peak).cpu().numpy()
            want = ref if peak == 0.0 else np.stack([(r * (np.float32(peak) / np.abs(r).max())).astype(np.float32) for r in ref])
            assert np.array_equal(bits(got), bits(want)), (nb, peak)
        # a row stride wider than the frame: the frame is the same, the floats between two frames are not written
        wide = e.tx_coded_var(dev(coded), peak=0.8, out_stride=n_out + 100).cpu().numpy()
        assert np.array_equal(bits(wide[:, :n_out]), bits(want)) and not wide[:, n_out:].any()
    full = coded_rows(324)
    assert np.array_equal(bits(e.tx_coded_var(dev(full), peak=0.8).cpu().numpy()), bits(e.tx_coded(dev(full), peak=0.8).cpu().numpy()))
    assert np.array_equal(bits(e.tx_coded_var(dev(full), peak=0.0).cpu().numpy()), bits(e.tx_coded(dev(full), peak=0.0).cpu().numpy()))


def test_tx_coded_var_rejects_what_it_cannot_send():
    e = engine("DQPSK", "R1_4")
    for nb in (0, 325):
        with pytest.raises(RiaError):
            e.var_frame_samples(nb)
    with pytest.raises(RiaError):
        e.tx_coded_var(dev(coded_rows(81)), out_stride=10367)
    assert e.tx_coded_var(dev(np.zeros((0, 81), np.uint8))).shape == (0, 10368)


_received = {}


def received(oracle, name):
    """per handle, computed once: a full frame through AWGN 20 dB and through Watterson moderate 12 dB, a silent frame and a
    frame with one NaN in the third data symbol -> float32 [4, frame_samples]"""
    if name not in _received:
        mod, rate = ids(name)
        x = oracle.modulate(mod, rate, coded_rows(324, 1)[0])
        x = (x * (np.float32(0.8) / np.abs(x).max())).astype(np.float32)
        rows = [oracle.channel(0, 20.0, 71, x), oracle.channel(2, 12.0, 72, x), np.zeros_like(x), oracle.channel(0, 20.0, 73, x)]
        rows[3][4 * 1152 + 300] = np.nan
        _received[name] = np.stack(rows)
    return _received[name]


# (cfo_hz, abs_position, marker) of the four rows of a call
META = ((0.0, 0, 0), (1.5, 480123, 0), (-1.5, 77, 1), (0.0, 5, 0))


def check_against_oracle(oracle, name, llr, st, spans, metas, n_samples):
    mod, rate = ids(name)
    for f, (x, (cfo, ap, mk)) in enumerate(zip(spans, metas)):
        lo, aux = oracle.rx_process(mod, rate, x, cfo, ap, burst_marker=bool(mk))
        assert len(lo) == llr.shape[1], (name, n_samples, f)
        assert np.array_equal(bits(llr[f]), bits(lo)), (name, n_samples, f)
        for k in STATUS_BITS:
            a, b = np.float32(st[k][f]), np.float32(getattr(aux, k))
            assert bits(a) == bits(b) or (np.isnan(a) and np.isnan(b)), (name, n_samples, f, k, a, b)
        assert np.allclose(st["snr_db"][f], aux.snr_db, rtol=1e-5, atol=1e-5, equal_nan=True), (name, n_samples, f)
        assert st["n_llr"][f] == (len(lo) if len(lo) >= 648 else 0), (name, n_samples, f)


@pytest.mark.parametrize("name", list(DEMOD_HANDLES))
def test_demod_var_equals_the_oracle_on_every_span(oracle, name):
    e = engine(*DEMOD_HANDLES[name])
    rx = received(oracle, name)
    fs = e.geo.frame_samples
    cfo, ap, mk = (np.array(v) for v in zip(*META))
    for n in SPANS:
        n = fs if n is None else n
        if n > fs:       # a handle whose frame is shorter than 15 symbols: out of range
            with pytest.raises(RiaError):
                e.demod_var(torch.zeros((1, n), dtype=torch.float32, device="cuda"))
            continue
        spans = np.ascontiguousarray(rx[:, :n])
        llr, st = e.demod_var(dev(spans), cfo_hz=cfo.astype(np.float32), abs_pos=ap.astype(np.uint64), flags=mk.astype(np.uint32))
        check_against_oracle(oracle, name, llr.cpu().numpy(), e.frame_status(st), spans, META, n)
        if n == fs:
            l2, s2 = e.demod(dev(spans), cfo_hz=cfo.astype(np.float32), abs_pos=ap.astype(np.uint64), flags=mk.astype(np.uint32))
            assert torch.equal(llr.view(torch.int32), l2.view(torch.int32)) and torch.equal(st, s2)


@pytest.mark.parametrize("name", ["dqpsk_r14", "qam16_r12"])
def test_demod_var_unaligned_offsets_and_no_meta(oracle, name):
    """spans at unaligned sample offsets of one capture, in an order that is not ascending; and the call without offsets and
    without meta, whose frame f starts at f * n_samples - no multiple of a symbol"""
    e = engine(*DEMOD_HANDLES[name])
    rx = received(oracle, name)
    n = 9 * 1152 + 700
    offs = np.array([3, 1152 + 1, 777, 2 * e.geo.frame_samples + 5], np.uint64)
    cap = np.concatenate([rx[0], rx[1], rx[3], np.zeros(64, np.float32)])
    order = [2, 0, 3, 1]
    spans = [cap[int(offs[i]):int(offs[i]) + n] for i in order]
    metas = [META[i] for i in order]
    cfo, ap, mk = (np.array(v) for v in zip(*metas))
    llr, st = e.demod_var(dev(cap), n_samples=n, cfo_hz=cfo.astype(np.float32), abs_pos=ap.astype(np.uint64), flags=mk.astype(np.uint32),
                          offsets=offs[order])
    check_against_oracle(oracle, name, llr.cpu().numpy(), e.frame_status(st), spans, metas, n)
    rows = np.ascontiguousarray(np.stack([rx[1, :n], rx[0, :n], rx[3, :n]]))
    zeros = dict(cfo_hz=np.zeros(3, np.float32), abs_pos=np.zeros(3, np.uint64), flags=np.zeros(3, np.uint32))
    llr, st = e.demod_var(dev(rows), **zeros)
    check_against_oracle(oracle, name, llr.cpu().numpy(), e.frame_status(st), rows, [(0.0, 0, 0)] * 3, n)
    # without meta the frame starts at phase +0.0, as in ria_gpu_demod_batch; the reference's own product at CFO 0 is -0.0
    l0, s0 = e.demod_var(dev(rows))
    s0, s1 = e.frame_status(s0), e.frame_status(st)
    assert torch.equal(l0.view(torch.int32), llr.view(torch.int32))
    for k in s0.dtype.names:
        a, b = s0[k].view(np.uint32), s1[k].view(np.uint32)
        if k == "corr_phase":      # where the frame keeps CFO 0 the phase never moves: +0.0 here, -0.0 there
            still = s1["cfo_hz"] == 0
            assert still.any() and np.array_equal(a[still], np.zeros(still.sum(), np.uint32)) and np.array_equal(b[still], np.full(still.sum(), 0x80000000, np.uint32))
            assert np.array_equal(a[~still], b[~still])
        else:
            assert np.array_equal(a, b), k


def test_demod_var_rejects_spans_out_of_range():
    e = engine("DQPSK", "R1_4")
    fs = e.geo.frame_samples
    for n in (0, 1152, 3 * 1152 - 1, fs + 1):
        with pytest.raises(RiaError):
            e.demod_var(torch.zeros((2, n), dtype=torch.float32, device="cuda"))
    e.demod_var(torch.zeros((2, 3 * 1152), dtype=torch.float32, device="cuda"))
    assert e.demod_var(torch.zeros((0, 9 * 1152), dtype=torch.float32, device="cuda"))[0].shape == (0, 742)


def test_demod_var_host_gives_the_status_of_the_span_not_of_a_padded_frame(oracle):
    """the one-span host form behind the IWaveform adaptor: soft bits and status of a faded 9-symbol span equal the oracle's;
    the fading index of the same samples zero padded to a frame - what the adaptor reported before - is another number"""
    e = engine("DQPSK", "R1_4")
    x = received(oracle, "dqpsk_r14")[1, :9 * 1152]
    for cfo, ap, mk in ((0.0, 0, 0), (1.5, 480123, 1)):
        llr, st = e.demod_var_host(x, cfo, ap, mk)
        check_against_oracle(oracle, "dqpsk_r14", llr[None], np.array([st]), [x], [(cfo, ap, mk)], len(x))
    padded = np.zeros((1, e.geo.frame_samples), np.float32)
    padded[0, :len(x)] = x
    _, sp = e.demod(dev(padded), cfo_hz=np.zeros(1, np.float32), abs_pos=np.zeros(1, np.uint64), flags=np.zeros(1, np.uint32))
    _, sv = e.demod_var_host(x)
    assert e.frame_status(sp)["fading_index"][0] != sv["fading_index"]
    with pytest.raises(RiaError):
        e.demod_var_host(x[:2 * 1152])


def test_variable_spans_are_unsupported_by_the_one_wave_per_frame_kernel():
    """under RIA_DEMOD_FUSED=1 (read once per process: a fresh child) the three calls that demodulate spans return
    RIA_ERR_UNSUPPORTED (-4), as include/ria_gpu.h says, and the handle's fixed-frame call still runs"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "helpers", "var_fused_child.py")], env=dict(os.environ, RIA_DEMOD_FUSED="1"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "status -4 -4 -4"
