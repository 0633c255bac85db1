"""The retry cascade takes one GROUP of attempts of one codeword per queue unit (ldpc_fast.hip.h, kernel D2): per-frame
parity with the CPU oracle on samples chosen (with the oracle alone) to hold a winner at every position of a group,
independence of the batch split, and the noise-free attempt 26.  Bytes, codeword success, iteration and attempt counts are
compared bit for bit; the oracle's decodeFixedFrame returns exactly these fields of the decode status."""
import functools
import threading

import numpy as np
import pytest

import pyoracle as po

pytestmark = pytest.mark.gpu

# attempts field of a codeword that went to the cascade: 1 first decode + 4 other factors + (winner + 1), or + 34
CASCADE_BASE = 6
_engines = {}


def engine(mod, rate):
    from ria_amd.engine import RxEngine
    if (mod, rate) not in _engines:
        _engines[(mod, rate)] = RxEngine(mod, rate)
    return _engines[(mod, rate)]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def faded_frames(mod, rate, seed, first, n, snr):
    """Frames with oracle-made headers and fixed-seed payloads -> library TX -> reference-identical Watterson moderate
    channel (channel 2, seed + first + f per frame); returns the device tensor of received samples."""
    from ria_amd import capi
    e, O = engine(mod, rate), po.Oracle()
    cap = int(e.geo.info_bytes_per_frame) - 19
    info = np.stack([O.make_frame(np.random.default_rng([seed, f]).integers(0, 256, cap, dtype=np.uint8), f, capi.RATE[rate])
                     for f in range(n)])
    x = e.tx(dev(info), peak=0.8)
    e.channel_exact_(x, 2, snr, seed, first_frame=first)
    return x


def oracle_answers(mod, rate, y):
    """rx_process + decodeFixedFrame (flags 7) of the oracle for every frame of y, on the host cores."""
    from ria_amd import capi
    pm, pr = capi.MOD[mod], capi.RATE[rate]
    n = len(y)
    g = po.Oracle().geom(pm, pr)
    bps, nb = int(g.bits_per_symbol), 4 * int(g.bytes_per_cw)
    llr = [None] * n
    data, ok = np.zeros((n, nb), np.uint8), np.zeros((n, 4), np.uint8)
    iters, att = np.zeros((n, 4), np.uint16), np.zeros((n, 4), np.uint8)

    def work(lo, hi):
        O = po.Oracle()
        for f in range(lo, hi):
            l, _ = O.rx_process(pm, pr, y[f])
            llr[f] = l
            data[f], ok[f], it, at = O.decode_fixed_frame(l, pr, True, bps, flags=7)
            iters[f], att[f] = it, at
    nt = 16
    th = [threading.Thread(target=work, args=(k * n // nt, (k + 1) * n // nt)) for k in range(nt)]
    [t.start() for t in th]; [t.join() for t in th]
    return {"llr": np.stack(llr), "data": data, "ok": ok, "iters": iters, "att": att}


def assert_same(out, s, exp, what):
    for f in range(len(out)):
        assert np.array_equal(s["cw_ok"][f], exp["ok"][f]) and np.array_equal(out[f], exp["data"][f]), f"{what} frame {f}: bytes / success"
        assert np.array_equal(s["iterations"][f], exp["iters"][f]) and np.array_equal(s["attempts"][f], exp["att"][f]), \
            f"{what} frame {f}: iterations {s['iterations'][f]} vs {exp['iters'][f]}, attempts {s['attempts'][f]} vs {exp['att'][f]}"


def winners(exp):
    """cascade winners (0..33) of the sample's codewords and the number of codewords that failed all 34 attempts"""
    att, ok = exp["att"].astype(int).reshape(-1), exp["ok"].reshape(-1) != 0
    return att[(att >= CASCADE_BASE) & ok] - CASCADE_BASE, int(((att == CASCADE_BASE + 33) & ~ok).sum())


# QAM16 R1/2 at the bench's 20 dB: seed and size chosen once with the oracle alone (seeds 1..5 and 20261018 tried at 512
# and 256 frames; seed 1 x 512 is the first that holds a winner in the short last group)
R12_SAMPLE = ("QAM16", "R1_2", 1, 1000, 512, 20.0)


@functools.lru_cache(maxsize=None)
def r12_sample():
    mod, rate, seed, first, n, snr = R12_SAMPLE
    x = faded_frames(mod, rate, seed, first, n, snr)
    return x, oracle_answers(mod, rate, x.cpu().numpy())


def test_cascade_groups_per_frame_parity_with_the_oracle():
    """512 faded QAM16 R1/2 frames through ria_gpu_rx_batch (DECODE_FULL) against the oracle, every frame, every field.
    The sample holds (asserted from the oracle's attempts, for each group size 2, 4 and 8 the kernel can be built with):
    a winner at the first and at the last attempt of a group, a winner in the short last group, codewords that fail all 34
    attempts and winners >= 26 (attempt 26 ran and lost)."""
    from ria_amd import capi
    x, exp = r12_sample()
    w, n_fail = winners(exp)
    for G in (2, 4, 8):
        assert (w % G == 0).any() and (w % G == G - 1).any(), f"sample holds no winner at the first / last attempt of a group of {G}"
    assert (w >= 32).any(), "sample holds no winner in the short last group"
    assert n_fail >= 1, "sample holds no codeword that fails all 34 attempts"
    assert (w > 26).any(), "sample holds no winner above attempt 26"
    e = engine("QAM16", "R1_2")
    out, st = e.rx(x, flags=capi.DECODE_FULL)
    assert_same(out.cpu().numpy(), e.decode_status(st), exp, "QAM16 R1_2")


def test_cascade_groups_other_code_rate():
    """R1/4 (m = 486: another Shape and LDS footprint), DQPSK on Watterson moderate, 128 frames each at the marginal 7 dB
    of test_other_modes_vs_the_reference_library's mode table and at -1 dB, where the oracle sends codewords of this
    sample to the cascade (at 7 dB every first decode of these 128 frames converges)."""
    for snr, need_cascade in ((7.0, False), (-1.0, True)):
        x = faded_frames("DQPSK", "R1_4", 1, 1000, 128, snr)
        exp = oracle_answers("DQPSK", "R1_4", x.cpu().numpy())
        w, n_fail = winners(exp)
        assert not need_cascade or (len(w) >= 1 and n_fail >= 1), "sample holds no cascade codeword"
        e = engine("DQPSK", "R1_4")
        out, st = e.rx(x)
        assert_same(out.cpu().numpy(), e.decode_status(st), exp, f"DQPSK R1_4 {snr} dB")


def test_cascade_groups_do_not_depend_on_the_split():
    """4 200 faded frames (just above the 4 096-frame split threshold) through 1 part and through 3 parts, twice on one
    handle: all bytes and all status fields identical (seed scratch shared between stream slots, or state left over from
    the call before, would show here)."""
    import torch
    e = engine("QAM16", "R1_2")
    n, seed, first = 4200, 20261004, 7000
    x = e.tx(e.make_frames(seed, first, n), peak=0.8)
    e.channel_exact_(x, 2, 20.0, seed, first_frame=first)
    runs = []
    try:
        for parts in (1, 3, 1, 3):
            e.set_split_parts(parts)
            out, st = e.rx(x)
            torch.cuda.synchronize()
            runs.append((out.cpu().numpy(), st.cpu().numpy()))
    finally:
        e.set_split_parts(0)
    att = e.decode_status(dev(runs[0][1]))["attempts"]
    assert (att >= CASCADE_BASE).sum() >= 100, "sample does not exercise the cascade"
    for k in range(1, 4):
        assert np.array_equal(runs[0][0], runs[k][0]) and np.array_equal(runs[0][1], runs[k][1]), f"run {k} differs from run 0"


def test_attempt_26_winners_through_decode_batch():
    """LLR rows (from the parity sample) in which the oracle's cascade winner is exactly attempt 26, the attempt whose
    noise has sigma 0 and whose RNG set-up the kernel skips, through ria_gpu_decode_batch: same bytes, success,
    iterations and attempts as the oracle."""
    _, exp = r12_sample()
    att, ok = exp["att"].astype(int), exp["ok"] != 0
    rows = np.nonzero(((att == CASCADE_BASE + 26) & ok).any(axis=1))[0]
    assert len(rows) >= 1, "sample holds no attempt-26 winner"
    e = engine("QAM16", "R1_2")
    out, st = e.decode(dev(exp["llr"][rows]))
    sub = {k: v[rows] for k, v in exp.items()}
    assert_same(out.cpu().numpy(), e.decode_status(st), sub, "attempt 26")
