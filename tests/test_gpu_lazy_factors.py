"""GPU tests (-m gpu) of the lazy min-sum factor table: fast_phase0_kernel skips the (codeword, factor) decodes behind a
codeword's first converging factor, recovery_fill_kernel completes the table for the frames whose fallback stage reads
it.  Everything through the C ABI, bit-exact against the CPU oracle's decodeFixedFrame.

The sample is cut from one stream of faded QAM16 R1/2 frames (Watterson moderate, 20 dB; frame idx has the payload drawn
from (seed, idx) and the channel seed seed + idx, tools/count_lazy_factors.py): the first 96 frames and ten frames picked
with the oracle alone (count_lazy_factors.py --scan over frames 0 .. 119 999) for the cases that are rare at this
operating point.  In those 120 000 frames a first decode that fails converges at factor 0.875 in 107 codewords, at 0.75
in 10 and at 0.625 or 0.5 in none; 27 frames of four first-try codewords are repaired by the fallback stage.  So t* = 3 and t* = 4 after a failed
first decode are not in this sample: test_later_factors_through_decode_batch
reaches them with constructed R1/4 codewords."""
import os
import sys
import threading

import numpy as np
import pytest

import pyoracle as po
from test_gpu_parity import dev

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import count_lazy_factors as clf  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 20261004
# 0..95: the common cases; 174, 280, 665: first decode fails, 0.875 converges; 5667, 11638: 0.75 converges;
# 25749, 27604, 39139: the fallback repairs at substitution 12, 13, 1; 41970: at substitution 0
FRAMES = list(range(96)) + [174, 280, 665, 5667, 11638, 25749, 27604, 39139, 41970]
STATUS_FIELDS = ("cw_ok", "iterations", "attempts", "frame_valid", "needs_recovery")


def _threads(work, n, nt=16):
    th = [threading.Thread(target=work, args=(k * n // nt, (k + 1) * n // nt)) for k in range(nt)]
    [t.start() for t in th]; [t.join() for t in th]


@pytest.fixture(scope="module")
def sample(oracle):
    """samples, oracle LLRs and the oracle's classification of every frame of the sample (computed once, never changed)"""
    y = [clf.frame_sample(oracle, po.QAM16, po.R1_2, i, SEED, 2, 20.0) for i in FRAMES]
    llr = [oracle.rx_process(po.QAM16, po.R1_2, s)[0] for s in y]
    cls = [None] * len(y)
    clf.classify(oracle, llr[0], po.R1_2, 188)

    def work(lo, hi):
        for q in range(lo, hi):
            cls[q] = clf.classify(oracle, llr[q], po.R1_2, 188)
    _threads(work, len(y))
    return np.stack(y), np.stack(llr), cls


def _expected(oracle, cls):
    d = np.stack([c["full"][0] for c in cls])
    st = {"cw_ok": np.stack([c["full"][1] for c in cls]),
          "iterations": np.stack([c["full"][2] for c in cls]).astype(np.uint16),
          "attempts": np.stack([c["full"][3] for c in cls]).astype(np.uint8)}
    st["frame_valid"] = np.array([int(bool(c["full"][1].all()) and clf.verify(oracle, c["full"][0], 40)) for c in cls], np.uint8)
    st["needs_recovery"] = np.zeros(len(cls), np.uint8)
    return d, st


def _check(out, s, exp_d, exp_st, what):
    assert np.array_equal(out, exp_d), f"{what}: payload bytes of frames {np.nonzero((out != exp_d).any(axis=1))[0][:8]}"
    for k in STATUS_FIELDS:
        assert np.array_equal(s[k], exp_st[k]), f"{what}: status field {k}"


def test_sample_holds_every_case(sample):
    """the counts the other tests rely on, from the oracle alone: the sample cannot drift"""
    _, _, cls = sample
    tstar = [c["tstar"][cw] for c in cls for cw in range(4) if c["first_fails"][cw]]
    assert tstar.count(1) == 3 and tstar.count(2) == 2, tstar      # frames 174, 280, 665 and 5667, 11638
    assert tstar.count(5) >= 40                                     # fails all four: enters the cascade
    inherit = [c["inherit"][cw] for c in cls for cw in range(4) if c["inherit"][cw] is not None]
    assert inherit.count(True) >= 10 and inherit.count(False) >= 10  # first decode at the inherited 0.875 (f == 1)
    stages = [c["stage"] for c in cls]
    assert stages.count(1) >= 5                                     # repaired by stage 1
    assert sorted(c["s2_index"] for c in cls if c["stage"] == 2) == [0, 1, 12, 13]
    assert stages.count(3) >= 10                                    # stage 2 walks all 16 and cannot repair


def test_rx_batch_unsplit_and_three_parts_twice(oracle, sample):
    """ria_gpu_rx_batch with DECODE_FULL: the sample alone, then tiled to more than 4096 frames (the size from which
    the call is cut into parts) on one stream and in 3 parts, each twice on one handle: every copy equals the oracle"""
    import torch
    from ria_amd.engine import RxEngine
    y, _, cls = sample
    exp_d, exp_st = _expected(oracle, cls)
    n, reps = len(y), 4096 // len(y) + 1
    e = RxEngine("QAM16", "R1_2", max_batch=n * reps)
    x1, xt = dev(y), dev(np.tile(y, (reps, 1)))
    for parts in (1, 3):
        e.set_split_parts(parts)
        for rep in range(2):
            out, st = e.rx(x1)
            torch.cuda.synchronize()
            _check(out.cpu().numpy(), e.decode_status(st), exp_d, exp_st, f"parts {parts} run {rep}")
            out, st = e.rx(xt)
            torch.cuda.synchronize()
            out, s = out.cpu().numpy(), e.decode_status(st)
            for k in range(reps):
                _check(out[k * n:(k + 1) * n], {f: s[f][k * n:(k + 1) * n] for f in STATUS_FIELDS}, exp_d, exp_st,
                       f"parts {parts} run {rep} copy {k}")
    assert e.lib.ria_gpu_debug_queue_fault(e.h) == 0
    e.close()


@pytest.mark.parametrize("flags", [1, 2, 7])
def test_decode_batch_flag_subsets(oracle, sample, flags):
    """ria_gpu_decode_batch with phase 0 only, the perturbation cascade only and the full flags on the oracle's LLRs"""
    from test_gpu_parity import engine
    _, llr, cls = sample
    e = engine("QAM16", "R1_2")
    exp = [None] * len(llr)

    def work(lo, hi):
        for q in range(lo, hi):
            exp[q] = cls[q]["full"] if flags == 7 else oracle.decode_fixed_frame(llr[q], po.R1_2, True, 188, flags=flags)
    _threads(work, len(llr))
    for rep in range(2):
        out, st = e.decode(dev(llr), flags=flags)
        out, s = out.cpu().numpy(), e.decode_status(st)
        for q in range(len(llr)):
            d, ok, iters, att = exp[q]
            assert np.array_equal(s["cw_ok"][q], ok) and np.array_equal(out[q], d), f"flags {flags} frame {FRAMES[q]}"
            assert np.array_equal(s["iterations"][q], iters.astype(np.uint16)), f"flags {flags} frame {FRAMES[q]}: iterations"
            assert np.array_equal(s["attempts"][q], att.astype(np.uint8)), f"flags {flags} frame {FRAMES[q]}: attempts"


def test_another_shape_r14_vs_oracle(oracle):
    """DQPSK R1/4 (another Shape of every decode kernel), 256 frames on Watterson moderate at a marginal -2 dB"""
    from test_gpu_parity import engine
    e = engine("DQPSK", "R1_4")
    n, bps = 256, int(e.geo.bits_per_symbol)
    y = np.stack([clf.frame_sample(oracle, po.DQPSK, po.R1_4, i, 4711, 2, -2.0) for i in range(n)])
    out, st, llr, _ = e.rx(dev(y), want_llr=True)
    out, s, llr = out.cpu().numpy(), e.decode_status(st), llr.cpu().numpy()
    exp = [None] * n

    def work(lo, hi):
        for q in range(lo, hi):
            exp[q] = oracle.decode_fixed_frame(llr[q], po.R1_4, True, bps, flags=7)
    oracle.decode_fixed_frame(llr[0], po.R1_4, True, bps, flags=7)
    _threads(work, n)
    n_retry = 0
    for q in range(n):
        d, ok, iters, att = exp[q]
        assert np.array_equal(s["cw_ok"][q], ok) and np.array_equal(out[q], d), f"frame {q}"
        assert np.array_equal(s["iterations"][q], iters.astype(np.uint16)) and np.array_equal(s["attempts"][q], att.astype(np.uint8)), f"frame {q}"
        n_retry += int((att > 1).any())
    assert 20 <= n_retry <= n - 20, n_retry    # marginal: both the first-try frames and the retry machinery are in it


# ---- later factors: constructed R1/4 codewords at the edge of convergence ----------------------------------------------
# At the faded operating points above a first decode that fails converges at 0.875 or 0.75 or not at all.  Codewords
# whose FIRST converging factor is 0.625 or 0.5 were found with the oracle alone among noisy R1/4 codewords (the recipe
# of oracle/gen_golden.py robust_fixture, one generator per index): LATER[t] lists indices with t* = t, 5 = no factor.
LATER = {1: (18, 21), 2: (7, 53), 3: (360, 681), 4: (9375,), 5: (1, 10)}
NOISE_SCALE = {9375: 1.02}    # t* = 3 as drawn; with 2 % more of its noise only 0.5 converges (found by walking the scale up)


def _edge_codeword(oracle, idx, clean=False):
    rng = np.random.default_rng([60606, idx])
    info = rng.integers(0, 256, 21, dtype=np.uint8)
    info[-1] &= 0xC0
    bits = np.unpackbits(oracle.ldpc_encode(po.R1_4, info)[:81])[:648].astype(np.float32)
    sigma = (1.3, 1.4, 1.5)[idx % 3]
    noise = rng.normal(0, sigma, 648) * NOISE_SCALE.get(idx, 1.0)
    if clean:
        return ((1.0 - 2.0 * bits) * 8.0).astype(np.float32)
    return np.clip(((1.0 - 2.0 * bits) + noise) * (2.0 / sigma ** 2), -20, 20).astype(np.float32)


def test_later_factors_through_decode_batch(oracle):
    """Frames of four R1/4 codewords through ria_gpu_decode_batch: an edge codeword with t* = 1, 2, 3, 4 or none in every
    position, clean codewords behind it (listed, first decode converged: phase 0 runs 0.875 for them and skips the
    rest), two edge codewords in one frame.  Phase 0 only, phase 0 + cascade, and the full flags against the oracle."""
    from test_gpu_parity import engine
    e = engine("DQPSK", "R1_4")
    bps, mi = int(e.geo.bits_per_symbol), oracle.geom(po.DQPSK, po.R1_4).max_iter
    table = oracle.gather_table(bps, True)
    plans = []
    for t, idxs in LATER.items():
        a, b = idxs[0], idxs[-1]
        plans += [(a, None, None, None), (None, b, None, None), (None, None, None, a), (a, None, b, None)]
    plans += [(LATER[3][0], LATER[4][0], LATER[2][0], LATER[1][0]), (LATER[5][0], LATER[4][-1], LATER[3][-1], None)]
    llr = np.zeros((len(plans), 2592), np.float32)
    tstar, listed_first_ok = [], 0
    for q, plan in enumerate(plans):
        listed = False
        for cw, idx in enumerate(plan):
            v = _edge_codeword(oracle, 1000 + 4 * q + cw, clean=True) if idx is None else _edge_codeword(oracle, idx)
            llr[q, table[cw * 648:(cw + 1) * 648]] = v
            first = oracle.ldpc_decode(po.R1_4, v, mi, clf.FACTORS[0])[0]
            if not first:
                tstar.append(next((t for t in range(1, 5) if oracle.ldpc_decode(po.R1_4, v, mi, clf.FACTORS[t])[0]), 5))
            listed_first_ok += int(listed and first)
            listed = listed or not first
    for t in (1, 2, 3, 4, 5):
        assert tstar.count(t) >= 1, (t, tstar)          # a failed first decode whose first converging factor is t (5: none)
    assert listed_first_ok >= 10                         # listed codewords whose first decode converged
    for flags in (1, 3, 7):
        exp = [None] * len(plans)

        def work(lo, hi):
            for q in range(lo, hi):
                exp[q] = oracle.decode_fixed_frame(llr[q], po.R1_4, True, bps, flags=flags)
        oracle.decode_fixed_frame(llr[0], po.R1_4, True, bps, flags=flags)
        _threads(work, len(plans))
        out, st = e.decode(dev(llr), flags=flags)
        out, s = out.cpu().numpy(), e.decode_status(st)
        for q in range(len(plans)):
            d, ok, iters, att = exp[q]
            assert np.array_equal(s["cw_ok"][q], ok) and np.array_equal(out[q], d), f"flags {flags} frame {plans[q]}"
            assert np.array_equal(s["iterations"][q], iters.astype(np.uint16)), f"flags {flags} frame {plans[q]}: iterations"
            assert np.array_equal(s["attempts"][q], att.astype(np.uint8)), f"flags {flags} frame {plans[q]}: attempts"
