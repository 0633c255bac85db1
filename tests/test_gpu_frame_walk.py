"""GPU tests (-m gpu) of the frame walk of the first decodes: fast_primary_kernel walks a frame's four codewords in order
and, with RIA_DECODE_PERTURB, does not make the 0.9375 decode of a codeword behind a failed one (the reference's decoder
object stays at 0.875 there); it lists and stages those codewords itself.  Behind a phase-0 rescue the decoder is back at
0.9375: fast_chain_kernel defers such a frame and fast_late_kernel makes the missing decode.  Everything through the C
ABI, bit for bit over the payload bytes and every DECODE_STATUS field against the CPU oracle's decode_fixed_frame; the
counters (ria_gpu_debug_first_decodes) against tools/count_unread_first_decodes.py walk() on the same soft bits.

The pinned sample is cut from the bench-like stream of tools/count_lazy_factors.py (QAM16 R1/2, Watterson moderate, 20 dB,
seed 20261004): frames 0 .. 91 and the four frames of the first 3 000 in which phase 0 rescues a codeword at 0.875
(174, 280, 665, 2344; in 174, 665 and 2344 a codeword follows the rescued one, which is the late decode).  The classes
it must hold are asserted from the oracle alone (test_sample_holds_every_class)."""
import os
import sys
import threading

import numpy as np
import pytest

import pyoracle as po
from test_gpu_parity import dev

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import count_lazy_factors as clf  # noqa: E402
import count_unread_first_decodes as cuf  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 20261004
FRAMES = list(range(92)) + [174, 280, 665, 2344]
RESCUED_T2 = (5667, 11638)      # bench-stream frames with a codeword phase 0 rescues at 0.75 (count_lazy_factors.py --scan)
TILED = 4104                    # three parts of 1368 frames
STATUS_FIELDS = ("cw_ok", "iterations", "attempts", "frame_valid", "needs_recovery")


def _threads(work, n, nt=16):
    th = [threading.Thread(target=work, args=(k * n // nt, (k + 1) * n // nt)) for k in range(nt)]
    [t.start() for t in th]; [t.join() for t in th]


def _expect(oracle, llr, mod, rate, bps, flags):
    """the oracle's decode of every row of llr under `flags` -> (payload bytes, status fields); computed once per use"""
    n, bpc = len(llr), oracle.geom(mod, rate).bytes_per_cw
    res = [None] * n
    oracle.decode_fixed_frame(llr[0], rate, True, bps, flags=flags)

    def work(lo, hi):
        for q in range(lo, hi):
            res[q] = oracle.decode_fixed_frame(llr[q], rate, True, bps, flags=flags)
    _threads(work, n)
    d = np.stack([r[0] for r in res])
    all_ok = np.array([bool(r[1].all()) for r in res])
    valid = np.array([bool(all_ok[q]) and clf.verify(oracle, res[q][0], bpc) for q in range(n)])
    st = {"cw_ok": np.stack([r[1] for r in res]).astype(np.uint8),
          "iterations": np.stack([r[2] for r in res]).astype(np.uint16),
          "attempts": np.stack([r[3] for r in res]).astype(np.uint8),
          "frame_valid": valid.astype(np.uint8),
          # without RIA_DECODE_CRC_RECOVER (bit 2) a frame of four converged codewords that fails its check stays flagged
          "needs_recovery": (np.zeros(n, np.uint8) if flags & 4 else (all_ok & ~valid).astype(np.uint8))}
    return d, st


def _check(out, s, exp, what, idx=None, names=None):
    exp_d, exp_st = exp
    if idx is not None:
        exp_d, exp_st = exp_d[idx], {k: v[idx] for k, v in exp_st.items()}
    bad = np.nonzero((out != exp_d).any(axis=1))[0]
    assert bad.size == 0, f"{what}: payload bytes of rows {bad[:8]}" + (f" = {[names[b] for b in bad[:8]]}" if names else "")
    for k in STATUS_FIELDS:
        rows = np.nonzero((np.asarray(s[k]) != exp_st[k]).reshape(len(exp_d), -1).any(axis=1))[0]
        assert rows.size == 0, f"{what}: status field {k}, rows {rows[:8]}"


def _counts(walks, idx=None):
    sk = np.array([sum(w["skipped"]) for w in walks])
    late = np.array([sum(w["late"]) for w in walks])
    if idx is not None:
        sk, late = sk[idx], late[idx]
    return {"skipped": int(sk.sum()), "late": int(late.sum())}


def _first_decodes(e, slots=1):
    tot = {"skipped": 0, "late": 0}
    for s in range(slots):
        c = e.first_decodes(s)
        tot = {k: tot[k] + c[k] for k in tot}
    return tot


@pytest.fixture(scope="module")
def sample(oracle):
    """samples and oracle LLRs of the pinned frames, the tool's walk of each (flags 3) and the oracle's full decode: computed
    once, never changed"""
    y = [clf.frame_sample(oracle, po.QAM16, po.R1_2, i, SEED, 2, 20.0) for i in FRAMES]
    llr = np.stack([oracle.rx_process(po.QAM16, po.R1_2, s)[0] for s in y])
    walks = [None] * len(y)

    def work(lo, hi):
        for q in range(lo, hi):
            walks[q] = cuf.walk(oracle, llr[q], po.R1_2, 188)
    work(0, 1)
    _threads(work, len(y))
    return np.stack(y), llr, walks, _expect(oracle, llr, po.QAM16, po.R1_2, 188, 7)


def test_sample_holds_every_class(oracle, sample):
    """the classes the other tests rely on, from the oracle alone: the sample cannot drift"""
    _, llr, walks, (exp_d, exp_st) = sample
    assert len(FRAMES) <= 96
    classes = [cuf.frame_classes(w) for w in walks]
    for c in ("no failure", "first failure at cw 0", "first failure at cw 1", "first failure at cw 2", "first failure at cw 3",
              "failing behind failing", "converging behind failing", "late decode"):
        assert sum(c in k for k in classes) >= 3, c
    # flagged for the fallback with a skipped slot 0: the walk skipped a first decode of the frame, phases 0..2 leave four
    # converged codewords whose frame check fails (flags 3), and the full decode cannot repair it, so stage 1 failed and the
    # fallback stage ran
    d3, st3 = _expect(oracle, llr, po.QAM16, po.R1_2, 188, 3)
    n_fb = sum(1 for q, w in enumerate(walks) if any(w["skipped"]) and st3["needs_recovery"][q] and not exp_st["cw_ok"][q].all())
    assert n_fb >= 3, n_fb
    # the tool counts no fallback trial that reads a skipped slot: the substitutions are factors 0.75, 0.625, 0.5, 0.875
    assert sum(w["fill_back"] for w in walks) == 0
    assert _counts(walks)["late"] == 3 and _counts(walks)["skipped"] >= 60


def test_rx_batch_layouts_twice_with_counters(oracle, sample):
    """ria_gpu_rx_batch with DECODE_FULL: the sample in order, reversed, and tiled to 4 104 frames on one stream and in three
    parts, each twice on one handle: every layout equals the oracle, the split result equals the un-split one, and the
    counters equal the tool's counts"""
    import torch
    from ria_amd.engine import RxEngine
    y, _, walks, exp = sample
    n = len(y)
    e = RxEngine("QAM16", "R1_2", max_batch=TILED)
    layouts = {"in order": np.arange(n), "reversed": np.arange(n)[::-1].copy(), "tiled": np.arange(TILED) % n}
    outs = {}
    for name, idx in layouts.items():
        x = dev(y[idx])
        for parts in ((1, 3) if name == "tiled" else (1,)):
            e.set_split_parts(parts)
            for rep in range(2):
                out, st = e.rx(x)
                torch.cuda.synchronize()
                out, s = out.cpu().numpy(), e.decode_status(st)
                _check(out, s, exp, f"{name}, parts {parts}, run {rep}", idx)
                assert _first_decodes(e, parts) == _counts(walks, idx), f"{name}, parts {parts}, run {rep}"
                outs[(name, parts)] = (out, {k: s[k].copy() for k in STATUS_FIELDS})
    a, b = outs[("tiled", 1)], outs[("tiled", 3)]
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][k], b[1][k]) for k in STATUS_FIELDS)
    assert e.lib.ria_gpu_debug_queue_fault(e.h) == 0
    e.close()


@pytest.mark.parametrize("flags", [1, 2, 0, 7])
def test_decode_batch_flag_combinations(oracle, sample, flags):
    """ria_gpu_decode_batch on the oracle's LLRs, in order and reversed, twice: phase 0 only, the cascade only, neither, and
    DECODE_FULL.  Without RIA_DECODE_PERTURB nothing is skipped; without RIA_DECODE_PHASE0 nothing is rescued, so nothing
    is made late"""
    from test_gpu_parity import engine
    _, llr, walks, exp7 = sample
    e = engine("QAM16", "R1_2")
    exp = exp7 if flags == 7 else _expect(oracle, llr, po.QAM16, po.R1_2, 188, flags)
    if flags == 7:
        want = _counts(walks)
    elif flags == 2:
        want = {"skipped": _counts(walks)["skipped"], "late": 0}
    else:
        want = {"skipped": 0, "late": 0}
    for name, idx in (("in order", np.arange(len(llr))), ("reversed", np.arange(len(llr))[::-1].copy())):
        x = dev(llr[idx])
        for rep in range(2):
            out, st = e.decode(x, flags=flags)
            _check(out.cpu().numpy(), e.decode_status(st), exp, f"flags {flags}, {name}, run {rep}", idx, [FRAMES[i] for i in idx])
            assert e.first_decodes(0) == want, f"flags {flags}, {name}, run {rep}"
    assert e.lib.ria_gpu_debug_queue_fault(e.h) == 0


# ---- the rare path: a rescued codeword in position k, every kind of codeword behind it ------------------------------------
def _synthetic(oracle, rate, mod, bps, n_llr, rescued, clean, hopeless):
    """frames of four codeword rows scattered through the gather table: clean rows, a rescued row in position k = 0, 1, 2, and
    behind it a clean row, a hopeless one or a second rescued one -> (llr, walks under flags 3, plan names)"""
    table = oracle.gather_table(bps, True)
    plans = []
    for i, (name, r) in enumerate(rescued):
        other = rescued[(i + 1) % len(rescued)]
        for k in (0, 1, 2):
            for bname, b in (("clean", clean[0]), ("hopeless", hopeless), other):
                rows = [clean[j % len(clean)] for j in range(4)]
                rows[k], rows[k + 1] = r, b
                plans.append((f"{name} at {k}, {bname} behind", rows))
    llr = np.zeros((len(plans), n_llr), np.float32)
    for q, (_, rows) in enumerate(plans):
        for cw in range(4):
            llr[q, table[cw * 648:(cw + 1) * 648]] = rows[cw]
    walks = [None] * len(plans)

    def work(lo, hi):
        for q in range(lo, hi):
            walks[q] = cuf.walk(oracle, llr[q], rate, bps, mod)
    work(0, 1)
    _threads(work, len(plans))
    return llr, walks, [p[0] for p in plans]


def _run_synthetic(oracle, e, mod, rate, bps, llr, walks, names, tstars):
    assert {w["rescued"][cw] for w in walks for cw in range(4)} >= set(tstars), "a rescue at every factor"
    assert sum(sum(w["late"]) >= 2 for w in walks) >= 2, "more than one late decode in one frame"
    assert sum(sum(1 for t in w["rescued"] if t) >= 2 for w in walks) >= 2, "a double rescue"
    late_fails = sum(1 for w in walks for cw in range(4) if w["late"][cw] and not w["d0"][cw][0])
    assert late_fails >= 2 and _counts(walks)["late"] - late_fails >= 2, "late decodes that fail and that converge"
    exp = _expect(oracle, llr, mod, rate, bps, 7)
    x = dev(llr)
    for rep in range(2):
        out, st = e.decode(x, flags=7)
        _check(out.cpu().numpy(), e.decode_status(st), exp, f"run {rep}", None, names)
        assert e.first_decodes(0) == _counts(walks), f"run {rep}"
    assert e.lib.ria_gpu_debug_queue_fault(e.h) == 0


def test_rescue_then_every_kind_of_codeword_r12(oracle, sample):
    """QAM16 R1/2: the bench stream's own rescued codewords (0.875: frames 174, 280, 665; 0.75: frames 5667, 11638)"""
    from test_gpu_parity import engine
    _, llr, walks, _ = sample
    table = oracle.gather_table(188, True)
    rows = lambda v, cw: v[table[cw * 648:(cw + 1) * 648]].copy()  # noqa: E731
    rescued = []
    for fr in (174, 280, 665):
        q = FRAMES.index(fr)
        rescued += [(f"frame {fr} cw {cw}", rows(llr[q], cw)) for cw in range(4) if walks[q]["rescued"][cw]]
    for fr in RESCUED_T2:
        v = oracle.rx_process(po.QAM16, po.R1_2, clf.frame_sample(oracle, po.QAM16, po.R1_2, fr, SEED, 2, 20.0))[0]
        w = cuf.walk(oracle, v, po.R1_2, 188)
        rescued += [(f"frame {fr} cw {cw}", rows(v, cw)) for cw in range(4) if w["rescued"][cw]]
    q0 = next(q for q, w in enumerate(walks) if w["first_fail"] is None)
    qh = next(q for q, w in enumerate(walks) if w["cascade"][0])
    e = engine("QAM16", "R1_2")
    s_llr, s_walks, names = _synthetic(oracle, po.R1_2, po.QAM16, 188, int(e.geo.llrs_per_frame), rescued,
                                       [rows(llr[q0], cw) for cw in range(4)], rows(llr[qh], 0))
    _run_synthetic(oracle, e, po.QAM16, po.R1_2, 188, s_llr, s_walks, names, (1, 2))


def test_rescue_at_every_factor_r14(oracle):
    """DQPSK R1/4 (another Shape): constructed codewords at the edge of convergence whose first converging factor is 0.875,
    0.75, 0.625 and 0.5 (tests/test_gpu_lazy_factors.py LATER)"""
    from test_gpu_parity import engine
    from test_gpu_lazy_factors import LATER, _edge_codeword
    e = engine("DQPSK", "R1_4")
    bps = int(e.geo.bits_per_symbol)
    rescued = [(f"edge {LATER[t][0]} (t* = {t})", _edge_codeword(oracle, LATER[t][0])) for t in (1, 2, 3, 4)]
    clean = [_edge_codeword(oracle, 2000 + j, clean=True) for j in range(4)]
    s_llr, s_walks, names = _synthetic(oracle, po.R1_4, po.DQPSK, bps, 2592, rescued, clean, _edge_codeword(oracle, LATER[5][0]))
    _run_synthetic(oracle, e, po.DQPSK, po.R1_4, bps, s_llr, s_walks, names, (1, 2, 3, 4))


@pytest.mark.parametrize("mod,rate,kind,snr", [("DQPSK", "R1_4", 2, -2.0), ("QAM16", "R3_4", 1, 20.0)])
def test_other_rates_vs_oracle(oracle, mod, rate, kind, snr):
    """two more Shapes of the walk: 64 faded frames each at a marginal operating point (Watterson moderate / good) through
    ria_gpu_rx_batch"""
    from test_gpu_parity import engine
    e = engine(mod, rate)
    pm, pr = getattr(po, mod), getattr(po, rate)
    n, bps = 64, int(e.geo.bits_per_symbol)
    y = np.stack([clf.frame_sample(oracle, pm, pr, i, 4711, kind, snr) for i in range(n)])
    out, st, llr, _ = e.rx(dev(y), want_llr=True)
    out, s, llr = out.cpu().numpy(), e.decode_status(st), llr.cpu().numpy()
    walks = [cuf.walk(oracle, llr[q], pr, bps, pm) for q in range(n)]
    n_walk = sum(any(w["skipped"]) for w in walks)
    assert 8 <= n_walk <= n - 8, n_walk    # marginal: frames with skipped first decodes and frames without
    _check(out, s, _expect(oracle, llr, pm, pr, bps, 7), f"{mod} {rate}")
    assert e.first_decodes(0) == _counts(walks)
