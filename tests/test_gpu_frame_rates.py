"""GPU tests (-m gpu) of ria_gpu_decode_batch at all six code rates and every step of the CRC recovery, on the constructed
frames of tests/ldpc_domain_inputs.py: the four noise shapes at DBPSK R1/3, D8PSK R2/3, QAM32 R5/6, QAM64 R3/4 and
QAM256 R2/3 (grades taken from each rate's waterfall), and at all seven modes one set per recovery step that the step
REPAIRS (hdr1, hdr2, single, crc, pair, triple, quad, and the fallback fill where a search found such frames) and one
that no step repairs, so bytes per codeword 20, 27, 40, 54, 60 and 67 all pass through the recovery's index arithmetic.
Reference answers come live from oracle/_ref where it is built, else from tests/golden/ldpc_domain.npz; iterations,
attempts and the recovery step from the CPU oracle."""
import os
import sys

import numpy as np
import pytest

import ldpc_domain_inputs as L
import pyoracle as po
from test_gpu_ldpc_domain import RATE_NAME, check_frame_family, dev, engine

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import count_state_repeats as csr  # noqa: E402

pytestmark = pytest.mark.gpu

STATUS_FIELDS = ("cw_ok", "iterations", "attempts", "frame_valid", "needs_recovery")
BATCH_SIZES = (1, 63, 64, 65, 257, 4100)
_mix = {}


@pytest.mark.parametrize("mod,rate,shape,n,seed", L.NEW_FRAME_SETS)
def test_decode_fixed_frame_families_at_every_rate(golden, oracle, monkeypatch, mod, rate, shape, n, seed):
    """what test_gpu_ldpc_domain.test_decode_fixed_frame_families asserts, on every new set; for the sets a recovery step
    repairs also the recovery's counters: frames flagged, and frames that reach the fallback stage"""
    from ria_amd import capi
    check_frame_family(golden, oracle, monkeypatch, mod, rate, shape, n, seed)
    if shape in L.STAGES + (L.FILL, L.BEYOND):
        e = engine(mod, RATE_NAME[rate])
        llr, infos = L.frames(oracle, mod, rate, shape, n, seed)
        cl = L.recovery_classes(oracle, mod, rate, llr, infos)
        d, st = e.decode(dev(llr), flags=capi.DECODE_FULL)
        cnt = e.recovery_counts(0)
        assert cnt["flagged"] == sum(s != "none" for s, _ in cl) == n, (cnt, cl)
        assert cnt["fallback"] == sum(s in (L.FILL, "failed") for s, _ in cl), (cnt, cl)
        # the repaired frames give the sent bytes back, the others ("an earlier wrong match wins") validate other bytes
        good = np.array([k == "repaired" for _, k in cl])
        d, s = d.cpu().numpy(), e.decode_status(st)
        assert np.array_equal(s["frame_valid"] != 0, np.array([k in ("repaired", "wrong") for _, k in cl])), cl
        assert np.array_equal((d == infos).all(1), good), cl
        assert e.lib.ria_gpu_debug_queue_fault(e.h) == 0


def oracle_answers(oracle, rate, bps, llr):
    """the oracle's whole decodeFixedFrame answer for every row, as the fields of the decode status, and the recovery step"""
    full = L._pool_map(lambda x: oracle.decode_fixed_frame_stage(x, rate, True, bps, flags=7), list(llr))
    return {"data": np.stack([f[0] for f in full]), "cw_ok": np.stack([f[1] for f in full]),
            "iterations": np.stack([f[2] for f in full]).astype(np.uint16), "attempts": np.stack([f[3] for f in full]).astype(np.uint8),
            "frame_valid": np.array([f[1].all() for f in full], np.uint8), "needs_recovery": np.zeros(len(llr), np.uint8),
            "stage": [f[4] for f in full]}


def mix(oracle, mod, rate, noise=False):
    """the recovery frames of one mode with clean frames (and, with noise, the mode's noise-shape sets, hopeless codewords
    included), and the oracle's whole answer for every frame"""
    key = (mod, rate, noise)
    if key not in _mix:
        llr, infos = L.recovery_mix(oracle, mod, rate)
        if noise:
            shapes = [s for s in L.ALL_FRAME_SETS if s[:2] == (mod, rate) and s[2] in L.NOISE_SHAPES]
            llr = np.concatenate([llr] + [L.frames(oracle, *s)[0] for s in shapes])
        _mix[key] = (llr, oracle_answers(oracle, rate, oracle.geom(getattr(po, mod), rate).bits_per_symbol, llr))
    return _mix[key]


def check_rows(out, s, exp, idx, what):
    bad = np.nonzero((out != exp["data"][idx]).any(1))[0]
    assert len(bad) == 0, f"{what}: bytes of rows {bad[:8]} (frames {idx[bad[:8]]}, recovery step {[exp['stage'][i] for i in idx[bad[:8]]]})"
    for k in STATUS_FIELDS:
        bad = np.nonzero((s[k] != exp[k][idx]).reshape(len(idx), -1).any(1))[0]
        assert len(bad) == 0, f"{what}: {k} of rows {bad[:8]} (frames {idx[bad[:8]]}, recovery step {[exp['stage'][i] for i in idx[bad[:8]]]})"


@pytest.mark.parametrize("mod,rate", L.ALL_FRAME_MODES)
def test_recovery_frames_in_batches_of_any_size(oracle, mod, rate):
    """n recovery frames of the mode (repaired by each step, wrongly repaired, unrepaired: tiled and shuffled) and the 8 clean
    frames shuffled among them, for n = 1, 63, 64, 65, 257 and 4100: the list of flagged frames holds less than a wave, a
    wave, just over one, just over a 256-thread block and over 4096 entries.  Every row equals the oracle's answer for that
    frame alone in every status field, and the counters the oracle's counts.  This is ria_gpu_decode_batch: one launch on
    stream slot 0 whatever the size (the parts of ria_gpu_rx_batch are test_split_rx_batch_repairs_transmitted_wrong_frames)."""
    from ria_amd import capi
    from ria_amd.engine import RxEngine
    llr, exp = mix(oracle, mod, rate)
    assert set(exp["stage"]) >= set(L.STAGES) | {"none", "failed"}, set(exp["stage"])
    flagged = np.array([i for i, s in enumerate(exp["stage"]) if s != "none"])
    clean = np.array([i for i, s in enumerate(exp["stage"]) if s == "none"])
    assert len(clean) == 8
    e = RxEngine(mod, RATE_NAME[rate], max_batch=max(BATCH_SIZES) + len(clean))
    rng = np.random.default_rng(5150 + int(rate))
    try:
        for n in BATCH_SIZES:
            idx = rng.permutation(np.concatenate([rng.permutation(np.resize(flagged, max(n, len(flagged))))[:n], clean]))
            out, st = e.decode(dev(llr[idx]), flags=capi.DECODE_FULL)
            cnt = e.recovery_counts(0)
            check_rows(out.cpu().numpy(), e.decode_status(st), exp, idx, f"{mod} {RATE_NAME[rate]} n={n}")
            assert cnt["flagged"] == n, (n, cnt)
            assert cnt["fallback"] == sum(exp["stage"][i] in (L.FILL, "failed") for i in idx), (n, cnt)
        assert e.lib.ria_gpu_debug_queue_fault(e.h) == 0
    finally:
        e.close()


@pytest.mark.parametrize("mod,rate", L.ALL_FRAME_MODES)
def test_split_rx_batch_repairs_transmitted_wrong_frames(oracle, mod, rate):
    """The parts of ria_gpu_rx_batch (stream slots 1.., recovery lists at an offset into the shared workspace) with frames a
    recovery step repairs.  Constructed soft bits cannot enter that call, so the frames are TRANSMITTED with wrong bytes
    (ldpc_domain_inputs.wrong_bytes) and received over a clean channel: the header flips, the single-bit and the CRC-field
    step repair theirs, the two-bit frames go on to the fallback stage and fail.  The pair, triple and quad searches and the
    fill never repair a frame here: they need weak soft bits, and run only on slot 0 (the tests above).  4104 frames, un-split
    and in 2, 3 (the default) and 4 parts: every row equals the oracle's answer on the soft bits the call itself returns,
    and every slot's counters equal the oracle's counts for its part."""
    import torch
    from ria_amd.engine import RxEngine
    n = 4104
    send, meant = L.wrong_bytes(oracle, mod, rate)
    rng = np.random.default_rng(6160 + int(rate))
    idx = rng.permutation(np.resize(np.arange(len(send)), n))
    e = RxEngine(mod, RATE_NAME[rate], max_batch=n)
    try:
        x = e.tx(dev(send[idx]), peak=0.8)
        e.set_split_parts(1)
        out, st, llr, _ = e.rx(x, want_llr=True)
        torch.cuda.synchronize()
        first = [int(np.nonzero(idx == k)[0][0]) for k in range(len(send))]
        rows = llr[dev(np.array(first))].cpu().numpy()
        exp = oracle_answers(oracle, rate, int(e.geo.bits_per_symbol), rows)
        # what the sample holds (tests/test_ldpc_domain_cpu.py pins the same counts on the oracle's own transmit chain)
        assert L.tx_counts(exp["stage"], exp["data"], meant) == L.TX_COUNTS[L.fill_key(mod, rate)], exp["stage"]
        check_rows(out.cpu().numpy(), e.decode_status(st), exp, idx, f"{mod} {RATE_NAME[rate]} un-split, soft bits returned")
        for parts in (1, 2, 0, 4):
            e.set_split_parts(parts)
            out, st = e.rx(x)
            torch.cuda.synchronize()
            what = f"{mod} {RATE_NAME[rate]} split_parts {parts}"
            check_rows(out.cpu().numpy(), e.decode_status(st), exp, idx, what)
            n_parts = parts or 3
            share = n if n_parts == 1 else ((n + n_parts - 1) // n_parts + 7) & ~7      # as ria_gpu_rx_batch cuts a batch
            for slot in range(n_parts):
                part = idx[slot * share:min((slot + 1) * share, n)]
                cnt = e.recovery_counts(slot)
                assert len(part) > 0 and cnt["flagged"] == sum(exp["stage"][q] != "none" for q in part) > 0, (what, slot, cnt)
                assert cnt["fallback"] == sum(exp["stage"][q] in (L.FILL, "failed") for q in part) > 0, (what, slot, cnt)
        assert e.lib.ria_gpu_debug_queue_fault(e.h) == 0
    finally:
        e.set_split_parts(0)
        e.close()


def exit_bounds(oracle, rate, bps, max_iter, llr, stages):
    """the repeated-state exits the retry kernels certainly (lo) and possibly (hi) make on these frames, counted with
    tools/count_state_repeats.py as tests/test_gpu_state_exit.py counts them"""
    oracle.decode_fixed_frame(llr[0], rate, True, bps, flags=7)
    csr.helper()
    lo = {"phase0": 0, "cascade": 0, "fill": 0}
    hi = {"phase0": 0, "cascade": 0, "fill": 0}
    recs = L._pool_map(lambda x: csr.walk(x, rate, bps, max_iter, every=True)[3], list(llr))
    for q in range(len(llr)):
        dec = csr.gpu_decodes(recs[q])
        for (kern, _, _), (r, certain) in dec.items():
            x = csr.exit_iteration(r, max_iter) is not None
            lo[kern] += int(x and certain); hi[kern] += int(x)
        if stages[q] != "none":                  # a flagged frame: the fill may re-decode what phase 0 has not
            for r in recs[q]:
                if r["stage"] == 1 and ("phase0", r["cw"], r["idx"]) not in dec:
                    hi["fill"] += int(csr.exit_iteration(r, max_iter) is not None)
    return lo, hi


@pytest.mark.parametrize("mod,rate", L.ALL_FRAME_MODES)
def test_options_do_not_change_a_row(oracle, mod, rate):
    """the recovery frames, clean frames and the noise-shape sets of the mode (hopeless codewords included): queueing every
    fallback re-decode or only the relevant ones, the repeated-state exit on and off - every output equals the oracle's, so
    all are identical.  Where the exit exists (R1/2, R1/3) its counters lie between the exits the oracle's decodes make
    certain and those they allow, as tests/test_gpu_state_exit.py bounds them; elsewhere they stay 0.  (RIA_OPT_SPLIT_PARTS
    acts in ria_gpu_rx_batch alone, which these soft bits cannot enter: see
    test_split_rx_batch_repairs_transmitted_wrong_frames, and tests/test_gpu_modes.py for noisy frames.)"""
    from ria_amd import capi
    from ria_amd.engine import RxEngine
    llr, exp = mix(oracle, mod, rate, noise=True)
    g = oracle.geom(getattr(po, mod), rate)
    lo, hi = exit_bounds(oracle, rate, g.bits_per_symbol, g.max_iter, llr, exp["stage"])
    idx = np.arange(len(llr))
    zero = {"all": 0, "phase0": 0, "cascade": 0, "fill": 0}
    e = RxEngine(mod, RATE_NAME[rate], max_batch=len(llr))
    x = dev(llr)
    try:
        for queue_all in (0, 1):
            for state_exit in (1, 0):
                e.set_fallback_queue_all(queue_all); e.set_state_exit(state_exit)
                out, st = e.decode(x, flags=capi.DECODE_FULL)
                c = e.state_exits(0)
                what = f"{mod} {RATE_NAME[rate]} queue_all {queue_all} state_exit {state_exit}"
                check_rows(out.cpu().numpy(), e.decode_status(st), exp, idx, what)
                print(f"{what}: exits {c}, certain {lo}, possible {hi}")
                if not state_exit or rate not in (po.R1_2, po.R1_3):
                    assert c == zero, (what, c)
                    continue
                assert c["all"] == c["phase0"] + c["cascade"] + c["fill"] and c["all"] > 0
                assert 0 < lo["cascade"] <= c["cascade"] <= hi["cascade"], (what, c, lo, hi)
                assert 0 < lo["phase0"] <= c["phase0"] <= hi["phase0"], (what, c, lo, hi)
                assert c["phase0"] + c["fill"] <= hi["phase0"] + hi["fill"], (what, c, hi)
        assert e.lib.ria_gpu_debug_queue_fault(e.h) == 0
    finally:
        e.close()
