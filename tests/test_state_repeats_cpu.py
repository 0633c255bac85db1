"""CPU tests of tools/count_state_repeats.py: its restated decoder (tools/state_repeats_helper.c, the message vector of
every iteration kept) against the oracle's ro_ldpc_decode, its cascade walk against ro_decode_fixed_frame, and the rule
that turns a decode's first repeat into the iteration at which the copy schedule of fast_decode ends it."""
import os
import sys
import threading

import numpy as np
import pytest

import pyoracle as po

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import count_state_repeats as csr  # noqa: E402

SEED = 20261004
FRAMES = list(range(24))


def _threads(work, n, nt=8):
    th = [threading.Thread(target=work, args=(k * n // nt, (k + 1) * n // nt)) for k in range(nt)]
    [t.start() for t in th]; [t.join() for t in th]


@pytest.fixture(scope="module")
def llrs(oracle):
    csr.helper()
    return {rate: [csr.frame_llr(oracle, po.QAM16, rate, i, SEED, 2, 20.0) for i in FRAMES] for rate in (po.R1_2, po.R1_3)}


@pytest.mark.parametrize("rate", [po.R1_2, po.R1_3])
def test_restated_decoder_equals_ro_ldpc_decode(oracle, llrs, rate):
    """96 codewords of the bench stream at each of the five min-sum factors (480 rows, converging and failing), and at a
    shorter iteration limit: success, iteration count and bytes"""
    table = oracle.gather_table(188, True)
    mi = oracle.geom(po.QAM16, rate).max_iter
    rows = [llr[table[cw * 648:(cw + 1) * 648]] for llr in llrs[rate] for cw in range(4)]
    oracle.code(rate)
    n_ok = n_fail = n_rep = 0
    for f in csr.clf.FACTORS:
        for limit in (mi, 7):
            for v in rows:
                ok, by, it, rep_t, rep_p = csr.decode(rate, v, limit, f)
                ok_o, by_o, it_o = oracle.ldpc_decode(rate, v, limit, f)
                assert (ok, it) == (ok_o, it_o) and np.array_equal(by, by_o)
                n_ok += int(ok); n_fail += int(not ok)
                if rep_t >= 0:
                    n_rep += 1
                    assert not ok and 1 <= rep_p < rep_t < limit and rep_t - rep_p >= 1
    assert n_ok >= 100 and n_fail >= 100 and n_rep >= 10, (n_ok, n_fail, n_rep)


@pytest.mark.parametrize("rate", [po.R1_2, po.R1_3])
def test_cascade_walk_equals_ro_decode_fixed_frame(oracle, llrs, rate):
    """per codeword: success, iterations and attempts of decodeFixedFrame with phase 0 and the perturbation cascade; the
    walk that also runs the decodes the reference skips reports the same and marks the same decodes as needed"""
    mi = oracle.geom(po.QAM16, rate).max_iter
    exp, got, gote = [None] * len(FRAMES), [None] * len(FRAMES), [None] * len(FRAMES)
    oracle.decode_fixed_frame(llrs[rate][0], rate, True, 188, flags=3)

    def work(lo, hi):
        for q in range(lo, hi):
            exp[q] = oracle.decode_fixed_frame(llrs[rate][q], rate, True, 188, flags=3)
            got[q] = csr.walk(llrs[rate][q], rate, 188, mi)
            gote[q] = csr.walk(llrs[rate][q], rate, 188, mi, every=True)
    _threads(work, len(FRAMES))
    n_casc = 0
    for q in range(len(FRAMES)):
        _, ok, it, att = exp[q]
        for g in (got[q], gote[q]):
            assert np.array_equal(g[0], ok) and np.array_equal(g[1], it) and np.array_equal(g[2], att), f"frame {FRAMES[q]}"
        key = lambda r: (r["cw"], r["stage"], r["idx"])   # noqa: E731
        needed = {key(r): r for r in gote[q][3] if r["needed"]}
        assert needed == {key(r): r for r in got[q][3] if r["needed"]}
        # the needed decodes account for the reference's attempt counts: the first decode, the factors, the cascade attempts
        for cw in range(4):
            n = sum(1 for k in needed if k[0] == cw)
            assert n == att[cw], f"frame {FRAMES[q]} cw {cw}"
        n_casc += sum(1 for r in got[q][3] if r["stage"] == 2)
    assert n_casc >= 100, n_casc


def test_exit_iteration_rule():
    """state(t) == state(t - p) first at t: pre-period mu = t - p; the comparison at c sees it iff c - 24 >= mu and p | 24"""
    r = lambda t, p, ok=0: {"ok": ok, "rep_t": t, "rep_p": p}   # noqa: E731
    assert csr.exit_iteration(r(30, 8), 80) == 46            # mu = 22: the first copy is already on the cycle
    assert csr.exit_iteration(r(31, 8), 80) == 70            # mu = 23: only the second copy is
    assert csr.exit_iteration(r(46, 24), 80) == 46
    assert csr.exit_iteration(r(60, 12), 80) is None         # mu = 48 > 46: no later comparison below 80
    assert csr.exit_iteration(r(60, 48), 80) is None         # the period does not divide the stride
    assert csr.exit_iteration(r(-1, -1), 80) is None
    assert csr.exit_iteration(r(30, 8), 50) == 46 and csr.exit_iteration(r(30, 8), 46) is None
    assert csr.exit_iteration(r(10, 4, ok=1), 80) is None
