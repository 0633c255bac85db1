"""GPU tests (-m gpu) of the 16-byte accesses of the retry decoders: the copy of a decode's state
that the repeated-state exit compares with is stored and loaded four words per lane at a time ([quad][lane][4] in the
workgroup's area), and the seeded mt19937 states of a cascade attempt group are kept attempt-major and written four words per
store.  Neither changes a result: everything here goes through the C ABI and is compared with the CPU oracle, on frames of the
bench stream (QAM16, Watterson moderate, 20 dB, the bench seed; frame idx as tools/count_lazy_factors.py draws it) that were
chosen with the oracle and tools/count_state_repeats.py alone, on the CPU, over the first 3 000 frames of the stream."""
from unittest import mock

import numpy as np
import pytest

import pyoracle as po
import test_gpu_cascade_groups as tcg
import test_gpu_state_exit as tse
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

csr = tse.csr
# 48 frames disjoint from tse.FRAMES: 200..243 and the next four of the stream that hold a decode converging after
# iteration 46 (a comparison that finds no repeat, then the second store, then success)
SECOND_SAMPLE = list(range(200, 244)) + [1292, 1363, 2175, 2447]
# cascade winners of these frames at R1/2 (attempt numbers of the oracle's decodeFixedFrame): 322: 32; 2509: 33, 31 and a
# codeword that fails all 34; 2816: 33 and one that fails; 285: 0; 319: 1, 2; 210: 2, 23; 6: 3 and one that fails; 224: 9;
# 2144: 7; 383: 5; 526: 27; 122: 31, 8 and one that fails.  Attempt 33 does occur in the first 3 000 frames (2509, 2816).
GROUP_FRAMES = [322, 2509, 2816, 285, 319, 210, 6, 224, 2144, 383, 526, 122]
# each holds a codeword that fails all 34 attempts (92: one and no winner; 2816: one, and a winner at attempt 33)
HOPELESS_FRAMES = [92, 2816]


def _second_sample(oracle, rate):
    assert not set(SECOND_SAMPLE) & set(tse.FRAMES) and len(SECOND_SAMPLE) == 48
    with mock.patch.object(tse, "FRAMES", SECOND_SAMPLE):
        return tse._sample(oracle, rate)


@pytest.fixture(scope="module")
def second_r12(oracle):
    return _second_sample(oracle, po.R1_2)


@pytest.fixture(scope="module")
def stream_frames(oracle):
    """samples and the oracle's full decode of GROUP_FRAMES + HOPELESS_FRAMES at R1/2, keyed by frame idx"""
    g = oracle.geom(po.QAM16, po.R1_2)
    idx = sorted(set(GROUP_FRAMES + HOPELESS_FRAMES))
    y = [csr.clf.frame_sample(oracle, po.QAM16, po.R1_2, i, tse.SEED, 2, 20.0) for i in idx]
    full = [None] * len(idx)
    oracle.decode_fixed_frame(oracle.rx_process(po.QAM16, po.R1_2, y[0])[0], po.R1_2, True, g.bits_per_symbol, flags=7)

    def work(lo, hi):
        for q in range(lo, hi):
            full[q] = oracle.decode_fixed_frame(oracle.rx_process(po.QAM16, po.R1_2, y[q])[0], po.R1_2, True, g.bits_per_symbol, flags=7)
    tse._threads(work, len(idx))
    return {i: {"y": y[q], "data": full[q][0], "ok": full[q][1], "iters": full[q][2].astype(np.uint16), "att": full[q][3].astype(np.uint8)}
            for q, i in enumerate(idx)}


def _pick(stream_frames, idx):
    return np.stack([stream_frames[i]["y"] for i in idx]), {k: np.stack([stream_frames[i][k] for i in idx]) for k in ("data", "ok", "iters", "att")}


def test_second_sample_holds_every_kind(second_r12):
    """from the oracle and the tool alone, among the decodes the kernels certainly run"""
    kinds = [csr.kinds(r, second_r12["max_iter"]) for r in second_r12["recs"]]
    n = lambda k: sum(k in s for s in kinds)   # noqa: E731
    assert n("exit at 46") >= 1 and n("exit at 70") >= 1 and n("period 48") >= 1 and n("converges after 46") >= 1, \
        {k: n(k) for k in ("exit at 46", "exit at 70", "period 48", "converges after 46")}
    assert second_r12["lo"]["cascade"] >= 1 and second_r12["lo"]["phase0"] >= 1, second_r12["lo"]


def test_second_sample_r12_on_off_on(second_r12):
    """ria_gpu_decode_batch (flags 7) and ria_gpu_rx_batch, exit on, off and on again: every byte and status field equals the
    oracle's, the counters are within the tool's certain and possible bounds when on and zero when off"""
    tse._on_off("R1_2", second_r12)


def test_second_sample_r13_on_off_on(oracle):
    """the same frame indices at R1/3, the other shape with the exit"""
    tse._on_off("R1_3", _second_sample(oracle, po.R1_3))


def test_winners_in_every_position_of_a_group(stream_frames):
    """cascade winners at attempt mod 4 = 0, 1, 2 and 3, in the last, partial group (attempts 32 and 33) and codewords that
    fail all 34 attempts: bytes, success, `attempts` and `iterations` equal the oracle's"""
    y, exp = _pick(stream_frames, GROUP_FRAMES)
    w, n_fail = tcg.winners(exp)
    assert {int(a) % 4 for a in w} == {0, 1, 2, 3}, sorted(w)
    assert (w == 32).any() and (w == 33).any(), sorted(w)
    assert n_fail >= 1
    e = tcg.engine("QAM16", "R1_2")
    out, st = e.rx(dev(y))
    tcg.assert_same(out.cpu().numpy(), e.decode_status(st), exp, "winners")
    assert e.lib.ria_gpu_debug_queue_fault(e.h) == 0


def test_one_frame_calls(stream_frames):
    """a call of one frame with a hopeless codeword has fewer units than the persistent grid has workgroups (most of them find
    the queue empty); two such calls on one handle, on different frames, with the exit on"""
    import torch
    from ria_amd.engine import RxEngine
    e = RxEngine("QAM16", "R1_2", max_batch=1)
    e.set_state_exit(1)
    for i in HOPELESS_FRAMES:
        y, exp = _pick(stream_frames, [i])
        assert tcg.winners(exp)[1] >= 1, f"frame {i} holds no codeword that fails all 34 attempts"
        out, st = e.rx(dev(y))
        torch.cuda.synchronize()
        tcg.assert_same(out.cpu().numpy(), e.decode_status(st), exp, f"frame {i} alone")
    assert e.lib.ria_gpu_debug_queue_fault(e.h) == 0
    e.close()
