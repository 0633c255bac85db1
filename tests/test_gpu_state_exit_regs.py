"""GPU tests (-m gpu) of the register form of the repeated-state exit: the copy of a decode's state
lives in an area of global memory that its persistent workgroup owns, one set of areas per stream slot.  What the existing
tests/test_gpu_state_exit.py does not reach: the handle's default, a batch large enough to be cut into parts (three slots and
three sets of areas live at once), and calls on different frames following each other on one handle (an area still holds the
copy of an earlier call's decode when the next one starts).  Everything through the C ABI, against the CPU oracle."""
import numpy as np
import pytest

import pyoracle as po
import test_gpu_state_exit as tse
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

csr = tse.csr
DEFAULT_ON = True                       # the default of RIA_OPT_STATE_EXIT in a fresh handle
OTHER_FRAMES = list(range(100, 184))    # a second set of 84 frames of the same stream
ZERO = {"all": 0, "phase0": 0, "cascade": 0, "fill": 0}


@pytest.fixture(scope="module")
def sample_a(oracle):
    """frames tse.FRAMES with the tool's bounds on the exit counters"""
    return tse._sample(oracle, po.R1_2)


@pytest.fixture(scope="module")
def sample_b(oracle):
    """frames OTHER_FRAMES: samples and the oracle's full decode"""
    g = oracle.geom(po.QAM16, po.R1_2)
    y = [csr.clf.frame_sample(oracle, po.QAM16, po.R1_2, i, tse.SEED, 2, 20.0) for i in OTHER_FRAMES]
    full = [None] * len(y)
    oracle.decode_fixed_frame(oracle.rx_process(po.QAM16, po.R1_2, y[0])[0], po.R1_2, True, g.bits_per_symbol, flags=7)

    def work(lo, hi):
        for q in range(lo, hi):
            llr = oracle.rx_process(po.QAM16, po.R1_2, y[q])[0]
            full[q] = oracle.decode_fixed_frame(llr, po.R1_2, True, g.bits_per_symbol, flags=7)
    tse._threads(work, len(y))
    exp_st = {"cw_ok": np.stack([f[1] for f in full]), "iterations": np.stack([f[2] for f in full]).astype(np.uint16),
              "attempts": np.stack([f[3] for f in full]).astype(np.uint8),
              "frame_valid": np.array([int(bool(f[1].all()) and csr.clf.verify(oracle, f[0], g.bytes_per_cw)) for f in full], np.uint8),
              "needs_recovery": np.zeros(len(y), np.uint8)}
    return {"y": np.stack(y), "exp_d": np.stack([f[0] for f in full]), "exp_st": exp_st}


def test_default_handle(sample_a, monkeypatch):
    """a fresh handle with no option set: outputs equal the oracle's; the exit counters are within the tool's bounds if the
    exit is on by default and zero if it is off"""
    import torch
    from ria_amd.engine import RxEngine
    monkeypatch.delenv("RIA_STATE_EXIT", raising=False)
    e = RxEngine("QAM16", "R1_2", max_batch=len(tse.FRAMES))
    out, st = e.rx(dev(sample_a["y"]))
    torch.cuda.synchronize()
    c = e.state_exits(0)
    tse._check(out.cpu().numpy(), e.decode_status(st), sample_a, "default handle")
    if DEFAULT_ON:
        tse._check_counts(c, sample_a, "default handle")
    else:
        assert c == ZERO, c
    assert e.lib.ria_gpu_debug_queue_fault(e.h) == 0
    e.close()


def test_split_parts_on_equals_off():
    """4 096 faded bench-stream frames, the smallest batch ria_gpu_rx_batch cuts into parts: three stream slots decode at
    once, each with its own areas.  Exit on and off: every payload byte and every byte of the status records identical, no
    queue fault, and every slot used has ended decodes"""
    import torch
    from ria_amd.engine import RxEngine
    n, first, seed = 4096, 25000 * 3 + 77, 20261004
    e = RxEngine("QAM16", "R1_2", max_batch=n)
    x = e.tx(e.make_frames(seed, first, n), peak=0.8)
    e.channel_exact_(x, 2, 20.0, seed, first_frame=first)
    res = {}
    for on in (0, 1):
        e.set_state_exit(on)
        out, st = e.rx(x)
        torch.cuda.synchronize()
        res[on] = (out.cpu().numpy(), st.cpu().numpy(), [e.state_exits(slot) for slot in range(4)])
    assert np.array_equal(res[0][0], res[1][0]), np.nonzero((res[0][0] != res[1][0]).any(axis=1))[0][:8]
    assert np.array_equal(res[0][1], res[1][1]), np.nonzero((res[0][1] != res[1][1]).any(axis=1))[0][:8]
    s = res[1][1].view(RxEngine.DECODE_STATUS).reshape(-1)
    assert (s["attempts"] > 5).any() and (s["attempts"] == 1).any() and s["frame_valid"].any()
    assert e.lib.ria_gpu_debug_queue_fault(e.h) == 0
    print("exits per slot, on:", res[1][2])
    assert all(c == ZERO for c in res[0][2]), res[0][2]
    for slot in range(3):                      # the default split is three parts
        c = res[1][2][slot]
        assert c["all"] > 0 and c["all"] == c["phase0"] + c["cascade"] + c["fill"], (slot, c)
    e.close()


def test_no_leak_between_calls(sample_a, sample_b):
    """one handle, exit on: frames A, then 84 other frames, then A again.  The areas hold the copies of the call before when a
    call starts; each call's outputs equal the oracle's for its own frames"""
    import torch
    from ria_amd.engine import RxEngine
    e = RxEngine("QAM16", "R1_2", max_batch=len(tse.FRAMES))
    e.set_state_exit(1)
    ya, yb = dev(sample_a["y"]), dev(sample_b["y"])
    for what, y, sm in (("first set", ya, sample_a), ("other set", yb, sample_b), ("first set again", ya, sample_a)):
        out, st = e.rx(y)
        torch.cuda.synchronize()
        c = e.state_exits(0)
        tse._check(out.cpu().numpy(), e.decode_status(st), sm, what)
        if sm is sample_a:
            tse._check_counts(c, sm, what)
        else:
            assert c["all"] > 0, c
    assert e.lib.ria_gpu_debug_queue_fault(e.h) == 0
    e.close()
