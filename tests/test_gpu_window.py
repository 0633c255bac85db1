"""GPU tests (-m gpu) of ria_gpu_rx_window_batch: every field of every output of every pinned window
(tests/window_inputs.py) against the CPU restatement of StreamingDecoder's connected-mode window
(tests/window_restatement.py) on the oracle, bit for bit; batching and call-after-call behaviour; the control path against
ria_gpu_control_acquire_batch; a window without CFO feedback against ria_gpu_rx_acquire_batch and
ria_gpu_decode_frame_batch; argument checks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import control_restatement as CR
import decode_frame_restatement as DF
import window_inputs as WI
import window_restatement as WR
from ria_amd import capi
from ria_amd.acquire import WINDOW_COUNTERS, window_tally
from ria_amd.capi import RiaError
from test_gpu_parity import bits, dev, engine

pytestmark = pytest.mark.gpu

ACQ_FIELDS = ("detected", "accepted", "sync_start", "frame_start", "delta", "candidates", "burst_interleaved")


def control_engine():
    return engine("DQPSK", "R1_4")


def data_engine(link):
    return engine(*WI.LINK_NAMES[link])


def run(link, ws, kws, interleave=False, retry=True, engines=None):
    """one call on windows of one length -> numpy outputs; engines: (control, data) instead of the shared pair"""
    ce, de = engines or (control_engine(), data_engine(link))
    frames, res, acq, cres, st = de.rx_window(ce, dev(np.stack(ws)), WI.SEARCH_LEN,
                                              known_cfo=np.array([k["known_cfo"] for k in kws], np.float32),
                                              detect_threshold=np.array([k["detect_threshold"] for k in kws], np.float32),
                                              min_confidence=np.array([k["min_confidence"] for k in kws], np.float32),
                                              abs_base=np.array([k["abs_base"] for k in kws], np.uint64), interleave=interleave, retry=retry)
    return frames.cpu().numpy(), res, acq, cres, de.frame_status(st)


def same_bits(a, b):
    return bits(a) == bits(b) or (np.isnan(a) and np.isnan(b))


def check_row(tag, out, i, exp):
    """row i of a call's outputs against one restatement result"""
    frames, res, acq, cres, st = out
    for k in WR.WINDOW_FIELDS:
        assert int(res[k][i]) == int(exp[k]), (tag, k, int(res[k][i]), exp[k])
    for k in WR.WINDOW_WORDS:
        assert same_bits(np.float32(res[k][i]), np.float32(exp[k])), (tag, k, res[k][i], exp[k])
    f = exp["frame"]
    for k in DF.RESULT_FIELDS:
        assert int(res["frame"][k][i]) == int(f[k]), (tag, "frame." + k, int(res["frame"][k][i]), f[k])
    n = len(f["frame"])
    assert np.array_equal(frames[i][:n], f["frame"]) and not frames[i][n:].any(), tag
    for k in ACQ_FIELDS:
        assert int(acq[k][i]) == int(exp["acq"][k]), (tag, k, int(acq[k][i]), exp["acq"][k])
    assert bits(acq["correlation"][i]) == bits(exp["acq"]["correlation"]), tag
    assert same_bits(np.float32(acq["cfo_hz"][i]), np.float32(exp["acq"]["cfo_hz"])), (tag, acq["cfo_hz"][i], exp["acq"]["cfo_hz"])
    for k in CR.RESULT_FIELDS:
        assert int(cres[k][i]) == int(exp["control"][k]), (tag, "control." + k)
    if exp["status"] is None:
        assert not st[i:i + 1].view(np.uint8).any(), tag
        return
    for k in CR.STATUS_WORDS:
        a, b = np.float32(st[k][i]), exp["status"][k]
        if k == "snr_db":
            assert np.allclose(a, b, rtol=1e-5, atol=1e-5, equal_nan=True), (tag, k)
        else:
            assert same_bits(a, b), (tag, k, a, b)
    assert int(st["n_llr"][i]) == exp["status_n_llr"], tag


def batches(oracle):
    """the table's rows grouped into calls: one link, one window length, one set of call flags each"""
    groups = {}
    for r in WI.rows():
        w, kw = WI.window(oracle, r)
        groups.setdefault((r["link"], len(w), kw["interleave"], kw["retry"]), []).append((r, w, kw))
    return groups


@pytest.fixture(scope="module")
def table(oracle):
    """every batch run once on the GPU, with the restatement of its rows"""
    out = {}
    WI.expected_all(oracle)
    for key, items in batches(oracle).items():
        link, _, il, retry = key
        got = run(link, [w for _, w, _ in items], [kw for _, _, kw in items], il, retry)
        out[key] = (items, got, [WI.expected(oracle, r) for r, _, _ in items])
    return out


def test_the_table_reaches_every_statement(oracle):
    WI.assert_coverage(oracle)


def test_every_output_equals_the_restatement(table):
    for key, (items, got, exp) in table.items():
        for i, (r, _, _) in enumerate(items):
            check_row(r["name"], got, i, exp[i])
        tally = dict(zip(WINDOW_COUNTERS, window_tally(got[1], got[2])))
        assert sum(tally[f"outcome_{k.lower()}"] for k in capi.WIN_OUTCOME) == len(items)
        assert tally["success"] == sum(int(e["frame"]["success"]) for e in exp)


def test_order_and_batching_do_not_change_a_row(oracle, table):
    """the largest batch reversed, and split into two calls on the same handles (a smaller call after a larger one: the
    workspace is carved anew), give the same rows"""
    key = max(table, key=lambda k: len(table[k][0]))
    items, got, _ = table[key]
    link, _, il, retry = key
    ws, kws = [w for _, w, _ in items], [kw for _, _, kw in items]
    n = len(ws)
    rev = run(link, ws[::-1], kws[::-1], il, retry)
    a = run(link, ws[:n // 3], kws[:n // 3], il, retry)
    b = run(link, ws[n // 3:], kws[n // 3:], il, retry)
    for x, y, p, q in zip(got, rev, a, b):
        flat = lambda t: np.ascontiguousarray(t).view(np.uint8).reshape(len(t), -1)
        assert np.array_equal(flat(x), flat(y)[::-1])
        assert np.array_equal(flat(x), np.concatenate([flat(p), flat(q)]))


def test_workspace_growth_leaves_results_alone(oracle, table):
    """A call on 2 windows, then one on the whole largest batch (RIA_DECODE_FULL), on fresh control and data handles created
    for 2 frames: every array of the second equals the same call on another fresh pair that never ran the first, and the
    first equals that call's first two rows."""
    from ria_amd.engine import RxEngine
    key = max(table, key=lambda k: len(table[k][0]))
    items, got, _ = table[key]
    link, _, il, retry = key
    ws, kws = [w for _, w, _ in items], [kw for _, _, kw in items]
    fresh = lambda: (RxEngine("DQPSK", "R1_4", max_batch=2), RxEngine(*WI.LINK_NAMES[link], max_batch=2))
    a, b = fresh(), fresh()
    small = run(link, ws[:2], kws[:2], il, retry, engines=a)
    big = run(link, ws, kws, il, retry, engines=a)
    ref = run(link, ws, kws, il, retry, engines=b)
    assert len(ws) > 2 and (ref[1]["outcome"] == capi.WIN_OUTCOME["DECODED"]).sum() > 2     # decodeFrame ran on more than the first call's rows
    flat = lambda t: np.ascontiguousarray(t).view(np.uint8).reshape(len(t), -1)
    for k, (s, g, r, shared) in enumerate(zip(small, big, ref, got)):
        assert np.array_equal(flat(g), flat(r)) and np.array_equal(flat(r), flat(shared)), k
        assert np.array_equal(flat(s), flat(r)[:2]), k
    for e in a + b:
        e.close()


def test_control_rows_equal_control_acquire(oracle, table):
    seen = 0
    for (link, _, il, _), (items, got, exp) in table.items():
        ce, de = control_engine(), data_engine(link)
        ws, kws = [w for _, w, _ in items], [kw for _, _, kw in items]
        frames, res, acq, st = ce.control_acquire(dev(np.stack(ws)), WI.SEARCH_LEN, ce.control_frame_samples(de),
                                                  known_cfo=np.array([k["known_cfo"] for k in kws], np.float32),
                                                  detect_threshold=np.array([k["detect_threshold"] for k in kws], np.float32),
                                                  min_confidence=np.array([k["min_confidence"] for k in kws], np.float32),
                                                  abs_base=np.array([k["abs_base"] for k in kws], np.uint64), interleave=il)
        frames, st = frames.cpu().numpy(), ce.frame_status(st)
        assert np.array_equal(res.view(np.uint8), got[3].view(np.uint8))
        for i in np.nonzero(got[1]["outcome"] == capi.WIN_OUTCOME["CONTROL_PROFILE"])[0]:
            assert res["success"][i] == 1 and np.array_equal(frames[i], got[0][i][:20]) and not got[0][i][20:].any()
            assert st[i] == got[4][i] and acq[i] == got[2][i]
            seen += 1
    assert seen >= len(WI.LINKS)


def test_a_window_without_feedback_equals_rx_acquire_and_decode_frame(oracle, table):
    """peek CFO estimate == known CFO and pending 4: pass 2 is ria_gpu_rx_acquire_batch's primary candidate, its soft bits
    through ria_gpu_decode_frame_batch the result"""
    seen = 0
    for (link, wlen, il, _), (items, got, exp) in table.items():
        de = data_engine(link)
        _, res, acq, _, st = got
        pick = [i for i in range(len(items)) if res["outcome"][i] == capi.WIN_OUTCOME["DECODED"] and res["pending_total_cw"][i] == 4 and
                res["small_frame"][i] == 0 and acq["delta"][i] == 0 and bits(res["peek_cfo_hz"][i]) == bits(np.float32(items[i][2]["known_cfo"])) and
                not acq["burst_interleaved"][i]]
        if not pick or wlen < acq["sync_start"][pick].max() + de.geo.frame_samples:
            continue
        ws, kws = [items[i][1] for i in pick], [items[i][2] for i in pick]
        W = dev(np.stack(ws))
        known = np.array([k["known_cfo"] for k in kws], np.float32)
        base = np.array([k["abs_base"] for k in kws], np.uint64)
        _, _, acq1, fst1 = de.rx_acquire(W, WI.SEARCH_LEN, known_cfo=known, detect_threshold=np.array([k["detect_threshold"] for k in kws], np.float32),
                                         min_confidence=np.array([k["min_confidence"] for k in kws], np.float32), abs_base=base, retry=False,
                                         want_demod_status=True)
        fst1 = de.frame_status(fst1)
        starts = acq1["sync_start"].astype(np.uint64)
        llr, _ = de.demod(W.reshape(-1), cfo_hz=known, abs_pos=base + starts, offsets=np.arange(len(pick), dtype=np.uint64) * np.uint64(wlen) + starts)
        frames2, res2, _ = de.decode_frame(llr)
        frames2 = frames2.cpu().numpy()
        for j, i in enumerate(pick):
            assert acq1["accepted"][j] == 1 and acq1["sync_start"][j] == acq["sync_start"][i]
            assert fst1[j] == st[i], items[i][0]["name"]
            assert res2[j] == res["frame"][i] and np.array_equal(frames2[j], got[0][i][:frames2.shape[1]]), items[i][0]["name"]
            seen += 1
    assert seen >= 3


def test_zero_and_one_window(oracle, table):
    key = next(k for k in table if k[0] == "qam16_r12" and len(table[k][0]) > 3)
    items, got, exp = table[key]
    de = data_engine("qam16_r12")
    empty = de.rx_window(control_engine(), torch.zeros((0, key[1]), dtype=torch.float32, device="cuda"), WI.SEARCH_LEN)
    assert empty[0].shape[0] == 0 and len(empty[1]) == 0
    for i in (0, 1, len(items) - 1):
        one = run("qam16_r12", [items[i][1]], [items[i][2]], key[2], key[3])
        check_row(items[i][0]["name"] + "_alone", one, 0, exp[i])


def test_bad_handles_and_flags(oracle, table):
    key = next(k for k in table if k[0] == "qam16_r12")
    items = table[key][0]
    de, ce = data_engine("qam16_r12"), control_engine()
    W = dev(np.stack([items[0][1]]))
    with pytest.raises(RiaError):
        de.rx_window(de, W, WI.SEARCH_LEN)                               # the control handle is not DQPSK R1/4
    with pytest.raises(RiaError):
        de.rx_window(ce, W, WI.SEARCH_LEN, flags=capi.DECODE_FULL | capi.RX_DEMOD_ONLY)
    with pytest.raises(RiaError):
        de.rx_window(ce, W, WI.SEARCH_LEN, flags=capi.DECODE_FULL | capi.BURST_NO_CONTINUE)
    with pytest.raises(RiaError):
        de.rx_window(ce, W, W.shape[1] + 1)                              # search_len > window_len
    row = de.window_frame_row()
    out = [torch.zeros((1, k), dtype=torch.uint8, device="cuda") for k in (row - 1, 64, 32)]
    rc = de.lib.ria_gpu_rx_window_batch(ce.h, de.h, W.data_ptr(), W.shape[1], WI.SEARCH_LEN, W.shape[1], 1, de.acq_params(1).data_ptr(), 7,
                                        out[0].data_ptr(), row - 1, out[1].data_ptr(), out[2].data_ptr(), None, None, None)
    assert rc == -1                                                      # RIA_ERR_INVALID: the frame row is too short


def test_unsupported_by_the_one_wave_per_frame_kernel():
    """under RIA_DEMOD_FUSED=1 (read once per process: a fresh child) the call returns RIA_ERR_UNSUPPORTED (-4)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "helpers", "window_fused_child.py")], env=dict(os.environ, RIA_DEMOD_FUSED="1"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "status -4"
