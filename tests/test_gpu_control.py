"""GPU tests (-m gpu) of the control hypothesis: ria_gpu_rx_control_batch on pre-synced spans and
ria_gpu_control_acquire_batch on capture windows, every field of every output against the CPU restatement of
StreamingDecoder's control-first path (tests/control_restatement.py) on the oracle and against what the compiled reference
recorded for the same spans (tests/golden/control_frames.npz); and the chain rx_acquire_control_first on mixed ACK / data
traffic, which rx_acquire alone does not deliver."""
import numpy as np
import pytest
import torch

import pyoracle as po
import control_inputs as CI
import control_restatement as R
from acquire_restatement import window as data_window
from ria_amd.acquire import rx_acquire_control_first
from ria_amd.capi import RiaError
from test_gpu_parity import bits, dev, engine

pytestmark = pytest.mark.gpu

ACQ_FIELDS = ("detected", "accepted", "sync_start", "frame_start", "delta", "candidates", "burst_interleaved")
MIN_CONF = 0.5


def zero_meta(n):
    """CFO 0 at position 0 as the reference computes it (correction phase -0.0; a call without meta starts at +0.0)"""
    return dict(cfo_hz=np.zeros(n, np.float32), abs_pos=np.zeros(n, np.uint64), flags=np.zeros(n, np.uint32))


def control_engine():
    return engine("DQPSK", "R1_4")


def check_result(tag, res, frames, st, i, exp):
    """row i of a call's outputs against one restatement result"""
    for k in R.RESULT_FIELDS:
        assert int(res[k][i]) == int(exp[k]), (tag, k, int(res[k][i]), exp[k])
    assert not res["reserved0"][i].any() and not res["reserved"][i].any(), tag
    assert np.array_equal(frames[i], exp["frame"]), tag
    if exp["status"] is None:
        assert not st[i:i + 1].view(np.uint8).any(), tag
        return
    for k in R.STATUS_WORDS:
        a, b = np.float32(st[k][i]), exp["status"][k]
        if k == "snr_db":
            assert np.allclose(a, b, rtol=1e-5, atol=1e-5, equal_nan=True), (tag, k)
        else:
            assert bits(a) == bits(b) or (np.isnan(a) and np.isnan(b)), (tag, k, a, b)
    assert int(st["n_llr"][i]) == exp["n_llr"], tag


@pytest.fixture(scope="module")
def spans(oracle):
    """the pinned spans and their restatement, computed once"""
    xs = [CI.span(oracle, row) for row in CI.SPANS]
    exp = [R.control_hypothesis(oracle, x, row[7], row[8], row[9]) for x, row in zip(xs, CI.SPANS)]
    return xs, exp


def test_rx_control_equals_the_restatement_and_the_recorded_reference(oracle, spans, golden):
    e = control_engine()
    xs, exp = spans
    g = golden("control_frames")
    for n in sorted({len(x) for x in xs}):
        idx = [i for i, x in enumerate(xs) if len(x) == n]
        rows = [CI.SPANS[i] for i in idx]
        frames, res, st = e.rx_control(dev(np.stack([xs[i] for i in idx])), cfo_hz=np.array([r[7] for r in rows], np.float32),
                                       abs_pos=np.array([r[8] for r in rows], np.uint64), flags=np.array([r[9] for r in rows], np.uint32))
        frames, st = frames.cpu().numpy(), e.frame_status(st)
        for j, i in enumerate(idx):
            check_result(CI.SPANS[i][0], res, frames, st, j, exp[i])
            assert [int(res[k][j]) for k in R.RESULT_FIELDS] == list(g["outcome"][i]), CI.SPANS[i][0]
            assert np.array_equal(frames[j], g["frames"][i]), CI.SPANS[i][0]
            assert np.array_equal(bits(np.array([st[k][j] for k in R.STATUS_WORDS[1:]])), g["status"][i][1:]), CI.SPANS[i][0]


def test_rx_control_offsets_batching_and_handle_check(oracle, spans):
    e = control_engine()
    xs, exp = spans
    idx = [i for i, x in enumerate(xs) if len(x) == CI.CTRL_SAMPLES and CI.SPANS[i][7] == 0.0]
    cap = np.concatenate([np.zeros(5, np.float32)] + [xs[i] for i in idx])
    offs = np.array([5 + k * CI.CTRL_SAMPLES for k in range(len(idx))], np.uint64)[::-1]
    frames, res, st = e.rx_control(dev(cap), n_samples=CI.CTRL_SAMPLES, offsets=offs, **zero_meta(len(idx)))
    frames, st = frames.cpu().numpy(), e.frame_status(st)
    for j, i in enumerate(idx[::-1]):
        check_result(CI.SPANS[i][0], res, frames, st, j, exp[i])
    # a smaller batch after a larger one, and a larger one again: the workspace is carved per call
    one = e.rx_control(dev(xs[idx[0]][None]), **zero_meta(1))
    check_result("single", one[1], one[0].cpu().numpy(), e.frame_status(one[2]), 0, exp[idx[0]])
    with pytest.raises(RiaError):
        engine("QAM16", "R1_2").rx_control(dev(xs[idx[0]][None]))
    with pytest.raises(RiaError):
        e.rx_control(torch.zeros((1, 2 * 1152), dtype=torch.float32, device="cuda"))


@pytest.fixture(scope="module")
def windows(oracle):
    """the pinned windows, each with its min_confidence (the offset rows take it from the window's own correlation)"""
    ws = [CI.window(oracle, row) for row in CI.WINDOWS]
    conf = []
    for w, row in zip(ws, CI.WINDOWS):
        if row[8] is None:
            conf.append(np.float32(MIN_CONF))
        else:
            det = oracle.detect_data_sync(w[:CI.SEARCH_LEN], 0.0, 0.15)
            assert det[0]
            conf.append(np.float32(np.float32(det[2]) + np.float32(row[8])))
    return ws, conf


def check_window(tag, e, out, i, exp, acq_exp):
    frames, res, acq, st = out
    check_result(tag, res, frames, st, i, exp)
    for k in ACQ_FIELDS:
        assert int(acq[k][i]) == int(acq_exp[k]), (tag, k, int(acq[k][i]), acq_exp[k])
    assert bits(acq["correlation"][i]) == bits(acq_exp["correlation"]), tag
    assert bits(acq["cfo_hz"][i]) == bits(acq_exp["cfo_hz"]), tag
    assert int(acq["reserved"][i]) == 0, tag


def run_windows(e, ws, conf, n_samples, interleave=False, abs_base=None, known_cfo=None):
    frames, res, acq, st = e.control_acquire(dev(np.stack(ws)), CI.SEARCH_LEN, n_samples, known_cfo=known_cfo, min_confidence=np.array(conf, np.float32),
                                             abs_base=abs_base, interleave=interleave)
    return frames.cpu().numpy(), res, acq, e.frame_status(st)


@pytest.mark.parametrize("n_samples,interleave", [(CI.CTRL_SAMPLES, False), (CI.CTRL_SAMPLES, True), (15 * R.SYM, False)],
                         ids=["span_10368", "span_10368_interleave", "span_17280_dbpsk_link"])
def test_control_acquire_equals_the_restatement(oracle, windows, n_samples, interleave):
    """every field of every output, window by window; windows of one length go into one call.  17 280 is the span of a
    DBPSK data link (ria_gpu_control_frame_samples)"""
    e = control_engine()
    if n_samples != CI.CTRL_SAMPLES:
        assert n_samples == e.control_frame_samples(engine("DBPSK", "R1_2")) == R.control_frame_samples(po.DBPSK, po.R1_2)
    else:
        assert n_samples == e.control_frame_samples(engine("QAM16", "R1_2")) == e.control_frame_samples(e)
    ws, conf = windows
    seen = dict(tried=0, not_accepted=0, skipped_marked=0, success=0)
    for wlen in sorted({len(w) for w in ws}):
        idx = [i for i, w in enumerate(ws) if len(w) == wlen]
        base = np.array([1000 * i + 7 for i in idx], np.uint64)
        # the long-span case also hands every other window a known CFO, so that the position enters the correction phase
        known = np.array([0.0 if n_samples == CI.CTRL_SAMPLES or i % 2 else 1.25 for i in idx], np.float32)
        out = run_windows(e, [ws[i] for i in idx], [conf[i] for i in idx], n_samples, interleave, abs_base=base, known_cfo=known)
        for j, i in enumerate(idx):
            exp, acq_exp = R.control_acquire_window(oracle, po.QAM16, po.R1_2, ws[i], CI.SEARCH_LEN, n_samples, float(known[j]), 0.15, conf[i], int(base[j]), interleave)
            check_window(CI.WINDOWS[i][0], e, out, j, exp, acq_exp)
            seen["tried"] += exp["tried"]; seen["success"] += exp["success"]
            seen["not_accepted"] += 1 - acq_exp["accepted"]
            seen["skipped_marked"] += int(acq_exp["accepted"] and not exp["tried"])
    if n_samples == CI.CTRL_SAMPLES:      # the set holds what it is meant to hold
        assert seen["not_accepted"] == 3 and seen["skipped_marked"] == (1 if interleave else 0) and seen["success"] == (4 if interleave else 5)


def test_control_acquire_fit_and_confidence_edges(oracle, windows):
    """the span that ends on the window's last sample is tried, one sample less is not; min_confidence just below the
    correlation accepts, just above rejects"""
    ws, conf = windows
    name = [r[0] for r in CI.WINDOWS]
    r = {n: R.control_acquire_window(oracle, po.QAM16, po.R1_2, ws[name.index(n)], CI.SEARCH_LEN, CI.CTRL_SAMPLES, 0.0, 0.15, conf[name.index(n)])
         for n in ("ack_fits", "ack_fits_not", "ack_conf_below", "ack_conf_above")}
    assert r["ack_fits"][1]["sync_start"] + CI.CTRL_SAMPLES == len(ws[name.index("ack_fits")]) and r["ack_fits"][0]["success"] == 1
    assert r["ack_fits_not"][1]["detected"] == 1 and r["ack_fits_not"][1]["accepted"] == 0 and r["ack_fits_not"][0]["tried"] == 0
    assert r["ack_conf_below"][0]["success"] == 1 and r["ack_conf_above"][1]["accepted"] == 0 and r["ack_conf_above"][1]["detected"] == 1


def test_control_acquire_across_the_scan_tile_and_call_after_call(oracle, windows):
    """1030 windows tiled from the distinct full-length ones cross the plan kernel's 1024-window tile; the same handle then
    takes a smaller batch and the large one again, with identical results"""
    e = control_engine()
    ws, conf = windows
    idx = [i for i, w in enumerate(ws) if len(w) == CI.WINDOW_LEN]
    exp = [R.control_acquire_window(oracle, po.QAM16, po.R1_2, ws[i], CI.SEARCH_LEN, CI.CTRL_SAMPLES, 0.0, 0.15, conf[i]) for i in idx]
    tile = [idx[k % len(idx)] for k in range(1030)]
    big = run_windows(e, [ws[i] for i in tile], [conf[i] for i in tile], CI.CTRL_SAMPLES)
    for k in range(1030):
        check_window(f"tile{k}", e, big, k, *exp[k % len(idx)])
    small = run_windows(e, [ws[i] for i in idx[:3]], [conf[i] for i in idx[:3]], CI.CTRL_SAMPLES)
    for k in range(3):
        check_window(f"small{k}", e, small, k, *exp[k])
    again = run_windows(e, [ws[i] for i in tile], [conf[i] for i in tile], CI.CTRL_SAMPLES)
    for a, b in zip(big, again):
        assert np.array_equal(a.view(np.uint8) if a.dtype.names else a, b.view(np.uint8) if b.dtype.names else b)


def test_workspace_growth_leaves_results_alone(windows):
    """A call on 2 windows, then one on every full-length window, on a fresh handle created for 2 frames: every array of the
    second equals the same call on another fresh handle that never ran the first, and the first equals that call's first
    two rows."""
    from ria_amd.engine import RxEngine
    ws, conf = windows
    idx = [i for i, w in enumerate(ws) if len(w) == CI.WINDOW_LEN]
    ws, conf = [ws[i] for i in idx], [conf[i] for i in idx]
    a, b = RxEngine("DQPSK", "R1_4", max_batch=2), RxEngine("DQPSK", "R1_4", max_batch=2)
    small = run_windows(a, ws[:2], conf[:2], CI.CTRL_SAMPLES)
    big = run_windows(a, ws, conf, CI.CTRL_SAMPLES)
    ref = run_windows(b, ws, conf, CI.CTRL_SAMPLES)
    assert len(ws) > 2 and ref[1]["tried"].any()                             # the demodulator and the decoder ran
    for k, (s, g, r) in enumerate(zip(small, big, ref)):
        assert g.tobytes() == r.tobytes(), k
        assert s.tobytes() == r[:2].tobytes(), k
    a.close()
    b.close()


def test_control_acquire_rejects_bad_arguments(windows):
    e = control_engine()
    w = dev(np.stack([windows[0][0]]))
    with pytest.raises(RiaError):
        e.control_acquire(w, CI.SEARCH_LEN, 2 * 1152)
    with pytest.raises(RiaError):
        e.control_acquire(w, CI.WINDOW_LEN + 1, CI.CTRL_SAMPLES)
    with pytest.raises(RiaError):
        engine("QAM16", "R1_2").control_acquire(w, CI.SEARCH_LEN, CI.CTRL_SAMPLES)


CHAIN_WINDOW, CHAIN_SEARCH = 33000, 14000


def test_control_first_chain_on_mixed_traffic(oracle):
    """32 windows alternate ACK / NACK frames and QAM16 R1/2 data frames.  Control first, then the data call: window by window
    the restatement's result.  The same windows through rx_acquire alone deliver no ACK: the behaviour this call adds."""
    ce, de = control_engine(), engine("QAM16", "R1_2")
    n_samples = ce.control_frame_samples(de)
    ws, sent_ctl, sent_data = [], {}, {}
    for k in range(32):
        lead = 500 + 311 * k
        if k % 2 == 0:
            row = (f"chain{k}", "ack" if k % 4 == 0 else "nack", 100 + k, lead, CHAIN_WINDOW, CI.AWGN if k % 8 else CI.MODERATE, 20.0 if k % 8 else 12.0, 900 + k, None, 0)
            ws.append(CI.window(oracle, row))
            sent_ctl[k] = CI.frame_bytes(row[1], row[2])
        else:
            rng = np.random.default_rng(900 + k)
            w, info = data_window(oracle, po.QAM16, po.R1_2, rng.integers(0, 256, 141, dtype=np.uint8), 100 + k, lead, CHAIN_WINDOW, 0, 20.0, 900 + k)
            ws.append(w)
            sent_data[k] = info
    W = dev(np.stack(ws))
    frames, res, acq, info, st, dacq = rx_acquire_control_first(ce, de, W, CHAIN_SEARCH, n_samples)
    frames, info, st = frames.cpu().numpy(), info.cpu().numpy(), de.decode_status(st)
    for k in range(32):
        r, a, d = R.rx_acquire_control_first(oracle, po.QAM16, po.R1_2, ws[k], CHAIN_SEARCH, n_samples, min_confidence=0.78)
        for f in R.RESULT_FIELDS:
            assert int(res[f][k]) == int(r[f]), (k, f)
        assert np.array_equal(frames[k], r["frame"]), k
        for f in ACQ_FIELDS:
            assert int(acq[f][k]) == int(a[f]), (k, f)
        if k % 2 == 0:
            assert r["success"] == 1 and d is None and np.array_equal(frames[k], sent_ctl[k]), k
            # the data call sees the window, detects the frame and does not accept it: nothing is demodulated or decoded
            assert dacq["detected"][k] == 1 and dacq["accepted"][k] == 0 and dacq["candidates"][k] == 0 and not info[k].any(), k
        else:
            assert r["success"] == 0 and d is not None, k
            for f in ACQ_FIELDS:
                assert int(dacq[f][k]) == int(d[f]), (k, f)
            assert np.array_equal(info[k], d["info"]) and np.array_equal(st["cw_ok"][k], d["cw_ok"]), k
            assert st["frame_valid"][k] == 0 or np.array_equal(info[k], sent_data[k]), k
    data = np.arange(1, 32, 2)
    assert st["frame_valid"][data].sum() >= 8       # AWGN at 20 dB: the data frames arrive, bar what the detector's start costs
    # today's call alone: every data frame, no ACK
    info1, st1, acq1 = de.rx_acquire(W, CHAIN_SEARCH)
    st1 = de.decode_status(st1)
    info1 = info1.cpu().numpy()
    for k in range(32):
        if k % 2 == 0:
            assert st1["frame_valid"][k] == 0 and not st1["cw_ok"][k].all(), k
        else:        # the data windows come out of the chain exactly as out of the data call alone
            assert np.array_equal(info1[k], info[k]) and st1[k] == st[k], k
            for f in acq1.dtype.names:
                assert acq1[f][k] == dacq[f][k] or f in ("correlation", "cfo_hz") and bits(acq1[f][k]) == bits(dacq[f][k]), (k, f)
