"""GPU tests of ria_gpu_search_batch against the CPU restatement of searchForSync (tests/search_restatement.py) on every row
of tests/search_inputs.py, in the three modes, with feed_step 0 and 4800.  Every field of the result and of the state is
compared bit for bit (floats as bit patterns, NaN = NaN).  What the rows reach on the restatement is asserted in
tests/test_search_cpu.py.  Without the entry point every test here fails at symbol lookup."""
import ctypes as C

import numpy as np
import pytest
import torch

import search_inputs as SI
import search_restatement as SR
from mcdpsk_acquire_restatement import oracle

pytestmark = pytest.mark.gpu
MODE = {SR.LTS: "OFDM_LTS", SR.ZC: "MCDPSK_ZC", SR.CHIRP: "MCDPSK_CHIRP"}


@pytest.fixture(scope="module")
def engines():
    from ria_amd.engine import RxEngine
    made = {}

    def get(modulation):
        if modulation not in made:
            made[modulation] = RxEngine(modulation, "R1_4", max_batch=8)
        return made[modulation]
    yield get
    for e in made.values():
        e.close()


def same(a, b):
    """two structured records or arrays: every field equal, floats by bit pattern, NaN = NaN"""
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    assert a.dtype.names == b.dtype.names and a.shape == b.shape
    bad = []
    for f in a.dtype.names:
        x, y = a[f], b[f]
        if x.dtype.kind == "f":
            ok = (x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))
        else:
            ok = x == y
        if not np.all(ok):
            bad.append((f, x[~ok.reshape(x.shape)][:4].tolist(), y[~ok.reshape(x.shape)][:4].tolist()))
    return bad


def stack(eng, caps):
    stride = max(len(c) for c in caps)
    x = np.zeros((len(caps), stride), np.float32)
    for i, c in enumerate(caps):
        x[i, :len(c)] = c
    return torch.from_numpy(x).to(eng.device), np.array([len(c) for c in caps], np.int32)


def run_rows(engines, rows, feed_step, max_inv=None, chunk=0):
    """rows of one mode / modulation / connected flag in one call -> (result, state)"""
    O = oracle()
    r0 = rows[0]
    eng = engines(r0["modulation"])
    args = [SI.row_args(O, r, feed_step) for r in rows]
    x, lens = stack(eng, [a[0] for a in args])
    st = np.array([a[2] for a in args], SR.STATE)
    eng.set_search_chunk(chunk)
    try:
        return eng.search(x, lens, st, MODE[r0["mode"]], feed_step=feed_step, max_invocations=max_inv or r0["max_inv"], connected=r0["connected"],
                          carriers=10, modulation="DQPSK" if r0["mode"] == SR.ZC else "DBPSK")
    finally:
        eng.set_search_chunk(0)


def groups():
    g = {}
    for r in SI.ROWS:
        g.setdefault((r["mode"], r["modulation"], r["connected"], r["max_inv"]), []).append(r)
    return list(g.values())


def test_record_layouts():
    from ria_amd.engine import RxEngine
    from ria_amd import capi
    assert RxEngine.SEARCH_STATE == SR.STATE and RxEngine.SEARCH_RESULT == SR.RESULT
    assert C.sizeof(capi.SearchState) == 32 == SR.STATE.itemsize and C.sizeof(capi.SearchResult) == 112 == SR.RESULT.itemsize
    assert capi.SEARCH_MIN_SEARCH == {m: SR.min_search_of(m) for m in (SR.LTS, SR.ZC, SR.CHIRP)}


@pytest.mark.parametrize("feed_step", SI.FEED_STEPS)
def test_table_equals_restatement(engines, feed_step):
    O = oracle()
    for rows in groups():
        res, st = run_rows(engines, rows, feed_step)
        for i, r in enumerate(rows):
            e_res, e_st = SI.expected(O, r, feed_step)
            assert not same(res[i], e_res), (r["name"], feed_step, same(res[i], e_res))
            assert not same(st[i], e_st), (r["name"], feed_step, same(st[i], e_st))


@pytest.mark.parametrize("mode", [SR.LTS, SR.ZC, SR.CHIRP])
def test_batch_independence(engines, mode):
    """the same rows reversed, split into two calls, and one stream per call; a chunked gather"""
    rows = [r for r in SI.ROWS if r["mode"] == mode and r["modulation"] == "DQPSK" and not r["connected"]]
    for fs in SI.FEED_STEPS:
        res, st = run_rows(engines, rows, fs, max_inv=12)
        assert (res["detector_runs"] > 0).sum() >= 3
        rres, rst = run_rows(engines, rows[::-1], fs, max_inv=12)
        assert not same(rres[::-1], res) and not same(rst[::-1], st)
        h = len(rows) // 2
        a, b = run_rows(engines, rows[:h], fs, max_inv=12), run_rows(engines, rows[h:], fs, max_inv=12)
        assert not same(np.concatenate([a[0], b[0]]), res) and not same(np.concatenate([a[1], b[1]]), st)
        cres, cst = run_rows(engines, rows, fs, max_inv=12, chunk=2)         # three or more listed streams: two chunks and more
        assert not same(cres, res) and not same(cst, st)
        for i, r in enumerate(rows):                                         # one stream per call, every row
            one = run_rows(engines, [r], fs, max_inv=12)
            assert not same(one[0], res[i:i + 1]) and not same(one[1], st[i:i + 1]), (r["name"], fs)


def test_search_tally(engines):
    from ria_amd.acquire import SEARCH_COUNTERS, search_tally
    rows = [r for r in SI.ROWS if r["mode"] == SR.LTS and r["modulation"] == "DQPSK" and r["max_inv"] == 40]
    res, _ = run_rows(engines, rows, 0)
    t = dict(zip(SEARCH_COUNTERS, search_tally(res)))
    O = oracle()
    want = [SI.expected(O, r, 0)[0] for r in rows]
    assert t["outcome_sync_found"] == sum(int(e["outcome"] == SR.SYNC_FOUND) for e in want) > 0
    assert t["outcome_need_samples"] + t["outcome_limit"] + t["outcome_sync_found"] == len(rows)
    for k in SEARCH_COUNTERS[3:]:
        assert t[k] == sum(int(e[k]) for e in want), k
    assert t["rejects"] > 0 and t["weak_accepts"] > 0 and t["detector_runs"] > t["outcome_sync_found"]


def test_limit_continues(engines):
    O = oracle()
    for name in ("lts_noisy_diff", "zc_weak", "lts_replay"):
        row = next(r for r in SI.ROWS if r["name"] == name)
        eng = engines(row["modulation"])
        for fs in SI.FEED_STEPS:
            x, n, st, _, conn = SI.row_args(O, row, fs)
            xd, lens = stack(eng, [x])
            kw = dict(feed_step=fs, connected=conn, modulation="DQPSK" if row["mode"] == SR.ZC else "DBPSK")
            whole, st_whole = eng.search(xd, lens, np.array([st]), MODE[row["mode"]], max_invocations=row["max_inv"], **kw)
            k = max(1, int(whole["invocations"][0]) // 2)
            a, st_a = eng.search(xd, lens, np.array([st]), MODE[row["mode"]], max_invocations=k, **kw)
            assert a["outcome"][0] == SR.LIMIT and a["invocations"][0] == k
            b, st_b = eng.search(xd, lens, st_a, MODE[row["mode"]], max_invocations=row["max_inv"] - k, **kw)
            assert not same(st_b, st_whole), (name, fs)
            assert b["outcome"][0] == whole["outcome"][0] and int(a["invocations"][0]) + int(b["invocations"][0]) == int(whole["invocations"][0])
            keep = ["search_start", "sync_position", "correlation", "sync_cfo_hz", "sync_snr_db", "min_confidence", "detect_threshold"]
            assert not same(b[keep], whole[keep]), (name, fs)


def test_zero_streams(engines):
    eng = engines("DQPSK")
    res, st = eng.search(torch.zeros((0, 1000), dtype=torch.float32, device=eng.device), 0, np.zeros(0, SR.STATE), "OFDM_LTS")
    assert len(res) == 0 and len(st) == 0


def test_list_scan_crosses_its_tile(engines):
    """1030 streams, two before index 1024 and two behind it pass the gate, the rest are silence"""
    O = oracle()
    eng = engines("DQPSK")
    names = {3: "zc_clean", 1000: "zc_clean_cfo", 1025: "zc_clean_cfo_far", 1029: "zc_clean"}
    rows = {i: next(r for r in SI.ROWS if r["name"] == n) for i, n in names.items()}
    n, stride, silent_len = 1030, 48000, SI.ZC_MIN + 4800
    x = torch.zeros((n, stride), dtype=torch.float32, device=eng.device)
    lens = np.full(n, silent_len, np.int32)
    st = SR.fresh_state(n, fed=silent_len)
    for i, r in rows.items():
        c, ln, s, _, _ = SI.row_args(O, r, 0)
        x[i, :ln] = torch.from_numpy(c).to(eng.device)
        lens[i], st[i] = ln, s
    res, out = eng.search(x, lens, st, "MCDPSK_ZC", max_invocations=64, modulation="DQPSK")
    quiet, quiet_st = SR.search(O, np.zeros(silent_len, np.float32), silent_len, SR.fresh_state(1, fed=silent_len)[0], SR.ZC, SR.ZC_MODE, False, 0, 64)
    assert quiet["outcome"] == SR.NEED_SAMPLES and quiet["detector_runs"] == 0
    for i in range(n):
        if i in rows:
            e_res, e_st = SI.expected(O, rows[i], 0)
            assert rows[i]["max_inv"] == 64 and e_res["detector_runs"] > 0
        else:
            e_res, e_st = quiet, quiet_st
        assert not same(res[i], e_res) and not same(out[i], e_st), i


def test_window_calls_repeat_the_detection(engines):
    """search_start, search_len, known_cfo_hz, detect_threshold and min(min_confidence, correlation) of a SYNC_FOUND row, given
    to the window calls on the window at search_start, reproduce sync_start = sync_position - search_start and the correlation"""
    from ria_amd.engine import RxEngine
    O = oracle()
    eng = engines("DQPSK")
    for name, kind in (("lts_clean", "lts"), ("lts_noisy_weak", "lts"), ("zc_clean", "zc"), ("zc_weak_streak", "zc"), ("chirp_clean", "chirp")):
        row = next(r for r in SI.ROWS if r["name"] == name)
        x, n, st, _, conn = SI.row_args(O, row, 0)
        xd, lens = stack(eng, [x])
        res, _ = eng.search(xd, lens, np.array([st]), MODE[row["mode"]], max_invocations=row["max_inv"], connected=conn,
                            modulation="DQPSK" if kind == "zc" else "DBPSK")
        r = res[0]
        assert r["outcome"] == SR.SYNC_FOUND, name
        ss, sl = int(r["search_start"]), int(r["search_len"])
        w = torch.from_numpy(np.ascontiguousarray(x[ss:])[None, :]).to(eng.device)
        conf = min(float(r["min_confidence"]), float(r["correlation"]))
        if kind == "lts":
            ctrl = RxEngine("DQPSK", "R1_4", max_batch=2)
            acq = eng.rx_window(ctrl, w, sl, known_cfo=float(r["known_cfo_hz"]), detect_threshold=float(r["detect_threshold"]), min_confidence=conf)[2]
            ctrl.close()
        else:
            acq = eng.mcdpsk_window(w, sl, carriers=10, modulation="DQPSK" if kind == "zc" else "DBPSK", sync=kind, disconnected=(kind == "chirp"),
                                    known_cfo=float(r["known_cfo_hz"]), detect_threshold=float(r["detect_threshold"]), min_confidence=conf)[2]
        assert acq["detected"][0] == 1 and int(acq["sync_start"][0]) == int(r["sync_position"]) - ss, name
        assert acq["correlation"][0].view(np.uint32) == r["correlation"].view(np.uint32), name


def test_bad_arguments(engines):
    from ria_amd import capi
    eng = engines("DQPSK")
    lib = eng.lib
    x = torch.zeros((1, 1000), dtype=torch.float32, device=eng.device)
    st = SR.fresh_state(1)
    assert lib.ria_gpu_search_batch(None, 0, 0, None, None, 0, None, 1, None, 0, 1, None, None) == -1      # RIA_ERR_INVALID
    with pytest.raises(capi.RiaError):
        eng.search(x, 1000, st, 7)
    with pytest.raises(capi.RiaError):
        eng.search(x, 1000, st, "OFDM_LTS", max_invocations=0)
    with pytest.raises(capi.RiaError):
        eng.search(x, 1001, st, "OFDM_LTS")                        # longer than the stride
    with pytest.raises(capi.RiaError):
        eng.search(x, -1, st, "OFDM_LTS")
    big = torch.zeros((1, 960000), dtype=torch.float32, device=eng.device)
    with pytest.raises(capi.RiaError):
        eng.search(big, 960000, st, "OFDM_LTS")                    # the ring would wrap
    res, _ = eng.search(big, 959999, SR.fresh_state(1, fed=959999), "OFDM_LTS")
    assert res["outcome"][0] == SR.NEED_SAMPLES and res["rms_skips"][0] > 100
    bad = SR.fresh_state(1, fed=2000)
    with pytest.raises(capi.RiaError):
        eng.search(x, 1000, bad, "OFDM_LTS")                       # fed beyond the capture
    with pytest.raises(capi.RiaError):
        eng.search(x, 1000, st, "MCDPSK_ZC", carriers=0)           # a bad MC-DPSK configuration


def test_invalid_call_writes_nothing(engines):
    """one stream outside the domain fails the whole call before any state or result is written"""
    eng = engines("DQPSK")
    n = SI.LTS_MIN + 9600
    x = torch.zeros((2, n), dtype=torch.float32, device=eng.device)
    lens = torch.full((2,), n, dtype=torch.int32, device=eng.device)
    st = SR.fresh_state(2, fed=n)
    st["fed"][1] = n + 1
    st_d = torch.from_numpy(st.view(np.uint8).reshape(2, 32).copy()).to(eng.device)
    res_d = torch.full((2, 112), 0xAB, dtype=torch.uint8, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = eng.lib.ria_gpu_search_batch(eng.h, 0, 0, None, p(x), n, p(lens), 2, p(st_d), 0, 10, p(res_d), None)
    torch.cuda.synchronize()
    assert rc == -1
    assert np.array_equal(st_d.cpu().numpy().reshape(-1), st.view(np.uint8)) and bool((res_d == 0xAB).all())
    st["fed"][1] = n                                               # the same call, valid: the silent stream walks to its end
    res, out = eng.search(x, n, st, "OFDM_LTS", max_invocations=10)
    assert (res["outcome"] == SR.NEED_SAMPLES).all() and (out["correlation_pos"] > 0).all()
