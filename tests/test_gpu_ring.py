"""GPU tests of ria_gpu_search_ring_batch: against ria_gpu_search_batch on every row of tests/search_inputs.py (captures that
never wrap: the same result and state), and against the ring restatement (tests/ring_restatement.py, a literal 960 000-float
ring) on every row of tests/ring_inputs.py and on one 2.9 M-sample stream of three laps.  Every field of the result and of
the state is compared for equality, floats as bit patterns (NaN = NaN); there is no tolerance.  What the rows reach on the
restatement is asserted in tests/test_ring_cpu.py.  Without the entry point every test here fails at symbol lookup."""
import ctypes as C

import numpy as np
import pytest
import torch

import ring_inputs as RI
import ring_restatement as RR
import search_inputs as SI
import search_restatement as SR
from mcdpsk_acquire_restatement import oracle

pytestmark = pytest.mark.gpu
MODE = {RR.LTS: "OFDM_LTS", RR.ZC: "MCDPSK_ZC", RR.CHIRP: "MCDPSK_CHIRP"}
RING = RR.MAX_BUFFER_SAMPLES


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
    return torch.from_numpy(x).to(eng.device)


def mc_modulation(mode):
    return "DQPSK" if mode == RR.ZC else "DBPSK"


def run_ring(engines, rows, max_inv=None, chunk=0):
    """ring rows of one mode / modulation / connected flag / feed_step in one call -> (result, state)"""
    O = oracle()
    r0 = rows[0]
    assert len({(r["mode"], r["modulation"], r["connected"], r["feed_step"]) for r in rows}) == 1
    eng = engines(r0["modulation"])
    args = [RI.row_args(O, r) for r in rows]
    x = stack(eng, [a[0] for a in args])
    lens = np.array([a[1] for a in args], np.int32)
    st = np.array([a[2] for a in args], RR.STATE)
    eng.set_search_chunk(chunk)
    try:
        return eng.search_ring(x, lens, st, MODE[r0["mode"]], feed_step=r0["feed_step"], max_invocations=max_inv or r0["max_inv"], connected=r0["connected"],
                               carriers=10, modulation=mc_modulation(r0["mode"]))
    finally:
        eng.set_search_chunk(0)


def ring_groups(mode):
    g = {}
    for r in RI.ROWS:
        if r["mode"] == mode:
            g.setdefault((r["modulation"], r["connected"], r["max_inv"], r["feed_step"]), []).append(r)
    return list(g.values())


def test_record_layouts():
    from ria_amd.engine import RxEngine
    from ria_amd import capi
    assert RxEngine.RING_STATE == RR.STATE and RxEngine.RING_SEARCH_RESULT == RR.RESULT
    assert C.sizeof(capi.RingState) == 48 == RR.STATE.itemsize and C.sizeof(capi.RingSearchResult) == 144 == RR.RESULT.itemsize
    assert RR.RESULT.names[:len(SR.RESULT.names)] == SR.RESULT.names
    assert all(RR.RESULT.fields[f][1] == SR.RESULT.fields[f][1] for f in SR.RESULT.names)         # ria_search_result's layout first
    assert capi.RING_SAMPLES == RING and capi.RING_MAX_CAPTURE == 2 ** 31 - 1 - RING


@pytest.mark.parametrize("feed_step", SI.FEED_STEPS)
def test_search_table_equals_search_batch(engines, feed_step):
    """captures of at most 959 999 samples: the old call's result fields and (mapped) state, and nothing of the ring happens"""
    O = oracle()
    g = {}
    for r in SI.ROWS:
        g.setdefault((r["mode"], r["modulation"], r["connected"], r["max_inv"]), []).append(r)
    for rows in g.values():
        r0 = rows[0]
        eng = engines(r0["modulation"])
        args = [SI.row_args(O, r, feed_step) for r in rows]
        x = stack(eng, [a[0] for a in args])
        lens = np.array([a[1] for a in args], np.int32)
        st = np.array([a[2] for a in args], SR.STATE)
        kw = dict(feed_step=feed_step, max_invocations=r0["max_inv"], connected=r0["connected"], carriers=10, modulation=mc_modulation(r0["mode"]))
        old_res, old_st = eng.search(x, lens, st, MODE[r0["mode"]], **kw)
        res, out = eng.search_ring(x, lens, RR.from_search_state(st), MODE[r0["mode"]], **kw)
        names = [r["name"] for r in rows]
        assert not same(res[list(SR.RESULT.names)], old_res), (names, same(res[list(SR.RESULT.names)], old_res))
        assert not same(RR.to_search_state(out), old_st), (names, same(RR.to_search_state(out), old_st))
        assert (res["abs_search_start"] == res["search_start"]).all()
        for f in ("span_wraps", "overflows", "overflow_dropped", "drift_snaps", "cursor_inits"):
            assert not res[f].any(), f
        assert not out["overflow_events"].any() and not out["overflow_dropped"].any()


@pytest.mark.parametrize("mode", [RR.LTS, RR.ZC, RR.CHIRP])
def test_ring_table_equals_restatement(engines, mode):
    O = oracle()
    for rows in ring_groups(mode):
        res, st = run_ring(engines, rows)
        for i, r in enumerate(rows):
            e_res, e_st = RI.expected(O, r)
            assert not same(res[i], e_res), (r["name"], same(res[i], e_res))
            assert not same(st[i], e_st), (r["name"], same(st[i], e_st))


def test_batch_independence(engines):
    """the same rows reversed, split into two calls, one stream per call, and chunks of 1 and 2; the batch is ragged and mixes
    streams before the wrap (short captures of tests/search_inputs.py) with streams behind it"""
    O = oracle()
    eng = engines("DQPSK")
    ring_rows = [r for r in RI.ROWS if r["mode"] == RR.LTS and r["feed_step"] == 0 and r["modulation"] == "DQPSK"]
    short_rows = [r for r in SI.ROWS if r["name"] in ("lts_clean", "lts_replay", "lts_noisy_weak")]
    caps, lens, states = [], [], []
    for r in ring_rows:
        x, n, st, _, _ = RI.row_args(O, r)
        caps.append(x), lens.append(n), states.append(st)
    for r in short_rows:
        x, n, st, _, _ = SI.row_args(O, r, 0)
        caps.append(x), lens.append(n), states.append(RR.from_search_state(st)[0])
    order = [0, len(caps) - 1] + list(range(1, len(caps) - 1))                  # a short capture between the long ones
    caps, lens, states = [caps[i] for i in order], np.array([lens[i] for i in order], np.int32), np.array([states[i] for i in order], RR.STATE)
    xd = stack(eng, caps)
    assert len(set(lens.tolist())) > 3 and (states["total_fed"] < RING).sum() >= 3 and (states["total_fed"] > RING).sum() >= 3

    def run(idx, chunk=0):
        idx = list(idx)
        eng.set_search_chunk(chunk)
        try:
            return eng.search_ring(xd[idx].contiguous(), lens[idx], states[idx], "OFDM_LTS", max_invocations=12)
        finally:
            eng.set_search_chunk(0)
    n = len(caps)
    res, st = run(range(n))
    assert (res["detector_runs"] > 0).sum() >= 6 and (res["outcome"] == RR.SYNC_FOUND).sum() >= 4
    rres, rst = run(range(n - 1, -1, -1))
    assert not same(rres[::-1], res) and not same(rst[::-1], st)
    a, b = run(range(n // 2)), run(range(n // 2, n))
    assert not same(np.concatenate([a[0], b[0]]), res) and not same(np.concatenate([a[1], b[1]]), st)
    for chunk in (1, 2):
        cres, cst = run(range(n), chunk=chunk)
        assert not same(cres, res) and not same(cst, st), chunk
    for i in range(n):
        one = run([i])
        assert not same(one[0], res[i:i + 1]) and not same(one[1], st[i:i + 1]), i


def test_limit_continues_across_the_wrap(engines):
    """cuts before, at and behind the wrap equal one call"""
    O = oracle()
    row = next(r for r in RI.ROWS if r["name"] == "lts_cross_feed")
    eng = engines(row["modulation"])
    x, n, st, _, _ = RI.row_args(O, row)
    xd = stack(eng, [x])
    kw = dict(feed_step=row["feed_step"])
    whole, st_whole = eng.search_ring(xd, n, np.array([st]), "OFDM_LTS", max_invocations=row["max_inv"], **kw)
    assert whole["outcome"][0] == RR.SYNC_FOUND and st_whole["total_fed"][0] > RING > st["total_fed"]
    for k in (1, 2, int(whole["invocations"][0]) // 2):
        a, st_a = eng.search_ring(xd, n, np.array([st]), "OFDM_LTS", max_invocations=k, **kw)
        assert a["outcome"][0] == RR.LIMIT and a["invocations"][0] == k
        b, st_b = eng.search_ring(xd, n, st_a, "OFDM_LTS", max_invocations=row["max_inv"] - k, **kw)
        assert not same(st_b, st_whole), k
        assert b["outcome"][0] == whole["outcome"][0] and int(a["invocations"][0]) + int(b["invocations"][0]) == int(whole["invocations"][0])
        keep = ["search_start", "abs_search_start", "sync_position", "abs_position", "correlation", "sync_cfo_hz", "sync_snr_db", "span_wraps"]
        assert not same(b[keep], whole[keep]), k


def test_three_laps(engines):
    """one stream of 2.9 M samples, fed 4800 at a time, a frame in each lap: every sync, as the caller's loop sees it (a found
    sync becomes the last decoded position, so the next call steps over it as a replay), equals the restatement"""
    O = oracle()
    eng = engines("DQPSK")
    frame = SI._ofdm_frame(O, 1)
    n = 2900000
    x = np.zeros(n, np.float32)
    at = (500000, 1500000, 2400000)
    for a in at:
        x[a:a + len(frame)] = frame
    xd = torch.from_numpy(x[None, :]).to(eng.device)
    st_g = RR.fresh_state(1)
    st_g["snr_hint"] = 20.0
    st_c = st_g[0].copy()
    found = []
    for leg in range(8):
        res, st_g = eng.search_ring(xd, n, st_g, "OFDM_LTS", feed_step=4800, max_invocations=1000)
        e_res, st_c = RR.search(O, x, n, st_c, RR.LTS, RR.DIFFERENTIAL, False, 4800, 1000)
        assert not same(res[0], e_res), (leg, same(res[0], e_res))
        assert not same(st_g[0], st_c), (leg, same(st_g[0], st_c))
        if res["outcome"][0] != RR.SYNC_FOUND:
            break
        found.append(int(res["abs_position"][0]))
        st_g["last_decoded_sync_pos"] = res["sync_position"]
        st_c["last_decoded_sync_pos"] = e_res["sync_position"]
    assert res["outcome"][0] == RR.NEED_SAMPLES and st_g["total_fed"][0] == n
    assert len(found) == 3 and all(0 <= a - f < 200 for a, f in zip(at, found)), found


def test_zero_streams(engines):
    eng = engines("DQPSK")
    res, st = eng.search_ring(torch.zeros((0, 1000), dtype=torch.float32, device=eng.device), 0, np.zeros(0, RR.STATE), "OFDM_LTS")
    assert len(res) == 0 and len(st) == 0


def test_bad_arguments(engines):
    """each bound of the domain"""
    from ria_amd import capi
    eng = engines("DQPSK")
    x = torch.zeros((1, 1000), dtype=torch.float32, device=eng.device)
    st = RR.fresh_state(1)
    assert eng.lib.ria_gpu_search_ring_batch(None, 0, 0, None, None, 0, None, 1, None, 0, 1, None, None) == -1      # RIA_ERR_INVALID
    eng.search_ring(x, 1000, st, "OFDM_LTS", max_invocations=2)                                                        # the valid call
    for bad_kw in (dict(mode=7), dict(max_invocations=0), dict(feed_step=-1), dict(capture_len=1001), dict(capture_len=-1), dict(mode="MCDPSK_ZC", carriers=0)):
        kw = dict(capture_len=1000, mode="OFDM_LTS", max_invocations=2)
        kw.update(bad_kw)
        with pytest.raises(capi.RiaError):
            eng.search_ring(x, kw.pop("capture_len"), st, kw.pop("mode"), **kw)
    for field, value in (("total_fed", 1001), ("total_fed", -1), ("correlation_pos", -1), ("correlation_pos", RING), ("reject_streak", -1),
                         ("last_decoded_sync_pos", RING), ("last_decoded_sync_pos", -1), ("last_decoded_sync_pos", -2 ** 31 + 1)):
        bad = RR.fresh_state(1)
        bad[field] = value
        with pytest.raises(capi.RiaError):
            eng.search_ring(x, 1000, bad, "OFDM_LTS", max_invocations=2)
    for field, value in (("total_fed", 1000), ("correlation_pos", RING - 1), ("last_decoded_sync_pos", RING - 1), ("last_decoded_sync_pos", 0)):
        ok = RR.fresh_state(1)
        ok[field] = value
        eng.search_ring(x, 1000, ok, "OFDM_LTS", max_invocations=2)
    # capture_len above 2^31 - 1 - 960000: the stride is only claimed, no sample is read before the check
    lens = torch.tensor([capi.RING_MAX_CAPTURE + 1], dtype=torch.int32, device=eng.device)
    st_d = torch.from_numpy(st.view(np.uint8).reshape(1, 48).copy()).to(eng.device)
    res_d = torch.full((1, 144), 0xAB, dtype=torch.uint8, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = eng.lib.ria_gpu_search_ring_batch(eng.h, 0, 0, None, p(x), 2 ** 31 - 1, p(lens), 1, p(st_d), 0, 2, p(res_d), None)
    torch.cuda.synchronize()
    assert rc == -1 and bool((res_d == 0xAB).all())


def test_invalid_call_writes_nothing(engines):
    """one stream outside the domain fails the whole call before any state or result is written"""
    eng = engines("DQPSK")
    n = SI.LTS_MIN + 9600
    x = torch.zeros((2, n), dtype=torch.float32, device=eng.device)
    lens = torch.full((2,), n, dtype=torch.int32, device=eng.device)
    st = RR.fresh_state(2, total_fed=n)
    st["total_fed"][1] = n + 1
    st_d = torch.from_numpy(st.view(np.uint8).reshape(2, 48).copy()).to(eng.device)
    res_d = torch.full((2, 144), 0xAB, dtype=torch.uint8, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = eng.lib.ria_gpu_search_ring_batch(eng.h, 0, 0, None, p(x), n, p(lens), 2, p(st_d), 0, 10, p(res_d), None)
    torch.cuda.synchronize()
    assert rc == -1
    assert np.array_equal(st_d.cpu().numpy().reshape(-1), st.view(np.uint8)) and bool((res_d == 0xAB).all())
    st["total_fed"][1] = n                                         # the same call, valid: the silent stream walks to its end
    res, out = eng.search_ring(x, n, st, "OFDM_LTS", max_invocations=10)
    assert (res["outcome"] == RR.NEED_SAMPLES).all() and (out["correlation_pos"] > 0).all()
