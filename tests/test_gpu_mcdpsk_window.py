"""GPU tests of ria_gpu_mcdpsk_window_batch against the CPU restatement (tests/mcdpsk_window_restatement.py) on the oracle, on
every row of tests/mcdpsk_window_inputs.py.  Every comparison is bit-exact: every field of the window result, of the acquire
row with the two channel-interleaving bits, and of the harq row, the frame bytes and the soft bits; floats are compared as bit
patterns, NaN = NaN.  What every row does on the restatement is asserted in tests/test_mcdpsk_window_cpu.py, which also pins the
restatement to the compiled reference.  Without the entry point every test here fails at symbol lookup."""
import ctypes as C

import numpy as np
import pytest
import torch

import pyoracle as po
import mcdpsk_window_inputs as WI
import mcdpsk_window_restatement as MW
from mcdpsk_acquire_restatement import oracle
from mcdpsk_harq_restatement import ChaseCache, cache_snapshot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from ria_amd.engine import RxEngine
    e = RxEngine("DQPSK", "R1_4", max_batch=64)
    yield e
    e.close()


@pytest.fixture(scope="module")
def expected():
    return WI.expected_all(oracle())


def dev(eng, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(eng.device)


def same_float(a, b):
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32) or (np.isnan(a) and np.isnan(b))


def run(eng, call, x, kw, pool=None, ids=None, **more):
    cfg = call["cfg"]
    a = dict(carriers=cfg["carriers"], modulation=cfg["bps"], spreading=cfg["spreading"], sync="chirp" if cfg["chirp"] else "zc",
             disconnected=cfg["disconnected"], retry=cfg["retry"], channel_interleave=cfg["B"] is not None, interleaver_bits=cfg["B"],
             min_confidence=0.0, want_llr=True, chase=pool, cache_id=ids if ids is not None else (-1 if pool is None else None),
             now_ms=call["now"], pending_total_cw=kw["pending_total_cw"], first_avail=kw["first_avail"],
             last_decoded_sync=kw["last_decoded_sync"])
    a.update(more)
    frames, res, acq, hq, llr = eng.mcdpsk_window(dev(eng, x), call["search_len"], **a)
    return frames.cpu().numpy(), res, acq, hq, llr.cpu().numpy()


def check_row(tag, i, got, e, cache_id=None):
    frames, res, acq, hq, llr = got
    for f in MW.RESULT_FIELDS:
        assert int(res[f][i]) == int(e[f]), (tag, f, res[f][i], e[f])
    for f in MW.RESULT_WORDS:
        assert same_float(res[f][i], e[f]), (tag, f, res[f][i], e[f])
    assert int(res["reserved0"][i]) == 0 and not res["reserved"][i].any(), tag
    a = e["acq"]
    for f in MW.ACQ_FIELDS:
        assert int(acq[f][i]) == int(a[f]), (tag, f, acq[f][i], a[f])
    for f in MW.ACQ_WORDS:
        assert same_float(acq[f][i], a[f]), (tag, f, acq[f][i], a[f])
    assert acq["reserved"][i].tolist() == [a["cw0_deinterleaved"] | a["ci_tried"] << 1, 0, 0, 0], tag
    nb, nl = a["frame_bytes"], a["n_llr"]
    assert np.array_equal(frames[i, :nb], a["frame"]) and not frames[i, nb:].any(), tag
    assert np.array_equal(llr[i, :nl].view(np.uint32), np.asarray(a["llr"], np.float32).view(np.uint32)) and not llr[i, nl:].view(np.uint32).any(), tag
    for f in MW.HARQ_FIELDS:
        assert int(hq[f][i]) == int(e["harq"][f]), (tag, f, hq[f][i], e["harq"][f])
    if cache_id is not None:
        assert int(hq["cache_id"][i]) == (cache_id if e["harq"]["valid"] else 0), tag


def compare_caches(pool, caches):
    for c, cache in enumerate(caches):
        assert pool.stats(c) == cache.stats, (c, pool.stats(c), cache.stats)
        ent, sums = pool.export(c)
        want = cache_snapshot(cache)
        assert sorted((int(e["seq"]), int(e["src_hash"]), int(e["dst_hash"])) for e in ent) == sorted(want), c
        for e, s in zip(ent, sums):
            w = want[(int(e["seq"]), int(e["src_hash"]), int(e["dst_hash"]))]
            assert e["combine_count"].tolist() == w["count"] and e["decoded"].tolist() == w["decoded"] and e["has_sum"].tolist() == w["has_sum"], c
            assert np.array_equal(s.view(np.uint32), w["sums"].view(np.uint32)), c


CALLS = [c["name"] for c in WI.calls() if c["pool"] is None]


# ---- 1. every row of the table
@pytest.mark.parametrize("name", CALLS)
def test_table_rows(eng, expected, name):
    call, x, kw, exp = next(t for t in expected if t[0]["name"] == name)
    got = run(eng, call, x, kw)
    for i, (r, e) in enumerate(zip(call["rows"], exp)):
        check_row(r["name"], i, got, e)


def test_interleaved_chase_pair_across_two_calls(eng, expected):
    """the two receptions of the interleaved link into one pool: stored in the first call, combined and recovered in the second"""
    pair = [t for t in expected if t[0]["pool"] == "link"]
    assert len(pair) == 2
    pool = eng.chase_pool(4)
    caches = [ChaseCache() for _ in range(4)]
    for call, x, kw, exp in pair:
        got = run(eng, call, x, kw, pool=pool, ids=[0, 1, 2, 3])
        again = WI.expected_call(oracle(), call, x, kw, caches)          # the caches of this test, beside the pool
        for i, (r, e) in enumerate(zip(call["rows"], exp)):
            check_row(r["name"], i, got, e, cache_id=i)
            assert again[i]["harq"] == e["harq"]
        compare_caches(pool, caches)
    assert exp[3]["harq"]["recovered_mask"] == 4
    pool.close()


# ---- 2. order and batch independence
def test_largest_batch_reversed_and_split(eng, expected):
    call, x, kw, exp = next(t for t in expected if t[0]["name"] == "chirp_disconnected")
    n = len(x)
    rev = np.arange(n)[::-1].copy()
    got = run(eng, call, x[rev], {k: v[rev] for k, v in kw.items()})
    for j, i in enumerate(rev):
        check_row(("reversed", call["rows"][i]["name"]), j, got, exp[i])
    h = n // 2 + 1
    for lo, hi in ((0, h), (h, n)):
        got = run(eng, call, x[lo:hi], {k: v[lo:hi] for k, v in kw.items()})
        for i in range(lo, hi):
            check_row(("split", call["rows"][i]["name"]), i - lo, got, exp[i])


def test_workspace_growth_leaves_results_alone(expected):
    """A call on 2 windows, then one on the whole largest batch, on a fresh handle created for 2 frames: every array of the
    second equals the same call on another fresh handle that never ran the first, and the first equals that call's first
    two rows."""
    from ria_amd.engine import RxEngine
    call, x, kw, _ = next(t for t in expected if t[0]["name"] == "chirp_disconnected")
    assert len(x) > 2
    a, b = RxEngine("DQPSK", "R1_4", max_batch=2), RxEngine("DQPSK", "R1_4", max_batch=2)
    small = run(a, call, x[:2], {k: v[:2] for k, v in kw.items()})
    big = run(a, call, x, kw)
    ref = run(b, call, x, kw)
    assert ref[2]["accepted"].sum() > 2 and ref[1]["deliver"].any()          # rounds ran behind the peek pass
    for k, (s, g, r) in enumerate(zip(small, big, ref)):
        assert g.tobytes() == r.tobytes(), k
        assert s.tobytes() == r[:2].tobytes(), k
    a.close()
    b.close()


def test_1030_windows_cross_the_scan_tile(eng, expected):
    """1030 windows tiled from 8 distinct one-codeword-span ZC windows: every list kernel crosses its 1024-thread tile"""
    call, x, kw, exp = next(t for t in expected if t[0]["name"] == "zc_cut_short")
    call2, x2, kw2, exp2 = next(t for t in expected if t[0]["name"] == "zc_connected")
    wl = call["wl"]
    pick = [(x[0], exp[0], kw, 0), (x[1], exp[1], kw, 1)]
    base_x, base_e, base_kw = [], [], []
    for i in (0, 1, 7, 6, 2, 8):                       # ack, data2, noise, connect_says_1, data3 (NEED_SAMPLES here), replay
        w = x2[i][:wl]
        base_x.append(w)
        base_kw.append({k: int(v[i]) for k, v in kw2.items()})
    for xx, e, k, i in pick:
        base_x.append(xx)
        base_kw.append({kk: int(v[i]) for kk, v in k.items()})
    base_x = np.stack(base_x)
    assert len(base_x) == 8
    base_e = [MW.mcdpsk_window(oracle(), base_x[j], call["search_len"], bps=2, chirp=False, disconnected=False, **base_kw[j]) for j in range(8)]
    assert len({e["outcome"] for e in base_e}) >= 4 and sum(e["outcome"] == MW.DECODED for e in base_e) >= 4
    order = np.random.default_rng(1030).integers(0, 8, 1030)
    order[:8] = np.arange(8)
    order[1020:1030] = np.arange(10) % 8                # every kind on both sides of the tile's end
    big = np.ascontiguousarray(base_x[order])
    kwb = {k: np.array([base_kw[j][k] for j in order], np.int64) for k in base_kw[0]}
    got = run(eng, call, big, kwb)
    for j, o in enumerate(order):
        check_row(("tile", j, int(o)), j, got, base_e[o])


# ---- 3. against the sibling calls
def _acq_call(eng, x, search_len, frame_cw, pending=False):
    frames, res, llr, hq = eng.mcdpsk_acquire(dev(eng, x), search_len, frame_cw, modulation=2, sync="zc", want_llr=True, channel_interleave=True,
                                              interleaver_bits=20, harq_entry=True, min_confidence=0.0)
    return frames.cpu().numpy(), res, llr.cpu().numpy(), hq


ACQ_SAME = ("detected", "accepted", "sync_start", "frame_start", "correlation", "cfo_hz", "fading_index", "delta", "modulation",
            "candidates", "success", "codewords_ok", "codewords_failed", "frame_type", "header_total_cw", "frame_bytes", "n_llr",
            "cw0_deinterleaved", "ci_tried")


def _same_as_acquire(win, acqc, rows, frame_cw):
    frames, res, acq, hq, llr = win
    f2, a2, l2, h2 = acqc
    for i in rows:
        for f in ACQ_SAME:
            assert acq[f][i].tobytes() == a2[f][i].tobytes(), (i, f, acq[f][i], a2[f][i])
        nb = 40 * frame_cw
        assert np.array_equal(frames[i, :nb], f2[i]) and not frames[i, nb:].any(), i
        n = l2.shape[1]
        assert np.array_equal(llr[i, :n].view(np.uint32), l2[i].view(np.uint32)) and not llr[i, n:].view(np.uint32).any(), i
        assert hq[i].tobytes() == h2[i].tobytes(), i


def test_fall_through_equals_acquire_ci_at_one_codeword(eng, expected):
    """first_avail 0, no replay position, a connected ZC window whose peek falls through: the outputs of
    ria_gpu_mcdpsk_acquire_ci_batch at frame_cw 1"""
    call, x, kw, exp = next(t for t in expected if t[0]["name"] == "zc_interleaved_chase_0")
    got = run(eng, call, x, kw)
    rows = [i for i, e in enumerate(exp) if e["outcome"] == MW.DECODED and e["pending_total_cw"] == 0] + \
           [i for i, e in enumerate(exp) if e["outcome"] == MW.NOT_ACCEPTED]
    assert len(rows) >= 2
    _same_as_acquire(got, _acq_call(eng, x, call["search_len"], 1), rows, 1)


def test_pending_on_input_equals_acquire_ci_at_that_count(eng, expected):
    call, x, kw, exp = next(t for t in expected if t[0]["name"] == "zc_interleaved_chase_0")
    for n in (1, 3):
        got = run(eng, call, x, dict(kw, pending_total_cw=np.full(len(x), n)))
        assert all(int(got[1]["outcome"][i]) == (MW.DECODED if exp[i]["acq"]["accepted"] else MW.NOT_ACCEPTED) for i in range(len(x)))
        assert all(int(got[1]["peek"][i]) == 0 for i in range(len(x)))
        _same_as_acquire(got, _acq_call(eng, x, call["search_len"], n), range(len(x)), n)


def test_pool_null_equals_the_call_without_chase(eng, expected):
    call, x, kw, exp = next(t for t in expected if t[0]["name"] == "zc_interleaved_chase_0")
    a = run(eng, call, x, kw)                                            # a pool-less call, cache ids -1
    pool = eng.chase_pool(4)
    b = run(eng, call, x, kw, pool=pool, ids=[-1, -1, -1, -1])          # a pool, chase off for every window
    pool.close()
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    assert not a[3].view(np.uint8).any()


# ---- 4. arguments
def test_argument_checks(eng, expected):
    from ria_amd import capi
    call, x, kw, exp = next(t for t in expected if t[0]["name"] == "zc_cut_short")
    L, h = eng.lib, eng.h
    n, wl = x.shape
    xd = dev(eng, x)
    p = np.zeros(n, eng.MCWIN_PARAMS)
    p["detect_threshold"], p["last_decoded_sync"] = 0.2, capi.MWIN_NO_LAST_SYNC
    frames = torch.zeros((n, 320), dtype=torch.uint8, device=eng.device)
    res = torch.zeros((n, 64), dtype=torch.uint8, device=eng.device)
    acq = torch.zeros((n, 64), dtype=torch.uint8, device=eng.device)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def go(params=p, cfg=(10, 2, 1), flags=0, stride=wl, search=call["search_len"], window_len=wl, count=n, row=320, xs=xd, llr=None, llr_stride=0,
           pool=None, ids=None, now=None, bits=0, handle=None):
        pd = torch.from_numpy(params.view(np.uint8).reshape(len(params), 32).copy()).to(eng.device)
        c = capi.McdpskConfig(*cfg, 0)
        rc = L.ria_gpu_mcdpsk_window_batch(handle or h, C.byref(c), ptr(xs) if xs is not None else None, stride, search, window_len, count, ptr(pd), flags,
                                           ptr(frames), row, ptr(res), ptr(acq), ptr(llr) if llr is not None else None, llr_stride,
                                           pool, ptr(ids) if ids is not None else None, ptr(now) if now is not None else None, None, bits, None)
        torch.cuda.synchronize()
        return rc

    OK, INVALID = 0, -1
    assert L.ria_gpu_mcdpsk_window_batch(None, None, None, 0, 0, 0, 0, None, 0, None, 0, None, None, None, 0, None, None, None, None, 0, None) == INVALID
    assert go() == OK
    assert go(count=0, xs=None) == OK
    assert go(count=-1) == INVALID and go(cfg=(0, 2, 1)) == INVALID and go(cfg=(10, 3, 1)) == INVALID and go(cfg=(10, 2, 3)) == INVALID
    assert go(search=wl + 1) == INVALID and go(stride=wl - 1) == INVALID and go(search=-1) == INVALID
    assert go(flags=0x10) == INVALID and go(flags=capi.MACQ_DISCONNECTED) == INVALID            # unknown flag; ZC only when connected
    assert go(row=319) == INVALID and go(xs=None) == INVALID
    assert go(flags=capi.MACQ_CHANNEL_INTERLEAVE, bits=0) == INVALID and go(flags=capi.MACQ_CHANNEL_INTERLEAVE, bits=649) == INVALID
    assert go(flags=capi.MACQ_CHANNEL_INTERLEAVE, bits=20) == OK
    llr = torch.zeros((n, 2 * 33 * 10 * 2), dtype=torch.float32, device=eng.device)
    assert go(llr=llr, llr_stride=2 * 33 * 10 * 2 - 1) == INVALID and go(llr=llr, llr_stride=2 * 33 * 10 * 2) == OK
    # the per-window inputs, found on the device and read with the first control read
    for field, value, want in (("pending_total_cw", 256, INVALID), ("pending_total_cw", 255, OK), ("first_avail", 9607, INVALID),
                               ("first_avail", 9608, INVALID), ("first_avail", 4608 + 33 * 512 - 1, INVALID), ("first_avail", 4608 + 33 * 512, OK)):
        q = p.copy()
        q[field][n - 1] = value          # connected: a first_avail below the 1-codeword span is refused too
        assert go(params=q) == want, (field, value)
    # a pool: foreign, without ids, duplicate ids
    other = eng.chase_pool(2)
    ids = torch.tensor([0, 0], dtype=torch.int32, device=eng.device)
    now = torch.zeros(n, dtype=torch.int64, device=eng.device)
    assert go(pool=other.p, ids=None, now=now) == INVALID
    assert go(pool=other.p, ids=ids, now=now) == INVALID                                      # duplicate cache ids
    assert all(other.stats(c)["stores"] == 0 for c in range(2))
    ids = torch.tensor([0, 1], dtype=torch.int32, device=eng.device)
    assert go(pool=other.p, ids=ids, now=now) == OK
    other.close()
    # a handle of another rate
    from ria_amd.engine import RxEngine
    e2 = RxEngine("DQPSK", "R1_2", max_batch=4)
    assert go(handle=e2.h) == INVALID
    e2.close()
    assert go() == OK


# ---- 5. the device-built handshake mix and the counters
def test_handshake_mix_and_tally(eng):
    from ria_amd import capi
    from ria_amd.acquire import HANDSHAKE_KINDS, MCDPSK_WINDOW_COUNTERS, make_handshake_windows, mcdpsk_window_tally
    n = 10
    w, sl, kinds = make_handshake_windows(eng, n, 0, 10.0, np.arange(1, n + 1, dtype=np.uint32) * np.uint32(2654435761))
    frames, res, acq, hq, llr = eng.mcdpsk_window(w, sl, want_llr=True)
    got = (frames.cpu().numpy(), res, acq, hq, llr.cpu().numpy())
    x = w.cpu().numpy()
    for i in range(n):
        check_row(("mix", i), i, got, MW.mcdpsk_window(oracle(), x[i], sl))
    kind = np.array(HANDSHAKE_KINDS)[kinds]
    O = capi.MWIN_OUTCOME
    assert all(res["outcome"][kind == "ping"] == O["PING"]) and all(res["outcome"][kind == "noise"] == O["NOT_ACCEPTED"])
    for k, ftype, cw in (("connect", 0x12, 3), ("control", 0x20, 1), ("data", 0x30, 3)):
        m = kind == k
        assert all(res["outcome"][m] == O["DECODED"]) and all(acq["success"][m] == 1) and all(acq["frame_type"][m] == ftype) and \
            all(acq["codewords_ok"][m] == cw), k
    t = dict(zip(MCDPSK_WINDOW_COUNTERS, mcdpsk_window_tally(res, acq)))
    assert (t["windows"], t["pings"], t["outcome_ping"], t["outcome_decoded"], t["outcome_not_accepted"], t["success"], t["delivered"]) == (10, 2, 2, 6, 2, 6, 8)
    assert t["peek_header_multi"] == 4 and t["peek_header_single"] == 2 and t["peek_handshake_fallback"] == 2 and t["peek_none"] == 4
    assert sum(t[f"outcome_{k.lower()}"] for k in O) == 10


# ---- 6. one window from host memory
@pytest.mark.parametrize("name", ["chirp_cut_short", "zc_cut_short"])
def test_host_form_and_adaptor_window_by_window_equal_the_batch(eng, expected, tmp_path, name):
    """ria_gpu_mcdpsk_window_host and ria_host::mcdpskWindow (a g++ program against the C ABI), one window per call, give the
    batch call's rows"""
    import os
    import subprocess
    from ria_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    call, x, kw, exp = next(t for t in expected if t[0]["name"] == name)
    cfg = call["cfg"]
    frames, res, acq, hq, llr = run(eng, call, x, kw)
    fl = (capi.MACQ_SYNC_CHIRP if cfg["chirp"] else 0) | (capi.MACQ_DISCONNECTED if cfg["disconnected"] else 0)
    c = capi.McdpskConfig(cfg["carriers"], cfg["bps"], cfg["spreading"], 0)
    for i in range(len(x)):
        p = capi.McAcqParams(0.0, 0.15 if cfg["chirp"] else 0.2, 0.0, int(kw["pending_total_cw"][i]), 0, int(kw["first_avail"][i]),
                                int(kw["last_decoded_sync"][i]))
        out = np.zeros(320, np.uint8)
        r, a = capi.McWindowResult(), capi.McAcqResult()
        w = np.ascontiguousarray(x[i])
        rc = eng.lib.ria_gpu_mcdpsk_window_host(eng.h, C.byref(c), w.ctypes.data_as(C.c_void_p), call["search_len"], len(w), C.byref(p), fl,
                                                out.ctypes.data_as(C.c_void_p), 320, C.byref(r), C.byref(a), 0)
        assert rc == 0, (name, i, eng.lib.ria_gpu_last_error(eng.h))
        assert bytes(r) == res[i].tobytes() and np.array_equal(out, frames[i]), (name, i)
        assert bytes(a) == acq[i].tobytes()[:64], (name, i)          # the 64-byte row; the two ci fields follow it
    assert eng.lib.ria_gpu_mcdpsk_window_host(eng.h, C.byref(c), None, 0, 0, None, 0, None, 0, None, None, 0) == -1
    exe = str(tmp_path / "mcdpsk_window_host_test")
    lib = os.path.join(root, "ria_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(root, "tests", "helpers", "mcdpsk_window_host_test.cpp"),
                           "-L" + lib, "-lria_gpu", "-Wl,-rpath," + lib])
    fw, fp, fo = str(tmp_path / "w.f32"), str(tmp_path / "p.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(x, np.float32).tofile(fw)
    np.stack([kw["pending_total_cw"], kw["first_avail"], kw["last_decoded_sync"]], axis=1).astype(np.int32).tofile(fp)
    n = int(subprocess.check_output([exe, str(cfg["carriers"]), str(cfg["bps"]), str(cfg["spreading"]), str(int(cfg["chirp"])),
                                     str(int(not cfg["disconnected"])), str(call["search_len"]), str(x.shape[1]), fw, fp, fo]).decode())
    assert n == len(x)
    rec = np.fromfile(fo, np.uint8).reshape(n, 64 + 64 + 4 + 320)
    for i in range(n):
        assert rec[i, :64].tobytes() == res[i].tobytes(), (name, i)
        assert rec[i, 64:128].tobytes() == acq[i].tobytes()[:64], (name, i)
        nb = int(rec[i, 128:132].view(np.int32)[0])
        assert nb == int(acq["frame_bytes"][i]) and np.array_equal(rec[i, 132:], frames[i]), (name, i)
