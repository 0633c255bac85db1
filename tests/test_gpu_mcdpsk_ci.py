"""GPU tests of MC-DPSK channel interleaving: ria_gpu_mcdpsk_decode_frame_ci_batch, ria_gpu_mcdpsk_acquire_ci_batch and
ria_gpu_mcdpsk_interleave_batch against the CPU restatement (tests/mcdpsk_ci_restatement.py).  Every comparison is bit-exact:
the DecodeResult fields with the two channel-interleaving bits, the frame bytes, the soft bits, the harq result, the
counters of every cache and its exported entries and (raw) sums.

What every recipe of tests/mcdpsk_ci_inputs.py does on the restatement is asserted in tests/test_mcdpsk_ci_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import pyoracle as po
import mcdpsk_ci_inputs as I
from mcdpsk_acquire_restatement import ACK, CONNECT, control_frame, encode_frame, oracle
from mcdpsk_ci_restatement import acquire_window_ci, decode_mcdpsk_frame_ci, interleave_bytes
from mcdpsk_harq_restatement import STATS, ChaseCache, cache_snapshot, empty_harq

pytestmark = pytest.mark.gpu

RES_FIELDS = ("success", "codewords_ok", "codewords_failed", "frame_type", "header_total_cw", "cw0_deinterleaved", "ci_tried")
HARQ_FIELDS = ("valid", "seq", "src_hash", "dst_hash", "stored_mask", "sum_mask", "recovered_mask", "max_combine", "entry")
ACQ_FIELDS = ("detected", "accepted", "sync_start", "frame_start", "cfo_hz", "fading_index", "delta", "modulation", "candidates",
              "success", "codewords_ok", "codewords_failed", "frame_type", "header_total_cw", "frame_bytes", "n_llr", "correlation",
              "cw0_deinterleaved", "ci_tried")


@pytest.fixture(scope="module")
def eng():
    from ria_amd.engine import RxEngine
    e = RxEngine("DQPSK", "R1_4", max_batch=64)
    yield e
    e.close()


def dev(eng, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(eng.device)


class Links:
    """A pool on the device and the restatement's caches beside it (the pattern of tests/test_gpu_mcdpsk_harq.py);
    decode() and acquire() run one call through both and compare every output and every cache"""

    def __init__(self, eng, n_caches):
        self.eng, self.pool = eng, eng.chase_pool(n_caches)
        self.caches = [ChaseCache() for _ in range(n_caches)]

    def check_row(self, i, res, frames, hq, r, h, cache_id):
        h = h or empty_harq()
        for f in RES_FIELDS:
            assert int(res[f][i]) == int(r[f]), (i, f, res[f][i], r[f])
        assert int(res["reserved"][i]) == r["cw0_deinterleaved"] | r["ci_tried"] << 1, i
        nb = len(r["frame"])
        assert int(res["frame_bytes"][i]) == nb and np.array_equal(frames[i, :nb], r["frame"]) and not frames[i, nb:].any(), i
        for f in HARQ_FIELDS:
            assert int(hq[f][i]) == int(h[f]), (i, f, hq[f][i], h[f])
        assert int(hq["cache_id"][i]) == (cache_id if h["valid"] else 0), i

    def decode(self, rows, ids, now, B, n_llr=None):
        rows = np.stack(rows)
        n, stride = rows.shape
        n_llr = [stride] * n if n_llr is None else n_llr
        frames, res, hq = self.eng.mcdpsk_decode_frame(dev(self.eng, rows), n_llr=n_llr, chase=self.pool, cache_id=ids, now_ms=now,
                                                       channel_interleave=True, interleaver_bits=B)
        frames = frames.cpu().numpy()
        out = []
        for i in range(n):
            r, h = decode_mcdpsk_frame_ci(oracle(), rows[i, :max(0, min(n_llr[i], stride))], B, self.caches[ids[i]] if ids[i] >= 0 else None, now)
            self.check_row(i, res, frames, hq, r, h, ids[i])
            out.append((r, h))
        self.compare_caches()
        return out

    def acquire(self, x, search_len, ids, now, B, bps, chirp, **kw):
        eng = self.eng
        frames, res, llr, hq = eng.mcdpsk_acquire(dev(eng, x), search_len, 3, want_llr=True, chase=self.pool, cache_id=ids, now_ms=now,
                                                  modulation=bps, sync="chirp" if chirp else "zc", channel_interleave=True,
                                                  interleaver_bits=B, **kw)
        frames, llr = frames.cpu().numpy(), llr.cpu().numpy()
        out = []
        for i in range(len(x)):
            r, h = acquire_window_ci(oracle(), x[i], search_len, 3, B, self.caches[ids[i]] if ids[i] >= 0 else None, now, bps=bps, chirp=chirp,
                                     min_confidence=kw.get("min_confidence", 0.0))
            for f in ACQ_FIELDS:
                got, want = res[f][i], r[f]
                if isinstance(want, np.float32):
                    assert np.float32(got).view(np.uint32) == want.view(np.uint32), (i, f, got, want)
                else:
                    assert int(got) == int(want), (i, f, got, want)
            assert res["reserved"][i].tolist() == [r["cw0_deinterleaved"] | r["ci_tried"] << 1, 0, 0, 0], i
            nb, nl = r["frame_bytes"], r["n_llr"]
            assert np.array_equal(frames[i, :nb], r["frame"]) and not frames[i, nb:].any(), i
            assert np.array_equal(llr[i, :nl].view(np.uint32), np.asarray(r["llr"], np.float32).view(np.uint32)) and not llr[i, nl:].any(), i
            for f in HARQ_FIELDS:
                assert int(hq[f][i]) == int(h[f]), (i, f, hq[f][i], h[f])
            out.append((r, h))
        self.compare_caches()
        return out

    def compare_caches(self):
        for c, cache in enumerate(self.caches):
            assert self.pool.stats(c) == cache.stats, (c, self.pool.stats(c), cache.stats)
            ent, sums = self.pool.export(c)
            want = cache_snapshot(cache)
            assert sorted((int(e["seq"]), int(e["src_hash"]), int(e["dst_hash"])) for e in ent) == sorted(want), c
            for e, s in zip(ent, sums):
                w = want[(int(e["seq"]), int(e["src_hash"]), int(e["dst_hash"]))]
                assert (int(e["total_cw"]), int(e["frame_type"]), int(e["last_access_ms"]), int(e["order"]), int(e["used"])) == \
                       (w["total_cw"], w["frame_type"], w["last_access"], w["order"], 1), (c, e, w)
                assert e["combine_count"].tolist() == w["count"] and e["decoded"].tolist() == w["decoded"] and e["has_sum"].tolist() == w["has_sum"], (c, e, w)
                assert np.array_equal(s.view(np.uint32), w["sums"].view(np.uint32)), c

    def close(self):
        self.pool.close()


# ---- 1. decode-frame rows
@pytest.mark.parametrize("B", [10, 20])
def test_decode_frame_rows(eng, B):
    """twelve rows in one call: both CW0 paths, mixed codewords, noise, partial and short rows, the wrong width, a
    one-codeword data frame, and rows without a cache"""
    rows, n_llr, ids, want = I.decode_rows(B)
    L = Links(eng, 10)
    out = L.decode(rows, ids, 5, B, n_llr=n_llr)
    assert [I.outcome(r) for r, _ in out] == want
    L.close()


# ---- 2. flag off
def _decode_frame_call(eng, fn, rows, n_llr, pool, ids, extra):
    from ria_amd.engine import _ptr, _stream_ptr
    n, stride = rows.shape
    frames = torch.full((n, 20 * (stride // 648)), 0xEE, dtype=torch.uint8, device=eng.device)
    res = torch.full((n, 16), 0xEE, dtype=torch.uint8, device=eng.device)
    harq = torch.full((n, 32), 0xEE, dtype=torch.uint8, device=eng.device)
    nl = dev(eng, np.asarray(n_llr, np.int32))
    cid, now = dev(eng, np.asarray(ids, np.int32)), dev(eng, np.full(n, 7, np.int64))
    eng._check(fn(eng.h, _ptr(rows), stride, _ptr(nl), n, pool.p if pool else None, _ptr(cid), _ptr(now), _ptr(frames), frames.shape[1], _ptr(res),
                  _ptr(harq), *extra, _stream_ptr()))
    torch.cuda.synchronize()
    return frames.cpu().numpy().tobytes(), res.cpu().numpy().tobytes(), harq.cpu().numpy().tobytes()


def _acquire_call(eng, fn, x, search_len, bps, flags, pool, ids, extra):
    from ria_amd import capi
    from ria_amd.engine import _ptr, _stream_ptr
    n, wl = x.shape
    p = np.zeros(n, eng.MCACQ_PARAMS)
    p["detect_threshold"], p["min_confidence"] = (0.15, 0.0) if flags & capi.MACQ_SYNC_CHIRP else (0.2, 0.25)
    params = dev(eng, p.view(np.uint8).reshape(n, 32))
    stride = 3 * -(-648 // (10 * bps)) * 10 * 2
    frames = torch.full((n, 120), 0xEE, dtype=torch.uint8, device=eng.device)
    acq = torch.full((n, 64), 0xEE, dtype=torch.uint8, device=eng.device)
    llr = torch.full((n, stride), 7.0, dtype=torch.float32, device=eng.device)
    harq = torch.full((n, 32), 0xEE, dtype=torch.uint8, device=eng.device)
    cid, now = dev(eng, np.asarray(ids, np.int32)), dev(eng, np.full(n, 7, np.int64))
    cfg = capi.McdpskConfig(10, bps, 1, 0)
    eng._check(fn(eng.h, C.byref(cfg), _ptr(x), wl, search_len, wl, n, 3, _ptr(params), flags, _ptr(frames), _ptr(acq), _ptr(llr), stride,
                  pool.p if pool else None, _ptr(cid), _ptr(now), _ptr(harq), *extra, _stream_ptr()))
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().tobytes() for t in (frames, acq, llr, harq))


def test_flag_off_is_the_old_call_byte_for_byte(eng):
    """ria_gpu_mcdpsk_decode_frame_ci_batch with flags 0 against ria_gpu_mcdpsk_decode_frame_batch on the rows of test 1 (with
    two pools that start equal), ria_gpu_mcdpsk_acquire_ci_batch without the flag against ria_gpu_mcdpsk_acquire_harq_batch on
    the handshake windows: every output buffer byte-equal, the reserved words included, and equal caches"""
    from ria_amd import capi
    rows, n_llr, ids, _ = I.decode_rows(10)
    rows = dev(eng, np.stack(rows))
    a, b = eng.chase_pool(10), eng.chase_pool(10)
    for t in range(2):                                       # the second call combines with what the first stored
        old = _decode_frame_call(eng, eng.lib.ria_gpu_mcdpsk_decode_frame_batch, rows, n_llr, a, ids, ())
        new = _decode_frame_call(eng, eng.lib.ria_gpu_mcdpsk_decode_frame_ci_batch, rows, n_llr, b, ids, (0, 12345))
        assert old == new
        for c in range(10):
            assert a.stats(c) == b.stats(c)
            (ea, sa), (eb, sb) = a.export(c), b.export(c)
            assert ea.tobytes() == eb.tobytes() and sa.tobytes() == sb.tobytes()
    assert sum(a.stats(c)["combines"] for c in range(10)) == 2       # mode off: row 4 (plain CW0, two codewords that fail) is the one that stores
    assert _decode_frame_call(eng, eng.lib.ria_gpu_mcdpsk_decode_frame_batch, rows, n_llr, None, ids, ()) == \
        _decode_frame_call(eng, eng.lib.ria_gpu_mcdpsk_decode_frame_ci_batch, rows, n_llr, None, ids, (0, 0))
    x = dev(eng, I.handshake_windows(oracle()))
    fl = capi.MACQ_SYNC_CHIRP | capi.MACQ_DISCONNECTED
    for pa, pb in ((a, b), (None, None)):
        old = _acquire_call(eng, eng.lib.ria_gpu_mcdpsk_acquire_harq_batch, x, I.CHIRP_SEARCH, 1, fl, pa, [0, 1, 2], ())
        new = _acquire_call(eng, eng.lib.ria_gpu_mcdpsk_acquire_ci_batch, x, I.CHIRP_SEARCH, 1, fl, pb, [0, 1, 2], (-3,))
        assert old == new
    acq = np.frombuffer(old[1], eng.MCACQ_RESULT)
    assert acq["accepted"].all() and not acq["reserved"].any()
    a.close()
    b.close()


# ---- 3. chase
@pytest.mark.parametrize("B", [10, 20])
def test_chase_stores_raw_sums_and_deinterleaves_them_when_gathered(eng, B):
    """four links x four receptions: recoveries at count 2 and 3, the ordering trap, and a cache that gets one reception
    interleaved and the next one plain; after every call the counters and the exported entries and sums equal the
    restatement's, whose cache holds the raw soft bits"""
    L = Links(eng, 4)
    hist = []
    for t, (rows, ids) in enumerate(I.chase_calls(B)):
        hist.append(L.decode(rows, ids, 1000 * t, B))
        if t == 0:
            ent, sums = L.pool.export(0)
            assert len(ent) == 1 and np.array_equal(sums[0][1].view(np.uint32), rows[0][648:1296].view(np.uint32))   # raw, bit for bit
    h = lambda t, l: hist[t][l][1]
    assert h(1, 0)["recovered_mask"] == 2 and h(2, 1)["recovered_mask"] == 4 and h(2, 1)["max_combine"] == 3
    assert (h(0, 2)["stored_mask"], h(1, 2)["stored_mask"]) == (4, 2)
    assert hist[1][3][0]["cw0_deinterleaved"] == 0 and h(1, 3)["sum_mask"] == 2 and h(1, 3)["recovered_mask"] == 0
    assert sum(c.stats["recoveries"] for c in L.caches) == 2
    L.close()


# ---- 4. list boundary
def test_a2_list_across_the_scan_tile(eng):
    """1030 rows of one codeword: the A2 list crosses the end of the 1024-thread scan tile; the same rows in two calls of
    515 give the same results"""
    B = 10
    base, order = I.boundary_rows(B)
    want = [decode_mcdpsk_frame_ci(oracle(), x, B)[0] for x in base]
    assert [I.outcome(r) for r in want] == I.BOUNDARY_WANT
    rows = dev(eng, np.stack(base)[order])
    frames, res, hq = eng.mcdpsk_decode_frame(rows, channel_interleave=True, interleaver_bits=B)
    frames = frames.cpu().numpy()
    for i, k in enumerate(order):
        r = want[k]
        assert [int(res[f][i]) for f in RES_FIELDS] == [int(r[f]) for f in RES_FIELDS], (i, k)
        nb = len(r["frame"])
        assert int(res["frame_bytes"][i]) == nb and np.array_equal(frames[i, :nb], r["frame"]) and not frames[i, nb:].any(), (i, k)
    assert not hq.view(np.uint8).any()
    for lo in (0, 515):
        f2, r2, _ = eng.mcdpsk_decode_frame(rows[lo:lo + 515].contiguous(), channel_interleave=True, interleaver_bits=B)
        assert np.array_equal(f2.cpu().numpy(), frames[lo:lo + 515]) and r2.tobytes() == res[lo:lo + 515].tobytes()


# ---- 5. acquire
def test_acquire_connected_zc_dqpsk(eng):
    """ZC, connected, DQPSK, B = 20: an interleaved data frame, a plain ACK, noise, and a link whose CW2 arrives weak twice
    and is recovered from the raw sum in the second call"""
    calls = I.zc_windows(oracle())
    L = Links(eng, 2)
    ids = [-1, -1, -1, 1]
    out = L.acquire(calls[0], I.ZC_SEARCH, ids, 0, 20, 2, False, min_confidence=0.25)
    assert [(r["success"], r["cw0_deinterleaved"], r["ci_tried"]) for r, _ in out] == [(1, 1, 1), (1, 0, 0), (0, 0, 0), (0, 1, 1)]
    assert out[3][1]["stored_mask"] == 4 and L.caches[1].size() == 1
    out = L.acquire(calls[1], I.ZC_SEARCH, ids, 1000, 20, 2, False, min_confidence=0.25)
    assert out[3][0]["success"] == 1 and out[3][1]["recovered_mask"] == 4 and L.caches[1].size() == 0
    L.close()


def test_acquire_disconnected_chirp_handshake(eng):
    """dual chirp, disconnected, primary DBPSK with B = 20, an interleaved CONNECT: the primary, a timing-recovery candidate
    and the alternate modulation each win through round A2, every candidate with the caller's B"""
    L = Links(eng, 1)
    out = L.acquire(I.handshake_windows(oracle()), I.CHIRP_SEARCH, [-1, -1, -1], 0, 20, 1, True)
    rs = [r for r, _ in out]
    assert [(r["success"], r["cw0_deinterleaved"], r["frame_type"]) for r in rs] == [(1, 1, CONNECT)] * 3
    assert rs[0]["candidates"] == 1 and rs[1]["delta"] != 0 and rs[1]["candidates"] > 2
    assert (rs[2]["candidates"], rs[2]["modulation"]) == (2, po.DQPSK)
    L.close()


# ---- 6. the interleave kernel
def test_interleave_kernel(eng):
    coded = np.random.default_rng(67).integers(0, 256, (67, 81), dtype=np.uint8)
    for B in (1, 10, 20, 40, 648):
        got = eng.mcdpsk_interleave(coded, B).cpu().numpy()
        assert np.array_equal(got, interleave_bytes(coded, B)), B
    frame = I.data3(33)
    plain = encode_frame(frame).reshape(1, -1)
    tx = eng.mcdpsk_modulate_batch(eng.mcdpsk_interleave(plain, 10), carriers=10, bits_per_symbol=1)
    llr, _ = eng.mcdpsk_demod(tx, carriers=10, bits_per_symbol=1)
    frames, res, _ = eng.mcdpsk_decode_frame(llr[:, :1944].contiguous(), channel_interleave=True)      # None: carriers x bits = 10
    assert (int(res["success"][0]), int(res["cw0_deinterleaved"][0]), int(res["frame_bytes"][0])) == (1, 1, len(frame))
    assert np.array_equal(frames.cpu().numpy()[0, :len(frame)], frame)
    _, res, _ = eng.mcdpsk_decode_frame(llr[:, :1944].contiguous())
    assert int(res["success"][0]) == 0 and int(res["reserved"][0]) == 0


# ---- 7. argument rejections
def test_argument_rejections(eng):
    from ria_amd.capi import RiaError
    from ria_amd.engine import RxEngine
    rows = dev(eng, np.stack(I.decode_rows(10)[0][:2]))
    x = dev(eng, I.handshake_windows(oracle())[:1])
    for B in (0, 649):
        with pytest.raises(RiaError, match="status -1"):
            eng.mcdpsk_decode_frame(rows, channel_interleave=True, interleaver_bits=B)
        with pytest.raises(RiaError, match="status -1"):
            eng.mcdpsk_acquire(x, I.CHIRP_SEARCH, 3, channel_interleave=True, interleaver_bits=B)
        with pytest.raises(RiaError, match="status -1"):
            eng.mcdpsk_interleave(np.zeros((1, 81), np.uint8), B)
    with pytest.raises(RiaError, match="status -1"):          # an unknown flag bit
        _decode_frame_call(eng, eng.lib.ria_gpu_mcdpsk_decode_frame_ci_batch, rows, [1944, 1944], None, [-1, -1], (0x8 | 0x1, 10))
    e2 = RxEngine("DQPSK", "R1_2", max_batch=64)
    try:
        with pytest.raises(RiaError, match="status -1"):
            e2.mcdpsk_decode_frame(dev(e2, rows.cpu().numpy()), channel_interleave=True, interleaver_bits=10)
        with pytest.raises(RiaError, match="status -1"):
            e2.mcdpsk_acquire(dev(e2, x.cpu().numpy()), I.CHIRP_SEARCH, 3, channel_interleave=True, interleaver_bits=10)
    finally:
        e2.close()
