"""GPU tests of the device-resident HARQ chase cache: ria_gpu_mcdpsk_decode_frame_batch and ria_gpu_mcdpsk_acquire_harq_batch
against the CPU restatement (tests/mcdpsk_harq_restatement.py: the Python ChaseCache and decodeMCDPSKFrame with its chase
statements, on the oracle's robust decoder).  Every comparison is bit-exact: the DecodeResult fields, the frame bytes, the
harq result, the seven counters of every cache and its exported entries and sums.

The robust decoder at R1/4 can converge on noise, so every test first asserts, on the restatement, that its rows give the
sequence of per-codeword outcomes it is about."""
import numpy as np
import pytest
import torch

import pyoracle as po
from mcdpsk_acquire_restatement import ACK, CONNECT, control_frame, data_frame, encode_frame, frame_len, oracle, window
from mcdpsk_harq_domain_inputs import DEAD, GOOD, HARQ_FIELDS, RES_FIELDS, WEAK2, WEAK3, Links, row   # row() and Links live there
from mcdpsk_harq_restatement import STATS, acquire_window, decode_mcdpsk_frame
from ria_amd.acquire import harq_tally

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from ria_amd.engine import RxEngine
    e = RxEngine("DQPSK", "R1_4", max_batch=64)
    yield e
    e.close()


def test_recoveries_the_trap_refused_stores_and_rows_without_a_cache(eng):
    """Nine rows per call (three blocks of one-wave entries, the last one partial), seven calls into one pool:
    row 0 recovers CW1 at count 2, row 1 CW2 at count 3, row 2 never (the fifth and sixth store are refused and the sum of
    four is decoded again), row 3 is the ordering trap, row 4 fails without a cache, row 5 is a control frame, row 6 has too
    few soft bits, row 7 a header that asks for more codewords than the row holds, row 8 decodes at once.  The last call
    decodes every frame at once: its list of sums is empty, and full success removes what is left."""
    L = Links(eng, 9)
    ids = [3, 0, 7, 5, -1, 1, 2, 8, 6]
    ack = control_frame(ACK, 40)
    trap = [(GOOD, GOOD, DEAD), (GOOD, DEAD, GOOD), (GOOD, DEAD, DEAD), (GOOD, GOOD, GOOD)]
    hist = []
    for t in range(7):
        last = t == 6
        rows = [row(5, (GOOD, WEAK2 if t < 2 else GOOD, GOOD), 100 + 50 * t),
                row(6, (GOOD, GOOD, WEAK3 if t < 3 else GOOD), 201 + 50 * t),
                row(7, (GOOD, GOOD if last else DEAD, GOOD), 300 + 10 * t),
                row(8, trap[min(t, 3)], 400 + t),
                row(9, (GOOD, DEAD, GOOD), 500 + t),
                row(0, (GOOD,), 600 + t, frame=ack),
                row(10, (GOOD, DEAD, DEAD), 700 + t),
                row(11, (GOOD, DEAD, DEAD), 800 + t),
                row(12, (GOOD, GOOD, GOOD), 900 + t)]
        hist.append(L.call(rows, ids, 1000 * t, n_llr=[1944, 1944, 1944, 1944, 1944, 648, 500, 1296, 1944]))
    h = lambda t, i: hist[t][i][1]
    r = lambda t, i: hist[t][i][0]
    # the rows do what they are meant to (on the restatement)
    assert r(0, 0)["codewords_failed"] == 1 and h(1, 0)["recovered_mask"] == 2 and h(1, 0)["max_combine"] == 2 and r(1, 0)["success"] == 1
    assert h(1, 0)["entry"] == po_entry("REMOVED") and L.caches[3].size() == 0
    assert [h(t, 1)["recovered_mask"] for t in range(3)] == [0, 0, 4] and h(1, 1)["sum_mask"] == 4 and h(2, 1)["max_combine"] == 3
    assert [h(t, 2)["stored_mask"] for t in range(6)] == [2, 2, 2, 2, 0, 0] and [h(t, 2)["sum_mask"] for t in range(6)] == [0, 2, 2, 2, 2, 2]
    assert all(h(t, 2)["recovered_mask"] == 0 for t in range(6)) and h(5, 2)["max_combine"] == 4 and h(6, 2)["entry"] == po_entry("REMOVED")
    assert (r(0, 3)["codewords_ok"], h(0, 3)["stored_mask"]) == (2, 4) and (r(1, 3)["codewords_ok"], h(1, 3)["stored_mask"]) == (2, 2)   # the trap
    assert h(2, 3)["stored_mask"] == 2 and h(2, 3)["sum_mask"] == 2      # CW2 was marked in reception 2: its store is refused
    assert h(3, 3)["entry"] == po_entry("REMOVED")
    assert all(r(t, 4)["codewords_failed"] == 1 and h(t, 4)["valid"] == 0 for t in range(7))
    assert r(0, 5)["success"] == 1 and r(0, 5)["header_total_cw"] == 1 and h(0, 5)["valid"] == 1 and L.caches[1].stats["stores"] == 0
    assert r(0, 6)["codewords_ok"] == 0 and h(0, 6)["valid"] == 0
    assert r(0, 7)["header_total_cw"] == 3 and r(0, 7)["success"] == 0 and len(r(0, 7)["frame"]) == 20 and L.caches[8].stats["stores"] == 0
    assert all(r(t, 8)["success"] == 1 and h(t, 8)["entry"] == 0 for t in range(7))
    assert all(r(6, i)["success"] == 1 for i in (0, 1, 2, 3, 8)) and all(h(6, i)["sum_mask"] == 0 for i in range(9))
    assert sum(c.stats["recoveries"] for c in L.caches) == 2 and L.caches[7].stats["combines"] == 3
    t = L.check_tally()
    assert t["delivered_by_combining"] == 2 and t["rows"] == 63 and t["sum_decodes"] >= 8
    L.close()


def po_entry(name):
    from ria_amd import capi
    return capi.HARQ_ENTRY[name]


def test_two_keys_eviction_and_expiry_in_one_cache(eng):
    """max_entries 2, ttl 1000 ms, one cache: two keys side by side, a touched entry outlives an older one, the third key
    evicts the oldest, and a late store expires what is left; rows of four codewords with one of them cut off by n_llr"""
    L = Links(eng, 1, max_entries=2, ttl_ms=1000)
    calls = [(10, 0), (11, 100), (10, 200), (12, 300), (13, 1300), (14, 1301)]
    for k, (seq, now) in enumerate(calls):
        L.call([row(seq, (GOOD, DEAD, GOOD), 1000 + k, stride=4 * 648)], [0], now, n_llr=[2500])
        if k == 1:
            assert L.caches[0].size() == 2
    s = L.caches[0].stats
    assert (s["stores"], s["combines"], s["entries_evicted"], s["entries_expired"]) == (6, 1, 1, 2), s   # 11 evicted; 10 expired at 1300 (1100 ms old), 12 kept at exactly ttl and expired at ttl + 1
    assert sorted(k[0] for k in L.caches[0].cache) == [13, 14]
    L.close()


def test_duplicate_cache_ids_are_refused_before_any_cache_is_touched(eng):
    from ria_amd.capi import RiaError
    L = Links(eng, 4)
    L.call([row(20, (GOOD, DEAD, GOOD), 1), row(21, (GOOD, GOOD, DEAD), 2)], [1, 2], 5)
    assert L.caches[1].size() == 1 and L.caches[2].size() == 1
    rows = torch.from_numpy(np.stack([row(20, (GOOD, DEAD, GOOD), 3), row(22, (GOOD, DEAD, GOOD), 4), row(21, (GOOD, DEAD, DEAD), 5)])).to(eng.device)
    for ids in ([1, 0, 1], [0, 4, 1], [2, 2, 2]):
        with pytest.raises(RiaError, match="status -1"):
            eng.mcdpsk_decode_frame(rows, chase=L.pool, cache_id=ids, now_ms=9)
        L.compare_caches()
    L.call(list(rows.cpu().numpy()), [1, -1, 2], 9)         # the same rows with distinct ids go through
    assert L.caches[1].stats["combines"] == 1
    L.close()


def test_clear_and_create_destroy_create(eng):
    L = Links(eng, 3)
    rows = [row(30 + i, (GOOD, DEAD, GOOD), 10 + i) for i in range(3)]
    L.call(rows, [0, 1, 2], 1)
    assert all(c.size() == 1 for c in L.caches)
    L.pool.clear([1, 7, -1])                               # ids outside the pool are skipped
    L.caches[1].clear()
    L.compare_caches()
    assert L.caches[1].stats["stores"] == 1 and L.pool.export(1)[0].size == 0
    L.call(rows, [0, 1, 2], 2)
    assert L.caches[0].stats["combines"] == 1 and L.caches[1].stats["combines"] == 0
    L.pool.clear()
    for c in L.caches:
        c.clear()
    L.compare_caches()
    L.close()
    M = Links(eng, 2, max_entries=3)
    M.compare_caches()                                     # a fresh pool: no entries, counters zero
    M.call(rows[:2], [1, 0], 3)
    assert M.caches[0].stats["stores"] == 1 and M.caches[0].stats["combines"] == 0
    M.close()


def test_pool_none_is_the_plain_decode(eng):
    """without a pool, and with every id -1, the call is decodeMCDPSKFrame without chase: the harq rows are zero"""
    rows = np.stack([row(40, (GOOD, DEAD, GOOD), 1), row(41, (GOOD, GOOD, GOOD), 2), row(0, (GOOD,), 3, frame=control_frame(ACK, 41))])
    dev = torch.from_numpy(rows).to(eng.device)
    f0, r0, h0 = eng.mcdpsk_decode_frame(dev)
    pool = eng.chase_pool(2)
    f1, r1, h1 = eng.mcdpsk_decode_frame(dev, chase=pool, cache_id=[-1, -1, -1])
    assert torch.equal(f0, f1) and r0.tobytes() == r1.tobytes() and not h0.view(np.uint8).any() and not h1.view(np.uint8).any()
    assert pool.stats(0) == dict.fromkeys(STATS, 0) and pool.export(0)[0].size == 0
    for i in range(3):
        r, _ = decode_mcdpsk_frame(oracle(), rows[i])
        assert [int(r0[f][i]) for f in RES_FIELDS] == [int(r[f]) for f in RES_FIELDS]
        assert np.array_equal(f0[i, :len(r["frame"])].cpu().numpy(), r["frame"])
    assert [int(v) for v in r0["success"]] == [0, 1, 1]
    pool.close()


# ---- ria_gpu_mcdpsk_acquire_harq_batch
ACQ_FIELDS = ("detected", "accepted", "sync_start", "frame_start", "cfo_hz", "fading_index", "delta", "modulation", "candidates",
              "success", "codewords_ok", "codewords_failed", "frame_type", "header_total_cw", "frame_bytes", "n_llr", "correlation")


def acquire_and_compare(L, x, search_len, frame_cw, ids, now, **kw):
    """one call of windows x into L's pool and through the restatement's caches; every output compared"""
    eng = L.eng
    chirp = kw.get("sync", "chirp") == "chirp"
    frames, res, llr, hq = eng.mcdpsk_acquire(torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(eng.device), search_len, frame_cw,
                                              want_llr=True, chase=L.pool, cache_id=ids, now_ms=now, **kw)
    frames, llr = frames.cpu().numpy(), llr.cpu().numpy()
    L.tally += harq_tally(res, hq)
    out = []
    for i in range(len(x)):
        r, h = acquire_window(oracle(), x[i], search_len, frame_cw, L.caches[ids[i]] if ids[i] >= 0 else None, now, chirp=chirp,
                              disconnected=kw.get("disconnected"), detect_threshold=kw.get("detect_threshold"),
                              min_confidence=kw.get("min_confidence", 0.0))
        for f in ACQ_FIELDS:
            got, want = res[f][i], r[f]
            if isinstance(want, np.float32):
                assert np.float32(got).view(np.uint32) == want.view(np.uint32), (i, f, got, want)
            else:
                assert int(got) == int(want), (i, f, got, want)
        nb, nl = r["frame_bytes"], r["n_llr"]
        assert np.array_equal(frames[i, :nb], r["frame"]) and not frames[i, nb:].any(), i
        assert np.array_equal(llr[i, :nl].view(np.uint32), np.asarray(r["llr"], np.float32).view(np.uint32)) and not llr[i, nl:].any(), i
        for f in HARQ_FIELDS:
            assert int(hq[f][i]) == int(h[f]), (i, f, hq[f][i], h[f])
        out.append((r, h))
    L.compare_caches()
    return out


def test_connected_links_retransmit_into_one_pool(eng):
    """Six links x four transmissions of one 3-codeword data frame over the moderate channel at -11 dB, ZC, connected,
    DBPSK, 10 carriers; one call per transmission, link l into cache l.  On the restatement the set holds a recovery at
    count 2, one at count 3, a trap pair (CW1 decodes and CW2 fails, then CW1 fails in the next reception and is stored) and
    a frame delivered only through combining."""
    O = oracle()
    coded = encode_frame(data_frame(0x30, 5, np.arange(25, dtype=np.uint8)))
    lead, wl = 2000, 110960
    search_len = lead + 2512 + 8 * 512
    L = Links(eng, 6)
    hist = []
    for tx in range(4):
        x = np.stack([window(O, coded, 10, po.DBPSK, 1, False, lead, wl, 2, -11.0, 1000 * link + tx + 1) for link in range(6)])
        hist.append(acquire_and_compare(L, x, search_len, 3, list(range(6)), 1000 * tx, sync="zc", detect_threshold=0.05, min_confidence=0.05))
    hs = [[hist[t][l][1] for t in range(4)] for l in range(6)]
    rs = [[hist[t][l][0] for t in range(4)] for l in range(6)]
    rec = [(l, t) for l in range(6) for t in range(4) if hs[l][t]["recovered_mask"]]
    assert any(hs[l][t]["max_combine"] == 2 for l, t in rec) and any(hs[l][t]["max_combine"] == 3 for l, t in rec)
    assert any(rs[l][t]["success"] for l, t in rec)                       # delivered only through combining
    trap = [(l, t) for l in range(6) for t in range(3)
            if (rs[l][t]["codewords_ok"], hs[l][t]["stored_mask"]) == (2, 4) and hs[l][t + 1]["stored_mask"] & 2]
    assert trap, "no trap pair in the set"
    t = L.check_tally()
    assert t["recoveries"] >= 2 and t["delivered_by_combining"] >= 1
    L.close()


def test_disconnected_candidates_store_and_the_next_candidate_sees_it(eng):
    """Disconnected chirp windows whose frame lies 48 samples behind the detector's place: the primary decodes no header,
    timing-recovery candidates decode the header but not the frame and store, later candidates of the same window combine
    with what they stored.  In the first window that recovers a codeword and delivers the frame at delta 64; in the second
    no candidate succeeds and the entry stays."""
    O = oracle()
    coded = encode_frame(data_frame(CONNECT, 7, np.arange(25, dtype=np.uint8)))
    fl = frame_len(3, 10, 1, 1)
    search_len, wl = 2000 + 57600 + 8 * 512, 2000 + 57600 + fl + 2000
    x = np.stack([window(O, coded, 10, po.DBPSK, 1, True, 2000, wl, 2, snr, seed, shift=48) for snr, seed in ((-8.0, 107), (-11.0, 102))])
    L = Links(eng, 3)
    (r0, h0), (r1, h1) = acquire_and_compare(L, x, search_len, 3, [2, 0], 77)
    assert r0["candidates"] > 2 and r0["success"] == 1 and r0["delta"] == 64 and h0["recovered_mask"] and h0["entry"] == po_entry("REMOVED")
    assert L.caches[2].stats["stores"] == 3 and L.caches[2].stats["combines"] == 2 and L.caches[2].stats["recoveries"] == 1
    assert r1["candidates"] == 26 and r1["codewords_ok"] == 0 and L.caches[0].stats["stores"] == 4 and L.caches[0].stats["combines"] == 2
    assert L.caches[0].size() == 1 and L.caches[1].stats == dict.fromkeys(STATS, 0)
    L.close()


def test_acquire_without_a_pool_equals_the_plain_call(eng):
    """pool NULL, and a pool with every id -1: frames, results and soft bits byte-equal to ria_gpu_mcdpsk_acquire_batch"""
    O = oracle()
    connect = encode_frame(data_frame(CONNECT, 7, np.arange(25, dtype=np.uint8)))
    bad = encode_frame(data_frame(CONNECT, 9, np.arange(25, dtype=np.uint8), total_cw=2))
    ack = encode_frame(control_frame(ACK, 10))
    fl = frame_len(3, 10, 1, 1)
    search_len, wl = 2000 + 57600 + 8 * 512, 2000 + 57600 + fl + 2000
    spec = [(connect, 1, 0, 10.0, 1), (None, 1, 0, 10.0, 2), (bad, 1, 0, 10.0, 4), (connect, 2, 0, 12.0, 5), (ack, 1, 2, 6.0, 6),
            (connect, 1, 2, -4.0, 100), (connect, 1, 2, -2.0, 102)]
    x = np.stack([window(O, c, 10, po.DBPSK if b == 1 else po.DQPSK, 1, True, 2000, wl, k, snr, seed) for c, b, k, snr, seed in spec])
    w = torch.from_numpy(x).to(eng.device)
    f0, r0, l0 = eng.mcdpsk_acquire(w, search_len, 3, want_llr=True)
    pool = eng.chase_pool(2)
    f1, r1, l1, h1 = eng.mcdpsk_acquire(w, search_len, 3, want_llr=True, chase=pool, cache_id=-1)
    assert torch.equal(f0, f1) and r0.tobytes() == r1.tobytes() and torch.equal(l0.view(torch.int32), l1.view(torch.int32))
    assert not h1.view(np.uint8).any() and pool.stats(0) == dict.fromkeys(STATS, 0) and pool.stats(1) == dict.fromkeys(STATS, 0)
    f2, r2, l2, h2 = eng.mcdpsk_acquire(w, search_len, 3, want_llr=True, harq_entry=True)        # pool NULL
    assert torch.equal(f0, f2) and r0.tobytes() == r2.tobytes() and torch.equal(l0.view(torch.int32), l2.view(torch.int32))
    assert not h2.view(np.uint8).any()
    assert [int(v) for v in r0["success"][:5]] == [1, 0, 0, 1, 1] and int(r0["candidates"][2]) == 26
    pool.close()
