"""RxEngine.mcdpsk_stream (ria_gpu_mcdpsk_stream_batch) on the GPU: against RxEngine.rx_stream where it adds nothing (byte
equality), against the composition ria_amd.acquire.mcdpsk_link_stream and the CPU restatement
tests/mcdpsk_stream_restatement.link_stream where it does - the chase pool on the audio clock, channel interleaving, the wait
at a found sync carried from call to call - and what it refuses.  The recordings and their claims are those
tests/test_mcdpsk_stream_cpu.py asserts on the restatement; nothing is tuned here.  No test provokes a fault: the refused calls
are argument errors returned before any launch, or found by the up-front check."""
import ctypes as C

import numpy as np
import pytest
import torch

import mcdpsk_stream_restatement as MS
import mcdpsk_window_restatement as WR
from mcdpsk_acquire_restatement import encode_frame, data_frame, frame_len, oracle
from mcdpsk_ci_restatement import interleave_bytes
from mcdpsk_harq_restatement import STATS, ChaseCache, cache_snapshot
from test_gpu_rx_stream import _stack, zc_recording
from test_gpu_stream_call import handshake_recording

pytestmark = pytest.mark.gpu
F = np.float32
G20 = dict(carriers=20, modulation="DQPSK", spreading=1)
G10 = dict(carriers=10, modulation="DBPSK", spreading=1)
NEED = 4                         # RIA_STREAM_WINDOW_NEED_SAMPLES


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def bits(v):
    return np.asarray(v, F).view(np.uint32)


class Rig:
    def __init__(self):
        from ria_amd.engine import RxEngine
        self.e = RxEngine("DQPSK", "R1_4", max_batch=8)
        self.O = O = oracle()
        self.harq, self.harq_frame, self.harq_at = MS.harq_recording(O, **MS.HARQ_PIN)
        self.clean, self.clean_sent, self.clean_at = MS.clean_recording(O, [5, 6])
        self.zc = [zc_recording(O, 7)[0], zc_recording(O, 8)[0]]
        self.chirp = [handshake_recording(O, 9)[0]]
        self._cut = {}

    def cut_case(self, name):
        """(recording, sent, first samples, cut, parameters, engine keywords, restatement keywords) of a CUT_CASES entry"""
        if name not in self._cut:
            K = MS.CUT_CASES[name]
            x, sent, at = MS.clean_recording(self.O, [5, 6], carriers=K["carriers"], bps=K["bps"], n_payload=K["n_payload"])
            kw = dict(carriers=K["carriers"], modulation={1: "DBPSK", 2: "DQPSK"}[K["bps"]], spreading=1)
            self._cut[name] = (x, sent, at, at[0] + MS.ZC_LEN + K["cut_behind_sync"], K, kw, dict(carriers=K["carriers"], bps=K["bps"], spreading=1))
        return self._cut[name]

    def stack(self, recs):
        return _stack(recs, self.e.device)


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.e.close()


def check_against_cpu(out, cpu, streams=None):
    """the call's records (state, results, events, frames, harq) against link_stream's (state, closed, events)"""
    st, res, ev, frames, harq = out
    cst, cclosed, cev = cpu
    frames = frames.cpu().numpy() if torch.is_tensor(frames) else frames
    for s in (range(len(cev)) if streams is None else streams):
        assert res["n_events"][s] == len(cev[s]) and res["closed"][s] == cclosed[s], (s, res[s], cclosed[s], MS.show(cev[s]))
        for k, c in enumerate(cev[s]):
            g = ev[s, k]
            for f in MS.EVENT_FIELDS:
                assert int(g[f]) == int(c[f]), (s, k, f, g[f], c[f])
            for f in MS.EVENT_WORDS:
                assert bits(g[f]) == bits(c[f]), (s, k, f, g[f], c[f])
            assert (frames[s, k, :int(g["frame_bytes"])].tobytes() if g["delivered"] else None) == c["frame"], (s, k)
            for f in MS.HARQ_FIELDS:
                assert int(harq[s, k][f]) == int(c["harq"][f]), (s, k, f, harq[s, k], c["harq"])
        assert st[s:s + 1].tobytes() == cst[s:s + 1].tobytes(), (s, st[s], cst[s])


def check_against_composition(out, comp):
    st, res, ev, frames, harq = out
    cst, cclosed, cev, cframes, charq = comp
    assert same_bytes(st, cst), (st, cst)
    assert np.array_equal(res["closed"], cclosed)
    assert same_bytes(ev, cev), (ev, cev)
    assert np.array_equal(frames.cpu().numpy(), cframes)
    for f in ("seq", "valid", "entry", "src_hash", "dst_hash", "stored_mask", "sum_mask", "recovered_mask", "max_combine"):
        assert np.array_equal(harq[f], charq[f]), f


def check_cache(pool, cache_id, cache):
    """ria_gpu_chase_stats and _export of one cache against the Python ChaseCache"""
    stats = pool.stats(cache_id)
    assert stats == {k: cache.stats[k] for k in STATS}, (cache_id, stats, cache.stats)
    ent, sums = pool.export(cache_id)
    snap = cache_snapshot(cache)
    assert len(ent) == len(snap)
    for i, e in enumerate(ent):
        w = snap[int(e["seq"]), int(e["src_hash"]), int(e["dst_hash"])]
        assert (int(e["total_cw"]), int(e["frame_type"]), int(e["last_access_ms"])) == (w["total_cw"], w["frame_type"], w["last_access"] & MS.M64)
        assert list(e["combine_count"]) == w["count"] and list(e["decoded"]) == w["decoded"] and list(e["has_sum"]) == w["has_sum"]
        assert same_bytes(sums[i], w["sums"])


# ---- 1. nothing added: byte equality with ria_gpu_rx_stream_batch
@pytest.mark.parametrize("feed_step", [0, 4800])
@pytest.mark.parametrize("name", ["zc", "chirp"])
def test_without_pool_flag_or_pending_equals_rx_stream(rig, name, feed_step):
    e = rig.e
    recs, mode, kw = (rig.zc, "MCDPSK_ZC", dict(carriers=10, modulation="DQPSK", spreading=1)) if name == "zc" else (rig.chirp, "MCDPSK_CHIRP", G10)
    x, lens = rig.stack(recs)
    st0, res0, ev0, fr0 = e.rx_stream(x, lens, mode, feed_step=feed_step, max_events=8, **kw)
    st, res, ev, fr, hq = e.mcdpsk_stream(x, lens, mode, feed_step=feed_step, max_events=8, **kw)
    if (name, feed_step) != ("zc", 0):      # a ZC recording that "has all arrived" is a backlog: the catch-up jumps to its end (rx_stream's note)
        assert res0["n_events"].sum() >= 3
    search = np.zeros(len(lens), e.SEARCH_STATE)
    for f in e.SEARCH_STATE.names:
        search[f] = st[f]
    assert same_bytes(search, st0) and same_bytes(res, res0) and same_bytes(ev, ev0) and np.array_equal(fr.cpu().numpy(), fr0.cpu().numpy())
    assert not hq.view(np.uint8).any()
    pend = res["closed"] == NEED
    assert not any(st[f][~pend].any() for f in MS.PENDING)
    if name == "chirp" and feed_step == 0:       # and a capture cut inside the CONNECT: the same records, and the wait in the state
        k = int(np.flatnonzero(ev0["frame_bytes"][0] > 20)[0])
        cut = int(ev0["sync_position"][0, k]) + frame_len(3, 10, 1, 1) - 20001
        st0, res0, ev0, fr0 = e.rx_stream(x[:, :cut].contiguous(), [cut], mode, max_events=8, **kw)
        st, res, ev, fr, hq = e.mcdpsk_stream(x[:, :cut].contiguous(), [cut], mode, max_events=8, **kw)
        assert res0["closed"][0] == NEED and same_bytes(res, res0) and same_bytes(ev, ev0)
        last = ev[0, res["n_events"][0] - 1]
        assert st["pending_total_cw"][0] == last["pending_total_cw"] > 0 and st["need_samples"][0] == last["need_samples"]
        assert st["pend_sync_position"][0] == last["sync_position"] and st["pend_search_start"][0] == last["search_start"]


# ---- 2. the HARQ recording: the call, the composition and the CPU restatement
def harq_streams(rig):
    """the HARQ recording on cache 0, the same recording with the cache off, a clean recording on cache 1, and the HARQ
    recording cut between its two receptions on cache 2 (its failed codeword stays stored)"""
    recs = [rig.harq, rig.harq, rig.clean, rig.harq[:rig.harq_at[1] - 1000]]
    return recs, np.array([0, -1, 1, 2], np.int32)


def test_harq_recording_equals_composition_and_restatement(rig):
    from ria_amd.acquire import LINK_STREAM_COUNTERS, link_stream_tally, mcdpsk_link_stream
    e = rig.e
    recs, ids = harq_streams(rig)
    x, lens = rig.stack(recs)
    caches = [ChaseCache() for _ in range(3)]
    cpu = MS.link_stream(rig.O, recs, "MCDPSK_ZC", feed_step=4800, max_events=4, caches=caches, cache_id=ids, t0_ms=[1000, 2000, 3000, 4000], **MS.GEOM)
    # the claims (tests/test_mcdpsk_stream_cpu.py asserts them one by one): recovery with the cache, none without
    assert [ev["success"] for ev in cpu[2][0]] == [0, 1] and cpu[2][0][1]["frame"] == rig.harq_frame and cpu[2][0][1]["harq"]["recovered_mask"] == 2
    assert [ev["success"] for ev in cpu[2][1]] == [0, 0] and [ev["success"] for ev in cpu[2][3]] == [0] and caches[2].size() == 1
    pool, pool2 = e.chase_pool(3), e.chase_pool(3)
    try:
        out = e.mcdpsk_stream(x, lens, "MCDPSK_ZC", feed_step=4800, max_events=4, chase=pool, cache_id=ids, t0_ms=[1000, 2000, 3000, 4000], **G20)
        check_against_cpu(out, cpu)
        for c in range(3):
            check_cache(pool, c, caches[c])
        comp = mcdpsk_link_stream(e, x, lens, "MCDPSK_ZC", feed_step=4800, max_events=4, chase=pool2, cache_id=ids, t0_ms=[1000, 2000, 3000, 4000], **G20)
        check_against_composition(out, comp)
        for c in range(3):
            check_cache(pool2, c, caches[c])
        # cache id -1: that stream's records are the no-pool call's
        alone = e.mcdpsk_stream(x[1:2].contiguous(), lens[1:2], "MCDPSK_ZC", feed_step=4800, max_events=4, **G20)
        assert same_bytes(alone[0], out[0][1:2]) and same_bytes(alone[2], out[2][1:2]) and not out[4][1].view(np.uint8).any()
        tally = dict(zip(LINK_STREAM_COUNTERS, link_stream_tally(out[2], out[4])))
        assert tally["outcome_decoded"] == 7 and tally["delivered"] == 7 and tally["recovered_by_sum"] == 1 and tally["stores"] == 3 and tally["combines"] == 1
    finally:
        pool.close()
        pool2.close()


# ---- 3. TTL through the audio clock
def test_ttl_runs_on_the_audio_clock(rig):
    e = rig.e
    x, lens = rig.stack([rig.harq])
    sync = [a + MS.ZC_LEN for a in rig.harq_at]
    gap_ms = sync[1] * 1000 // 48000 - sync[0] * 1000 // 48000            # from the two receptions' sync positions
    assert 0 < gap_ms < 30000
    for ttl, t0, expired, recovered in ((gap_ms - 1, 0, 1, 0), (gap_ms, 0, 0, 1), (30000, 0, 0, 1), (gap_ms, 2 ** 64 - 1 - sync[0] * 1000 // 48000, 0, 1),
                                        (gap_ms - 1, 2 ** 64 - 1 - sync[0] * 1000 // 48000, 1, 0)):
        cache = ChaseCache(ttl_ms=ttl)
        cpu = MS.link_stream(rig.O, [rig.harq], "MCDPSK_ZC", feed_step=4800, max_events=4, caches=[cache], t0_ms=t0, **MS.GEOM)
        assert (cache.stats["entries_expired"], cache.stats["recoveries"]) == (expired, recovered), (ttl, t0, cache.stats)
        pool = e.chase_pool(1, ttl_ms=ttl)
        try:
            out = e.mcdpsk_stream(x, lens, "MCDPSK_ZC", feed_step=4800, max_events=4, chase=pool, t0_ms=np.array([t0], np.uint64), **G20)
            assert [int(ev["sync_position"]) for ev in out[2][0, :2]] == sync
            check_against_cpu(out, cpu)
            check_cache(pool, 0, cache)
            assert (pool.stats(0)["entries_expired"], pool.stats(0)["recoveries"], int(out[2][0, 1]["success"])) == (expired, recovered, recovered)
        finally:
            pool.close()


# ---- 4. channel interleaving
@pytest.mark.parametrize("B", [216, 648])
def test_channel_interleaving(rig, B):
    e, O = rig.e, rig.O
    # the transmitter: the engine's interleaver on the coded bytes (the restatement's, byte for byte), then the waveform
    frame = data_frame(MS.DATA, 5, MS.payload3(5))
    coded = encode_frame(frame)
    tx = e.mcdpsk_interleave(coded, B).cpu().numpy()
    assert np.array_equal(tx, interleave_bytes(coded, B)) and not np.array_equal(tx, coded)
    x, sent, at = MS.clean_recording(O, [5, 6], B=B)
    first = x[:at[1] - 1000].copy()
    a, b = MS.cw_span(1)
    first[at[0] + a:at[0] + b] += (np.random.default_rng(MS.HARQ_PIN["seeds"][0]).standard_normal(b - a) * MS.HARQ_PIN["sigma"]).astype(F)
    recs = [x, first]
    xs, lens = rig.stack(recs)
    with_flag = MS.link_stream(O, recs, "MCDPSK_ZC", feed_step=4800, max_events=4, B=B, caches=[ChaseCache(), ChaseCache()], **MS.GEOM)
    assert [ev["frame"] for ev in with_flag[2][0]] == sent
    assert with_flag[2][1][0]["harq"]["stored_mask"] == 2          # the noisy codeword fails and is stored: the pool holds a sum to look at
    caches = [ChaseCache(), ChaseCache()]
    cpu = MS.link_stream(O, recs, "MCDPSK_ZC", feed_step=4800, max_events=4, B=B, caches=caches, **MS.GEOM)
    pool = e.chase_pool(2)
    try:
        out = e.mcdpsk_stream(xs, lens, "MCDPSK_ZC", feed_step=4800, max_events=4, chase=pool, channel_interleave=True, interleaver_bits=B, **G20)
        check_against_cpu(out, cpu)
        for c in range(2):
            check_cache(pool, c, caches[c])                         # the stored sum is the raw soft bits, not the de-interleaved ones
        assert pool.export(1)[0]["has_sum"][0][1] == 1
    finally:
        pool.close()
    out = e.mcdpsk_stream(xs, lens, "MCDPSK_ZC", feed_step=4800, max_events=4, **G20)
    check_against_cpu(out, MS.link_stream(O, recs, "MCDPSK_ZC", feed_step=4800, max_events=4, **MS.GEOM))
    assert not out[2]["success"].any()


# ---- 5. re-entry
@pytest.mark.parametrize("case", list(MS.CUT_CASES))
def test_reentry_of_a_cut_capture(rig, case):
    e, O = rig.e, rig.O
    x, sent, at, cut, K, kw, ckw = rig.cut_case(case)
    need = frame_len(K["frame_cw"], K["carriers"], K["bps"], 1)
    dev = lambda r: rig.stack([r])
    whole = e.mcdpsk_stream(*dev(x), "MCDPSK_ZC", feed_step=4800, max_events=4, **kw)
    cpu_whole = MS.link_stream(O, [x], "MCDPSK_ZC", feed_step=4800, max_events=4, **ckw)
    check_against_cpu(whole, cpu_whole)
    assert [ev["frame"] for ev in cpu_whole[2][0]] == sent
    # call 1: the wait is written as the restatement writes it
    one = e.mcdpsk_stream(*dev(x[:cut]), "MCDPSK_ZC", feed_step=4800, max_events=4, **kw)
    cpu_one = MS.link_stream(O, [x[:cut]], "MCDPSK_ZC", feed_step=4800, max_events=4, **ckw)
    check_against_cpu(one, cpu_one)
    st1 = one[0]
    assert one[1]["closed"][0] == NEED and st1["pending_total_cw"][0] == K["frame_cw"] and st1["need_samples"][0] == need
    assert st1["pend_sync_position"][0] == at[0] + MS.ZC_LEN
    # still one sample short: no event, the 64 bytes untouched
    short = e.mcdpsk_stream(*dev(x[:at[0] + MS.ZC_LEN + need - 1]), "MCDPSK_ZC", state=st1, feed_step=4800, max_events=4, **kw)
    assert short[1]["closed"][0] == NEED and short[1]["n_events"][0] == 0 and short[0].tobytes() == st1.tobytes()
    assert not short[2].view(np.uint8).any() and not short[3].any()
    # exactly enough, and the whole capture
    exact = e.mcdpsk_stream(*dev(x[:at[0] + MS.ZC_LEN + need]), "MCDPSK_ZC", state=st1, feed_step=4800, max_events=4, **kw)
    assert exact[1]["n_events"][0] == 1 and exact[2][0, 0]["success"] == 1 and exact[3][0, 0, :len(sent[0])].cpu().numpy().tobytes() == sent[0]
    assert exact[2][0, 0]["window_len"] == at[0] + MS.ZC_LEN + need - st1["pend_search_start"][0]
    two = e.mcdpsk_stream(*dev(x), "MCDPSK_ZC", state=st1, feed_step=4800, max_events=4, **kw)
    check_against_cpu(two, MS.link_stream(O, [x], "MCDPSK_ZC", state=cpu_one[0], feed_step=4800, max_events=4, **ckw))
    assert two[0].tobytes() == whole[0].tobytes() and not any(two[0][f].any() for f in MS.PENDING)
    assert two[1]["n_events"][0] == whole[1]["n_events"][0] == 2
    for f in ("sync_position", "outcome", "next_pos", "frame_bytes", "delivered", "success", "codewords_ok", "codewords_failed", "frame_type"):
        assert np.array_equal(two[2][f], whole[2][f]), f
    assert np.array_equal(two[3].cpu().numpy(), whole[3].cpu().numpy())
    assert bits(two[2][0, 0]["correlation"]) == bits(st1["pend_correlation"][0]) and bits(two[2][0, 0]["snr_db"]) == bits(st1["snr_hint"][0])
    # the caller gives up: the stream searches on
    gave_up = st1.copy()
    gave_up["pending_total_cw"] = 0
    on = e.mcdpsk_stream(*dev(x), "MCDPSK_ZC", state=gave_up, feed_step=4800, max_events=4, **kw)
    cpu_state = cpu_one[0].copy()
    cpu_state["pending_total_cw"] = 0
    check_against_cpu(on, MS.link_stream(O, [x], "MCDPSK_ZC", state=cpu_state, feed_step=4800, max_events=4, **ckw))
    assert on[1]["search_legs"][0] >= 1 and on[1]["n_events"][0] >= 1


def test_reentry_in_a_mixed_batch(rig):
    """one call with a stream whose wait is over, one still a sample short, one that searches, and one with a state made by
    hand - pending_total_cw 12, so its re-entered window reaches past `full`: a second window length in the pending round, rows
    of their own stride, and RIA_MWIN_TOO_LONG - against the restatement, against each stream alone, and permuted"""
    e, O = rig.e, rig.O
    x, sent, at, cut, K, kw, ckw = rig.cut_case("c20_dqpsk_6cw")
    sync, need = at[0] + MS.ZC_LEN, frame_len(6, 20, 2, 1)
    st1 = e.mcdpsk_stream(*rig.stack([x[:cut]]), "MCDPSK_ZC", feed_step=4800, max_events=4, **kw)[0]
    assert st1["pending_total_cw"][0] == 6
    long_wait = st1.copy()
    long_wait["pending_total_cw"], long_wait["need_samples"] = 12, frame_len(12, 20, 2, 1)
    full = 31120 + frame_len(8, 20, 2, 1)
    assert sync - int(st1["pend_search_start"][0]) + frame_len(12, 20, 2, 1) > full and sync + frame_len(12, 20, 2, 1) <= len(x)
    recs = [x, x[:sync + need - 1], x, x]
    state = np.concatenate([st1, st1, e.mcdpsk_stream_state(1, fed=0), long_wait])
    xs, lens = rig.stack(recs)
    cpu = MS.link_stream(O, recs, "MCDPSK_ZC", state=state, feed_step=4800, max_events=4, **ckw)
    assert [len(v) for v in cpu[2]] == [2, 0, 2, 2] and cpu[1][1] == NEED
    assert cpu[2][3][0]["outcome"] == WR.TOO_LONG and cpu[2][3][0]["window_len"] > full and cpu[2][0][0]["window_len"] == full
    out = e.mcdpsk_stream(xs, lens, "MCDPSK_ZC", state=state, feed_step=4800, max_events=4, **kw)
    check_against_cpu(out, cpu)
    assert out[0][1:2].tobytes() == st1.tobytes()
    for s in range(4):
        one = e.mcdpsk_stream(xs[s:s + 1].contiguous(), lens[s:s + 1], "MCDPSK_ZC", state=state[s:s + 1], feed_step=4800, max_events=4, **kw)
        assert all(same_bytes(a, b[s:s + 1]) for a, b in zip(one[:3], out[:3])) and np.array_equal(one[3].cpu().numpy(), out[3].cpu().numpy()[s:s + 1])
    perm = np.array([3, 1, 0, 2])
    got = e.mcdpsk_stream(xs[torch.as_tensor(perm, device=xs.device)].contiguous(), lens[perm], "MCDPSK_ZC", state=state[perm], feed_step=4800,
                          max_events=4, **kw)
    assert all(same_bytes(a, b[perm]) for a, b in zip(got[:3], out[:3])) and np.array_equal(got[3].cpu().numpy(), out[3].cpu().numpy()[perm])


# ---- 6. re-entry with a pool: the failed codeword is stored once
def test_reentry_with_a_pool_stores_once(rig):
    e, O = rig.e, rig.O
    x, sent, at, cut, K, kw, ckw = rig.cut_case("c20_dqpsk_6cw")
    x = x[:at[1] - 1000].copy()
    a, b = MS.cw_span(1)
    # twice the HARQ recording's level: codeword 1 of this frame only has to fail (asserted on the restatement below)
    x[at[0] + a:at[0] + b] += (np.random.default_rng(MS.HARQ_PIN["seeds"][0]).standard_normal(b - a) * 2 * MS.HARQ_PIN["sigma"]).astype(F)
    cache = ChaseCache()
    cpu1 = MS.link_stream(O, [x[:cut]], "MCDPSK_ZC", feed_step=4800, max_events=4, caches=[cache], t0_ms=77, **ckw)
    assert cpu1[1][0] == NEED and cache.stats["stores"] == 0
    cpu2 = MS.link_stream(O, [x], "MCDPSK_ZC", state=cpu1[0], feed_step=4800, max_events=4, caches=[cache], t0_ms=77, **ckw)
    assert cache.stats["stores"] == 1 and cpu2[2][0][0]["harq"]["stored_mask"] == 2 and cpu2[2][0][0]["codewords_failed"] == 1
    pool = e.chase_pool(1)
    try:
        one = e.mcdpsk_stream(*rig.stack([x[:cut]]), "MCDPSK_ZC", feed_step=4800, max_events=4, chase=pool, t0_ms=77, **kw)
        check_against_cpu(one, cpu1)
        assert pool.stats(0)["stores"] == 0
        two = e.mcdpsk_stream(*rig.stack([x]), "MCDPSK_ZC", state=one[0], feed_step=4800, max_events=4, chase=pool, t0_ms=77, **kw)
        check_against_cpu(two, cpu2)
        check_cache(pool, 0, cache)
        assert pool.stats(0)["stores"] == 1
    finally:
        pool.close()


# ---- 7. and 8.: raw calls on outputs filled with a sentinel
def raw_call(e, x, lens_in, state_in, n_events, pool=None, ids=None, t0=None, fill=0xA5, geom=G20, **over):
    """ria_gpu_mcdpsk_stream_batch on outputs filled with `fill` -> (rc, state, results, events, frames, harq) as uint8 arrays"""
    from ria_amd import capi
    from ria_amd.engine import _ptr
    n, stride = x.shape
    dev = e.device
    lens_d = torch.from_numpy(np.asarray(lens_in, np.int32)).to(dev)
    st_d = torch.from_numpy(np.ascontiguousarray(state_in, e.MCSTREAM_STATE).view(np.uint8).reshape(-1, 64).copy()).to(dev)
    res_d = torch.full((max(n, 1), 64), fill, dtype=torch.uint8, device=dev)
    ev_d = torch.full((max(n, 1), n_events, 64), fill, dtype=torch.uint8, device=dev)
    fr_d = torch.full((max(n, 1), n_events, 320), fill, dtype=torch.uint8, device=dev)
    hq_d = torch.full((max(n, 1), n_events, 32), fill, dtype=torch.uint8, device=dev)
    ids_d = torch.from_numpy(np.asarray(np.arange(n) if ids is None else ids, np.int32)).to(dev)
    t0_d = torch.from_numpy(np.asarray(np.zeros(n) if t0 is None else t0, np.uint64).view(np.int64).copy()).to(dev)
    cfg = capi.McdpskConfig(geom["carriers"], {"DBPSK": 1, "DQPSK": 2}[geom["modulation"]], geom["spreading"], 0)
    a = dict(h=e.h, mode=capi.SEARCH_MODE["MCDPSK_ZC"], flags=0, window_flags=0, bits=0, cfg=C.byref(cfg), samples=_ptr(x), stride=stride,
             lens=_ptr(lens_d), n=n, state=_ptr(st_d), feed_step=4800, max_invocations=1 << 20, max_events=n_events,
             pool=pool.p if pool is not None else None, ids=_ptr(ids_d), t0=_ptr(t0_d), events=_ptr(ev_d), frames=_ptr(fr_d), frame_row=320,
             harq=_ptr(hq_d), results=_ptr(res_d))
    a.update(over)
    rc = e.lib.ria_gpu_mcdpsk_stream_batch(*a.values(), None)
    torch.cuda.synchronize()
    return rc, st_d.cpu().numpy(), res_d.cpu().numpy(), ev_d.cpu().numpy(), fr_d.cpu().numpy(), hq_d.cpu().numpy()


def test_refused_calls_leave_everything_untouched(rig):
    from ria_amd import capi
    from ria_amd.engine import RxEngine
    e = rig.e
    # two streams whose windows fall into different length groups of the first round: the recording whole and cut short
    first = int(MS.link_stream(rig.O, [rig.clean], "MCDPSK_ZC", feed_step=4800, max_events=1, **MS.GEOM)[2][0][0]["search_start"])
    full = 31120 + frame_len(8, 20, 2, 1)
    cut = first + full - 5000
    assert rig.clean_at[0] + MS.ZC_LEN + frame_len(3, 20, 2, 1) < cut < len(rig.clean)
    x, lens = rig.stack([rig.clean, rig.clean[:cut]])
    fresh = e.mcdpsk_stream_state(2, fed=0)
    pool = e.chase_pool(2)
    other = RxEngine("DQPSK", "R1_4", max_batch=8)
    foreign = other.chase_pool(2)
    half = RxEngine("DQPSK", "R1_2", max_batch=8)
    try:
        # the claim: with distinct ids the two streams do run in different groups of one round
        ok = raw_call(e, x, lens, fresh, 4, pool=pool, ids=[0, 1])
        ev = ok[3].view(e.STREAM_EVENT).reshape(2, 4)
        assert ok[0] == 0 and ev["window_len"][0, 0] == full and 0 < ev["window_len"][1, 0] < full
        pool.clear()
        before = [pool.stats(c) for c in range(2)]
        foreign_before = [foreign.stats(c) for c in range(2)]
        pend = fresh.copy()
        pend["pending_total_cw"][1] = 256
        neg = fresh.copy()
        neg["pending_total_cw"][0], neg["need_samples"][0], neg["pend_search_start"][0], neg["pend_sync_position"][0] = 3, -1, 0, 100
        outside = fresh.copy()
        outside["pending_total_cw"][1], outside["need_samples"][1], outside["pend_search_start"][1], outside["pend_sync_position"][1] = 3, 30720, 0, cut
        bad = [("duplicate ids", dict(ids=[0, 0]), fresh), ("id >= n_caches", dict(ids=[0, 2]), fresh), ("foreign pool", dict(pool=foreign), fresh),
               ("pending 256", {}, pend), ("negative need_samples", {}, neg), ("sync outside the capture", {}, outside),
               ("OFDM mode", dict(mode=capi.SEARCH_MODE["OFDM_LTS"]), fresh), ("unknown window flag", dict(window_flags=1), fresh),
               ("interleaver_bits 0", dict(window_flags=capi.MACQ_CHANNEL_INTERLEAVE, bits=0), fresh), ("frame_row", dict(frame_row=319), fresh),
               ("handle not at R1/4", dict(h=half.h, pool=None), fresh)]
        for what, over, state in bad:
            kw = dict(pool=pool)
            kw.update({k: over.pop(k) for k in ("pool", "ids") if k in over})
            out = raw_call(e, x, lens, state, 4, **kw, **over)
            assert out[0] == -1, what
            assert all((o == 0xA5).all() for o in out[2:]) and same_bytes(out[1].reshape(-1), state), what
            assert [pool.stats(c) for c in range(2)] == before and all(len(pool.export(c)[0]) == 0 for c in range(2)), what
            assert [foreign.stats(c) for c in range(2)] == foreign_before and all(len(foreign.export(c)[0]) == 0 for c in range(2)), what
            err = (half if what == "handle not at R1/4" else e).lib.ria_gpu_last_error(half.h if what == "handle not at R1/4" else e.h).decode()
            assert err.startswith("ria_gpu_mcdpsk_stream_batch: "), (what, err)
        # negative ids may repeat; n_streams == 0 is RIA_OK and writes nothing
        out = raw_call(e, x, lens, fresh, 4, pool=pool, ids=[-1, -7])
        assert out[0] == 0 and [pool.stats(c) for c in range(2)] == before
        out = raw_call(e, x, lens, fresh, 4, pool=pool, n=0)
        assert out[0] == 0 and all((o == 0xA5).all() for o in out[2:]) and same_bytes(out[1].reshape(-1), fresh)
        with pytest.raises(Exception, match="ria_gpu_mcdpsk_stream_host"):
            e.mcdpsk_stream_host(rig.clean, "MCDPSK_ZC", max_events=0, **G20)
        with pytest.raises(Exception, match="ria_gpu_mcdpsk_stream_host"):
            e.mcdpsk_stream_host(rig.clean, "OFDM_LTS", **G20)
    finally:
        foreign.close()
        other.close()
        half.close()
        pool.close()


def test_every_output_row_is_written(rig):
    """outputs filled with 0xA5 first: every record comes back written - events, payload rows and chase records past a
    stream's events zero, payload bytes past frame_bytes zero"""
    e = rig.e
    recs, ids = harq_streams(rig)
    x, lens = rig.stack(recs)
    pool = e.chase_pool(3)
    try:
        rc, st, res, ev, fr, hq = raw_call(e, x, lens, e.mcdpsk_stream_state(4, fed=0), 5, pool=pool, ids=ids)
    finally:
        pool.close()
    assert rc == 0
    res, ev, hq = res.view(e.STREAM_RESULT).reshape(-1), ev.view(e.STREAM_EVENT).reshape(4, 5), hq.view(e.HARQ_RESULT).reshape(4, 5)
    assert list(res["n_events"]) == [2, 2, 2, 1] and not (res["reserved"] != 0).any()
    for s in range(4):
        for k in range(5):
            live = k < res["n_events"][s]
            nbytes = int(ev["frame_bytes"][s, k]) if live and ev["delivered"][s, k] else 0
            assert not fr[s, k, nbytes:].any(), (s, k)
            if not live:
                assert not ev[s, k:k + 1].view(np.uint8).any() and not hq[s, k:k + 1].view(np.uint8).any(), (s, k)
    assert hq["valid"][0, 0] == 1 and not hq[1].view(np.uint8).any() and not (hq["reserved"] != 0).any()


def test_forms_of_the_call_agree(rig):
    """a ragged batch, permuted, with a search chunk of one, one event per call and continued, and the host form: the records of
    the plain call"""
    e = rig.e
    recs, ids = harq_streams(rig)
    recs = recs + [np.zeros(0, F), (np.random.default_rng(3).standard_normal(50001) * 0.012).astype(F), rig.clean[3:][:(len(rig.clean) - 12348) | 1]]
    ids = np.concatenate([ids, [3, 4, 5]]).astype(np.int32)
    t0 = np.arange(7, dtype=np.uint64) * np.uint64(1000)
    x, lens = rig.stack(recs)
    n = len(recs)
    assert len(set(lens)) == 5 and lens[-1] % 2 == 1

    def run(x, lens, ids, t0, **more):
        pool = e.chase_pool(6)
        try:
            out = e.mcdpsk_stream(x, lens, "MCDPSK_ZC", feed_step=4800, chase=pool, cache_id=ids, t0_ms=t0, **more, **G20)
            return out, [(pool.stats(c), [a.tobytes() for a in pool.export(c)]) for c in range(6)]
        finally:
            pool.close()

    want, want_pool = run(x, lens, ids, t0, max_events=4)
    assert list(want[1]["n_events"]) == [2, 2, 2, 1, 0, 0, 2] and want[2][0, 1]["success"] == 1
    # a permutation of the streams permutes the records
    perm = np.array([6, 2, 4, 0, 3, 5, 1])
    got, got_pool = run(x[torch.as_tensor(perm, device=x.device)].contiguous(), lens[perm], ids[perm], t0[perm], max_events=4)
    for a, b in zip(got[:3], want[:3]):
        assert same_bytes(a, b[perm])
    assert np.array_equal(got[3].cpu().numpy(), want[3].cpu().numpy()[perm]) and same_bytes(got[4], want[4][perm]) and got_pool == want_pool
    # a search chunk of one
    e.set_search_chunk(1)
    try:
        got, got_pool = run(x, lens, ids, t0, max_events=4)
    finally:
        e.set_search_chunk(0)
    assert all(same_bytes(a, b) for a, b in zip(got[:3], want[:3])) and same_bytes(got[4], want[4]) and got_pool == want_pool
    # one event per call, continued with the returned state
    pool = e.chase_pool(6)
    try:
        state, live = e.mcdpsk_stream_state(n, fed=0), np.arange(n)
        events, harq, calls = [[] for _ in range(n)], [[] for _ in range(n)], 0
        closed = np.zeros(n, np.int64)
        while len(live):
            calls += 1
            assert calls < 10
            st, res, ev, fr, hq = e.mcdpsk_stream(x[torch.as_tensor(live, device=x.device)].contiguous(), lens[live], "MCDPSK_ZC", state=state[live],
                                                  feed_step=4800, max_events=1, chase=pool, cache_id=ids[live], t0_ms=t0[live], **G20)
            state[live], closed[live] = st, res["closed"]
            for i, s in enumerate(live):
                events[s] += [ev[i, k].tobytes() for k in range(res["n_events"][i])]
                harq[s] += [hq[i, k].tobytes() for k in range(res["n_events"][i])]
            live = live[res["closed"] == 5]                                  # RIA_STREAM_EVENTS_FULL
        assert calls == 3 and same_bytes(state, want[0]) and np.array_equal(closed, want[1]["closed"])
        for s in range(n):
            assert events[s] == [want[2][s, k].tobytes() for k in range(want[1]["n_events"][s])]
            assert harq[s] == [want[4][s, k].tobytes() for k in range(want[1]["n_events"][s])]
        assert [(pool.stats(c), [a.tobytes() for a in pool.export(c)]) for c in range(6)] == want_pool
    finally:
        pool.close()
    # the host form, stream by stream
    pool = e.chase_pool(6)
    try:
        for s in (0, 3, 6):
            h = e.mcdpsk_stream_host(recs[s], "MCDPSK_ZC", feed_step=4800, max_events=4, chase=pool, cache_id=int(ids[s]), t0_ms=int(t0[s]), **G20)
            assert same_bytes(h[0], want[0][s:s + 1]) and same_bytes(h[1], want[1][s:s + 1]) and same_bytes(h[2], want[2][s:s + 1])
            assert np.array_equal(h[3], want[3].cpu().numpy()[s:s + 1]) and same_bytes(h[4], want[4][s:s + 1])
        assert [(pool.stats(c), [a.tobytes() for a in pool.export(c)]) for c in (0, 2)] == [want_pool[0], want_pool[2]]
    finally:
        pool.close()
