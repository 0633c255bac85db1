"""RxEngine.mcdpsk_ring / mcdpsk_ring_host (ria_gpu_mcdpsk_ring_batch, ria_gpu_mcdpsk_ring_host) on the GPU: against
RxEngine.rx_ring where it adds nothing and against RxEngine.mcdpsk_stream on recordings that never wrap (byte equality);
against the composition ria_amd.acquire.mcdpsk_link_ring and the CPU restatement tests/mcdpsk_ring_restatement.link_ring on
recordings a little over one ring long - HARQ across the wrap on the absolute audio clock, re-entry across the wrap, channel
interleaving behind it, the ring call's three recordings with a pool; a mixed batch against each stream alone; max_events = 1
repeated and the host form; every output row written; and what it refuses.  The recordings and their claims are those
tests/test_mcdpsk_ring_cpu.py asserts on the restatement; nothing is tuned here.  No test provokes a fault: the refused calls
are argument errors returned before any launch, or found by the up-front check, which reads states and lengths only."""
import ctypes as C

import numpy as np
import pytest
import torch

import mcdpsk_ring_restatement as MR
import mcdpsk_stream_restatement as MS
import mcdpsk_window_restatement as WR
from mcdpsk_acquire_restatement import frame_len, oracle
from mcdpsk_harq_restatement import ChaseCache
from test_gpu_mcdpsk_stream import G10, G20, bits, check_cache, same_bytes
from test_gpu_ring_stream import recordings
from test_gpu_rx_stream import _stack, zc_recording

pytestmark = pytest.mark.gpu
F = np.float32
RING = MR.RING
NEED, FULL_EVENTS = 4, 5         # RIA_STREAM_WINDOW_NEED_SAMPLES, RIA_STREAM_EVENTS_FULL
COUNTERS = ("overflow_dropped", "overflows", "drift_snaps", "cursor_inits")
SET4 = {"zc": ("MCDPSK_ZC", dict(carriers=10, modulation="DQPSK", spreading=1), dict(carriers=10, bps=2, spreading=1)),
        "chirp": ("MCDPSK_CHIRP", G10, dict(carriers=10, bps=1, spreading=1))}


class Rig:
    def __init__(self):
        from ria_amd.engine import RxEngine
        self.e = RxEngine("DQPSK", "R1_4", max_batch=8)
        self.O = O = oracle()
        self.harq, self.harq_frame, self.harq_at = MR.harq_recording(O)
        self.short_harq, _, self.short_harq_at = MS.harq_recording(O, **MS.HARQ_PIN)
        self.clean, self.clean_sent, self.clean_at = MS.clean_recording(O, [5, 6])
        self.set4 = {name: recordings(O, name) for name in SET4}
        self._re = {}

    def reentry(self, where):
        if where not in self._re:
            self._re[where] = MR.reentry_recording(self.O, where)
        return self._re[where]

    def stack(self, recs):
        return _stack(recs, self.e.device)


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.e.close()


def pool_state(pool, n):
    return [(pool.stats(c), [a.tobytes() for a in pool.export(c)]) for c in range(n)]


def check_against_cpu(out, cpu, streams=None):
    """the call's records (state, results, events, frames, harq) against link_ring's (state, closed, events, counters):
    integers equal, float fields equal as bit patterns, the 80-byte state byte for byte"""
    st, res, ev, frames, harq = out
    cst, cclosed, cev, ccnt = cpu
    frames = frames.cpu().numpy() if torch.is_tensor(frames) else frames
    for s in (range(len(cev)) if streams is None else streams):
        assert res["n_events"][s] == len(cev[s]) and res["closed"][s] == cclosed[s], (s, res[s], cclosed[s], MR.show(cev[s]))
        assert {k: int(res[k][s]) for k in COUNTERS} == ccnt[s], (s, res[s], ccnt[s])
        for k, c in enumerate(cev[s]):
            g = ev[s, k]
            for f in MR.EVENT_FIELDS:
                assert int(g[f]) == int(c[f]), (s, k, f, g[f], c[f])
            for f in MR.EVENT_WORDS:
                assert bits(g[f]) == bits(c[f]), (s, k, f, g[f], c[f])
            assert (frames[s, k, :int(g["frame_bytes"])].tobytes() if g["delivered"] else None) == c["frame"], (s, k)
            for f in MR.HARQ_FIELDS:
                assert int(harq[s, k][f]) == int(c["harq"][f]), (s, k, f, harq[s, k], c["harq"])
        assert st[s:s + 1].tobytes() == cst[s:s + 1].tobytes(), (s, st[s], cst[s])


def check_against_composition(out, comp):
    st, res, ev, frames, harq = out
    cst, cclosed, cev, cframes, charq, ccnt = comp
    assert same_bytes(st, cst), (st, cst)
    assert np.array_equal(res["closed"], cclosed) and np.array_equal(res["n_events"], (cev["window_len"] > 0).sum(axis=1))
    assert np.array_equal(np.stack([res[k].astype(np.int64) for k in ("overflows", "overflow_dropped", "drift_snaps", "cursor_inits")], axis=1), ccnt)
    assert same_bytes(ev, cev), (ev, cev)
    assert np.array_equal(frames.cpu().numpy(), cframes)
    for f in ("seq", "valid", "entry", "src_hash", "dst_hash", "stored_mask", "sum_mask", "recovered_mask", "max_combine"):
        assert np.array_equal(harq[f], charq[f]), f


def three_ways(rig, recs, mode, kw, ckw, n_caches, ttl_ms=30000, cache_id=None, state=None, max_events=4, **more):
    """one call, the composition and the restatement on the same recordings, each on a pool (cache) of its own:
    -> (the call's records, the restatement's, the restatement's caches); the three agree"""
    from ria_amd.acquire import mcdpsk_link_ring
    e = rig.e
    x, lens = rig.stack(recs)
    caches = [ChaseCache(ttl_ms=ttl_ms) for _ in range(n_caches)]
    cmore = dict(more)
    if "channel_interleave" in cmore:
        cmore.pop("channel_interleave")
        cmore["B"] = cmore.pop("interleaver_bits")
    cpu = MR.link_ring(rig.O, recs, mode, state=state, max_events=max_events, caches=caches if n_caches else None, cache_id=cache_id, **cmore, **ckw)
    pool, pool2 = (e.chase_pool(n_caches, ttl_ms=ttl_ms), e.chase_pool(n_caches, ttl_ms=ttl_ms)) if n_caches else (None, None)
    try:
        out = e.mcdpsk_ring(x, lens, mode, state=state, max_events=max_events, chase=pool, cache_id=cache_id, **more, **kw)
        check_against_cpu(out, cpu)
        comp = mcdpsk_link_ring(e, x, lens, mode, state=state, max_events=max_events, chase=pool2, cache_id=cache_id, **more, **kw)
        check_against_composition(out, comp)
        for c in range(n_caches):
            check_cache(pool, c, caches[c])
        if n_caches:
            assert pool_state(pool, n_caches) == pool_state(pool2, n_caches)
    finally:
        if n_caches:
            pool.close()
            pool2.close()
    return out, cpu, caches


# ---- 1. adds nothing: byte equality with ria_gpu_rx_ring_batch on the ring call's own recordings
@pytest.mark.parametrize("name", ["zc", "chirp"])
def test_without_pool_flag_or_pending_equals_rx_ring(rig, name):
    e = rig.e
    mode, kw, _ = SET4[name]
    x, lens = rig.stack([r[0] for r in rig.set4[name]])
    st0, res0, ev0, fr0 = e.rx_ring(x, lens, mode, feed_step=4800, max_events=8, **kw)
    st, res, ev, fr, hq = e.mcdpsk_ring(x, lens, mode, feed_step=4800, max_events=8, **kw)
    assert list(res0["n_events"]) == [3, 2, 3] and (st0["total_fed"] > RING).all()
    ring = np.zeros(len(lens), e.RING_STATE)
    for f in e.RING_STATE.names:
        ring[f] = st[f]
    assert same_bytes(ring, st0) and same_bytes(res, res0) and same_bytes(ev, ev0) and np.array_equal(fr.cpu().numpy(), fr0.cpu().numpy())
    assert not hq.view(np.uint8).any() and not any(st[f].any() for f in MR.PENDING)


# ---- 2. never wraps: byte equality with ria_gpu_mcdpsk_stream_batch
def equals_stream(e, ring_out, stream_out):
    st, res, ev, fr, hq = ring_out
    st0, res0, ev0, fr0, hq0 = stream_out
    assert same_bytes(st, MR.from_stream_state(st0)), (st, st0)
    for f in res0.dtype.names:
        assert np.array_equal(res[f], res0[f]), f
    assert not any(res[k].any() for k in COUNTERS) and not res["reserved1"].any()
    assert same_bytes(ev, ev0) and np.array_equal(fr.cpu().numpy(), fr0.cpu().numpy()) and same_bytes(hq, hq0)


def test_short_recordings_equal_mcdpsk_stream(rig):
    e, O = rig.e, rig.O
    # the HARQ pin, a clean recording, the HARQ recording with the cache off, on two pools
    recs, ids = [rig.short_harq, rig.clean, rig.short_harq], np.array([0, 1, -1], np.int32)
    x, lens = rig.stack(recs)
    pool, pool0 = e.chase_pool(2), e.chase_pool(2)
    try:
        t0 = np.array([1000, 2 ** 64 - 5, 7], np.uint64)
        want = e.mcdpsk_stream(x, lens, "MCDPSK_ZC", feed_step=4800, max_events=4, chase=pool0, cache_id=ids, t0_ms=t0, **G20)
        got = e.mcdpsk_ring(x, lens, "MCDPSK_ZC", feed_step=4800, max_events=4, chase=pool, cache_id=ids, t0_ms=t0, **G20)
        assert want[2][0, 1]["success"] == 1 and want[4][0, 1]["recovered_mask"] == 2 and list(want[1]["n_events"]) == [2, 2, 2]
        equals_stream(e, got, want)
        assert pool_state(pool, 2) == pool_state(pool0, 2)
    finally:
        pool.close()
        pool0.close()
    for fs in (0, 4800):                                  # ZC control frames at 10 carriers, with everything arrived and fed
        zx, zlens = rig.stack([zc_recording(O, 7)[0], zc_recording(O, 8)[0]])
        kw = dict(carriers=10, modulation="DQPSK", spreading=1)
        equals_stream(e, e.mcdpsk_ring(zx, zlens, "MCDPSK_ZC", feed_step=fs, max_events=8, **kw), e.mcdpsk_stream(zx, zlens, "MCDPSK_ZC", feed_step=fs, max_events=8, **kw))
    # one cut case through its three calls
    K = MS.CUT_CASES["c20_dqpsk_6cw"]
    cx, sent, at = MS.clean_recording(O, [5, 6], carriers=K["carriers"], bps=K["bps"], n_payload=K["n_payload"])
    sync, need = at[0] + MS.ZC_LEN, frame_len(K["frame_cw"], K["carriers"], K["bps"], 1)
    s_state, r_state = None, None
    for upto, n_ev in ((sync + K["cut_behind_sync"], 1), (sync + need - 1, 0), (len(cx), 2)):
        xs, ls = rig.stack([cx[:upto]])
        want = e.mcdpsk_stream(xs, ls, "MCDPSK_ZC", state=s_state, feed_step=4800, max_events=4, **G20)
        got = e.mcdpsk_ring(xs, ls, "MCDPSK_ZC", state=r_state, feed_step=4800, max_events=4, **G20)
        assert want[1]["n_events"][0] == n_ev
        equals_stream(e, got, want)
        s_state, r_state = want[0], got[0]
    assert got[3][0, 0, :len(sent[0])].cpu().numpy().tobytes() == sent[0]
    # one channel-interleave case
    ix, isent, _ = MS.clean_recording(O, [5, 6], B=216)
    xs, ls = rig.stack([ix])
    want = e.mcdpsk_stream(xs, ls, "MCDPSK_ZC", feed_step=4800, max_events=4, channel_interleave=True, interleaver_bits=216, **G20)
    got = e.mcdpsk_ring(xs, ls, "MCDPSK_ZC", feed_step=4800, max_events=4, channel_interleave=True, interleaver_bits=216, **G20)
    assert want[2]["success"][0, :2].all()
    equals_stream(e, got, want)


# ---- 3. against the composition and the restatement
def test_harq_across_the_wrap(rig):
    """recording 1: the retransmission lies behind the wrap at a smaller ring index than the first reception.  ttl >= the gap:
    recovery through the sum; ttl below the gap: the entry has expired, no combine - the run a clock on the ring index fails
    (the pool's age is signed: a clock that jumps back keeps the entry alive); and a clock that wraps 2^64 between the two"""
    from ria_amd.acquire import LINK_STREAM_COUNTERS, link_stream_tally
    sync = [a + MS.ZC_LEN for a in rig.harq_at]
    gap_ms = sync[1] * 1000 // 48000 - sync[0] * 1000 // 48000
    assert sync[0] < RING < sync[1] and sync[1] % RING < sync[0] and 0 < gap_ms < 20000
    t_edge = 2 ** 64 - 1 - sync[0] * 1000 // 48000
    for ttl, t0, expired, recovered in ((gap_ms, 0, 0, 1), (gap_ms - 1, 0, 1, 0), (gap_ms, t_edge, 0, 1), (gap_ms - 1, t_edge, 1, 0)):
        out, cpu, caches = three_ways(rig, [rig.harq], "MCDPSK_ZC", G20, MR.GEOM, 1, ttl_ms=ttl, t0_ms=np.array([t0], np.uint64))
        st, res, ev, fr, hq = out
        assert (caches[0].stats["entries_expired"], caches[0].stats["recoveries"], caches[0].stats["combines"]) == (expired, recovered, recovered)
        assert [int(v) for v in ev["sync_position"][0, :2]] == sync and res["n_events"][0] == 2
        assert [int(v) for v in hq["stored_mask"][0, :2]] == [2, 2] and [int(v) for v in hq["sum_mask"][0, :2]] == [0, 2 * recovered]
        assert [int(v) for v in hq["recovered_mask"][0, :2]] == [0, 2 * recovered] and ev["success"][0, 1] == recovered
        if recovered:
            assert fr[0, 1, :len(rig.harq_frame)].cpu().numpy().tobytes() == rig.harq_frame and caches[0].size() == 0
        tally = dict(zip(LINK_STREAM_COUNTERS, link_stream_tally(ev, hq)))
        assert (tally["outcome_decoded"], tally["delivered"], tally["recovered_by_sum"], tally["stores"], tally["combines"]) == (2, 2, recovered, 2, recovered)


@pytest.mark.parametrize("where", ["across", "behind"])
def test_reentry_across_the_wrap(rig, where):
    x, sent, at, cut, K = rig.reentry(where)
    ckw = dict(carriers=K["carriers"], bps=K["bps"], spreading=1)
    sync, need = at[0] + MS.ZC_LEN, frame_len(K["frame_cw"], K["carriers"], K["bps"], 1)
    whole, _, _ = three_ways(rig, [x], "MCDPSK_ZC", G20, ckw, 0)
    assert whole[1]["n_events"][0] == 2 and whole[2]["success"][0, :2].all()
    # call 1: the wait is written in absolute indices
    one, cpu_one, _ = three_ways(rig, [x[:cut]], "MCDPSK_ZC", G20, ckw, 0)
    st1 = one[0]
    assert one[1]["closed"][0] == NEED and one[1]["n_events"][0] == 1 and one[2][0, 0]["outcome"] == WR.NEED_SAMPLES
    assert (st1["pending_total_cw"][0], st1["need_samples"][0], st1["pend_sync_position"][0]) == (K["frame_cw"], need, sync)
    assert st1["total_fed"][0] > RING and st1["pend_search_start"][0] == one[2][0, 0]["search_start"]
    assert (sync < RING < sync + need) if where == "across" else st1["pend_search_start"][0] > RING
    # call 2: still a sample short - no event, the 80 bytes untouched
    short, _, _ = three_ways(rig, [x[:sync + need - 1]], "MCDPSK_ZC", G20, ckw, 0, state=st1)
    assert short[1]["closed"][0] == NEED and short[1]["n_events"][0] == 0 and short[0].tobytes() == st1.tobytes()
    assert not short[2].view(np.uint8).any() and not short[3].any() and short[1]["search_legs"][0] == 0
    # call 3: the whole capture - that window first, then events and final state of the one-shot call
    two, _, _ = three_ways(rig, [x], "MCDPSK_ZC", G20, ckw, 0, state=st1)
    assert two[0].tobytes() == whole[0].tobytes() and not any(two[0][f].any() for f in MR.PENDING)
    assert two[1]["n_events"][0] == 2 and two[2][0, 0]["search_start"] == st1["pend_search_start"][0]
    assert two[3][0, 0, :len(sent[0])].cpu().numpy().tobytes() == sent[0] and two[3][0, 1, :len(sent[1])].cpu().numpy().tobytes() == sent[1]
    for f in ("sync_position", "outcome", "next_pos", "frame_bytes", "delivered", "success", "codewords_ok", "codewords_failed", "frame_type"):
        assert np.array_equal(two[2][f], whole[2][f]), f
    assert same_bytes(two[2][0, 1:], whole[2][0, 1:]) and np.array_equal(two[3].cpu().numpy(), whole[3].cpu().numpy())
    assert bits(two[2][0, 0]["correlation"]) == bits(st1["pend_correlation"][0]) and bits(two[2][0, 0]["snr_db"]) == bits(st1["snr_hint"][0])


def test_channel_interleaving_behind_the_wrap(rig):
    e, O = rig.e, rig.O
    x, sent, at = MR.ci_recording(O)
    out, cpu, _ = three_ways(rig, [x], "MCDPSK_ZC", G20, MR.GEOM, 1, channel_interleave=True, interleaver_bits=MR.CI_B)
    assert at[0] > RING and out[1]["n_events"][0] == 2 and out[2]["success"][0, :2].all()
    for k in range(2):
        assert out[3][0, k, :len(sent[k])].cpu().numpy().tobytes() == sent[k]
    plain, _, _ = three_ways(rig, [x], "MCDPSK_ZC", G20, MR.GEOM, 0)
    assert plain[1]["n_events"][0] == 2 and not plain[2]["success"].any()


@pytest.mark.parametrize("name", ["zc", "chirp"])
def test_frames_around_the_wrap_with_a_pool(rig, name):
    mode, kw, ckw = SET4[name]
    recs = rig.set4[name]
    out, cpu, caches = three_ways(rig, [r[0] for r in recs], mode, kw, ckw, 3, max_events=8)
    st, res, ev, fr, hq = out
    assert list(res["n_events"]) == [3, 2, 3] and ev["success"][ev["window_len"] > 0].all() and (st["total_fed"] > RING).all()
    for i, (_, placed) in enumerate(recs):
        want = [sent for _, sent in placed if sent is not None]
        for k, sent in enumerate(want):
            assert fr[i, k, :len(sent)].cpu().numpy().tobytes() == sent, (name, i, k)
    assert hq["valid"][ev["window_len"] > 0].all() and not hq["stored_mask"].any()


# ---- 4. a mixed batch in one call
def test_mixed_batch_equals_each_stream_alone(rig):
    """a stream whose wait is over (its span crosses the wrap), one still a sample short, one that searches a long recording,
    a short capture that never wraps, one with the cache off, and one whose first window is cut at the capture's end (a second
    window length in the first round): each row is the row of its single-stream call"""
    e = rig.e
    x, sent, at, cut, K = rig.reentry("across")
    sync, need = at[0] + MS.ZC_LEN, frame_len(K["frame_cw"], K["carriers"], K["bps"], 1)
    st1 = e.mcdpsk_ring(*rig.stack([x[:cut]]), "MCDPSK_ZC", max_events=4, **G20)[0]
    assert st1["pending_total_cw"][0] == K["frame_cw"]
    first = int(e.mcdpsk_ring(*rig.stack([rig.clean]), "MCDPSK_ZC", max_events=1, **G20)[2][0, 0]["search_start"])
    full = 31120 + frame_len(8, 20, 2, 1)
    end = first + full - 5000
    assert rig.clean_at[0] + MS.ZC_LEN + frame_len(3, 20, 2, 1) < end < len(rig.clean)
    recs = [x, x[:sync + need - 1], rig.harq, rig.clean, rig.harq, rig.clean[:end]]
    state = np.concatenate([st1, st1, e.mcdpsk_ring_state(4, total_fed=0)])
    ids = np.array([0, 1, 2, 3, -1, 4], np.int32)
    t0 = np.arange(6, dtype=np.uint64) * np.uint64(1000)
    xs, lens = rig.stack(recs)
    pool = e.chase_pool(5)
    try:
        out = e.mcdpsk_ring(xs, lens, "MCDPSK_ZC", state=state, max_events=4, chase=pool, cache_id=ids, t0_ms=t0, **G20)
        want_pool = pool_state(pool, 5)
        st, res, ev, fr, hq = out
        assert list(res["n_events"][:5]) == [2, 0, 2, 2, 2] and res["n_events"][5] >= 1 and res["closed"][1] == NEED and st[1:2].tobytes() == st1.tobytes()
        assert ev["window_len"][0, 0] == full and ev["window_len"][3, 0] == full and 0 < ev["window_len"][5, 0] == end - first < full
        assert ev["success"][2, 1] == 1 and ev["success"][4, 1] == 0 and not hq[4].view(np.uint8).any() and ev["success"][5, 0] == 1
        frames = fr.cpu().numpy()
        for s in range(6):
            alone = e.chase_pool(5)                         # a pool of its own: a cache's counters run on through a clear
            try:
                one = e.mcdpsk_ring(xs[s:s + 1, :lens[s]].contiguous(), lens[s:s + 1], "MCDPSK_ZC", state=state[s:s + 1], max_events=4, chase=alone,
                                    cache_id=ids[s:s + 1], t0_ms=t0[s:s + 1], **G20)
                if ids[s] >= 0:
                    assert pool_state(alone, 5)[ids[s]] == want_pool[ids[s]], s
            finally:
                alone.close()
            assert all(same_bytes(a, b[s:s + 1]) for a, b in zip((one[0], one[1], one[2], one[4]), (st, res, ev, hq))), s
            assert np.array_equal(one[3].cpu().numpy(), frames[s:s + 1]), s
        # n_streams 0: RIA_OK, nothing written
        rc, *outs = raw_call(e, xs, lens, state, 4, pool=pool, ids=ids, n=0)
        assert rc == 0 and all((o == 0xA5).all() for o in outs[1:]) and same_bytes(outs[0].reshape(-1), state)
    finally:
        pool.close()


# ---- 5. re-entrancy and the host form
def test_one_event_per_call_and_the_host_form(rig):
    e = rig.e
    recs = [rig.harq, rig.reentry("across")[0], rig.set4["zc"][0][0]]
    # the third recording is at 10 carriers: it delivers nothing at 20, and only has to give the same records
    x, lens = rig.stack(recs)
    n = len(recs)
    t0 = np.array([5, 6, 7], np.uint64)
    pool, first, host = e.chase_pool(n), e.chase_pool(n), e.chase_pool(n)      # a cache's counters run on through a clear: a pool per form
    try:
        want = e.mcdpsk_ring(x, lens, "MCDPSK_ZC", max_events=4, chase=first, t0_ms=t0, **G20)
        want_pool = pool_state(first, n)
        assert list(want[1]["n_events"][:2]) == [2, 2] and want[2][0, 1]["success"] == 1
        state, live = e.mcdpsk_ring_state(n, total_fed=0), np.arange(n)
        events, harq, calls = [[] for _ in range(n)], [[] for _ in range(n)], 0
        closed = np.zeros(n, np.int64)
        while len(live):
            calls += 1
            assert calls < 10
            st, res, ev, fr, hq = e.mcdpsk_ring(x[torch.as_tensor(live, device=x.device)].contiguous(), lens[live], "MCDPSK_ZC", state=state[live],
                                                max_events=1, chase=pool, cache_id=live.astype(np.int32), t0_ms=t0[live], **G20)
            state[live], closed[live] = st, res["closed"]
            for i, s in enumerate(live):
                events[s] += [ev[i, k].tobytes() for k in range(res["n_events"][i])]
                harq[s] += [hq[i, k].tobytes() for k in range(res["n_events"][i])]
            live = live[res["closed"] == FULL_EVENTS]
        assert same_bytes(state, want[0]) and np.array_equal(closed, want[1]["closed"])
        for s in range(n):
            assert events[s] == [want[2][s, k].tobytes() for k in range(want[1]["n_events"][s])]
            assert harq[s] == [want[4][s, k].tobytes() for k in range(want[1]["n_events"][s])]
        assert pool_state(pool, n) == want_pool
        # the host form on recording 1: 1.1 M samples, five pieces of the pinned block
        h = e.mcdpsk_ring_host(rig.harq, "MCDPSK_ZC", max_events=4, chase=host, cache_id=0, t0_ms=5, **G20)
        assert same_bytes(h[0], want[0][:1]) and same_bytes(h[1], want[1][:1]) and same_bytes(h[2], want[2][:1])
        assert np.array_equal(h[3], want[3].cpu().numpy()[:1]) and same_bytes(h[4], want[4][:1]) and pool_state(host, 1) == want_pool[:1]
    finally:
        pool.close()
        first.close()
        host.close()


# ---- 6. and 7.: raw calls on outputs filled with a sentinel
def raw_call(e, x, lens_in, state_in, n_events, pool=None, ids=None, t0=None, fill=0xA5, geom=G20, **over):
    """ria_gpu_mcdpsk_ring_batch on outputs filled with `fill` -> (rc, state, results, events, frames, harq) as uint8 arrays"""
    from ria_amd import capi
    from ria_amd.engine import _ptr
    n, stride = x.shape
    dev = e.device
    lens_d = torch.from_numpy(np.asarray(lens_in, np.int32)).to(dev)
    st_d = torch.from_numpy(np.ascontiguousarray(state_in, e.MCRING_STATE).view(np.uint8).reshape(-1, 80).copy()).to(dev)
    res_d = torch.full((max(n, 1), 88), fill, dtype=torch.uint8, device=dev)
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
    rc = e.lib.ria_gpu_mcdpsk_ring_batch(*a.values(), None)
    torch.cuda.synchronize()
    return rc, st_d.cpu().numpy(), res_d.cpu().numpy(), ev_d.cpu().numpy(), fr_d.cpu().numpy(), hq_d.cpu().numpy()


def test_every_output_row_is_written(rig):
    """outputs filled with 0xA5 first: every record comes back written - events, payload rows and chase records past a
    stream's events zero, payload bytes past frame_bytes zero, the results' reserved words zero"""
    e = rig.e
    x, sent, at, cut, K = rig.reentry("behind")
    recs = [rig.harq, rig.harq, x[:cut], np.zeros(0, F)]
    ids = np.array([0, -1, 1, 2], np.int32)
    xs, lens = rig.stack(recs)
    pool = e.chase_pool(3)
    try:
        rc, st, res, ev, fr, hq = raw_call(e, xs, lens, e.mcdpsk_ring_state(4, total_fed=0), 5, pool=pool, ids=ids)
    finally:
        pool.close()
    assert rc == 0
    st = st.view(e.MCRING_STATE).reshape(-1)
    res, ev, hq = res.view(e.RING_STREAM_RESULT).reshape(-1), ev.view(e.STREAM_EVENT).reshape(4, 5), hq.view(e.HARQ_RESULT).reshape(4, 5)
    assert list(res["n_events"]) == [2, 2, 1, 0] and list(res["closed"]) == [2, 2, NEED, 2]
    assert not res["reserved"].any() and not res["reserved1"].any() and (res["mode"] == 1).all() and list(res["search_legs"]) == [3, 3, 1, 1]
    for s in range(4):
        for k in range(5):
            live = k < res["n_events"][s]
            nbytes = int(ev["frame_bytes"][s, k]) if live and ev["delivered"][s, k] else 0
            assert not fr[s, k, nbytes:].any(), (s, k)
            if not live:
                assert not ev[s, k:k + 1].view(np.uint8).any() and not hq[s, k:k + 1].view(np.uint8).any(), (s, k)
    assert hq["valid"][0, 0] == 1 and not hq[1].view(np.uint8).any() and not (hq["reserved"] != 0).any()
    assert st["pending_total_cw"][2] == K["frame_cw"] and st["pend_sync_position"][2] > RING and not any(st[f][[0, 1, 3]].any() for f in MR.PENDING)


def test_refused_calls_leave_everything_untouched(rig):
    """RIA_ERR_INVALID before anything is written: arguments the host rejects, and states and lengths the up-front check
    rejects.  The captures are zeros and are never read: nothing here runs a search or a window."""
    from ria_amd import capi
    from ria_amd.engine import RxEngine
    e = rig.e
    x = torch.zeros((2, 1100000), dtype=torch.float32, device=e.device)
    lens = np.array([1100000, 200000])
    fresh = e.mcdpsk_ring_state(2, total_fed=0)

    def pending(stream=0, ok=False, **f):
        """a valid wait on `stream` - 3 codewords at sync 102 512 of a window from 100 000, the ring fed to 150 000 - with f
        changed, which takes it out of the domain unless ok"""
        s = fresh.copy()
        v = dict(pending_total_cw=3, need_samples=30720, pend_search_start=100000, pend_sync_position=102512, total_fed=150000)
        v.update(f)
        for k, val in v.items():
            s[k][stream] = val
        assert MR.pending_domain_ok(*(int(s[k][stream]) for k in ("pending_total_cw", "need_samples", "pend_search_start", "pend_sync_position")),
                                    int(lens[stream]), 31120, int(s["total_fed"][stream])) == ok
        return s

    pool = e.chase_pool(2)
    other = RxEngine("DQPSK", "R1_4", max_batch=8)
    foreign = other.chase_pool(2)
    try:
        before = pool_state(pool, 2)
        foreign_before = pool_state(foreign, 2)
        CI = capi.MACQ_CHANNEL_INTERLEAVE
        unknown = next(b for b in (1, 2, 4, 8, 16) if b != CI)
        bad_ring = fresh.copy()
        bad_ring["correlation_pos"][1] = 960000
        bad = [("OFDM mode", dict(mode=capi.SEARCH_MODE["OFDM_LTS"]), fresh), ("foreign pool", dict(pool=foreign), fresh),
               ("duplicate ids", dict(ids=[1, 1]), fresh), ("id >= n_caches", dict(ids=[0, 2]), fresh),
               ("unknown window flag", dict(window_flags=unknown), fresh), ("unknown flag beside the known", dict(window_flags=CI | unknown, bits=40), fresh),
               ("interleaver_bits 0", dict(window_flags=CI, bits=0), fresh), ("interleaver_bits 649", dict(window_flags=CI, bits=649), fresh),
               ("pending 256", {}, pending(pending_total_cw=256)), ("pending -1", {}, pending(pending_total_cw=-1)),
               ("negative need_samples", {}, pending(need_samples=-1)),
               ("start below the capture", {}, pending(pend_search_start=-1)), ("start behind the capture", {}, pending(1, pend_search_start=200000, total_fed=200000)),
               ("sync below the capture", {}, pending(pend_sync_position=-1)), ("sync behind the capture", {}, pending(1, pend_sync_position=200000)),
               ("the capture no longer holds the search span", {}, pending(1, pend_search_start=168881, pend_sync_position=170000, total_fed=200000)),
               ("a span of 960 000", {}, pending(need_samples=960000 - 2512)),
               ("total_fed more than one ring past the window", {}, pending(total_fed=100000 + 960001)),
               ("the search span was never fed", {}, pending(total_fed=100000 + 31119)),
               ("a capture one sample above the domain", dict(stride=2 ** 31, lens_over=[capi.RING_MAX_CAPTURE + 1, 200000]), fresh),
               ("a ring state outside the search's domain", {}, bad_ring)]
        for what, over, state in bad:
            over = dict(over)
            kw = dict(pool=pool)
            kw.update({k: over.pop(k) for k in ("pool", "ids") if k in over})
            lens_in = over.pop("lens_over", lens)
            out = raw_call(e, x, lens_in, state, 4, **kw, **over)
            assert out[0] == -1, what
            assert all((o == 0xA5).all() for o in out[2:]) and same_bytes(out[1].reshape(-1), state), what
            assert pool_state(pool, 2) == before and pool_state(foreign, 2) == foreign_before, what
            assert e.lib.ria_gpu_last_error(e.h).decode().startswith("ria_gpu_mcdpsk_ring_batch: "), what
        # the same wait inside the domain is taken: the span's last value, 959 999, is not refused by the check (it closes
        # at once: the capture does not hold it)
        edge = pending(ok=True, need_samples=959999 - 2512, pend_search_start=150000, pend_sync_position=152512, total_fed=200000)
        out = raw_call(e, x, lens, edge, 4, pool=pool)
        res = out[2].view(e.RING_STREAM_RESULT).reshape(-1)
        assert out[0] == 0 and res["closed"][0] == NEED and res["n_events"][0] == 0 and out[1].reshape(-1)[:80].tobytes() == edge[:1].tobytes()
        with pytest.raises(Exception, match="ria_gpu_mcdpsk_ring_host"):
            e.mcdpsk_ring_host(np.zeros(1000, F), "MCDPSK_ZC", max_events=0, **G20)
        with pytest.raises(Exception, match="ria_gpu_mcdpsk_ring_host"):
            e.mcdpsk_ring_host(np.zeros(1000, F), "OFDM_LTS", **G20)
        with pytest.raises(capi.RiaError):
            e.mcdpsk_ring(x[:, :1000].contiguous(), [1000, 1000], "MCDPSK_ZC", carriers=1, modulation="DBPSK", spreading=4)     # full > 959 999
    finally:
        foreign.close()
        other.close()
        pool.close()
