"""CPU: the claims the GPU tests of ria_gpu_mcdpsk_ring_batch rely on, asserted on the restatement's loop alone
(tests/mcdpsk_ring_restatement.link_ring: the ring search on a literal ring buffer, the window, the cache and the interleaver
restated on the checkers).  Every recording is a little over one ring long and mostly zeros.

(1) HARQ across the wrap: reception 1 lies before absolute 960 000, its retransmission behind it at a smaller ring index.
    Each fails alone, the second window decodes the sum, the cache is empty afterwards.  The pool's age is signed
    (chase_policy.hpp), so a clock on the ring index - 20 s back at the wrap - does not expire the entry, it keeps it alive:
    with a TTL one millisecond below the gap the call's clock expires the entry and nothing is combined, a ring-index clock
    combines all the same.  That run is the one a wrong clock fails; link_ring(clock="ring") shows it.
(2) re-entry across the wrap: the capture cut inside a frame whose sync lies shortly before absolute 960 000 (and, second
    variant, behind it) leaves absolute pending fields; a capture still too short changes nothing; the whole capture decodes
    that window first, and from there on events and state are the one-shot call's.
(3) a frame behind the wrap sent through the channel interleaver is delivered with the flag only.
(4) the three recordings of tests/test_gpu_ring_stream.py for zc and chirp with a cache attached: the frames before, across
    and behind the wrap are delivered, the lap-later frame is rejected by the anti-replay rule, the one 300 samples later not."""
import pytest

import mcdpsk_ring_restatement as MR
import mcdpsk_stream_restatement as MS
import mcdpsk_window_restatement as WR
from mcdpsk_acquire_restatement import frame_len
from mcdpsk_harq_restatement import ChaseCache

RING = MR.RING
NEED = MR.CLOSED["WINDOW_NEED_SAMPLES"]


# ---- (1)
@pytest.fixture(scope="module")
def harq(oracle):
    return MR.harq_recording(oracle)


def test_harq_across_the_wrap_recovers_through_the_sum(oracle, harq):
    x, frame, at = harq
    sync = [a + MS.ZC_LEN for a in at]
    gap_ms = sync[1] * 1000 // 48000 - sync[0] * 1000 // 48000
    assert sync[0] < RING < sync[1] and sync[1] % RING < sync[0] % RING and 0 < gap_ms < 20000 and 1100000 <= len(x) <= 1300000
    cache = ChaseCache(ttl_ms=gap_ms)                     # >= the gap, < the gap + 20 000 ms
    st, closed, ev, cnt = MR.link_ring(oracle, [x], "MCDPSK_ZC", caches=[cache], **MR.GEOM)
    ev = ev[0]
    assert [e["sync_position"] for e in ev] == sync and all(e["outcome"] == WR.DECODED for e in ev), MR.show(ev)
    first, second = ev
    assert (first["success"], first["codewords_ok"], first["codewords_failed"]) == (0, 2, 1) and first["harq"]["valid"] == 1
    assert (first["harq"]["stored_mask"], first["harq"]["sum_mask"], first["harq"]["recovered_mask"]) == (0b10, 0, 0)
    assert (second["harq"]["stored_mask"], second["harq"]["sum_mask"], second["harq"]["recovered_mask"]) == (0b10, 0b10, 0b10)
    assert second["success"] == 1 and second["frame"] == frame
    assert cache.stats["stores"] == 2 and cache.stats["combines"] == 1 and cache.stats["recoveries"] == 1 and cache.stats["entries_expired"] == 0
    assert cache.size() == 0
    assert st["total_fed"][0] == len(x) > RING and closed[0] == MR.CLOSED["SEARCH_NEED_SAMPLES"] and not any(cnt[0].values())
    # each reception fails alone: no cache at all
    _, _, alone, _ = MR.link_ring(oracle, [x], "MCDPSK_ZC", **MR.GEOM)
    assert [(e["success"], e["codewords_failed"]) for e in alone[0]] == [(0, 1), (0, 1)]
    # a TTL below the gap: the entry has expired when the retransmission arrives, nothing is combined
    short = ChaseCache(ttl_ms=gap_ms - 1)
    _, _, ev3, _ = MR.link_ring(oracle, [x], "MCDPSK_ZC", caches=[short], **MR.GEOM)
    assert short.stats["entries_expired"] == 1 and short.stats["combines"] == 0 and not any(e["success"] for e in ev3[0])
    # ... which a clock on the ring index gets wrong: it runs backwards over the wrap, the age is negative, the sum is made
    wrong = ChaseCache(ttl_ms=gap_ms - 1)
    _, _, ev4, _ = MR.link_ring(oracle, [x], "MCDPSK_ZC", caches=[wrong], clock="ring", **MR.GEOM)
    assert wrong.stats["entries_expired"] == 0 and wrong.stats["combines"] == 1 and ev4[0][1]["success"] == 1
    # the caller's clock near 2^64 - 1: it wraps between the two receptions
    t0 = 2 ** 64 - 1 - MR.now_ms(0, sync[0])
    edge = ChaseCache(ttl_ms=gap_ms)
    _, _, ev5, _ = MR.link_ring(oracle, [x], "MCDPSK_ZC", caches=[edge], t0_ms=t0, **MR.GEOM)
    assert MR.now_ms(t0, sync[0]) == 2 ** 64 - 1 and MR.now_ms(t0, sync[1]) == gap_ms - 1
    assert edge.stats["entries_expired"] == 0 and edge.stats["recoveries"] == 1 and ev5[0][1]["success"] == 1
    late = ChaseCache(ttl_ms=gap_ms - 1)
    MR.link_ring(oracle, [x], "MCDPSK_ZC", caches=[late], t0_ms=t0, **MR.GEOM)
    assert late.stats["entries_expired"] == 1 and late.stats["recoveries"] == 0


# ---- (2)
@pytest.mark.parametrize("where", ["across", "behind"])
def test_reentry_across_the_wrap_continues_as_one_call(oracle, where):
    x, sent, at, cut, K = MR.reentry_recording(oracle, where)
    geom = dict(carriers=K["carriers"], bps=K["bps"], spreading=1)
    sync, need = at[0] + MS.ZC_LEN, frame_len(K["frame_cw"], K["carriers"], K["bps"], 1)
    assert 1100000 <= len(x) <= 1300000 and sync < cut < sync + need
    whole_state, whole_closed, whole, _ = MR.link_ring(oracle, [x], "MCDPSK_ZC", **geom)
    assert [e["frame"] for e in whole[0]] == sent, MR.show(whole[0])
    # call 1: the event, the close reason, absolute pending fields
    st1, closed1, ev1, _ = MR.link_ring(oracle, [x[:cut]], "MCDPSK_ZC", **geom)
    assert closed1[0] == NEED and len(ev1[0]) == 1 and ev1[0][0]["outcome"] == WR.NEED_SAMPLES, (closed1, MR.show(ev1[0]))
    s = st1[0]
    assert (s["pending_total_cw"], s["need_samples"], s["pend_sync_position"]) == (K["frame_cw"], need, sync)
    assert s["pend_search_start"] == ev1[0][0]["search_start"] and s["pend_correlation"] == ev1[0][0]["correlation"]
    assert s["total_fed"] > RING and s["correlation_pos"] < RING          # the search itself was past the wrap when it found the sync
    if where == "across":
        assert s["pend_search_start"] < s["pend_sync_position"] < RING < sync + need
    else:
        assert s["pend_search_start"] > RING
    # call 2: still a sample short
    st_s, closed_s, ev_s, _ = MR.link_ring(oracle, [x[:sync + need - 1]], "MCDPSK_ZC", state=st1, **geom)
    assert closed_s[0] == NEED and ev_s[0] == [] and st_s.tobytes() == st1.tobytes()
    # call 3: the whole capture
    st2, closed2, ev2, _ = MR.link_ring(oracle, [x], "MCDPSK_ZC", state=st1, **geom)
    assert len(ev2[0]) == len(whole[0]) == 2 and ev2[0][0]["search_start"] == s["pend_search_start"] and ev2[0][0]["frame"] == sent[0]
    for got, want in zip(ev2[0], whole[0]):
        for f in ("sync_position", "outcome", "next_pos", "frame", "delivered", "success", "codewords_ok", "codewords_failed", "frame_type", "frame_bytes",
                  "pending_total_cw"):
            assert got[f] == want[f], (f, got[f], want[f])
    assert closed2[0] == whole_closed[0] and not any(st2[f][0] for f in MR.PENDING)
    assert st2.tobytes() == whole_state.tobytes(), (st2, whole_state)


# ---- (3)
def test_interleaved_frames_behind_the_wrap_need_the_flag(oracle):
    x, sent, at = MR.ci_recording(oracle)
    assert at[0] > RING
    _, _, ev, _ = MR.link_ring(oracle, [x], "MCDPSK_ZC", B=MR.CI_B, **MR.GEOM)
    assert [e["frame"] for e in ev[0]] == sent and all(e["success"] for e in ev[0]), MR.show(ev[0])
    _, _, ev, _ = MR.link_ring(oracle, [x], "MCDPSK_ZC", **MR.GEOM)
    assert len(ev[0]) == 2 and not any(e["success"] for e in ev[0]), MR.show(ev[0])


# ---- (4)
RING_SET = {"zc": ("MCDPSK_ZC", dict(carriers=10, bps=2, spreading=1)), "chirp": ("MCDPSK_CHIRP", dict(carriers=10, bps=1, spreading=1))}


@pytest.mark.parametrize("name", ["zc", "chirp"])
def test_frames_around_the_wrap_with_a_cache(oracle, name):
    from test_gpu_ring_stream import recordings
    mode, geom = RING_SET[name]
    recs = recordings(oracle, name)
    caches = [ChaseCache() for _ in recs]
    st, closed, ev, cnt = MR.link_ring(oracle, [r[0] for r in recs], mode, caches=caches, **geom)
    near = 62000 if name == "chirp" else 3000      # chirp: the sync is the training, behind 57 600 samples of preamble
    for i, (_, placed) in enumerate(recs):
        got = [e for e in ev[i] if e["frame"] is not None]
        want = [(a, sent) for a, sent in placed if sent is not None]
        assert len(got) == len(want) == len(ev[i]), (name, i, MR.show(ev[i]))
        for e, (a, sent) in zip(got, want):
            assert e["frame"][:len(sent)] == sent and abs(e["sync_position"] - a) < near and e["success"] == 1, (name, i, MR.show(ev[i]))
        for a, sent in placed:
            if sent is None:                       # the lap-later frame never left the search
                assert not [e for e in ev[i] if abs(e["sync_position"] - a) < near], (name, i, MR.show(ev[i]))
        assert closed[i] == MR.CLOSED["SEARCH_NEED_SAMPLES"] and st["total_fed"][i] == len(recs[i][0]) > RING
        assert caches[i].size() == 0 and caches[i].stats["stores"] == 0
    straddle = ev[0][1]
    assert straddle["search_start"] < RING < straddle["search_start"] + straddle["window_len"]
    assert [len(e) for e in ev] == [3, 2, 3]
