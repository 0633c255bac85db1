"""The ring restatement (tests/ring_restatement.py: feedAudio and searchForSync on a literal 960 000-float buffer_) on its own:
the rows of tests/ring_inputs.py reach every hit name the restatement can emit (the one that no input can reach is listed with the reason); on every row of
tests/search_inputs.py it gives search_restatement.search's result and state, which ties this yardstick to the merged one; and
the closed form the kernels read the capture through (ria_amd/csrc/ring_rules.hpp) names the literal ring's content."""
import numpy as np
import pytest

import pyoracle as po
import ring_inputs as RI
import ring_restatement as RR
import search_inputs as SI
import search_restatement as SR

RING = RR.MAX_BUFFER_SAMPLES


@pytest.fixture(scope="module")
def O():
    return po.Oracle()


@pytest.fixture(scope="module")
def traced(O):
    out = {}
    for r in RI.ROWS:
        t = RR.Trace()
        res, st = RI.expected(O, r, t)
        out[r["name"]] = (res, st, t.seen)
    return out


def closed_form(T, p):
    """ring_rules.hpp's ring_source: the capture index ring index p holds after T samples, -1 = never written"""
    if T < RING:
        return np.where(p < T, p, -1)
    return T - 1 - ((T - 1 - p) % RING)


def test_rows_are_small(O):
    assert len({r["name"] for r in RI.ROWS}) == len(RI.ROWS)
    for r in RI.ROWS:
        x, n, st, _, _ = RI.row_args(O, r)
        assert n <= len(x) <= 1300000 and 0 <= st["total_fed"] <= n, r["name"]


# hit names the restatement can emit but no input of this time model can reach, each with the reason
UNREACHABLE = {
    "feed_clamp_after": "the second pre-wrap clamp (:289-291): the clamp at :204 and the overflow drop (need_to_drop <= unsearched) both leave the "
                        "cursor at or behind the OLD write position, and the write position only grows before the wrap",
}


def hit_names():
    """every plain hit name in ring_restatement.py's source: the string literals inside its hit(...) calls"""
    import inspect
    import re
    names = set()
    for call in re.findall(r"\bhit\((.*)\)\s*$", inspect.getsource(RR), flags=re.M):
        if call.lstrip().startswith("("):
            continue                                   # the tuple hits: ("outcome", n), ("sync_after_wrap", mode), asserted below
        names |= set(re.findall(r'"([a-z0-9_]+)"', call))
    return names


def test_coverage(traced):
    """no unreached statement: every hit name of the restatement is reached by a row, but for the listed unreachable ones"""
    seen = set().union(*(s for _, _, s in traced.values()))
    names = hit_names()
    assert len(names) >= 35 and {"feed_clamp", "wait_fed", "replay", "drift_guard", "span_wraps", "feed_clamp_after"} <= names and set(UNREACHABLE) <= names
    want = (names - set(UNREACHABLE)) | {("sync_after_wrap", RR.LTS), ("sync_after_wrap", RR.ZC), ("sync_after_wrap", RR.CHIRP),
                                         ("outcome", RR.SYNC_FOUND), ("outcome", RR.NEED_SAMPLES), ("outcome", RR.LIMIT)}
    assert want <= seen, want - seen
    assert not set(UNREACHABLE) & seen


def test_rows_do_what_they_are_there_for(traced):
    r = lambda name: traced[name][0]
    s = lambda name: traced[name][1]
    a = r("lts_cross_feed")
    assert a["outcome"] == RR.SYNC_FOUND and a["sync_position"] == RI.A_STRADDLE_SYNC == a["abs_position"] and s("lts_cross_feed")["total_fed"] > RING
    assert a["search_start"] + a["search_len"] > RING and a["abs_search_start"] == a["search_start"] and a["span_wraps"] == 0
    assert r("lts_cross_limit")["outcome"] == RR.LIMIT and s("lts_cross_limit")["total_fed"] == RING - 4800 + 5 * 4800
    assert s("lts_from_959999")["total_fed"] == RING - 1 + 3 * 4800
    b = r("lts_sync_wraps")
    assert b["outcome"] == RR.SYNC_FOUND and b["sync_position"] == RI.B_SYNC_RING and b["abs_position"] == RING + RI.B_SYNC_RING and b["rms_skips"] == 1
    c = r("lts_backtrack_underflow")
    assert c["search_start"] == RING + 5000 - 9600 and c["abs_search_start"] == c["search_start"] and 0 <= c["sync_position"] < 100   # the detector's grid moves with the span
    assert r("zc_prewrap_clip")["search_start"] == 0 and r("zc_prewrap_clip")["outcome"] == RR.SYNC_FOUND
    assert s("lts_prewrap_clamp")["reject_streak"] == 0 and s("lts_prewrap_clamp")["correlation_pos"] == 20000 and r("lts_prewrap_clamp")["waits"] == 3
    assert r("lts_cursor_init")["cursor_inits"] == 1 and r("lts_cursor_init")["waits"] >= 14
    assert r("lts_cursor_init_at_zero")["cursor_inits"] == 2 and s("lts_cursor_init_at_zero")["correlation_pos"] == 4800
    for name in ("lts_replay_across_end", "lts_replay_same_index"):
        assert r(name)["replays"] == 1 and r(name)["outcome"] == RR.NEED_SAMPLES and s(name)["correlation_pos"] == RI.B_SYNC_RING + 14400, name
    assert r("lts_no_replay_200")["replays"] == 0 and r("lts_no_replay_200")["outcome"] == RR.SYNC_FOUND
    assert r("lts_replay_cursor_wraps")["replays"] == 1 and r("lts_replay_cursor_wraps")["sync_position"] == RI.A_STRADDLE_SYNC
    assert r("zc_severe_circular")["catchups_severe"] == 1 and r("zc_moderate_circular")["catchups_moderate"] == 1
    assert r("zc_wait_circular")["outcome"] == RR.NEED_SAMPLES and r("zc_wait_circular")["waits"] == 1
    z = r("zc_sync_after_wrap")
    assert z["outcome"] == RR.SYNC_FOUND and abs(int(z["abs_position"]) - RI.ZC_FRAME) < 8000 and z["abs_position"] == z["sync_position"] + RING
    ch = r("chirp_sync_after_wrap")
    assert ch["outcome"] == RR.SYNC_FOUND and ch["abs_position"] == ch["sync_position"] + RING and ch["abs_position"] > RI.CHIRP_FRAME
    d = r("lts_drift_guard")
    assert d["drift_snaps"] == 1 and d["overflows"] == 0 and s("lts_drift_guard")["correlation_pos"] == 100000
    oa, sa = r("lts_overflow_all"), s("lts_overflow_all")
    assert oa["overflows"] == 1 and oa["overflow_dropped"] == 95200 and sa["overflow_events"] == 1 and sa["overflow_dropped"] == 95200 and sa["total_fed"] == 1100000
    op, sp = r("lts_overflow_part"), s("lts_overflow_part")
    assert op["overflows"] == 1 and op["overflow_dropped"] == 645200 and sp["overflow_events"] == 0 and sp["overflow_dropped"] == 645207
    w = r("lts_span_wraps")
    assert w["span_wraps"] == 1 and w["detector_runs"] == 1 and w["abs_search_start"] == 1100000 - (140000 - int(w["search_start"]))


def test_limit_continues_across_the_wrap(O, traced):
    """a LIMIT state fed back continues to the same end as one long call; the cut lies before, at and behind the wrap"""
    row = next(r for r in RI.ROWS if r["name"] == "lts_cross_feed")
    x, n, st, cls, conn = RI.row_args(O, row)
    whole, st_whole = traced["lts_cross_feed"][0], traced["lts_cross_feed"][1]
    assert int(whole["invocations"]) > 6
    for k in (1, 2, int(whole["invocations"]) // 2):
        a, st_a = RR.search(O, x, n, st, row["mode"], cls, conn, row["feed_step"], k)
        assert a["outcome"] == RR.LIMIT
        b, st_b = RR.search(O, x, n, st_a, row["mode"], cls, conn, row["feed_step"], row["max_inv"] - k)
        assert st_b.tobytes() == st_whole.tobytes() and b["outcome"] == whole["outcome"]
        assert int(a["invocations"]) + int(b["invocations"]) == int(whole["invocations"])
        for fld in ("search_start", "abs_search_start", "sync_position", "abs_position", "correlation", "sync_cfo_hz", "sync_snr_db", "span_wraps"):
            assert b[fld].tobytes() == whole[fld].tobytes(), (k, fld)


def test_equals_the_search_restatement_before_the_wrap(O):
    """every row of tests/search_inputs.py, both feed steps: the same result fields and the same decoder state"""
    for r in SI.ROWS:
        for fs in SI.FEED_STEPS:
            x, n, st, cls, conn = SI.row_args(O, r, fs)
            want_res, want_st = SI.expected(O, r, fs)
            res, out = RR.search(O, x, n, RR.from_search_state(st)[0], r["mode"], cls, conn, fs, r["max_inv"])
            for f in SR.RESULT.names:
                assert res[f].tobytes() == want_res[f].tobytes(), (r["name"], fs, f)
            assert RR.to_search_state(out)[0].tobytes() == want_st.tobytes(), (r["name"], fs)
            assert res["abs_search_start"] == res["search_start"] and not res["span_wraps"] and not res["overflows"] and not res["drift_snaps"]
            assert not res["cursor_inits"] and not out["overflow_events"] and not out["overflow_dropped"]


def test_closed_form_names_the_literal_ring():
    """random chunked feeds up to T around one and two laps; every ring index compared, so every p around write_pos is"""
    rng = np.random.default_rng(5)
    totals = [1, 1000, RING - 1, RING, RING + 1, RING + 4800, 2 * RING - 1, 2 * RING, 2 * RING + 1, 2 * RING + 77777]
    x = np.arange(max(totals), dtype=np.float32)          # sample k has value k (exact in float32 below 2^24)
    p = np.arange(RING)
    for T in totals:
        ring, fed = RR.Ring(), 0
        while fed < T:
            n = min(T - fed, int(rng.integers(1, 300000)))
            ring.write(x[fed:fed + n])
            fed += n
        assert ring.write_pos == T % RING
        src = closed_form(T, p)
        want = np.where(src >= 0, x[np.maximum(src, 0)], np.float32(0))
        assert np.array_equal(ring.buffer, want), T
        assert src.max() == T - 1 and (src[src >= 0] % RING == p[src >= 0]).all()
        wp = T % RING
        near = (wp + np.arange(-3, 4)) % RING              # the newest sample sits just before write_pos, the oldest at it
        if T >= RING:
            assert closed_form(T, (wp - 1) % RING) == T - 1 and closed_form(T, wp) == T - RING
        assert np.array_equal(ring.buffer[near], np.where(closed_form(T, near) >= 0, x[np.maximum(closed_form(T, near), 0)], np.float32(0)))
