"""The table of tests/search_inputs.py on the restatement alone (tests/search_restatement.py, searchForSync on the oracle's
detectors): the rows reach every statement the GPU test compares on, with no waiver.  What the library must equal is only as
good as what the rows make the restatement do."""
import numpy as np
import pytest

import pyoracle as po
import search_inputs as SI
import search_restatement as SR


@pytest.fixture(scope="module")
def traced():
    O = po.Oracle()
    out = {}
    for r in SI.ROWS:
        for fs in SI.FEED_STEPS:
            t = SR.Trace()
            res, st = SI.expected(O, r, fs, t)
            out[(r["name"], fs)] = (res, st, t.seen)
    return out


def test_rows_are_small():
    O = po.Oracle()
    for r in SI.ROWS:
        n = len(SI.capture(O, r["cap"]))
        assert n <= SR.min_search_of(r["mode"]) + 80000 and n <= 959999, r["name"]
    assert len({r["name"] for r in SI.ROWS}) == len(SI.ROWS)


def test_min_search():
    assert (SR.min_search_of(SR.LTS), SR.min_search_of(SR.ZC), SR.min_search_of(SR.CHIRP)) == (67304, 31120, 120000)


def test_coverage(traced):
    seen = set().union(*(s for _, _, s in traced.values()))
    res = {k: v[0] for k, v in traced.items()}
    want = {("outcome", SR.SYNC_FOUND), ("outcome", SR.NEED_SAMPLES), ("outcome", SR.LIMIT),
            "wait_fed", "wait_unresolved", "feed_clamp", "rms_skip", "tracker_fast", "tracker_slow", "gate_low", "gate_high", "gate_mid",
            "gate_relaxed", "near_miss_up", "near_miss_down", "reject", "weak_accept", "weak_refused_coherent", "zc_breaker",
            "start_clipped", "replay", "cfo_sanity_taken", "cfo_sanity_kept", "rms_nan", "rms_inf"}
    assert want <= seen, want - seen
    f = np.float32
    tiers = {(SR.COHERENT_PSK, f(0.90)), (SR.COHERENT_QAM, f(0.78)), (SR.DIFFERENTIAL, f(0.72)), (SR.DIFFERENTIAL, f(0.68)),
             (SR.DIFFERENTIAL, f(0.65)), (SR.DIFFERENTIAL, f(0.62)), (SR.DIFFERENTIAL, f(0.56)), (SR.ZC_MODE, f(0.40))}
    got = {(h[1], f(h[2])) for h in seen if isinstance(h, tuple) and h[0] == "conf"}
    assert tiers <= got, tiers - got
    assert any(c == SR.ZC_MODE and f(0.25) <= v < f(0.40) for c, v in got)          # the breaker's relaxed threshold
    assert any(int(r["catchups_moderate"]) for r in res.values()) and any(int(r["catchups_severe"]) for r in res.values())


def test_rows_do_what_they_are_there_for(traced):
    r = lambda name, fs=0: traced[(name, fs)][0]
    s = lambda name, fs=0: traced[(name, fs)][1]
    for fs in SI.FEED_STEPS:
        assert r("lts_clean", fs)["outcome"] == SR.SYNC_FOUND and r("lts_clean", fs)["sync_position"] == SI.LTS_FIRST_SYNC
        assert r("lts_clean_second", fs)["outcome"] == SR.SYNC_FOUND and r("lts_clean_second", fs)["sync_position"] > 45000
        assert r("lts_replay", fs)["replays"] == 1 and r("lts_no_replay", fs)["replays"] == 0
        assert r("lts_no_replay", fs)["outcome"] == SR.SYNC_FOUND
        assert r("lts_noisy_weak", fs)["weak_accept"] == 1 and r("lts_noisy_weak", fs)["outcome"] == SR.SYNC_FOUND and s("lts_noisy_weak", fs)["reject_streak"] == 1
        assert r("lts_noisy_qam", fs)["weak_accepts"] == 0 and r("lts_noisy_qam", fs)["rejects"] > 0
        assert r("lts_limit", fs)["outcome"] == SR.LIMIT and r("lts_limit", fs)["invocations"] == 2
        assert r("lts_silence", fs)["outcome"] == SR.NEED_SAMPLES and r("lts_silence", fs)["detector_runs"] == 0
        assert r("zc_weak_streak", fs)["outcome"] == SR.SYNC_FOUND and r("zc_weak_streak", fs)["min_confidence"] < np.float32(0.40)
        assert r("zc_weak", fs)["near_misses"] >= 2
        assert r("chirp_clean", fs)["sync_cfo_hz"] != np.float32(5.0) and r("chirp_connected", fs)["sync_cfo_hz"] == np.float32(5.0)
        assert abs(r("chirp_cfo_kept", fs)["sync_cfo_hz"] - 12.0) < 0.5
    assert r("lts_clean", 4800)["waits"] > 0 and r("lts_short", 0)["waits"] == 1 and r("lts_short", 0)["outcome"] == SR.NEED_SAMPLES
    assert s("lts_cursor_ahead", 0)["correlation_pos"] == 50000 and s("lts_cursor_ahead", 4800)["correlation_pos"] == 20000
    assert s("lts_cursor_ahead", 4800)["reject_streak"] == 0 and s("lts_cursor_ahead", 0)["reject_streak"] == 5
    assert np.isfinite(s("lts_nan_floor")["noise_floor"]) and not np.isfinite(s("lts_nonfinite")["noise_floor"])
    assert r("zc_long", 0)["catchups_severe"] == 1 and r("zc_long", 0)["outcome"] == SR.SYNC_FOUND
    assert r("zc_mid", 0)["catchups_moderate"] >= 1


def test_limit_continues(traced):
    """a LIMIT state fed back continues to the same end as one long call, under either feed_step"""
    O = po.Oracle()
    for name in ("lts_noisy_diff", "zc_weak", "lts_replay"):
        row = next(r for r in SI.ROWS if r["name"] == name)
        for fs in SI.FEED_STEPS:
            x, n, st, cls, conn = SI.row_args(O, row, fs)
            whole, st_whole = traced[(name, fs)][0], traced[(name, fs)][1]
            k = max(1, int(whole["invocations"]) // 2)
            a, st_a = SR.search(O, x, n, st, row["mode"], cls, conn, fs, k)
            assert a["outcome"] == SR.LIMIT
            b, st_b = SR.search(O, x, n, st_a, row["mode"], cls, conn, fs, row["max_inv"] - k)
            assert st_b.tobytes() == st_whole.tobytes() and b["outcome"] == whole["outcome"]
            assert int(a["invocations"]) + int(b["invocations"]) == int(whole["invocations"])
            for fld in ("search_start", "sync_position", "correlation", "sync_cfo_hz", "sync_snr_db", "min_confidence", "detect_threshold"):
                assert b[fld].tobytes() == whole[fld].tobytes(), (name, fs, fld)
