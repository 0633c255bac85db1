"""The table of captures and injected decoder states for ria_gpu_search_ring_batch, shared by tests/test_ring_cpu.py (what the
rows make the restatement do) and tests/test_gpu_ring.py (the library against the restatement).  A row starts at a total_fed
and a cursor next to the statement it is there for - nothing walks 20 s of audio - on a capture of silence, low noise and a
few preambles placed by ABSOLUTE index.  Every row carries its own feed_step.  The table is an input, not a result: what the
rows reach is asserted by test_ring_cpu.py.  Test infrastructure only (not collected: no test_ prefix)."""
import numpy as np

import ring_restatement as RR
import search_inputs as SI
from search_inputs import _mc_frame, _noise, _ofdm_frame, _place

F = np.float32
RING = RR.MAX_BUFFER_SAMPLES
LTS_MIN, ZC_MIN, CHIRP_MIN = SI.LTS_MIN, SI.ZC_MIN, SI.CHIRP_MIN
LTS_LEAD = 14400 - SI.LTS_FIRST_SYNC      # the LTS detector places a frame in silence this many samples before its first sample
_cache = {}

# capture "lts_a": frames at absolute A_OLD (read one lap later, as the ring's oldest samples), A_STRADDLE (its samples lie on
# both sides of absolute index 960 000) and A_AFTER (behind the wrap)
A_OLD, A_STRADDLE, A_AFTER, A_LEN = 143000, 950000, 1040000, 1130000
# capture "lts_b": one frame whose sync lies at absolute 960 050 = ring index 50
B_FRAME, B_SYNC_RING, B_LEN = RING + 50 + LTS_LEAD, 50, 1060000
ZC_FRAME, ZC_LEN = 1000000, 1060000        # capture "zc": noise and one MC-DPSK frame behind the wrap (ring index 40 000)
CHIRP_FRAME, CHIRP_LEN = 970000, 1110000   # capture "chirp": noise and one chirp-preamble frame at ring index 10 000
QUIET_LEN = 1160000                        # capture "quiet": noise of rms 0.0064, under every gate


def _lts_a(O):
    x = np.zeros(A_LEN, F)
    _place(x, A_OLD, _ofdm_frame(O, 1))
    _place(x, A_STRADDLE, _ofdm_frame(O, 1))
    _place(x, A_AFTER, _ofdm_frame(O, 1))
    return x


def _lts_b(O):
    x = np.zeros(B_LEN, F)
    _place(x, B_FRAME, _ofdm_frame(O, 1))
    return x


def _zc(O):
    x = np.zeros(ZC_LEN, F)
    _place(x, ZC_FRAME, _mc_frame(O, 1, True))
    x[ZC_FRAME - 60000:] += _noise(O, ZC_LEN - ZC_FRAME + 60000, 41)
    return x


def _chirp(O):
    x = np.zeros(CHIRP_LEN, F)
    _place(x, CHIRP_FRAME, _mc_frame(O, 4, False))
    x[CHIRP_FRAME - 20000:] += _noise(O, CHIRP_LEN - CHIRP_FRAME + 20000, 42)
    return x


def _quiet(O):
    return _noise(O, QUIET_LEN, 43, scale=0.5)


_BUILD = {"lts_a": _lts_a, "lts_b": _lts_b, "zc": _zc, "chirp": _chirp, "quiet": _quiet}


def capture(O, key):
    if key.startswith("si:"):
        return SI.capture(O, key[3:])
    if key not in _cache:
        _cache[key] = np.ascontiguousarray(_BUILD[key](O), F)
    return _cache[key]


def R(name, mode, cap, purpose, total_fed, feed_step=0, modulation="DQPSK", connected=False, max_inv=8, capture_len=None, **state):
    return dict(name=name, mode=mode, cap=cap, purpose=purpose, total_fed=total_fed, feed_step=feed_step, modulation=modulation, connected=connected,
                max_inv=max_inv, capture_len=capture_len, state=state)


L, Z, C = RR.LTS, RR.ZC, RR.CHIRP
HI = dict(snr_hint=20.0)        # hints that leave the differential tier at 0.72
A_STRADDLE_SYNC = A_STRADDLE - LTS_LEAD           # ring index = absolute index: 949 944
ROWS = [
    # ---- the wrap itself
    R("lts_cross_feed", L, "lts_a", "total_fed 955 200 -> exactly 960 000 in one feed (write_pos 0), the backlog turns circular, skips up to the straddling "
      "frame, span over the ring end, SYNC_FOUND behind the wrap with ring_pos >= write_pos", RING - 4800, 4800, max_inv=40,
      correlation_pos=RING - 4800 - LTS_MIN, **HI),
    R("lts_cross_limit", L, "lts_a", "the same, LIMIT after 5 invocations: behind the wrap", RING - 4800, 4800, max_inv=5, correlation_pos=RING - 4800 - LTS_MIN, **HI),
    R("lts_from_959999", L, "quiet", "total_fed 959 999 -> 964 799 inside one feed", RING - 1, 4800, max_inv=3, correlation_pos=RING - 1 - LTS_MIN),
    R("lts_exactly_ring", L, "quiet", "total_fed exactly 960 000 given: write_pos 0, circular backlog of one min_search", RING, 4800, max_inv=3, correlation_pos=RING - LTS_MIN),
    R("lts_wait_linear", L, "quiet", "capture_len = total_fed = 1 100 000, cursor one min_search behind: skip, then the wait with write_pos >= cursor",
      1100000, 0, max_inv=4, capture_len=1100000, correlation_pos=140000 - LTS_MIN),
    R("lts_rms_straddle", L, "lts_a", "the RMS window at cursor 959 500 reads ring 959 500..959 999, 0..499", 1030000, 0, max_inv=2, correlation_pos=959500, **HI),
    R("lts_sync_wraps", L, "lts_b", "skip at 955 000, RMS at 959 800 over the ring end, span over the ring end, sync_position 960 050 -> 50, ring_pos < write_pos",
      1030000, 0, max_inv=3, correlation_pos=955000, **HI),
    R("lts_backtrack_underflow", L, "lts_b", "cursor 5000 behind the wrap: search_start = 960 000 + 5000 - 9600 (:604)", 1040000, 0, max_inv=2, correlation_pos=5000, **HI),
    R("zc_prewrap_clip", Z, "si:zc_clean", "before the wrap: search_start = 0 (:601)", 48000, 0, max_inv=64),
    R("lts_prewrap_clamp", L, "quiet", "before the wrap, a cursor ahead of total_fed: a wait (the library's limit), and the feed clamps it to write_pos_ and "
      "clears the streak (:204)", 20000, 4800, max_inv=3, correlation_pos=50000, reject_streak=5),
    R("lts_cursor_init", L, "quiet", "correlation_pos_ == 0 behind the wrap becomes write_pos_ (:462), then waits for a min_search", 1030000, 4800, max_inv=20),
    R("lts_cursor_init_at_zero", L, "quiet", "the same with write_pos 0: the cursor stays 0 and :462 runs again after the feed", RING, 4800, max_inv=3),
    # ---- anti-replay on the ring
    R("lts_replay_across_end", L, "lts_b", "last decoded at 959 950, sync at 50: circular distance 100, a replay; then the wait with write_pos >= cursor",
      1030000, 0, max_inv=6, correlation_pos=959800, last_decoded_sync_pos=RING - 50, **HI),
    R("lts_replay_same_index", L, "lts_b", "last decoded at ring index 50 one lap earlier: the same ring index is a replay", 1030000, 0, max_inv=6,
      correlation_pos=959800, last_decoded_sync_pos=B_SYNC_RING, **HI),
    R("lts_no_replay_200", L, "lts_b", "last decoded at 959 850: circular distance 200, no replay", 1030000, 0, max_inv=6, correlation_pos=959800,
      last_decoded_sync_pos=RING - 150, **HI),
    R("lts_replay_cursor_wraps", L, "lts_a", "a replay at 949 944: the cursor 949 944 + 14 400 wraps to 4344", 1030000, 0, max_inv=3, correlation_pos=950296,
      last_decoded_sync_pos=A_STRADDLE_SYNC + 10, **HI),
    # ---- ZC catch-up on the circular backlog
    R("zc_severe_circular", Z, "quiet", "write_pos 20 000 < min_search + 4800, cursor 890 000: backlog 90 000 = 2.89 x, severe: the snap wraps back",
      RING + 20000, 0, max_inv=2, correlation_pos=890000),
    R("zc_moderate_circular", Z, "quiet", "write_pos 20 000, cursor 930 000: backlog 50 000 = 1.6 x, moderate", RING + 20000, 0, max_inv=2, correlation_pos=930000),
    R("zc_wait_circular", Z, "quiet", "write_pos 1000, cursor 950 000: backlog 11 000, the wait on the circular branch, nothing can arrive", RING + 1000, 0, max_inv=2,
      capture_len=RING + 1000, correlation_pos=950000),
    R("zc_sync_after_wrap", Z, "zc", "an MC-DPSK frame at ring index 40 000 behind the wrap", 1040000, 0, max_inv=8, correlation_pos=40500),
    R("chirp_sync_after_wrap", C, "chirp", "a chirp preamble at ring index 10 000 behind the wrap", 1100000, 0, max_inv=8, correlation_pos=10500),
    # ---- feedAudio: drift guard and overflow
    R("lts_drift_guard", L, "quiet", "cursor 3000 ahead of write_pos behind the wrap: a skip, then the feed finds backlog 952 200 > 950 400 and snaps", 1060000, 4800,
      max_inv=3, correlation_pos=103000),
    R("lts_overflow_all", L, "quiet", "before the wrap, 900 000 samples arrive on a backlog of 95 200: need_to_drop == unsearched", 200000, 900000, max_inv=3,
      capture_len=1100000, correlation_pos=100000),
    R("lts_overflow_part", L, "quiet", "behind the wrap, 100 000 samples arrive on a backlog of 905 200: need_to_drop 645 200 < unsearched", 1060000, 100000, max_inv=3,
      correlation_pos=150000, overflow_events=0xFFFFFFFF, overflow_dropped=7),
    R("lts_span_wraps", L, "lts_a", "cursor 3500 ahead of write_pos on the oldest frame: the span crosses the write position", 1100000, 0, max_inv=2,
      correlation_pos=143500, **HI),
]


def row_args(O, r):
    """-> (capture, capture_len, STATE record, class, connected) of row r"""
    x = capture(O, r["cap"])
    st = RR.fresh_state(1, r["total_fed"])[0]
    for k, v in r["state"].items():
        st[k] = v
    return x, (len(x) if r["capture_len"] is None else r["capture_len"]), st, RR.modulation_class(r["mode"], r["modulation"]), r["connected"]


_results = {}


def expected(O, r, trace=None):
    """the restatement's (result, state) of row r, computed once"""
    if r["name"] not in _results or trace is not None:
        x, n, st, cls, conn = row_args(O, r)
        _results[r["name"]] = RR.search(O, x, n, st, r["mode"], cls, conn, r["feed_step"], r["max_inv"], trace)
    return _results[r["name"]]
