"""CPU restatement of ria_gpu_mcdpsk_ring_batch (include/ria_gpu.h) on the checkers: the rules of
ria_amd/csrc/mcdpsk_ring_rules.hpp one statement per function (tests/test_mcdpsk_ring_rules_host.py compares them with the
header, case by case), and link_ring(), the call's loop on ring_restatement.search (the literal 960 000-float buffer_),
mcdpsk_window_restatement.mcdpsk_window, the Python ChaseCache of mcdpsk_harq_restatement and mcdpsk_ci_restatement's
interleaver: the ring search, the window cut from the recording by absolute index, the host's part modulo the ring, the audio
clock on the absolute sync position, and the wait at a found sync carried in the state in absolute indices.  Then the
recordings the tests share: each a little over one ring long, zeros outside the short recording of
tests/mcdpsk_stream_restatement.py that it places next to absolute index 960 000, so the RMS gate skips most of it.

Test infrastructure only (not collected: no test_ prefix)."""
import numpy as np

import mcdpsk_stream_restatement as MS
import mcdpsk_window_restatement as WR
import ring_restatement as RR
import stream_restatement as SR
from mcdpsk_acquire_restatement import frame_len

F = np.float32
RING = RR.MAX_BUFFER_SAMPLES
MAX_SPAN = RING - 1
M64 = MS.M64
PENDING = MS.PENDING
STATE = np.dtype(RR.STATE.descr + [(n, "<i4") for n in PENDING[:4]] + [(n, "<f4") for n in PENDING[4:]])
assert STATE.itemsize == 80
EVENT_FIELDS, EVENT_WORDS, HARQ_FIELDS = MS.EVENT_FIELDS, MS.EVENT_WORDS, MS.HARQ_FIELDS
MODE = {"MCDPSK_ZC": RR.ZC, "MCDPSK_CHIRP": RR.CHIRP}
CLOSED = {"SEARCH_NEED_SAMPLES": 2, "SEARCH_LIMIT": 3, "WINDOW_NEED_SAMPLES": 4, "EVENTS_FULL": 5, "SPAN_LOST": 7}
NONE = RR.NO_LAST_SYNC


# ---- the rules
def now_ms(t0_ms, abs_position, sample_rate=MS.SAMPLE_RATE):
    """the audio clock on the ABSOLUTE sync position"""
    return (int(t0_ms) + int(abs_position) * 1000 // int(sample_rate)) & M64


def pending_domain_ok(pending_total_cw, need_samples, pend_search_start, pend_sync_position, capture_len, search_len, total_fed):
    if not MS.pending_domain_ok(pending_total_cw, need_samples, pend_search_start, pend_sync_position, capture_len, search_len):
        return False
    if pending_total_cw == 0:
        return True
    if pend_sync_position - pend_search_start + need_samples > MAX_SPAN:       # the span does not fit one ring
        return False
    if total_fed - pend_search_start > RING:                                   # the ring no longer holds the window's first sample
        return False
    return pend_search_start + search_len <= total_fed                         # the search that found the sync read that span


def reentry_fed(total_fed, pend_sync_position, need_samples):
    return max(total_fed, pend_sync_position + need_samples)


def reentry_arrival(total_fed, pend_search_start, pend_sync_position, need_samples, ahead, capture_len, abs_cursor):
    """backlog plus arrivals of the two total_fed assignments of a re-entry, were they feeds, and total_fed behind them
    (abs_cursor < 0: the window leaves the cursor where it was)"""
    backlog = total_fed - (pend_search_start + ahead)
    t1 = reentry_fed(total_fed, pend_sync_position, need_samples)
    t2 = max(t1, min(capture_len, abs_cursor)) if abs_cursor >= 0 else t1
    return backlog + (t1 - total_fed) + (t2 - t1), t2


def rebase_last_sync(last, search_start):
    """ring_rules.hpp's ring_rebase_last_sync: the circular difference to the window's origin, in -480 000 .. 479 999"""
    if last == NONE:
        return NONE
    d = (last - search_start) % RING
    return d - RING if d >= RING // 2 else d


def fresh_state(n, total_fed=0):
    s = np.zeros(n, STATE)
    for f in RR.STATE.names:
        s[f] = RR.fresh_state(n, total_fed)[f]
    return s


def from_stream_state(s):
    """a mcdpsk_stream_restatement.STATE array as this call's state: the same decoder before the wrap"""
    s = np.atleast_1d(s)
    out = np.zeros(len(s), STATE)
    ring = RR.from_search_state(s)
    for f in RR.STATE.names:
        out[f] = ring[f]
    for f in PENDING:
        out[f] = s[f]
    return out


# ---- the loop
def link_ring(O, recs, mode, state=None, feed_step=4800, max_invocations=1 << 20, max_events=256, connected=False, carriers=10, bps=1,
              spreading=1, caches=None, cache_id=None, t0_ms=None, B=None, clock=None):
    """recs: one float32 recording per stream.  caches / cache_id / t0_ms / B as in mcdpsk_stream_restatement.link_stream.
    clock: what the audio clock reads, "abs" (default: the call's) or "ring" - the sync's ring index, the mistake the
    recordings are built to expose.  -> (state (STATE), closed [n], events: per stream a list of dicts of EVENT_FIELDS,
    EVENT_WORDS, frame (bytes or None) and harq (dict of HARQ_FIELDS), counters: per stream a dict of the ring search's
    overflow_dropped, overflows, drift_snaps, cursor_inits summed over the legs)"""
    n = len(recs)
    m = MODE[mode]
    chirp = m == RR.CHIRP
    lens = np.array([len(r) for r in recs], np.int64)
    state = fresh_state(n, total_fed=0 if feed_step else lens) if state is None else np.array(state, STATE)
    ids = np.arange(n) if cache_id is None else np.broadcast_to(np.asarray(cache_id), (n,))
    t0 = [0] * n if t0_ms is None else [int(v) for v in np.broadcast_to(np.asarray(t0_ms, object), (n,))]
    assert len({int(c) for c in ids if c >= 0}) == sum(int(c) >= 0 for c in ids) or caches is None
    search_len = RR.min_search_of(m)
    first_frame, full = frame_len(1, carriers, bps, spreading), search_len + frame_len(8, carriers, bps, spreading)
    assert full <= MAX_SPAN
    events = [[] for _ in range(n)]
    closed = np.zeros(n, np.int64)
    counters = [dict(overflow_dropped=0, overflows=0, drift_snaps=0, cursor_inits=0) for _ in range(n)]

    def window(s, det, wl, pending):
        """det: search_start and sync_position (ring indices), abs_search_start, abs_position, known_cfo_hz, detect_threshold,
        min_confidence, correlation, snr_db"""
        start, sync = int(det["abs_search_start"]), int(det["abs_position"])
        ring_start = int(det["search_start"])
        x = np.zeros(wl, F)
        piece = recs[s][start:start + wl]
        x[:len(piece)] = piece
        conf = SR.min_confidence(det["min_confidence"], det["correlation"])
        cache = caches[int(ids[s])] if caches is not None and ids[s] >= 0 else None
        now = now_ms(t0[s], sync if clock != "ring" else int(det["sync_position"]))
        w = WR.mcdpsk_window(O, x, search_len, carriers=carriers, bps=bps, spreading=spreading, chirp=chirp, disconnected=chirp and not connected,
                             known_cfo=float(det["known_cfo_hz"]), detect_threshold=float(det["detect_threshold"]), min_confidence=float(conf), B=B,
                             cache=cache, now=now, pending_total_cw=int(pending),
                             last_decoded_sync=rebase_last_sync(int(state["last_decoded_sync_pos"][s]), ring_start))
        acq, outcome, nxt = w["acq"], w["outcome"], w["next_pos"]
        delivered = bool(w["deliver"])
        ev = dict(sync_position=sync, search_start=start, window_len=wl, outcome=outcome, next_pos=start + nxt if nxt >= 0 else -1,
                  frame_bytes=acq["frame_bytes"], need_samples=w["need_samples"], pending_total_cw=w["pending_total_cw"], delivered=int(delivered),
                  success=acq["success"], codewords_ok=acq["codewords_ok"], codewords_failed=acq["codewords_failed"], frame_type=acq["frame_type"],
                  correlation=F(det["correlation"]), cfo_hz=F(acq["cfo_hz"]), fading_index=F(acq["fading_index"]), snr_db=F(det["snr_db"]),
                  frame=bytes(acq["frame"]) if delivered else None, harq=w["harq"] if cache is not None else WR.empty_harq())
        events[s].append(ev)
        # step 5 of ria_gpu_rx_ring_batch
        if SR.moved(SR.MCDPSK, outcome):
            state["last_cfo_hz"][s], state["fading_hint"][s] = acq["cfo_hz"], acq["fading_index"]
        out_last = int(w["last_decoded_sync"])
        state["last_decoded_sync_pos"][s] = NONE if out_last == NONE else (out_last + ring_start) % RING
        abs_cursor = start + nxt if nxt >= 0 else (sync + first_frame if outcome == WR.TOO_LONG else None)
        if abs_cursor is not None:
            state["correlation_pos"][s] = abs_cursor % RING
            state["total_fed"][s] = max(int(state["total_fed"][s]), min(int(lens[s]), abs_cursor))
        keep = MS.keeps_pending(outcome)
        vals = (w["pending_total_cw"], w["need_samples"], start, sync, det["known_cfo_hz"], det["detect_threshold"], conf, det["correlation"])
        for name, v in zip(PENDING, vals):
            state[name][s] = v if keep else 0
        closed[s] = CLOSED["WINDOW_NEED_SAMPLES"] if keep else CLOSED["EVENTS_FULL"] if len(events[s]) >= max_events else 0

    for s in range(n):                                    # the streams that wait at a found sync, ahead of the first search
        st = state[s]
        if st["pending_total_cw"] <= 0:
            continue
        sync, need, start = int(st["pend_sync_position"]), int(st["need_samples"]), int(st["pend_search_start"])
        assert pending_domain_ok(int(st["pending_total_cw"]), need, start, sync, int(lens[s]), search_len, int(st["total_fed"]))
        if not MS.reentry_fits(int(lens[s]), sync, need):
            closed[s] = CLOSED["WINDOW_NEED_SAMPLES"]
            continue
        det = dict(search_start=start % RING, sync_position=sync % RING, abs_search_start=start, abs_position=sync, known_cfo_hz=st["pend_known_cfo_hz"],
                   detect_threshold=st["pend_detect_threshold"], min_confidence=st["pend_min_confidence"], correlation=st["pend_correlation"],
                   snr_db=st["snr_hint"])
        state["total_fed"][s] = reentry_fed(int(st["total_fed"]), sync, need)
        window(s, det, MS.reentry_window_len(full, int(lens[s]), start, sync, need), int(st["pending_total_cw"]))
    cls = RR.modulation_class(m)
    while (closed == 0).any():
        for s in np.flatnonzero(closed == 0):
            rst = np.zeros((), RR.STATE)
            for f in RR.STATE.names:
                rst[f] = state[f][s]
            r, st = RR.search(O, recs[s], int(lens[s]), rst, m, cls, connected, feed_step, max_invocations)
            for f in RR.STATE.names:
                state[f][s] = st[f]
            for k in counters[s]:
                counters[s][k] += int(r[k])
            if r["outcome"] != RR.SYNC_FOUND:
                closed[s] = int(r["outcome"])
                continue
            if r["span_wraps"]:
                closed[s] = CLOSED["SPAN_LOST"]
                continue
            det = {k: r[k] for k in ("search_start", "sync_position", "abs_search_start", "abs_position", "known_cfo_hz", "detect_threshold",
                                     "min_confidence", "correlation")}
            det["snr_db"] = r["sync_snr_db"]
            window(s, det, SR.window_len(full, int(lens[s]), int(r["abs_search_start"])), 0)
    return state, closed, events, counters


show = MS.show


# ---- recordings: a short recording of mcdpsk_stream_restatement behind `lead` zeros (a multiple of the 4800-sample feed
# step, so the search meets it with the cursor where a fresh decoder's would be), zeros to `total` behind it
GEOM = MS.GEOM
HARQ_LEAD = 189 * 4800          # 907 200: reception 1 at 921 200 .. 954 432, reception 2 from 963 432 = ring index 3432
HARQ_TOTAL = 1100000
# a search on this restatement, as MS.HARQ_PIN's was: MS.HARQ_PIN itself keeps its claim behind HARQ_LEAD zeros
# (tests/test_mcdpsk_ring_cpu.py asserts it)
HARQ_PIN = MS.HARQ_PIN
REENTRY_LEAD = {"across": 196 * 4800, "behind": 210 * 4800}     # the sync at 957 312 (its span ends at 1 014 144), and at 1 024 512
REENTRY_CASE = "c20_dqpsk_6cw"
CI_LEAD, CI_B = 210 * 4800, 216


def _embed(x, lead, total=None):
    out = np.zeros(max(lead + len(x), total or 0), F)
    out[lead:lead + len(x)] = x
    return out


def harq_recording(O):
    """-> (recording, frame bytes, the two receptions' first samples): reception 1 wholly before absolute 960 000, its
    retransmission behind it, at a smaller ring index"""
    x, frame, at = MS.harq_recording(O, **HARQ_PIN)
    at = [HARQ_LEAD + a for a in at]
    n = MS.ZC_LEN + frame_len(3, GEOM["carriers"], GEOM["bps"], 1)
    assert at[0] + n < RING < at[1] and at[1] % RING < at[0]
    return _embed(x, HARQ_LEAD, HARQ_TOTAL), frame, at


def reentry_recording(O, where):
    """-> (recording, sent frames, their first samples, cut, K): two clean 6-codeword frames; the capture cut at `cut` ends
    inside the first, whose sync lies shortly before absolute 960 000 ("across": the span it waits for crosses it) or behind
    it ("behind")"""
    K = MS.CUT_CASES[REENTRY_CASE]
    x, sent, at = MS.clean_recording(O, [5, 6], carriers=K["carriers"], bps=K["bps"], n_payload=K["n_payload"])
    lead = REENTRY_LEAD[where]
    at = [lead + a for a in at]
    sync = at[0] + MS.ZC_LEN
    need = frame_len(K["frame_cw"], K["carriers"], K["bps"], 1)
    assert (sync < RING < sync + need) if where == "across" else sync > RING
    return _embed(x, lead), sent, at, sync + K["cut_behind_sync"], K


def ci_recording(O):
    """-> (recording, sent frames, their first samples): two clean 3-codeword frames sent through the channel interleaver,
    both behind the wrap"""
    x, sent, at = MS.clean_recording(O, [5, 6], B=CI_B)
    return _embed(x, CI_LEAD), sent, [CI_LEAD + a for a in at]
