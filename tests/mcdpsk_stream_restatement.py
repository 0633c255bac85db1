"""CPU restatement of ria_gpu_mcdpsk_stream_batch (include/ria_gpu.h) on the checkers: the rules of
ria_amd/csrc/mcdpsk_stream_rules.hpp one statement per function (tests/test_mcdpsk_stream_cpu.py compares them with the
header, case by case), and link_stream(), the call's loop on search_restatement.search, mcdpsk_window_restatement.mcdpsk_window
and the Python ChaseCache of mcdpsk_harq_restatement: search, window, the host's part (stream_restatement's statements), the
audio clock for the cache, and the wait at a found sync carried in the state.  Then the recordings the tests share.

Test infrastructure only (not collected: no test_ prefix)."""
import numpy as np

import mcdpsk_window_restatement as WR
import pyoracle as po
import search_restatement as SRCH
import stream_restatement as SR
from mcdpsk_acquire_restatement import data_frame, encode_frame, frame_len
from mcdpsk_ci_restatement import interleave_bytes

F = np.float32
SAMPLE_RATE = 48000
M64 = 2 ** 64 - 1
PENDING = ("pending_total_cw", "need_samples", "pend_search_start", "pend_sync_position", "pend_known_cfo_hz", "pend_detect_threshold",
           "pend_min_confidence", "pend_correlation")
STATE = np.dtype(SRCH.STATE.descr + [(n, "<i4") for n in PENDING[:4]] + [(n, "<f4") for n in PENDING[4:]])
EVENT_FIELDS = ("sync_position", "search_start", "window_len", "outcome", "next_pos", "frame_bytes", "need_samples", "pending_total_cw",
                "delivered", "success", "codewords_ok", "codewords_failed", "frame_type")
EVENT_WORDS = ("correlation", "cfo_hz", "fading_index", "snr_db")
HARQ_FIELDS = ("valid", "seq", "src_hash", "dst_hash", "stored_mask", "sum_mask", "recovered_mask", "max_combine", "entry")
MODE = {"MCDPSK_ZC": SRCH.ZC, "MCDPSK_CHIRP": SRCH.CHIRP}


# ---- the rules
def now_ms(t0_ms, sync_position, sample_rate=SAMPLE_RATE):
    return (int(t0_ms) + int(sync_position) * 1000 // int(sample_rate)) & M64


def reentry_fits(capture_len, pend_sync_position, need_samples):
    return capture_len >= pend_sync_position + need_samples


def reentry_window_len(full, capture_len, pend_search_start, pend_sync_position, need_samples):
    return min(capture_len - pend_search_start, max(full, pend_sync_position - pend_search_start + need_samples))


def reentry_fed(fed, pend_sync_position, need_samples):
    return max(fed, pend_sync_position + need_samples)


def keeps_pending(outcome):
    return outcome == WR.NEED_SAMPLES


def pending_domain_ok(pending_total_cw, need_samples, pend_search_start, pend_sync_position, capture_len, search_len):
    if not 0 <= pending_total_cw <= 255:
        return False
    if pending_total_cw == 0:
        return True
    return need_samples >= 0 and 0 <= pend_search_start < capture_len and 0 <= pend_sync_position < capture_len and \
        capture_len - pend_search_start >= search_len


def fresh_state(n, fed=0):
    s = np.zeros(n, STATE)
    for f in SRCH.STATE.names:
        s[f] = SRCH.fresh_state(n, fed)[f]
    return s


# ---- the loop
def link_stream(O, recs, mode, state=None, feed_step=0, max_invocations=1 << 20, max_events=256, connected=False, carriers=10, bps=1,
                spreading=1, caches=None, cache_id=None, t0_ms=None, B=None):
    """recs: one float32 recording per stream.  caches: a list of ChaseCache (None: no pool); stream s uses caches[cache_id[s]]
    (default s; < 0: off) at now_ms(t0_ms[s], sync_position).  B: the interleaver width with channel interleaving, else None.
    -> (state (STATE), closed [n], events: per stream a list of dicts of EVENT_FIELDS, EVENT_WORDS, frame (bytes or None) and
    harq (dict of HARQ_FIELDS))"""
    n = len(recs)
    m = MODE[mode]
    chirp = m == SRCH.CHIRP
    lens = np.array([len(r) for r in recs], np.int64)
    state = fresh_state(n, fed=0 if feed_step else lens) if state is None else np.array(state, STATE)
    ids = np.arange(n) if cache_id is None else np.broadcast_to(np.asarray(cache_id), (n,))
    t0 = [0] * n if t0_ms is None else [int(v) for v in np.broadcast_to(np.asarray(t0_ms, object), (n,))]
    assert len({int(c) for c in ids if c >= 0}) == sum(int(c) >= 0 for c in ids) or caches is None
    search_len = SRCH.min_search_of(m)
    first_frame, full = frame_len(1, carriers, bps, spreading), search_len + frame_len(8, carriers, bps, spreading)
    events = [[] for _ in range(n)]
    closed = np.zeros(n, np.int64)

    def window(s, det, wl, pending):
        """det: search_start, sync_position, known_cfo_hz, detect_threshold, min_confidence, correlation, snr_db"""
        start, sync = int(det["search_start"]), int(det["sync_position"])
        x = np.zeros(wl, F)
        piece = recs[s][start:start + wl]
        x[:len(piece)] = piece
        conf = SR.min_confidence(det["min_confidence"], det["correlation"])
        cache = caches[int(ids[s])] if caches is not None and ids[s] >= 0 else None
        w = WR.mcdpsk_window(O, x, search_len, carriers=carriers, bps=bps, spreading=spreading, chirp=chirp, disconnected=chirp and not connected,
                             known_cfo=float(det["known_cfo_hz"]), detect_threshold=float(det["detect_threshold"]), min_confidence=float(conf), B=B,
                             cache=cache, now=now_ms(t0[s], sync), pending_total_cw=int(pending),
                             last_decoded_sync=SR.rebase_last_sync(int(state["last_decoded_sync_pos"][s]), start))
        acq, outcome, nxt = w["acq"], w["outcome"], w["next_pos"]
        delivered = bool(w["deliver"])
        ev = dict(sync_position=sync, search_start=start, window_len=wl, outcome=outcome, next_pos=start + nxt if nxt >= 0 else -1,
                  frame_bytes=acq["frame_bytes"], need_samples=w["need_samples"], pending_total_cw=w["pending_total_cw"], delivered=int(delivered),
                  success=acq["success"], codewords_ok=acq["codewords_ok"], codewords_failed=acq["codewords_failed"], frame_type=acq["frame_type"],
                  correlation=F(det["correlation"]), cfo_hz=F(acq["cfo_hz"]), fading_index=F(acq["fading_index"]), snr_db=F(det["snr_db"]),
                  frame=bytes(acq["frame"]) if delivered else None, harq=w["harq"] if cache is not None else WR.empty_harq())
        events[s].append(ev)
        if SR.moved(SR.MCDPSK, outcome):
            state["last_cfo_hz"][s], state["fading_hint"][s] = acq["cfo_hz"], acq["fading_index"]
        state["last_decoded_sync_pos"][s] = SR.last_sync(SR.MCDPSK, delivered, sync, int(state["last_decoded_sync_pos"][s]), w["last_decoded_sync"], start)
        state["correlation_pos"][s] = SR.cursor(SR.MCDPSK, outcome, nxt, start, sync, first_frame, int(state["correlation_pos"][s]))
        state["fed"][s] = SR.fed(state["fed"][s], lens[s], state["correlation_pos"][s])
        keep = keeps_pending(outcome)
        vals = (w["pending_total_cw"], w["need_samples"], start, sync, det["known_cfo_hz"], det["detect_threshold"], conf, det["correlation"])
        for name, v in zip(PENDING, vals):
            state[name][s] = v if keep else 0
        closed[s] = SR.close(SR.MCDPSK, outcome, len(events[s]), max_events, int(state["correlation_pos"][s]))

    for s in range(n):                                    # the streams that wait at a found sync, ahead of the first search
        st = state[s]
        if st["pending_total_cw"] <= 0:
            continue
        assert pending_domain_ok(int(st["pending_total_cw"]), int(st["need_samples"]), int(st["pend_search_start"]), int(st["pend_sync_position"]),
                                 int(lens[s]), search_len)
        sync, need, start = int(st["pend_sync_position"]), int(st["need_samples"]), int(st["pend_search_start"])
        if not reentry_fits(int(lens[s]), sync, need):
            closed[s] = SR.CLOSED["WINDOW_NEED_SAMPLES"]
            continue
        det = dict(search_start=start, sync_position=sync, known_cfo_hz=st["pend_known_cfo_hz"], detect_threshold=st["pend_detect_threshold"],
                   min_confidence=st["pend_min_confidence"], correlation=st["pend_correlation"], snr_db=st["snr_hint"])
        state["fed"][s] = reentry_fed(int(st["fed"]), sync, need)
        window(s, det, reentry_window_len(full, int(lens[s]), start, sync, need), int(st["pending_total_cw"]))
    cls = SRCH.modulation_class(m)
    while (closed == 0).any():
        for s in np.flatnonzero(closed == 0):
            sst = np.zeros((), SRCH.STATE)
            for f in SRCH.STATE.names:
                sst[f] = state[f][s]
            r, st = SRCH.search(O, recs[s], int(lens[s]), sst, m, cls, connected, feed_step, max_invocations)
            for f in SRCH.STATE.names:
                state[f][s] = st[f]
            if r["outcome"] != SRCH.SYNC_FOUND:
                closed[s] = int(r["outcome"])
                continue
            det = dict(search_start=r["search_start"], sync_position=r["sync_position"], known_cfo_hz=r["known_cfo_hz"],
                       detect_threshold=r["detect_threshold"], min_confidence=r["min_confidence"], correlation=r["correlation"], snr_db=r["sync_snr_db"])
            window(s, det, SR.window_len(full, int(lens[s]), int(r["search_start"])), 0)
    return state, closed, events


def show(events):
    return [(e["sync_position"], WR.OUTCOMES[e["outcome"]], e["success"], e["codewords_ok"], e["codewords_failed"], e["next_pos"],
             hex(e["harq"]["stored_mask"]), hex(e["harq"]["recovered_mask"])) for e in events]


# ---- recordings: ZC connected, 20 carriers DQPSK, spreading 1, unless said otherwise
GEOM = dict(carriers=20, bps=2, spreading=1)
DATA = 0x30
ZC_LEN = 2512
LEAD, GAP, TAIL = 14000, 9000, 40000


def _norm(s):
    return (s * F(0.8 / np.abs(s).max())).astype(F)


def payload3(seq):
    """35 bytes: with the 17-byte header and the frame CRC, three R1/4 codewords"""
    return ((np.arange(35) * 7 + seq) % 251).astype(np.uint8)


def tx_frame(O, frame, carriers=20, bps=2, B=None):
    coded = encode_frame(frame)
    if B is not None:
        coded = interleave_bytes(coded, B)
    return _norm(O.mcdpsk_wf_tx(carriers, po.DQPSK if bps == 2 else po.DBPSK, po.R1_4, 1, True, coded))


def cw_span(cw, carriers=20, bps=2):
    """the samples of a transmitted frame (tx_frame's output) whose symbols carry soft bits of codeword cw only, one symbol in
    from both ends (a differential symbol leans on the one before it)"""
    per = carriers * bps
    first, last = -(-cw * 648 // per) + 1, (cw + 1) * 648 // per - 1          # whole symbols inside [cw * 648, (cw + 1) * 648)
    base = ZC_LEN + 9 * 512
    return base + first * 512, base + last * 512


def harq_recording(O, seq, sigma, seeds, gap=GAP, carriers=20, bps=2, B=None, snr_db=25.0, chan_seed=1):
    """a 3-codeword data frame and its retransmission behind ZC preambles in the channel's noise (AWGN, snr_db), with Gaussian
    noise of standard deviation sigma on the symbols of codeword 1 of each reception, from numpy's generator at seeds[r]:
    (recording, frame bytes, the two frames' first samples)"""
    frame = data_frame(DATA, seq, payload3(seq))
    s = tx_frame(O, frame, carriers, bps, B)
    parts, at, pos = [np.zeros(LEAD, F)], [], LEAD
    for r in range(2):
        at.append(pos)
        parts += [s, np.zeros(gap if r == 0 else TAIL, F)]
        pos += len(s) + gap
    x = O.channel(0, snr_db, chan_seed, np.concatenate(parts).astype(F)).astype(F)
    a, b = cw_span(1, carriers, bps)
    for r in range(2):
        if sigma > 0:
            x[at[r] + a:at[r] + b] += (np.random.default_rng(seeds[r]).standard_normal(b - a) * sigma).astype(F)
    return np.ascontiguousarray(x, F), bytes(frame), at


# Found by a search on this restatement over sigma in {0.3, 0.45, 0.6} and the seed pairs (11, 12), (13, 14), ... (21, 22): the
# first at which reception 1 fails with a valid header and stores codeword 1, reception 2 fails on its own, and the sum of
# the two decodes to the transmitted bytes (at (13, 14) the sum passes the decoder's parity checks with a wrong byte, which
# decodeMCDPSKFrame cannot see).  At 0.45 and 0.6 no sum decodes.  tests/test_mcdpsk_stream_cpu.py asserts the claims.
HARQ_PIN = dict(seq=9, sigma=0.3, seeds=(15, 16))
# The cut captures of the re-entry tests.  The connected search reports a sync only once about 48 700 samples behind the
# frame's first sample have arrived (its cursor trails the write position by the 31 120-sample span, and the span starts
# 19 200 samples before the cursor that met the energy), so a capture cut inside a frame leaves a found sync only where the
# frame is longer than that: the 3-codeword frame at 10 carriers DBPSK (104 448 samples), and a 6-codeword frame at 20
# carriers DQPSK (56 832 samples; its 3-codeword frame, 30 720 samples, has ended before the search finds it).
CUT_CASES = {"c10_dbpsk_3cw": dict(carriers=10, bps=1, n_payload=35, frame_cw=3, cut_behind_sync=77000),
             "c20_dqpsk_6cw": dict(carriers=20, bps=2, n_payload=91, frame_cw=6, cut_behind_sync=56000)}


def clean_recording(O, seqs, carriers=20, bps=2, B=None, snr_db=20.0, chan_seed=3, gap=GAP, n_payload=35):
    """data frames of n_payload payload bytes (35: three codewords) behind ZC preambles, AWGN: (recording, the frames' bytes,
    their first samples)"""
    parts, sent, at, pos = [np.zeros(LEAD, F)], [], [], LEAD
    for seq in seqs:
        frame = data_frame(DATA, seq, ((np.arange(n_payload) * 7 + seq) % 251).astype(np.uint8))
        s = tx_frame(O, frame, carriers, bps, B)
        sent.append(bytes(frame))
        at.append(pos)
        parts += [s, np.zeros(gap, F)]
        pos += len(s) + gap
    parts.append(np.zeros(TAIL - gap, F))
    return np.ascontiguousarray(O.channel(0, snr_db, chan_seed, np.concatenate(parts).astype(F)), F), sent, at
