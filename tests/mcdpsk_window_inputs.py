"""The pinned table of windows for ria_gpu_mcdpsk_window_batch, shared by tests/test_mcdpsk_window_cpu.py (restatement on the
oracle against the fixture recorded from the compiled reference), tests/test_gpu_mcdpsk_window.py (the library against the
restatement) and tools/record_mcdpsk_window_golden.py.  10 carriers; the smallest geometry that can still go wrong: dual-chirp
windows of 2000 + 57600 + frame_len(3) + 2000 samples, ZC windows of 2000 + 2512 + frame_len(n) + 2000.  A call is one
invocation of the entry point: a configuration, a window length and its rows; calls that name a pool share chase caches, in
table order.  The table is an input, not a result: what each row does is asserted by assert_coverage and pinned by the fixture.
Test infrastructure only (not collected: no test_ prefix)."""
import numpy as np

import pyoracle as po
import mcdpsk_ci_inputs as MCI
import mcdpsk_window_restatement as MW
from mcdpsk_acquire_restatement import ACK, CONNECT, control_frame, data_frame, encode_frame, frame_len, window
from mcdpsk_harq_restatement import ChaseCache

LEAD, CHIRP_PRE, ZC_PRE = 2000, 57600, 2512
CHIRP_SEARCH = LEAD + CHIRP_PRE + 8 * 512
ZC_SEARCH = LEAD + ZC_PRE + 8 * 512
CHIRP_START = LEAD + CHIRP_PRE                      # where the detector places a clean frame (asserted by assert_coverage)
CHIRP_WL = LEAD + CHIRP_PRE + frame_len(3, 10, 1, 1) + 2000
CHIRP_SHORT_WL = LEAD + CHIRP_PRE + frame_len(1, 10, 1, 1) + 2000
SP4_WL = LEAD + CHIRP_PRE + frame_len(3, 10, 1, 4) + 2000
SP4_EARLY = max(frame_len(1, 10, 1, 4) // 2, 48000)           # checkIfReadyToDecode's early half-window (:1010)
ZC_WL = LEAD + ZC_PRE + frame_len(9, 10, 2, 1) + 2000          # holds a 9-codeword span: TOO_LONG, not NEED_SAMPLES
ZC_SHORT_WL = LEAD + ZC_PRE + frame_len(2, 10, 2, 1) + 2000

# the synthetic-tail rows: the training region is 0.5 throughout (training_rms 0.5 exactly), the 5000 samples behind it are
# 0.3f (TAIL_BODY) but for the last one, whose value (bit patterns below) makes the float32 chain give rms / 0.5 one ulp under
# 0.6f, 0.6f exactly and one ulp over; found by tools/record_mcdpsk_window_golden.py --search
TAIL_BODY = 0x3E99999A
TAIL_UNDER, TAIL_AT, TAIL_OVER = 0x3EA64C00, 0x3EA66000, 0x3EA67000

CONNECT3 = data_frame(CONNECT, 7, np.arange(25, dtype=np.uint8))
_cache = {}


def data_n(seq, n_cw):
    """a data frame of exactly n_cw codewords: 20 + 18 * (n_cw - 1) bytes or fewer"""
    return data_frame(0x30, seq, (np.arange(18 * (n_cw - 1) - 1 if n_cw > 1 else 1) % 251).astype(np.uint8))


def chirp_window(checker, frame, mod=po.DBPSK, wl=CHIRP_WL, kind=0, snr=10.0, seed=1, shift=0, spreading=1):
    coded = None if frame is None else encode_frame(frame)
    return window(checker, coded, 10, mod, spreading, True, LEAD, wl, kind, snr, seed, shift=shift)


def zc_window(checker, frame, wl=ZC_WL, kind=1, snr=3.0, seed=61, il=None):
    coded = None if frame is None else (encode_frame(frame) if il is None else MCI.coded_cws(frame, il))
    return window(checker, coded, 10, po.DQPSK, 1, False, LEAD, wl, kind, snr, seed)


def bare_chirp(checker, wl=CHIRP_WL, noise=None):
    """the dual-chirp preamble alone (a PING): in silence, or in the channel's noise"""
    w = np.zeros(wl, np.float32)
    pre = checker.mcdpsk_wf_tx(10, po.DBPSK, po.R1_4, 1, False, encode_frame(control_frame(ACK, 1)))[:CHIRP_PRE]
    w[LEAD:LEAD + CHIRP_PRE] = (pre * np.float32(0.8 / np.abs(pre).max())).astype(np.float32)
    return w if noise is None else checker.channel(0, noise[0], noise[1], w)


def ping(checker, snr, seed):
    """what StreamingEncoder::encodePing sends: the dual chirp, training and reference symbol, no data; in the channel's noise"""
    w = np.zeros(CHIRP_WL, np.float32)
    s = checker.mcdpsk_wf_tx(10, po.DBPSK, po.R1_4, 1, False, encode_frame(control_frame(ACK, 1)))[:CHIRP_PRE + 4608]
    w[LEAD:LEAD + len(s)] = (s * np.float32(0.8 / np.abs(s).max())).astype(np.float32)
    return checker.channel(0, snr, seed, w)


def synthetic_tail(checker, tail_bits):
    """a clean chirp, then a training region of 0.5 and 5000 samples of TAIL_BODY, the last one tail_bits, behind it"""
    w = bare_chirp(checker)
    w[CHIRP_START:CHIRP_START + 4608] = np.float32(0.5)
    w[CHIRP_START + 4608:CHIRP_START + 9608] = np.array([TAIL_BODY], np.uint32).view(np.float32)[0]
    w[CHIRP_START + 9607] = np.array([tail_bits], np.uint32).view(np.float32)[0]
    return w


def poisoned(checker, frame, at, value, **kw):
    """a window with one sample behind the detector's span replaced: at < 4608 lies in the training region, else in the data region"""
    w = chirp_window(checker, frame, **kw).copy()
    w[CHIRP_START + at] = np.float32(value)
    return w


def R(name, purpose, build, **kw):
    return dict(name=name, purpose=purpose, build=build, kw=kw)


DISC = dict(carriers=10, bps=1, spreading=1, chirp=True, disconnected=True, retry=True, B=None)
ZC = dict(carriers=10, bps=2, spreading=1, chirp=False, disconnected=False, retry=True, B=None)


def calls():
    """-> the calls in table order: dict(name, cfg, search_len, wl, pool, now, rows)"""
    c = []
    c.append(dict(name="chirp_disconnected", cfg=DISC, search_len=CHIRP_SEARCH, wl=CHIRP_WL, pool=None, now=0, rows=[
        R("ping_silence", "a bare chirp in silence: training_rms <= 0.001, ratio 0, PING", lambda k: bare_chirp(k)),
        R("chirp_in_noise", "a bare chirp in noise: ratio near 1, not a PING; no header, fallback to 3, every candidate fails",
          lambda k: bare_chirp(k, noise=(0.0, 3))),
        R("ping_preamble", "a PING as the encoder sends it, in noise at 10 dB: the data region holds noise only, PING", lambda k: ping(k, 10.0, 7)),
        R("tail_under", "ratio just under 0.6f: PING", lambda k: synthetic_tail(k, TAIL_UNDER)),
        R("tail_at", "ratio 0.6f exactly: not a PING", lambda k: synthetic_tail(k, TAIL_AT)),
        R("tail_over", "ratio just over 0.6f: not a PING", lambda k: synthetic_tail(k, TAIL_OVER)),
        R("nan_training", "a NaN in the training region: training_rms NaN, ratio 0, PING", lambda k: poisoned(k, CONNECT3, 4300, np.nan)),
        R("inf_training", "an Inf in the training region: ratio 0, PING", lambda k: poisoned(k, CONNECT3, 4300, np.inf)),
        R("connect_dbpsk", "CONNECT of 3 codewords in place: header multi, decoded at 3", lambda k: chirp_window(k, CONNECT3)),
        R("connect_dqpsk", "CONNECT sent DQPSK: the peek sees nothing, fallback to 3, the alternate modulation recovers it",
          lambda k: chirp_window(k, CONNECT3, mod=po.DQPSK, snr=12.0, seed=5)),
        R("connect_shift16", "CONNECT 16 samples behind the detector's place: recovered by a delta",
          lambda k: chirp_window(k, CONNECT3, kind=1, snr=-6.0, seed=106, shift=16)),
        R("connect_says_1", "a CONNECT header announcing total_cw 1: the peek's guard forces 3, the decode's guard rejects",
          lambda k: chirp_window(k, data_frame(CONNECT, 8, np.arange(25, dtype=np.uint8), total_cw=1), seed=2)),
        R("connect_says_2", "a CONNECT header announcing total_cw 2: forced to 3",
          lambda k: chirp_window(k, data_frame(CONNECT, 9, np.arange(25, dtype=np.uint8), total_cw=2), seed=3)),
        R("ack_disconnected", "a 1-codeword ACK: header single, the handshake fallback asks for 3, decoded as 1 of 3",
          lambda k: chirp_window(k, control_frame(ACK, 40), seed=4)),
        R("data2_disconnected", "a 2-codeword data frame: header multi to 2, the handshake window raises it to 3",
          lambda k: chirp_window(k, data_n(41, 2), seed=6)),
        R("replay_199", "the CONNECT window with the last decoded sync 199 samples back: REPLAY",
          lambda k: chirp_window(k, CONNECT3), last_decoded_sync=CHIRP_START - 199),
        R("replay_200", "... 200 samples back: decoded", lambda k: chirp_window(k, CONNECT3), last_decoded_sync=CHIRP_START - 200),
        R("replay_ahead_199", "... 199 samples ahead: REPLAY", lambda k: chirp_window(k, CONNECT3), last_decoded_sync=CHIRP_START + 199),
        R("noise_only", "noise: not detected", lambda k: chirp_window(k, None, seed=9)),
        R("reentry_3", "the re-entry of connect_cut_short with pending 3: no peek, decoded", lambda k: chirp_window(k, CONNECT3),
          pending_total_cw=3),
        R("reentry_1", "a re-entry with pending 1: the handshake window raises it to 3", lambda k: chirp_window(k, CONNECT3), pending_total_cw=1),
        R("reentry_9", "a re-entry with pending 9: the span does not fit the window, not accepted", lambda k: chirp_window(k, CONNECT3),
          pending_total_cw=9),
        R("early_full", "first_avail above the 1-codeword span: the whole span", lambda k: chirp_window(k, CONNECT3), first_avail=40000),
        R("early_half", "first_avail 20000 < the 1-codeword span: early window, 1, then 3", lambda k: chirp_window(k, CONNECT3),
          first_avail=20000),
        R("early_ping", "an early window on a bare chirp: PING on 9608 samples", lambda k: bare_chirp(k), first_avail=9608),
    ]))
    c.append(dict(name="chirp_no_retry", cfg=dict(DISC, retry=False), search_len=CHIRP_SEARCH, wl=CHIRP_WL, pool=None, now=0, rows=[
        R("nan_data", "a NaN in the data region: rms NaN, ratio NaN, not a PING", lambda k: poisoned(k, CONNECT3, 5000, np.nan)),
        R("inf_data", "an Inf in the data region: ratio Inf, not a PING", lambda k: poisoned(k, CONNECT3, 5000, np.inf)),
        R("connect_dqpsk_primary_only", "CONNECT sent DQPSK without the fallbacks: the primary's failure is the result",
          lambda k: chirp_window(k, CONNECT3, mod=po.DQPSK, snr=12.0, seed=5)),
    ]))
    c.append(dict(name="chirp_cut_short", cfg=DISC, search_len=CHIRP_SEARCH, wl=CHIRP_SHORT_WL, pool=None, now=0, rows=[
        R("connect_cut_short", "a window that ends behind CW0: header multi, NEED_SAMPLES for 3",
          lambda k: chirp_window(k, CONNECT3, wl=CHIRP_SHORT_WL)),
        R("ack_cut_short", "an ACK in the short window: the fallback waits for 3", lambda k: chirp_window(k, control_frame(ACK, 40), wl=CHIRP_SHORT_WL, seed=4)),
        R("early_cut_short", "an early window in the short window: 1, then NEED_SAMPLES for 3",
          lambda k: chirp_window(k, CONNECT3, wl=CHIRP_SHORT_WL), first_avail=20000),
    ]))
    c.append(dict(name="chirp_spreading4", cfg=dict(DISC, spreading=4), search_len=CHIRP_SEARCH, wl=SP4_WL, pool=None, now=0, rows=[
        R("early_spreading4", "first_avail below one codeword at 4x spreading: pending 1, then 3, decoded",
          lambda k: chirp_window(k, CONNECT3, wl=SP4_WL, spreading=4), first_avail=SP4_EARLY),
    ]))
    c.append(dict(name="zc_connected", cfg=ZC, search_len=ZC_SEARCH, wl=ZC_WL, pool=None, now=0, rows=[
        R("ack_connected", "the ACK over ZC, connected: header single, falls through on 1 codeword",
          lambda k: zc_window(k, control_frame(ACK, 22), seed=62)),
        R("data2", "a connected data frame of 2 codewords", lambda k: zc_window(k, data_n(50, 2), seed=64)),
        R("data3", "... of 3", lambda k: zc_window(k, data_n(51, 3), seed=65)),
        R("data5", "... of 5", lambda k: zc_window(k, data_n(52, 5), seed=66)),
        R("data8", "... of 8", lambda k: zc_window(k, data_n(53, 8), seed=67)),
        R("header_9", "a header announcing 9 codewords in a window that holds them: TOO_LONG",
          lambda k: zc_window(k, data_frame(0x30, 54, np.arange(25, dtype=np.uint8), total_cw=9), seed=68)),
        R("connect_says_1_connected", "a CONNECT announcing 1 while connected: no forcing, falls through, the decode's guard rejects",
          lambda k: zc_window(k, data_frame(CONNECT, 8, np.arange(25, dtype=np.uint8), total_cw=1), seed=69)),
        R("zc_noise", "noise over ZC", lambda k: zc_window(k, None, seed=63)),
        R("zc_replay", "the ACK with the last decoded sync at its place: REPLAY", lambda k: zc_window(k, control_frame(ACK, 22), seed=62),
          last_decoded_sync=LEAD + ZC_PRE),
        R("zc_reentry_5", "the 5-codeword frame on re-entry with pending 5", lambda k: zc_window(k, data_n(52, 5), seed=66), pending_total_cw=5),
    ]))
    c.append(dict(name="zc_cut_short", cfg=ZC, search_len=ZC_SEARCH, wl=ZC_SHORT_WL, pool=None, now=0, rows=[
        R("data3_cut_short", "3 codewords in a window that holds 2: NEED_SAMPLES", lambda k: zc_window(k, data_n(51, 3), wl=ZC_SHORT_WL, seed=65)),
        R("data2_fits", "2 codewords in the same window: decoded", lambda k: zc_window(k, data_n(50, 2), wl=ZC_SHORT_WL, seed=64)),
    ]))
    # the channel-interleaved link with a chase pool: mcdpsk_ci_inputs.zc_windows' two receptions (an interleaved data frame,
    # a plain ACK, noise, an interleaved data frame whose CW2 arrives weak twice) into caches 0..3
    for call in range(2):
        c.append(dict(name=f"zc_interleaved_chase_{call}", cfg=dict(ZC, B=20), search_len=MCI.ZC_SEARCH, wl=MCI.ZC_WL, pool="link", now=1000 * call,
                      rows=[R(f"ci_{n}_{call}", p, (lambda k, i=i, call=call: zc_pair(k)[call][i]))
                            for i, (n, p) in enumerate((("data3", "interleaved data: the de-interleaved CW0 decides"), ("ack", "a plain ACK on the interleaved link"),
                                                        ("noise", "noise: both CW0 decodes fail"),
                                                        ("weak_cw2", "CW2 weak in both receptions: stored, then combined")))]))
    return c


def zc_pair(checker):
    key = ("zc_pair", type(checker).__name__)
    if key not in _cache:
        _cache[key] = MCI.zc_windows(checker)
    return _cache[key]


def rows():
    return [r for c in calls() for r in c["rows"]]


def build(checker, call):
    """the call's windows float32 [rows, wl] and its per-window inputs"""
    key = (call["name"], type(checker).__name__)
    if key not in _cache:
        x = np.stack([np.ascontiguousarray(r["build"](checker), np.float32) for r in call["rows"]])
        assert x.shape[1] == call["wl"], (call["name"], x.shape)
        _cache[key] = x
    kw = {k: np.array([r["kw"].get(k, d) for r in call["rows"]], np.int64) for k, d in
          (("pending_total_cw", 0), ("first_avail", 0), ("last_decoded_sync", MW.NO_LAST_SYNC))}
    return _cache[key], kw


def expected_call(checker, call, x, kw, caches=None, order=None):
    """the restatement over the call's rows (in `order`, default table order; chase caches: one per row) -> list in table order"""
    cfg = call["cfg"]
    out = [None] * len(x)
    for i in (range(len(x)) if order is None else order):
        out[i] = MW.mcdpsk_window(checker, x[i], call["search_len"], carriers=cfg["carriers"], bps=cfg["bps"], spreading=cfg["spreading"],
                                  chirp=cfg["chirp"], disconnected=cfg["disconnected"], retry=cfg["retry"], B=cfg["B"],
                                  cache=None if caches is None else caches[i], now=call["now"],
                                  pending_total_cw=int(kw["pending_total_cw"][i]), first_avail=int(kw["first_avail"][i]),
                                  last_decoded_sync=int(kw["last_decoded_sync"][i]))
    return out


def expected_all(checker):
    """-> [(call, windows, kw, expected rows)] for the whole table, pools carried from call to call"""
    key = ("expected", type(checker).__name__)
    if key not in _cache:
        pools, out = {}, []
        for call in calls():
            x, kw = build(checker, call)
            caches = None
            if call["pool"] is not None:
                caches = pools.setdefault(call["pool"], [ChaseCache() for _ in range(len(x))])
            out.append((call, x, kw, expected_call(checker, call, x, kw, caches)))
        _cache[key] = out
    return _cache[key]


UNREACHED = {
    "PROCESS_FAILED": "process() of the MC-DPSK demodulator after an external detection fails only on a span without a data symbol; "
                      "every span here has >= 9608 samples = 9 symbols behind the training, so >= 2 data symbols at any spreading",
    "SALVAGE": "the peek of the same pass parses the same CW0 decode first and escalates every valid header with total_cw > avail_cw; "
               "the CONNECT headers it treats differently are rejected by decodeMCDPSKFrame with codewords_ok 0",
}


def assert_coverage(checker):
    """every outcome and every peek statement is reached by at least one row, except those listed in UNREACHED"""
    outcomes, whats, bits = set(), set(), set()
    named = {}
    for call, x, kw, exp in expected_all(checker):
        for r, e in zip(call["rows"], exp):
            named[r["name"]] = e
            outcomes.add(MW.OUTCOMES[e["outcome"]])
            whats.add(MW.WHAT[e["peek"] & 0xF])
            bits |= {n for n, b in MW.BITS.items() if e["peek"] & b}
    assert outcomes == set(MW.OUTCOMES) - {"PROCESS_FAILED"}, outcomes
    assert whats == set(MW.WHAT), whats
    assert bits == set(MW.BITS) - {"SALVAGE"}, bits
    assert set(UNREACHED) == {"PROCESS_FAILED", "SALVAGE"}
    # what the rows were built for
    o = lambda n: MW.OUTCOMES[named[n]["outcome"]]
    assert all(named[n]["acq"]["sync_start"] == CHIRP_START for n in ("connect_dbpsk", "ping_silence", "tail_at"))
    t = lambda n: np.float32(named[n]["rms"]) / np.float32(named[n]["training_rms"])
    assert [o(n) for n in ("ping_silence", "ping_preamble", "tail_under", "nan_training", "inf_training", "early_ping")] == ["PING"] * 6
    assert np.float32(0.1) < t("ping_preamble") < np.float32(0.6)
    assert named["ping_silence"]["training_rms"] <= np.float32(0.001)
    assert [o(n) for n in ("chirp_in_noise", "tail_at", "tail_over", "nan_data", "inf_data")] == ["DECODED"] * 5
    assert t("tail_under") < np.float32(0.6) and t("tail_at") == np.float32(0.6) and t("tail_over") > np.float32(0.6)
    assert np.isnan(named["nan_data"]["rms"]) and np.isinf(named["inf_data"]["rms"]) and np.isnan(named["nan_training"]["training_rms"])
    e = named["connect_dbpsk"]
    assert (e["peek"], e["pending_total_cw"], e["acq"]["success"], e["acq"]["codewords_ok"], e["acq"]["candidates"]) == (MW.HEADER_MULTI, 3, 1, 3, 1)
    e = named["connect_dqpsk"]
    assert e["peek"] == MW.NO_HEADER | MW.HANDSHAKE_FALLBACK and e["acq"]["success"] == 1 and e["acq"]["candidates"] == 2 and e["acq"]["modulation"] == po.DQPSK
    e = named["connect_shift16"]
    assert e["acq"]["success"] == 1 and e["acq"]["delta"] == 16 and e["next_pos"] == e["acq"]["sync_start"] + 16 + e["frame_len"]
    for n, total in (("connect_says_1", 1), ("connect_says_2", 2)):
        e = named[n]
        assert (e["peek"], e["peek_total_cw"], e["pending_total_cw"], e["acq"]["success"], e["acq"]["codewords_ok"]) == (MW.CONNECT_FORCED, total, 3, 0, 0)
    e = named["ack_disconnected"]
    assert (e["peek"], e["pending_total_cw"], e["acq"]["success"], e["acq"]["frame_type"]) == (MW.HEADER_SINGLE | MW.HANDSHAKE_FALLBACK, 3, 1, ACK)
    e = named["data2_disconnected"]
    assert e["peek"] == MW.HEADER_MULTI | MW.HANDSHAKE_WINDOW and e["passes"] == 3 and e["acq"]["success"] == 1
    assert [o(n) for n in ("replay_199", "replay_200", "replay_ahead_199", "zc_replay")] == ["REPLAY", "DECODED", "REPLAY", "REPLAY"]
    assert o("noise_only") == "NOT_ACCEPTED" and o("reentry_9") == "NOT_ACCEPTED" and named["reentry_9"]["acq"]["detected"] == 1
    assert (named["reentry_3"]["peek"], named["reentry_3"]["passes"], named["reentry_3"]["acq"]["success"]) == (0, 1, 1)
    assert (named["reentry_1"]["peek"], named["reentry_1"]["passes"], named["reentry_1"]["acq"]["success"]) == (MW.HANDSHAKE_WINDOW, 2, 1)
    assert named["early_full"]["peek"] == MW.HEADER_MULTI
    for n in ("early_half", "early_spreading4"):
        assert (named[n]["peek"], named[n]["passes"], named[n]["acq"]["success"]) == (MW.EARLY_WINDOW | MW.HANDSHAKE_WINDOW, 3, 1), n
    e = named["connect_cut_short"]
    assert (o("connect_cut_short"), e["pending_total_cw"], e["need_samples"], e["next_pos"]) == ("NEED_SAMPLES", 3, frame_len(3, 10, 1, 1), -1)
    assert o("ack_cut_short") == "NEED_SAMPLES" and o("early_cut_short") == "NEED_SAMPLES" and named["early_cut_short"]["passes"] == 2
    e = named["ack_connected"]
    assert (e["peek"], e["pending_total_cw"], e["frame_len"], e["acq"]["success"]) == (MW.HEADER_SINGLE, 0, frame_len(1, 10, 2, 1), 1)
    for n, cw in (("data2", 2), ("data3", 3), ("data5", 5), ("data8", 8)):
        e = named[n]
        assert (e["peek"], e["pending_total_cw"], e["acq"]["success"], e["acq"]["codewords_ok"], e["frame_len"]) == \
            (MW.HEADER_MULTI, cw, 1, cw, frame_len(cw, 10, 2, 1)), n
    assert (o("header_9"), named["header_9"]["pending_total_cw"]) == ("TOO_LONG", 9)
    e = named["connect_says_1_connected"]
    assert (e["peek"], o("connect_says_1_connected"), e["acq"]["codewords_ok"]) == (MW.HEADER_SINGLE, "DECODED", 0)
    assert named["zc_reentry_5"]["acq"]["success"] == 1 and named["zc_reentry_5"]["peek"] == 0
    assert (o("data3_cut_short"), o("data2_fits")) == ("NEED_SAMPLES", "DECODED")
    e = named["ci_data3_0"]
    assert e["peek"] == MW.HEADER_MULTI | MW.DEINTERLEAVED and e["acq"]["success"] == 1 and e["acq"]["cw0_deinterleaved"] == 1
    assert named["ci_ack_0"]["peek"] == MW.HEADER_SINGLE and o("ci_noise_0") == "NOT_ACCEPTED"
    a, b = named["ci_weak_cw2_0"], named["ci_weak_cw2_1"]
    assert a["acq"]["success"] == 0 and a["harq"]["stored_mask"] == 4 and b["acq"]["success"] == 1 and b["harq"]["recovered_mask"] == 4
