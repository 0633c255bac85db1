"""The pinned windows of the ria_gpu_rx_window_batch tests (test_window_cpu.py, test_gpu_window.py,
tools/record_window_golden.py): every window is a function of small integers - link, frame kind, seq, lead, channel kind,
SNR, seed, transmitter CFO - so nothing large is committed.  Each row names the statement of the ladder it is there for.

Frame kinds (frames built with the oracle's encoders, peak 0.8):
    ack          ACK control frame, one R1/4 codeword sent with the DQPSK R1/4 control profile
    fixed        encodeFixedFrame data frame (4 codewords) on the link
    varT         data frame of T codewords at the link rate, encodeFrameWithLDPC layout, sent with the data profile
    one_r14      one codeword at R1/4 with a valid data header, total_cw 1, sent with the data profile
    hdr3_r14     the same with total_cw 3 in the header (nothing behind it)
    bad_r14      a codeword at R1/4 with the magic and an inverted header CRC, sent with the data profile
    bad_rate     the same at the link rate
    hdr5         a CW0 at the link rate whose valid header says total_cw 5
    ack_data     an ACK control frame, one R1/4 codeword, sent with the DATA profile
    connect2     a 2-codeword frame of a connect-family type (0x12) at the link rate, sent with the data profile
    None         nothing is sent: the channel's noise, or (channel None) silence

Test infrastructure only (not collected: no test_ prefix)."""
import numpy as np

import pyoracle as po
import control_inputs as CI
import control_restatement as CR
import decode_frame_inputs as DI
import decode_frame_restatement as DF
import window_restatement as WR

AWGN, MODERATE = 0, 2
LINKS = {"dqpsk_r14": (po.DQPSK, po.R1_4), "dqpsk_r12": (po.DQPSK, po.R1_2), "d8psk_r12": (po.D8PSK, po.R1_2),
         "qam16_r12": (po.QAM16, po.R1_2), "qam256_r34": (po.QAM256, po.R3_4)}
LINK_NAMES = {"dqpsk_r14": ("DQPSK", "R1_4"), "dqpsk_r12": ("DQPSK", "R1_2"), "d8psk_r12": ("D8PSK", "R1_2"),
              "qam16_r12": ("QAM16", "R1_2"), "qam256_r34": ("QAM256", "R3_4")}
LEAD = 300
SEARCH_LEN = LEAD + 4 * CR.SYM
MIN_CONF = 0.5


def row(name, link, kind, seq, seed, purpose, lead=LEAD, chan=AWGN, snr=20.0, cfo=0.0, known=0.0, wlen=None, marked=0, interleave=0,
        min_conf=MIN_CONF, det_thr=0.15, retry=1, shift=0):
    """wlen: None (lead + a 4-codeword frame + 40), "short" / "exact" (cut one sample short of / exactly at pass 2's span of
    4 codewords behind the detected start), "long5" (room for 5 codewords).  retry 0: the row runs under
    RIA_ACQ_NO_TIMING_RETRY (rows whose eight failing candidates would only cost the CPU restatement time)."""
    return dict(name=name, link=link, kind=kind, seq=seq, seed=seed, purpose=purpose, lead=lead, chan=chan, snr=snr, cfo=cfo, known=known,
                wlen=wlen, marked=marked, interleave=interleave, min_conf=min_conf, det_thr=det_thr, retry=retry, shift=shift)


def _link_rows(link, base):
    rows = [
        row(f"{link}_ack", link, "ack", 1, base + 1, "control path"),
        row(f"{link}_fixed", link, "fixed", 2, base + 2, "peek fails or QAM partial, pending 4, pass 2 at the fed-back CFO"),
        row(f"{link}_fixed_cfo1p5", link, "fixed", 3, base + 3, "pass 2 demodulated at the peek's CFO estimate", cfo=1.5),
        row(f"{link}_var1", link, "var1", 6, base + 6, "one codeword at the rate: RATE_ONE (R14_ONE on an R1/4 link)"),
        # on D8PSK the CW0 peek of these two fails (pending 4) and the 4-codeword span decodes nothing: primary candidate only
        row(f"{link}_var2", link, "var2", 7, base + 7, "RATE_MULTI, pass 2 of exactly 2 codewords, legacy path", retry=int(link != "d8psk_r12")),
        row(f"{link}_var3", link, "var3", 8, base + 8, "RATE_MULTI, pass 2 of exactly 3 codewords, legacy path", retry=int(link != "d8psk_r12")),
    ]
    # the pilot estimator follows a transmitter CFO of 3 Hz on every link (estimate within 0.1 Hz), so the feedback lands on
    # known +- 2 exactly; at 5 Hz it gives up and reports the known CFO everywhere but on the short QAM256 span
    cheap = int(link == "qam256_r34")
    rows += [row(f"{link}_fixed_cfo_p3", link, "fixed", 9, base + 9, "the clamp lands on known + 2 exactly", cfo=3.0, retry=0),
             row(f"{link}_fixed_cfo_m3", link, "fixed", 10, base + 10, "the clamp lands on known - 2 exactly", cfo=-3.0, retry=0),
             row(f"{link}_fixed_cfo_p5", link, "fixed", 4, base + 4, "true CFO +5 Hz", cfo=5.0, retry=cheap),
             row(f"{link}_fixed_cfo_m5", link, "fixed", 5, base + 5, "true CFO -5 Hz", cfo=-5.0, retry=cheap)]
    return rows


ROWS = []
for _i, _l in enumerate(LINKS):
    ROWS += _link_rows(_l, 1000 + 100 * _i)
_Q = "qam16_r12"
ROWS += [
    row("one_r14", "dqpsk_r12", "one_r14", 20, 2001, "R14_ONE on an R1/2 link"),
    row("hdr3_r14", "dqpsk_r12", "hdr3_r14", 21, 2002, "R14_MULTI: pending 3 from the R1/4 decode"),
    row("bad_r14", "dqpsk_r12", "bad_r14", 22, 2003, "R1/4 decodes with a bad header: the rate fallback runs, then FAILED", retry=0),
    row("bad_rate", "dqpsk_r12", "bad_rate", 23, 2004, "RATE_BAD_HEADER: pending 4"),
    row("bad_r14_on_r14", "dqpsk_r14", "bad_r14", 24, 2005, "R1/4 link: a bad header is FAILED, no rate fallback"),
    row("hdr5_short", "dqpsk_r12", "hdr5", 25, 2006, "total_cw 5 in a window too short for it: NEED_SAMPLES"),
    row("hdr5_long", "dqpsk_r12", "hdr5", 25, 2006, "total_cw 5 with room: TOO_LONG", wlen="long5"),
    row("need_samples", _Q, "fixed", 26, 2007, "pass 2's span ends one sample behind the window: NEED_SAMPLES", wlen="short"),
    row("need_exact", _Q, "fixed", 26, 2007, "pass 2's span ends on the window's last sample", wlen="exact"),
    row("noise", "qam256_r34", None, 0, 2008, "noise accepted through a low min_confidence: small-frame finds nothing, eight candidates", min_conf=0.0, det_thr=0.0),
    row("noise_q16", _Q, None, 0, 2008, "the same on a link whose peek escalates (QAM_PARTIAL), primary candidate only", min_conf=0.0, det_thr=0.0, retry=0),
    row("silence", _Q, None, 0, 2009, "a silent window", chan=None, min_conf=0.0, det_thr=0.0),
    row("marker", _Q, "fixed", 27, 2010, "a marked window without RIA_BURST_INTERLEAVE: the marker is consumed by the control hypothesis", marked=1, retry=0),
    row("marker_il", _Q, "fixed", 27, 2010, "the same under RIA_BURST_INTERLEAVE: RIA_WIN_BURST", marked=1, interleave=1),
    row("nan_peek", _Q, "fixed", 28, 2011, "non-finite samples in the peek span", retry=0),
    row("not_detected", _Q, None, 0, 2012, "noise at the ordinary thresholds: RIA_WIN_NOT_ACCEPTED"),
    row("ack_data_d8", "d8psk_r12", "ack_data", 40, 2101, "consumed rule: an ACK codeword sent with the data profile is decoded by decodeFrame on "
        "the peek span (R14_ONE, CONTROL_R14) and consumes one codeword's samples, not frame_len"),
    row("ack_data_q16", _Q, "ack_data", 40, 2102, "consumed rule after escalation: the ACK is decoded on the 4-codeword span and consumes one codeword's samples"),
    row("connect2_dq12", "dqpsk_r12", "connect2", 41, 2105, "consumed rule: a 2-codeword connect-family frame on its exact span"),
    row("connect2_q16", _Q, "connect2", 41, 2104, "small-frame recovery's exact-size branch sets frame_len to 2 codewords; timing recovery then delivers the "
        "frame at +8 on that span"),
    row("data_shift16", _Q, "fixed", 42, 2106, "data symbols 16 samples behind the training symbols: 3 of 4 codewords, so codewords_ok > 0 keeps "
        "timing recovery off", shift=16),
    # rows whose link, channel and seed come from tools/record_window_golden.py --search (SEARCHED below).  Recovery at +8 is
    # qam16_r12_fixed's, the exact-size branch of small-frame recovery is entered by qam16_r12_var3 and hdr3_r14, by construction.
    row("delta_m16", _Q, "fixed", 31, 0, "timing recovery by decodeFrame: recovered at -16"),
    row("small_one", _Q, "var1", 31, 0, "small-frame: the one-codeword branch at R1/4 (CW0 decodes on the factor ladder only: decodeFrame's plain probe fails again)"),
    row("small_one_rate", _Q, "var1", 31, 0, "small-frame: the one-codeword branch at the rate"),
]
SEARCHED = {"delta_m16": dict(link="qam16_r12", kind="fixed", seq=31, chan=MODERATE, snr=12.0, seed=7007),
            "small_one": dict(link="dqpsk_r14", kind="var1", chan=MODERATE, snr=3.0, seed=6045),
            "small_one_rate": dict(link="dqpsk_r12", kind="var1", chan=MODERATE, snr=3.0, seed=6006)}
SMALL_FRAME_WAIVER = {}          # small_frame value -> the search's record, for a value 2 or 3 no seed reaches
# The record of tools/record_window_golden.py --search (SMALL_SEARCH_POINTS x SMALL_SEARCH_SEEDS: QAM16 R1/2 frames of 2 and 3
# codewords followed by noise, AWGN and Watterson moderate, 12 / 10 / 8 / 6 / 5 / 4 dB, seeds 5000 .. 5039, primary candidate only),
# per lead: windows, windows that entered small-frame recovery, windows that took one of its two branches, windows whose
# branch turned the failure into a success.  No seed of the range does: the span that fails on 4 codewords fails on its exact
# size too.  What the branch changes is frame_len, and with it what timing recovery decodes: connect2_q16 is delivered at +8 on
# the 2-codeword span the exact-size branch left.
SMALL_FRAME_SEARCH = {300: (960, 737, 346, 0), 302: (960, 735, 317, 0)}


def rows():
    out = []
    for r in ROWS:
        if r["name"] in SEARCHED:
            r = dict(r, **SEARCHED[r["name"]])     # what the search found: link, kind, channel kind, snr, seed
        out.append(r)
    return out


def reference_rows():
    """the rows the compiled reference's waveform can run: its configure() has no QAM256 (ofdm_chirp_waveform.cpp:81-89)"""
    return [r for r in rows() if r["link"] != "qam256_r34"]


def geometry(link):
    mod, rate = LINKS[link]
    bps = WR.po_oracle(None).geom(mod, rate).bits_per_symbol
    return dict(bps=bps, n_ctl=CR.control_frame_samples(mod, rate), frame=WR.samples_for_cw(bps, 4), window_len=LEAD + WR.samples_for_cw(bps, 4) + 40)


def _pack(bits):
    return np.packbits(np.asarray(bits, np.uint8))


def _cw0_frame(rate, seq, total):
    """a data frame's first codeword worth of bytes with total_cw = total in a valid header"""
    bpc = DF.bytes_per_cw(rate)
    payload = ((np.arange(bpc - 19) * 5 + seq) % 251).astype(np.uint8)
    return DF.data_frame(DI.DATA, seq, payload, total_cw=total)[:bpc]


def clean_samples(checker, r):
    """the transmitted samples of a row (None: nothing is sent)"""
    mod, rate = LINKS[r["link"]]
    kind, seq = r["kind"], r["seq"]
    O = WR.po_oracle(checker)
    bps = O.geom(mod, rate).bits_per_symbol
    if kind is None:
        return None
    if kind == "ack":
        return CI.clean_samples(checker, "ack", seq)
    if kind == "fixed":
        bpc = DF.bytes_per_cw(rate)
        s = checker.tx_frame(mod, rate, ((np.arange(4 * bpc - 24) * 3 + seq) % 251).astype(np.uint8), seq)[0]
        return (s * (np.float32(0.8) / np.abs(s).max())).astype(np.float32)
    if kind.startswith("var"):
        coded = _pack(DI.legacy_bits(rate, bps, True, DI.legacy_frame(rate, seq, int(kind[3]))))
    elif kind == "one_r14":
        coded = _pack(DI._encode_cw(po.R1_4, _cw0_frame(po.R1_4, seq, 1)))
    elif kind == "hdr3_r14":
        coded = _pack(DI._encode_cw(po.R1_4, _cw0_frame(po.R1_4, seq, 3)))
    elif kind in ("bad_r14", "bad_rate"):
        rt = po.R1_4 if kind == "bad_r14" else rate
        f = _cw0_frame(rt, seq, 2).copy()
        f[15] ^= 0xFF
        f[16] ^= 0xFF
        coded = _pack(DI._encode_cw(rt, f))
    elif kind == "ack_data":
        coded = _pack(DI._encode_cw(po.R1_4, CR.control_frame(CR.ACK, seq)))
    elif kind == "connect2":
        f = DI.legacy_frame(rate, seq, 2).copy()
        f[2] = 0x12                                   # a connect-family type; the header CRC covers it
        c = DF.crc16(f[:15])
        f[15], f[16] = c >> 8, c & 0xFF
        coded = _pack(DI.legacy_bits(rate, bps, True, f))
    elif kind == "hdr5":
        coded = _pack(DI._encode_cw(rate, _cw0_frame(rate, seq, 5)))
    else:
        raise ValueError(kind)
    return CR.tx_var(checker, mod, rate, coded)


_cache = {}


def window(checker, r):
    """-> (window float32, kwargs of window_restatement.rx_window / RxEngine.rx_window's per-window values)"""
    key = (type(checker).__name__, r["name"])
    if key in _cache:
        return _cache[key]
    g = geometry(r["link"])
    full = LEAD + WR.samples_for_cw(g["bps"], 5) + 40
    w = np.zeros(full, np.float32)
    s = clean_samples(checker, r)
    if s is not None:
        s = s.copy()
        if r["marked"]:
            s[:CR.SYM] = -s[:CR.SYM]
        if r["cfo"]:
            s = checker.apply_tx_cfo(s, r["cfo"])[0]
        if r.get("shift"):        # the data symbols displaced against the two training symbols
            t = 2 * CR.SYM
            w[r["lead"]:r["lead"] + t] = s[:t]
            w[r["lead"] + t + r["shift"]:r["lead"] + r["shift"] + len(s)] = s[t:]
        else:
            w[r["lead"]:r["lead"] + len(s)] = s
    if r["chan"] is not None:
        w = checker.channel(r["chan"], r["snr"], int(r["seed"]), w)
    if r["name"] == "nan_peek":
        w[r["lead"] + 3 * CR.SYM + 17] = np.float32(np.nan)
        w[r["lead"] + 5 * CR.SYM + 5] = np.float32(np.inf)
    wlen = g["window_len"]
    if r["wlen"] == "long5":
        wlen = full
    elif r["wlen"] in ("short", "exact"):
        det = checker.detect_data_sync(w[:SEARCH_LEN], r["known"], r["det_thr"]) if isinstance(checker, po.Oracle) else \
            checker.detect_data_sync(w[:SEARCH_LEN], r["known"], r["det_thr"], *LINKS[r["link"]])
        assert det[0]
        wlen = int(det[1]) + g["frame"] - (1 if r["wlen"] == "short" else 0)
    out = np.ascontiguousarray(w[:wlen]), dict(known_cfo=r["known"], detect_threshold=r["det_thr"], min_confidence=r["min_conf"],
                                               abs_base=1000 * r["seq"] + int(r["seed"]) % 997 + 7, interleave=bool(r["interleave"]), retry=bool(r["retry"]))
    _cache[key] = out
    return out


_expected = {}


def expected(checker, r):
    """the restatement's result of a row, computed once per checker"""
    key = (type(checker).__name__, r["name"])
    if key not in _expected:
        w, kw = window(checker, r)
        _expected[key] = WR.rx_window(checker, *LINKS[r["link"]], w, SEARCH_LEN, **kw)
    return _expected[key]


def expected_all(checker, rs=None):
    """the restatement's results of the rows (default: all), each computed once per session, one after the other: the
    oracle's detector keeps state between calls, so rows computed on several threads at once do not always repeat"""
    return [expected(checker, r) for r in (rows() if rs is None else rs)]


def coverage(checker):
    """what the table reaches, from the restatement: sets of outcomes, peek statements, small-frame values and deltas"""
    res = expected_all(checker)
    return dict(outcome={e["outcome"] for e in res}, peek={e["peek"] for e in res}, small={e["small_frame"] & 0xF for e in res},
                delta={e["acq"]["delta"] for e in res if e["outcome"] == WR.DECODED})


def clamped_rows(checker):
    """names of the rows whose peek estimate lies more than 2 Hz from the known CFO, with the sign of the landing"""
    out = {}
    for r, e in zip(rows(), expected_all(checker)):
        if e["peek"] != WR.PEEK_NONE and abs(np.float32(e["peek_cfo_hz"]) - np.float32(r["known"])) > 2:
            out[r["name"]] = 1 if e["peek_cfo_hz"] > r["known"] else -1
    return out


def assert_coverage(checker):
    c = coverage(checker)
    # the clamp lands on known +- 2, bit for bit, on every link - the four the compiled reference can run included; the
    # +-5 Hz rows reach it on QAM256 only (pinned here so that the gap stays visible)
    clamped = clamped_rows(checker)
    want = {f"{l}_fixed_cfo_{n}3": s for l in LINKS for n, s in (("p", 1), ("m", -1))}
    want.update({"qam256_r34_fixed_cfo_p5": 1, "qam256_r34_fixed_cfo_m5": -1, "noise": -1})
    assert clamped == want, clamped
    res = dict(zip([r["name"] for r in rows()], expected_all(checker)))
    for name, sign in want.items():
        r = next(r for r in rows() if r["name"] == name)
        e = res[name]
        land = np.float32(np.float32(r["known"]) + np.float32(2 * sign)).view(np.uint32)
        if e["pending_total_cw"]:      # pass 2 is demodulated at the landing; its own feedback then moves on from there
            assert np.float32(e["spans"][1][2]).view(np.uint32) == land, name
        elif e["acq"]["delta"] == 0:
            assert np.float32(e["sync_cfo_hz"]).view(np.uint32) == land, name
    # the consumed rule's non-data branch: fewer samples than frame_len
    short = {n for n, e in res.items() if e["outcome"] == WR.DECODED and e["next_pos"] < e["acq"]["frame_start"] + e["frame_len"]}
    assert short >= {"ack_data_d8", "ack_data_q16"}, short
    assert res["connect2_q16"]["small_frame"] & 0xF == 3 and res["connect2_q16"]["frame"]["success"] == 1
    assert c["outcome"] == set(range(6)), c
    assert c["peek"] >= set(range(1, 9)), c
    assert c["small"] | set(SMALL_FRAME_WAIVER) >= {0, 1, 2, 3} and set(SMALL_FRAME_WAIVER) <= {2, 3}, c
    assert c["delta"] >= {0, 8, -16}, c
