"""CPU restatement of ria_gpu_rx_burst_batch on pyoracle.Oracle: what StreamingDecoder does behind the first data frame of
a connected-mode window (src/gui/modem/streaming_decoder.cpp), step by step:

group mode (use_burst_interleave_ and the negated-LTS marker, :1378-1410, :3065-3239)
  frame 0 demodulated with the marker, then for f = 1 .. N-1: fit, energy gate, process() with the chained CFO, chain step;
  any stop discards the group; a complete group is de-interleaved and every logical frame goes to decodeFixedFrame
continuation mode (every other accepted window, :2015-2114)
  frame 0 = acquire_restatement.acquire_window; if it is a successful data frame found at delta 0: up to 8 blocks behind
  it with the same gate and chain, each decoded, until one decodes nothing

Neither checker exposes the energy gate (:3154-3171 = :2047-2059), so it is restated here in numpy: float32 products, a
sequential float32 sum, float32 divide and square root.  Test infrastructure only (not collected: no test_ prefix)."""
import zlib

import numpy as np

import pyoracle as po
from acquire_restatement import acquire_window, po_oracle
from test_oracle_golden import burst_cfo_feedback

SLOTS = 9                                  # RIA_BURST_MAX_FRAMES
STOP = {"NONE": 0, "ENERGY": 1, "PROCESS": 2, "WINDOW": 3, "DECODE": 4, "NOT_DATA": 5, "LIMIT": 6, "RECOVERED": 7}
NON_DATA_TYPES = {0x10, 0x11, 0x16, 0x17, 0x20, 0x21, 0x15, 0x40, 0x12, 0x13, 0x14}   # frame_v2.hpp:222-228, :348-351
AUX_FIELDS = ("snr_db", "cfo_hz", "fading_index", "noise_variance", "lts_phase_slope", "snr_linear", "corr_phase")


def gate_rms(block):
    """The energy gate's rms of one block of frame_samples samples (:3154-3163).  np.cumsum over a float32 array adds
    sequentially (tests/test_rx_burst_cpu.py checks that against an explicit loop)."""
    block = np.ascontiguousarray(block, np.float32)
    skip = min(1024, len(block))
    n = min(len(block) - skip, 5000)
    if n <= 0:
        return np.float32(0.0)
    seg = block[skip:skip + n]
    with np.errstate(all="ignore"):
        total = np.cumsum(seg * seg, dtype=np.float32)[-1]
        return np.sqrt(np.float32(total / np.float32(n)))


def gate_rms_loop(block):
    """gate_rms as the reference writes it: one float32 add per sample"""
    block = np.ascontiguousarray(block, np.float32)
    skip = min(1024, len(block))
    n = min(len(block) - skip, 5000)
    acc = np.float32(0.0)
    with np.errstate(all="ignore"):
        for i in range(n):
            acc = np.float32(acc + np.float32(block[skip + i] * block[skip + i]))
        return np.sqrt(np.float32(acc / np.float32(n))) if n > 0 else np.float32(0.0)


def crc16(data):
    """frame_v2.cpp:115-128"""
    crc = 0xFFFF
    for b in bytes(data):
        crc ^= b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def frame_valid(info, cw_ok, bpc):
    """ria_decode_status.frame_valid: parseHeader + DataFrame::deserialize on the concatenated codewords
    (frame_v2.cpp:1195-1252, :556-600).  The marker-byte quirk of CW1..3 (0xD5) is not restated: callers keep clear of it."""
    if not np.asarray(cw_ok).all():
        return 0
    d = bytes(np.asarray(info, np.uint8))
    if d[0] != 0x55 or d[1] != 0x4C:
        return 0
    ctl = d[2] in (0x10, 0x11, 0x16, 0x17, 0x20, 0x21, 0x15, 0x40)
    expected = 20 if ctl else 17 + ((d[13] << 8) | d[14]) + 2
    assert not any(cw * bpc < expected and d[cw * bpc] == 0xD5 for cw in range(1, 4)), "marker-byte quirk: pick another payload"
    if ctl:
        return int(crc16(d[:18]) == ((d[18] << 8) | d[19]))
    if crc16(d[:15]) != ((d[15] << 8) | d[16]) or expected > 4 * bpc:
        return 0
    return int(crc16(d[:expected - 2]) == ((d[expected - 2] << 8) | d[expected - 1]))


def _aux(a):
    return {f: np.float32(getattr(a, f)) for f in AUX_FIELDS}


def burst_window(O, mod, rate, x, search_len, group_size, interleave=True, continuation=True, known_cfo=0.0, detect_threshold=0.15,
                 min_confidence=0.78, abs_base=0, retry=True, ch_deint=True):
    """One window -> dict: the ria_burst_result fields, and per slot info [9, ib], cw_ok / iterations / attempts [9, 4],
    frame_valid [9], aux (list of 9: the demod status of PHYSICAL frame f as a dict, or None), cfo_used [9], rms [9]."""
    assert isinstance(O, po.Oracle)
    geo = O.geom(mod, rate)
    fs, bps, bpc = geo.frame_samples, geo.bits_per_symbol, geo.bytes_per_cw
    ib = 4 * bpc
    x = np.ascontiguousarray(x, np.float32)
    det = O.detect_data_sync(x[:search_len], known_cfo, detect_threshold)
    detected, corr, burst = bool(det[0]), np.float32(det[2]), int(det[3]) if det[0] else 0
    start = int(det[1]) if detected else -1
    accepted = detected and not (corr < np.float32(min_confidence)) and start >= 0 and start + fs <= len(x)
    out = dict(detected=int(detected), accepted=int(accepted), sync_start=start, frame_start=start if accepted else -1, correlation=corr,
               cfo_hz=np.float32(known_cfo if accepted else 0.0), delta=0, candidates=0, burst_interleaved=burst, mode=0, frames=0,
               frames_decoded=0, stop=STOP["NONE"], info=np.zeros((SLOTS, ib), np.uint8), cw_ok=np.zeros((SLOTS, 4), np.uint8),
               iterations=np.zeros((SLOTS, 4), np.uint16), attempts=np.zeros((SLOTS, 4), np.uint8), frame_valid=np.zeros(SLOTS, np.uint8),
               aux=[None] * SLOTS, cfo_used=np.zeros(SLOTS, np.float32), rms=np.zeros(SLOTS, np.float32))
    if not accepted:
        return out
    out["cfo_used"][0] = np.float32(known_cfo)

    def decode(slot, llr):
        data, ok, iters, att = O.decode_fixed_frame(llr, rate, ch_deint, bps, flags=7)
        out["info"][slot], out["cw_ok"][slot], out["iterations"][slot], out["attempts"][slot] = data, ok, iters, att
        out["frame_valid"][slot] = frame_valid(data, ok, bpc)
        return ok

    def next_block(f):
        """fit and gate of physical frame f -> its samples, or None with the stop reason set"""
        s = start + f * fs
        if s + fs > len(x):
            out["stop"] = STOP["WINDOW"]
            return None
        out["rms"][f] = gate_rms(x[s:s + fs])
        if out["rms"][f] < np.float32(0.04):
            out["stop"] = STOP["ENERGY"]
            return None
        out["cfo_used"][f] = out["cfo_hz"]
        return x[s:s + fs]

    def process(f, seg, marker):
        llr, aux = O.rx_process(mod, rate, seg, float(out["cfo_used"][f]), abs_base + start, burst_marker=marker)
        if len(llr) == 0:
            out["stop"] = STOP["PROCESS"]
            return None
        out["frames"] += 1
        out["aux"][f] = _aux(aux)
        out["cfo_hz"] = burst_cfo_feedback(out["cfo_used"][f], aux.cfo_hz)
        return llr

    if interleave and burst:
        out["mode"] = 2
        llrs = [process(0, x[start:start + fs], True)]
        for f in range(1, group_size):
            if llrs[-1] is None:
                break
            seg = next_block(f)
            if seg is None:
                break
            llrs.append(process(f, seg, False))
        if len(llrs) == group_size and llrs[-1] is not None:
            logical = O.burst_deinterleave(np.stack(llrs))
            for i in range(group_size):
                decode(i, logical[i])
            out["frames_decoded"] = group_size
        return out

    out["mode"] = 1
    r = acquire_window(O, mod, rate, x, search_len, known_cfo, detect_threshold, min_confidence, abs_base, retry, ch_deint)
    assert r["accepted"] and r["sync_start"] == start
    out.update(frame_start=r["frame_start"], delta=r["delta"], candidates=r["candidates"], frames=1, frames_decoded=1)
    out["info"][0], out["cw_ok"][0], out["iterations"][0], out["attempts"][0] = r["info"], r["cw_ok"], r["iterations"], r["attempts"]
    out["frame_valid"][0] = frame_valid(r["info"], r["cw_ok"], bpc)
    out["aux"][0] = _aux(r["aux"])
    s0 = r["frame_start"]
    if len(O.rx_process(mod, rate, x[s0:s0 + fs], float(known_cfo), abs_base + s0, burst_marker=bool(burst) and r["delta"] == 0)[0]) == 0:
        # frame 0 without soft bits: slot 0 stays what the acquire rounds report, no physical frame counts, the chain
        # does not step, and STOP_PROCESS is reported whatever the continuation flag says
        out.update(frames=0, stop=STOP["PROCESS"])
        return out
    out["cfo_hz"] = burst_cfo_feedback(np.float32(known_cfo), r["cfo_hz"])
    if not continuation:
        return out
    if not (r["cw_ok"].all() and out["frame_valid"][0]):
        out["stop"] = STOP["DECODE"]
    elif int(r["info"][2]) in NON_DATA_TYPES:
        out["stop"] = STOP["NOT_DATA"]
    elif r["delta"] != 0:
        out["stop"] = STOP["RECOVERED"]
    else:
        for k in range(1, SLOTS):
            seg = next_block(k)
            if seg is None:
                break
            llr = process(k, seg, False)
            if llr is None:
                break
            out["frames_decoded"] += 1
            if not decode(k, llr).any():
                out["stop"] = STOP["DECODE"]
                break
            if k == SLOTS - 1:
                out["stop"] = STOP["LIMIT"]
    return out


def capture(O, mod, rate, n_frames, lead, total_len, seed, kind=0, snr_db=22.0, marker=False, interleaved=False, cfo_hz=0.0,
            frame_type=None, silence=(), noise=(), scale=0.5):
    """A burst on the CPU from the oracle's TX pieces (the recipe of oracle/gen_golden.burst_buffer): n_frames serialized data
    frames -> encodeFixedFrame -> [burst interleave] -> modulate, [first LTS negated], scaled to peak `scale`, placed at
    `lead` of total_len zeros (cut where it runs past the end), frames listed in `silence` zeroed, frames listed in `noise`
    replaced by Gaussian noise of rms 0.1, optional CFO (analytic rotation), then the oracle's channel over the whole
    window.  frame_type: byte 2 of frame 0 is rewritten to that control type (with its 18-byte CRC).  -> (window, infos)"""
    rng = np.random.default_rng(seed)
    g = O.geom(mod, rate)
    ib = 4 * g.bytes_per_cw
    infos = np.stack([O.make_frame(rng.integers(0, 256, ib - 19, dtype=np.uint8), 100 + f, rate) for f in range(n_frames)])
    if frame_type is not None:
        infos[0, 2] = frame_type
        c = crc16(infos[0, :18])
        infos[0, 18], infos[0, 19] = c >> 8, c & 0xFF
    coded = np.stack([O.encode_fixed_frame(infos[f], rate, True, g.bits_per_symbol) for f in range(n_frames)])
    phys = O.burst_interleave(coded) if interleaved and n_frames >= 2 else coded
    frames = [O.modulate(mod, rate, phys[f]) for f in range(n_frames)]
    if marker:
        frames[0][:1152] = -frames[0][:1152]
    s = np.concatenate(frames)
    s = (s * np.float32(scale / np.abs(s).max())).astype(np.float32)
    fs = g.frame_samples
    for f in silence:
        s[f * fs:(f + 1) * fs] = 0.0
    for f in noise:
        s[f * fs:(f + 1) * fs] = (0.1 * rng.standard_normal(fs)).astype(np.float32)
    x = np.zeros(total_len, np.float32)
    n = min(len(s), total_len - lead)
    x[lead:lead + n] = s[:n]
    if cfo_hz:
        spec = np.fft.fft(x.astype(np.float64))
        h = np.zeros(total_len); h[0] = 1; h[1:(total_len + 1) // 2] = 2
        if total_len % 2 == 0:
            h[total_len // 2] = 1
        x = np.real(np.fft.ifft(spec * h) * np.exp(2j * np.pi * cfo_hz * np.arange(total_len) / 48000.0)).astype(np.float32)
    return O.channel(kind, snr_db, int(seed), x), infos


# ---- the scenario set of the CPU and GPU tests (QAM16 R1/2): one window length, one call
FS = 18432
WINDOW_LEN = 6000 + 9 * FS + 1152          # lead + 9 frames and the head of a tenth
SEARCH_LEN = 135000
GROUP = 4
LATE = WINDOW_LEN - 2 * FS - FS // 2       # a burst starting here has its block 2 cut by the window's end


def scenarios(O):
    """name -> (window, expected stop, expected mode, known_cfo).  Every window is WINDOW_LEN long."""
    Q, R = po.QAM16, po.R1_2
    S = {}
    S["energy"] = (capture(O, Q, R, 2, 6000, WINDOW_LEN, 9101)[0], "ENERGY", 1, 0.0)
    S["window"] = (capture(O, Q, R, 4, LATE, WINDOW_LEN, 9102)[0], "WINDOW", 1, 0.0)
    S["decode"] = (capture(O, Q, R, 3, 7000, WINDOW_LEN, 9103, noise=(2,))[0], "DECODE", 1, 0.0)
    S["not_data"] = (capture(O, Q, R, 3, 6500, WINDOW_LEN, 9104, frame_type=0x20)[0], "NOT_DATA", 1, 0.0)
    S["limit"] = (capture(O, Q, R, 10, 6000, WINDOW_LEN, 9105)[0], "LIMIT", 1, 0.0)
    S["recovered"] = (recovered_window(O), "RECOVERED", 1, 0.0)
    S["group_ok"] = (capture(O, Q, R, 4, 6200, WINDOW_LEN, 9106, marker=True, interleaved=True)[0], "NONE", 2, 0.0)
    S["group_energy"] = (capture(O, Q, R, 4, 6400, WINDOW_LEN, 9107, marker=True, interleaved=True, silence=(2,))[0], "ENERGY", 2, 0.0)
    S["group_window"] = (capture(O, Q, R, 4, LATE, WINDOW_LEN, 9108, marker=True, interleaved=True)[0], "WINDOW", 2, 0.0)
    S["clamp_up"] = (capture(O, Q, R, 4, 6600, WINDOW_LEN, 9109, marker=True, interleaved=True, cfo_hz=3.0)[0], "NONE", 2, 0.0)
    S["clamp_down"] = (capture(O, Q, R, 4, 6800, WINDOW_LEN, 9110, marker=True, interleaved=True, cfo_hz=-3.0)[0], "NONE", 2, 0.0)
    S["silence"] = (O.channel(0, 20.0, 9111, np.zeros(WINDOW_LEN, np.float32)), "NONE", 0, 0.0)
    return S


def recovered_window(O, s=15, snr_db=17.0):
    """A faded window of tests/test_gpu_rx_acquire.py's recipe (Watterson moderate: two rays) at 17 dB whose frame 0 decodes
    nothing at the detected start and completely at delta -16, padded with silence to WINDOW_LEN."""
    from acquire_restatement import window
    seed = 3000 + s
    rng = np.random.default_rng(seed)
    x, _ = window(O, po.QAM16, po.R1_2, rng.integers(0, 256, 141, dtype=np.uint8), seed, 4000 + (s * 1237) % 7000, 36000, 2, snr_db, seed)
    return np.concatenate([x, np.zeros(WINDOW_LEN - len(x), np.float32)])


def checksum(x):
    return zlib.crc32(np.ascontiguousarray(x, np.float32).tobytes())
