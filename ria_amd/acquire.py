"""Connected-mode OFDM data frames from capture windows: the acceptance rule, the Monte-Carlo window recipe and the
counter driver around RxEngine.rx_acquire (ria_gpu_rx_acquire_batch), and the same for bursts of frames around
RxEngine.rx_burst (ria_gpu_rx_burst_batch).

A window is what gui::StreamingDecoder searches for one DATA frame: silence, the frame at some offset, the channel
over the whole window.  The detector sees the first `search_len` samples; the window holds search_len + frame_samples,
so that every detected frame fits in it.
"""
import numpy as np
import torch

from . import capi
from .sweep import reduce_counters, shard_range, trial_seed32

SEARCH_LEN = 21000          # span of the LTS sync bench and the burst tests
DETECT_THRESHOLD = 0.15     # CORR_DETECT_THRESHOLD (streaming_decoder.hpp:457)
ACQ_COUNTERS = ("windows", "detected", "accepted", "primary_ok", "recovered", "frame_err", "byte_err", "decodes")

_PSK = (capi.MOD["BPSK"], capi.MOD["QPSK"])
_QAM = (capi.MOD["QAM16"], capi.MOD["QAM32"], capi.MOD["QAM64"], capi.MOD["QAM256"])


def lts_min_confidence(modulation, fading_hint=0.0, snr_hint=99.0, reject_streak=0):
    """light_sync_min_confidence of connected-mode OFDM (streaming_decoder.cpp:679-699): PSK 0.90, QAM 0.78,
    differential 0.72 lowered to 0.68 / 0.65 / 0.62 by the fading and SNR hints, then relaxed by 0.015 per rejection
    beyond the 7th (at most 0.12, never below 0.56).  Stateless: the caller keeps the hints and the reject streak.
    Float32 arithmetic, as the reference computes it."""
    mod = capi.MOD[modulation] if isinstance(modulation, str) else int(modulation)
    f32 = np.float32
    if mod in _PSK:
        return f32(0.90)
    if mod in _QAM:
        return f32(0.78)
    fading, snr = f32(fading_hint), f32(snr_hint)
    conf = f32(0.72)
    if fading >= f32(1.00) or snr < f32(10.0):
        conf = f32(0.62)
    elif fading >= f32(0.70) or snr < f32(14.0):
        conf = f32(0.65)
    elif fading >= f32(0.50) or snr < f32(18.0):
        conf = f32(0.68)
    if reject_streak >= 8:
        relax = min(f32(0.12), f32(0.015) * f32(reject_streak - 7))
        conf = max(f32(0.56), f32(conf - relax))
    return f32(conf)


def window_recipe(base_seed, point_index, trials, search_len=SEARCH_LEN):
    """(frame offsets int64, mt19937 channel seeds uint32) of the windows `trials` (global trial numbers) of one sweep
    point.  The offset is uniform over [0, search_len - 4 symbols], so that the frame's two LTS symbols lie inside the
    detector's span; both values depend on (base seed, point, trial) only, never on chunking or rank."""
    idx = np.asarray(trials, dtype=np.uint64)
    max_off = int(search_len) - 4 * 1152
    seeds = trial_seed32(base_seed, point_index, 2, idx)
    offs = trial_seed32(base_seed, point_index, 3, idx).astype(np.int64) % np.int64(max_off + 1)
    return offs, seeds


def make_windows(engine, base_seed, point, point_index, start, n, search_len=SEARCH_LEN, tx_cfo=None):
    """Windows of trials [start, start + n) of one sweep point on the engine's device: make_frames (seq = trial) ->
    tx(peak 0.8) -> [transmitter CFO] -> placed at the recipe offset in a zero window of search_len + frame_samples
    samples -> the reference-identical channel over the whole window (one mt19937 seed per trial).
    Returns (windows float32 [n, window_len], sent info uint8 [n, info_bytes], offsets int64 [n])."""
    fs = engine.geo.frame_samples
    offs, seeds = window_recipe(base_seed, point_index, np.arange(start, start + n), search_len)
    info = engine.make_frames(base_seed, start, n)
    x = engine.tx(info, peak=0.8)
    if tx_cfo is not None:
        x = engine.tx_cfo(x, float(tx_cfo))
    win = torch.zeros((n, search_len + fs), dtype=torch.float32, device=engine.device)
    offs_t = torch.from_numpy(offs).to(engine.device)
    win.scatter_(1, offs_t[:, None] + torch.arange(fs, device=engine.device)[None, :], x)   # placement only
    engine.channel_exact_seeded_(win, point.channel, point.snr_db, seeds)
    return win, info, offs


def tally(info, st, res, sent):
    """Counter row (ACQ_COUNTERS) of one chunk from rx_acquire's outputs and the sent payloads."""
    ok = st["cw_ok"].all(axis=1) & st["frame_valid"].astype(bool)
    same = (info == sent).all(dim=1).cpu().numpy()
    acc = res["accepted"] != 0
    any_primary = acc & (res["delta"] == 0) & st["cw_ok"].any(axis=1)
    return np.array([len(res), int((res["detected"] != 0).sum()), int(acc.sum()), int(any_primary.sum()),
                     int((acc & (res["delta"] != 0)).sum()), int((~(ok & same)).sum()), int((info != sent).sum().item()),
                     int(res["candidates"].sum())], dtype=np.int64)


def run_acquire_point(engine, point, base_seed, point_index, start, n, search_len=SEARCH_LEN, min_confidence=None,
                      tx_cfo=None):
    """One chunk of trials of one sweep point through ria_gpu_rx_acquire_batch.  Returns the counter row:
    windows, detected, accepted, primary_ok (the primary candidate decoded a codeword), recovered (a recovery candidate
    was reported), frame_err (not every codeword decoded, frame CRC failed or payload differs), byte_err (payload bytes
    that differ from the sent ones, undecoded windows included), decodes (candidates demodulated + decoded)."""
    win, sent, _ = make_windows(engine, base_seed, point, point_index, start, n, search_len, tx_cfo)
    info, st, res = engine.rx_acquire(win, search_len, known_cfo=0.0 if tx_cfo is None else float(tx_cfo),
                                      detect_threshold=DETECT_THRESHOLD, min_confidence=min_confidence)
    return tally(info, engine.decode_status(st), res, sent)


def run_acquire_sweep(engine, points, n_trials, base_seed, chunk=4096, **kw):
    """run_acquire_point over every point, trials sharded over ranks as sweep.run_sweep shards them; counters summed
    over ranks.  Returns int64 [n_points, len(ACQ_COUNTERS)]."""
    import torch.distributed as dist
    rank = dist.get_rank() if dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_initialized() else 1
    local = np.zeros((len(points), len(ACQ_COUNTERS)), dtype=np.int64)
    for pi, p in enumerate(points):
        for start, n in shard_range(n_trials, rank, world, chunk):
            local[pi] += run_acquire_point(engine, p, base_seed, pi, start, n, **kw)
    return reduce_counters(local, engine.device)


# ---- burst groups and burst continuation (ria_gpu_rx_burst_batch)
BURST_STOPS = ("none", "energy", "process", "window", "decode", "not_data", "limit", "recovered")   # RIA_BURST_STOP_*
BURST_COUNTERS = ("windows", "detected", "accepted") + tuple(f"mode{m}_{s}" for m in (1, 2) for s in BURST_STOPS) + \
    ("frames", "frames_decoded", "frames_ok")


def make_burst_windows(engine, base_seed, point, point_index, start, n, n_frames, interleaved=True, marker=None,
                       search_len=SEARCH_LEN, window_frames=None, peak=0.5):
    """Burst windows of trials [start, start + n) of one sweep point on the engine's device, as the air interface carries
    them (streaming_encoder.cpp:302-389): make_frames (seq = trial * n_frames + f) -> encodeFixedFrame -> [BurstInterleaver::
    interleave over the n_frames frames of a window] -> modulator per physical frame -> [first LTS of the burst negated:
    the marker] -> the whole burst scaled to `peak` -> placed at the recipe offset in a zero window of search_len +
    window_frames * frame_samples samples (window_frames >= n_frames, default n_frames + 1: room for the block behind the
    burst, which ends a continuation at the energy gate) -> the reference-identical channel over the whole window (one
    mt19937 seed per trial).  marker None: as `interleaved`.
    Returns (windows float32 [n, window_len], sent info uint8 [n, n_frames, info_bytes], offsets int64 [n])."""
    fs, N = engine.geo.frame_samples, int(n_frames)
    marker = bool(interleaved) if marker is None else bool(marker)
    window_frames = N + 1 if window_frames is None else int(window_frames)
    assert N >= 1 and window_frames >= N and (not interleaved or 2 <= N <= 8)
    offs, seeds = window_recipe(base_seed, point_index, np.arange(start, start + n), search_len)
    info = engine.make_frames(base_seed, start * N, n * N)
    coded = engine.encode_frames(info)
    if interleaved:
        coded = engine.burst_interleave(coded, N)
    x = engine.tx_coded(coded, peak=0.0).reshape(n, N * fs)
    if marker:
        x[:, :1152] = -x[:, :1152]
    x = x * (np.float32(peak) / x.abs().amax(dim=1, keepdim=True))
    win = torch.zeros((n, search_len + window_frames * fs), dtype=torch.float32, device=engine.device)
    offs_t = torch.from_numpy(offs).to(engine.device)
    win.scatter_(1, offs_t[:, None] + torch.arange(N * fs, device=engine.device)[None, :], x)   # placement only
    engine.channel_exact_seeded_(win, point.channel, point.snr_db, seeds)
    return win, info.reshape(n, N, -1), offs


def burst_tally(out, sent):
    """Counter row (BURST_COUNTERS) of one chunk from rx_burst's host-side outputs and the sent payloads
    (uint8 [n, n_frames, info_bytes], numpy or tensor): windows per mode and stop reason, physical frames demodulated,
    logical frames / blocks decoded, and those of them that are complete, CRC-valid and equal to what was sent."""
    res, st = out["result"], out["decode_status"]
    sent = sent.cpu().numpy() if torch.is_tensor(sent) else np.asarray(sent)
    row = dict.fromkeys(BURST_COUNTERS, 0)
    row.update(windows=len(res), detected=int((res["detected"] != 0).sum()), accepted=int((res["accepted"] != 0).sum()))
    for m in (1, 2):
        for k, name in enumerate(BURST_STOPS):
            row[f"mode{m}_{name}"] = int(((res["mode"] == m) & (res["stop"] == k)).sum())
    nf = min(sent.shape[1], out["info"].shape[1])
    valid = np.arange(nf)[None, :] < res["frames_decoded"][:, None]
    ok = st["cw_ok"][:, :nf].all(axis=2) & (st["frame_valid"][:, :nf] != 0) & (out["info"][:, :nf] == sent[:, :nf]).all(axis=2)
    row.update(frames=int(res["frames"].sum()), frames_decoded=int(res["frames_decoded"].sum()), frames_ok=int((ok & valid).sum()))
    return np.array([row[k] for k in BURST_COUNTERS], dtype=np.int64)


DFRAME_PATHS = ("NONE", "CONTROL_R14", "CONTROL_CW0", "FIXED", "SALVAGE_R14", "SALVAGE_RATE", "FIXED_FAILED", "LEGACY", "PARTIAL",
                "BAD_HEADER")                      # RIA_DFRAME_* by value
DFRAME_COUNTERS = ("rows", "success") + tuple("path_" + p for p in DFRAME_PATHS) + \
    ("stage_r14", "stage_rate", "stage_fixed", "stage_salvage_r14", "stage_salvage_rate", "stage_legacy", "probe_iterations")


def dframe_tally(result):
    """Counter row (DFRAME_COUNTERS) of decode_frame's result array: rows, successes, rows per RIA_DFRAME_* path, rows each
    stage ran for, and the iterations the two plain CW0 probes spent."""
    row = dict.fromkeys(DFRAME_COUNTERS, 0)
    row.update(rows=len(result), success=int((result["success"] != 0).sum()))
    for k, name in enumerate(DFRAME_PATHS):
        row["path_" + name] = int((result["path"] == k).sum())
    for bit, name in enumerate(("r14", "rate", "fixed", "salvage_r14", "salvage_rate", "legacy")):
        row["stage_" + name] = int(((result["stages"] >> bit) & 1).sum())
    row["probe_iterations"] = int(result["iters_r14"].astype(np.int64).sum() + result["iters_cw0"].astype(np.int64).sum())
    return np.array([row[k] for k in DFRAME_COUNTERS], dtype=np.int64)


def run_burst_point(engine, point, base_seed, point_index, start, n, n_frames, interleaved=True, search_len=SEARCH_LEN,
                    min_confidence=None, **kw):
    """One chunk of trials of one sweep point through ria_gpu_rx_burst_batch (group_size = n_frames for interleaved
    bursts).  Returns the counter row (BURST_COUNTERS)."""
    win, sent, _ = make_burst_windows(engine, base_seed, point, point_index, start, n, n_frames, interleaved, search_len=search_len)
    out = engine.rx_burst(win, search_len, group_size=max(2, int(n_frames)), detect_threshold=DETECT_THRESHOLD,
                          min_confidence=min_confidence, interleave=bool(interleaved), **kw)
    return burst_tally(out, sent)


# ---- control frames and the control hypothesis (ria_gpu_control_acquire_batch)
ACK, NACK = 0x20, 0x21                          # v2::FrameType
CONTROL_COUNTERS = ("windows", "detected", "accepted", "tried", "process_ok", "cw_ok", "magic", "header_valid", "success",
                    "delivered", "decodes")


def _crc16(b):
    """ControlFrame::calculateCRC (frame_v2.cpp:115-128): CRC-16/CCITT-FALSE"""
    crc = 0xFFFF
    for v in bytes(b):
        crc ^= v << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def control_frames(seqs, types=None):
    """Serialized 20-byte control frames (ControlFrame::serialize, frame_v2.cpp): magic 55 4C, type, flags 0, seq, the
    hashes of "TEST" / "RX" as make_frames uses them, 6 zero payload bytes, CRC-16 over 18.  types None: ACK for an even seq,
    NACK for an odd one.  uint8 [n, 20]."""
    seqs = np.asarray(seqs, np.int64)
    out = np.zeros((len(seqs), 20), np.uint8)

    def djb2(s):
        h = 5381
        for c in s.upper().encode():
            h = (((h << 5) + h) ^ c) & 0xFFFFFFFF
        return h & 0xFFFFFF
    hs, hd = djb2("TEST"), djb2("RX")
    for i, q in enumerate(seqs):
        t = (ACK if q % 2 == 0 else NACK) if types is None else int(np.asarray(types).reshape(-1)[i])
        out[i, :12] = [0x55, 0x4C, t, 0, (q >> 8) & 255, q & 255, hs >> 16, (hs >> 8) & 255, hs & 255, hd >> 16, (hd >> 8) & 255, hd & 255]
        c = _crc16(out[i, :18])
        out[i, 18], out[i, 19] = c >> 8, c & 255
    return out


def make_control_windows(control_engine, base_seed, point, point_index, start, n, n_samples, search_len=SEARCH_LEN, window_len=None):
    """ACK / NACK windows of trials [start, start + n) of one sweep point on the control engine's device, as encodeFrame's
    control branch sends them (streaming_encoder.cpp:216-245): the 20-byte frame (seq = trial) -> one R1/4 codeword
    (ldpc_encode) -> tx_coded_var at DQPSK (peak 0.8) -> placed like make_windows at the recipe offset in a zero window of
    window_len samples (default search_len + n_samples, so that every detected span fits) -> the reference-identical channel
    over the whole window.  Returns (windows float32 [n, window_len], sent frames uint8 [n, 20] on the device, offsets)."""
    e = control_engine
    window_len = int(search_len) + int(n_samples) if window_len is None else int(window_len)
    offs, seeds = window_recipe(base_seed, point_index, np.arange(start, start + n), search_len)
    frames = control_frames(np.arange(start, start + n) & 0xFFFF)
    info = np.zeros((n, (e.geo.ldpc_k + 7) // 8), np.uint8)
    info[:, :20] = frames
    coded = torch.from_numpy(e.ldpc_encode(info)).to(e.device)
    x = e.tx_coded_var(coded, peak=0.8)
    win = torch.zeros((n, window_len), dtype=torch.float32, device=e.device)
    offs_t = torch.from_numpy(offs).to(e.device)
    win.scatter_(1, offs_t[:, None] + torch.arange(x.shape[1], device=e.device)[None, :], x)   # placement only
    e.channel_exact_seeded_(win, point.channel, point.snr_db, seeds)
    return win, torch.from_numpy(frames).to(e.device), offs


def control_tally(frames, res, acq, sent):
    """Counter row (CONTROL_COUNTERS) of one chunk from control_acquire's outputs and the sent frames: windows, detected,
    accepted, tried, the five tests of the hypothesis in the reference's order, frames delivered (success and the 20 bytes
    equal to what was sent), robust decodes made."""
    same = (frames == sent).all(dim=1).cpu().numpy()
    row = [len(res), int((acq["detected"] != 0).sum()), int((acq["accepted"] != 0).sum())]
    row += [int((res[k] != 0).sum()) for k in ("tried", "process_ok", "cw_ok", "magic", "header_valid", "success")]
    row += [int(((res["success"] != 0) & same).sum()), int(res["tries"].astype(np.int64).sum())]
    return np.array(row, dtype=np.int64)


def rx_acquire_control_first(control_engine, data_engine, windows, search_len, n_samples=None, known_cfo=None,
                             detect_threshold=DETECT_THRESHOLD, min_confidence=None, abs_base=None, interleave=False, **kw):
    """What the connected receiver does with a window (streaming_decoder.cpp:1268-1344, then the data path): the control
    hypothesis on every window (control_acquire on the DQPSK R1/4 engine, with the DATA profile's min_confidence), then
    data_engine.rx_acquire with the same ria_acq_params except that min_confidence is +inf for the windows the hypothesis
    took - set by one torch op on the device - so that those windows are not accepted and cost the data call nothing.
    Returns (control frames [n, 20], control result, control acq, info, decode status, data acq)."""
    n = windows.shape[0]
    if n_samples is None:
        n_samples = control_engine.control_frame_samples(data_engine)
    if min_confidence is None:
        min_confidence = lts_min_confidence(data_engine.modulation)
    params = data_engine.acq_params(n, known_cfo, detect_threshold, min_confidence, abs_base)
    frames, res, acq, _, res_dev = control_engine.control_acquire(windows, search_len, n_samples, params=params, interleave=interleave,
                                                                  want_device_result=True)
    taken = res_dev[:, 6] != 0                                         # ria_control_result.success
    p2 = params.clone()
    p2.view(torch.float32)[:, 2] = torch.where(taken, torch.full_like(taken, float("inf"), dtype=torch.float32), params.view(torch.float32)[:, 2])
    info, st, dacq = data_engine.rx_acquire(windows, search_len, params=p2, **kw)
    return frames, res, acq, info, st, dacq


def make_mixed_windows(control_engine, data_engine, base_seed, point, n, search_len=12000):
    """Mixed connected-mode traffic for RxEngine.rx_window and rx_acquire_control_first, on the device: n windows (n even) of
    search_len + a data frame's samples; even windows carry an ACK / NACK control frame (make_control_windows), odd windows a
    fixed 4-codeword data frame of data_engine's profile (make_windows), each through the reference-identical channel of
    `point`.  Returns (windows float32 [n, window_len], sent control frames uint8 [n / 2, 20], sent data info [n / 2, info
    bytes], control span in samples)."""
    h = n // 2
    span = control_engine.control_frame_samples(data_engine)
    wlen = int(search_len) + data_engine.geo.frame_samples
    wd, sent_d, _ = make_windows(data_engine, base_seed, point, 0, 0, h, search_len)
    wc, sent_c, _ = make_control_windows(control_engine, base_seed + 1, point, 0, 0, h, span, search_len, window_len=wlen)
    w = torch.stack([wc, wd], dim=1).reshape(2 * h, wlen).contiguous()
    return w, sent_c, sent_d, span


WINDOW_COUNTERS = tuple(f"outcome_{k.lower()}" for k in capi.WIN_OUTCOME) + tuple(f"peek_{k.lower()}" for k in capi.WIN_PEEK) + \
    ("small_not_run", "small_nothing", "small_one_cw", "small_exact", "small_at_rate", "success", "partial") + \
    tuple(f"delta_{d:+d}" for d in (0, 8, -8, 16, -16, 24, -24, 32, -32))


def window_tally(res, acq):
    """Counter row (WINDOW_COUNTERS) of one rx_window call: windows per outcome, per peek statement and per small-frame branch
    (and how many took theirs at the link rate), frames delivered (success), results with some codewords only, and the timing
    candidate reported for the decoded windows."""
    row = [int((res["outcome"] == v).sum()) for v in capi.WIN_OUTCOME.values()]
    row += [int((res["peek"] == v).sum()) for v in capi.WIN_PEEK.values()]
    small = res["small_frame"] & 0xF
    row += [int((small == v).sum()) for v in range(4)] + [int(((res["small_frame"] & 0x10) != 0).sum())]
    ok = res["frame"]["success"] != 0
    row += [int(ok.sum()), int((~ok & (res["frame"]["codewords_ok"] != 0)).sum())]
    decoded = res["outcome"] == capi.WIN_OUTCOME["DECODED"]
    row += [int((decoded & (acq["delta"] == d)).sum()) for d in (0, 8, -8, 16, -16, 24, -24, 32, -32)]
    return np.array(row, dtype=np.int64)


# ---- MC-DPSK (ria_gpu_mcdpsk_acquire_batch)
def _zc_relax(streak):
    return min(np.float32(0.15), np.float32(0.025) * np.float32(streak - 3)) if streak >= 4 else np.float32(0.0)


def zc_min_confidence(reject_streak=0):
    """light_sync_min_confidence of connected ZC mode (streaming_decoder.cpp:679-717): 0.40, relaxed after 4 consecutive
    rejects by 0.025 per reject beyond the 3rd (at most 0.15), never below 0.25.  Float32 arithmetic."""
    return np.float32(max(np.float32(0.25), np.float32(np.float32(0.40) - _zc_relax(reject_streak))))


def zc_weak_floor(reject_streak=0):
    """weak_sync_floor of connected ZC mode: 0.30 with the same relaxation, never below 0.20."""
    return np.float32(max(np.float32(0.20), np.float32(np.float32(0.30) - _zc_relax(reject_streak))))


def mcdpsk_frame_len(frame_cw, carriers=10, bits_per_symbol=1, spreading=1):
    """MCDPSKWaveform::getMinSamplesForCWCount (mc_dpsk_waveform.cpp:470-485): training + reference + frame_cw codewords"""
    return 9 * 512 + int(frame_cw) * -(-648 // (int(carriers) * int(bits_per_symbol))) * 512 * int(spreading)


def mcdpsk_window_recipe(preamble_len, frame_cw, lead=2000, tail=2000, carriers=10, bits_per_symbol=1, spreading=1):
    """(search_len, window_len) of an MC-DPSK test / bench window: `lead` samples of silence, the preamble, the frame of
    frame_cw codewords, `tail` samples.  The detector sees the lead-in, the preamble and the first 8 symbols after it."""
    fl = mcdpsk_frame_len(frame_cw, carriers, bits_per_symbol, spreading)
    return lead + preamble_len + 8 * 512, lead + preamble_len + fl + tail


def make_mcdpsk_windows(engine, coded, preamble, n, frame_cw, kind, snr_db, seeds, lead=2000, tail=2000, carriers=10,
                        bits_per_symbol=1, spreading=1, gap=0):
    """n windows on the engine's device: the frame(s) `coded` (uint8 [m, n_bytes] coded bytes, row i % m for window i)
    modulated on the device behind `preamble` (float32 host array: engine.chirp_preamble() or a ZC preamble), peak 0.8,
    at sample `lead` of a zero window, then the reference-identical channel (one mt19937 seed per window).  gap > 0 puts
    that many zero samples between the preamble and the frame (windows that need the timing recovery).
    Returns (windows float32 [n, window_len], search_len)."""
    coded = np.ascontiguousarray(coded, np.uint8)
    body = engine.mcdpsk_modulate_batch(coded, carriers, bits_per_symbol, spreading)
    pre = torch.from_numpy(np.ascontiguousarray(preamble, np.float32)).to(engine.device)
    tx = torch.cat([pre[None, :].expand(body.shape[0], -1),
                    torch.zeros((body.shape[0], int(gap)), dtype=torch.float32, device=engine.device), body], dim=1)
    tx = tx * (0.8 / tx.abs().amax(dim=1, keepdim=True))
    search_len, window_len = mcdpsk_window_recipe(len(preamble), frame_cw, lead, tail, carriers, bits_per_symbol, spreading)
    win = torch.zeros((n, window_len), dtype=torch.float32, device=engine.device)
    m = min(tx.shape[1], window_len - lead)
    win[:, lead:lead + m] = tx[torch.arange(n, device=engine.device) % tx.shape[0], :m]
    engine.channel_exact_seeded_(win, kind, snr_db, np.ascontiguousarray(seeds, np.uint32))
    return win, search_len


# ---- HARQ chase combining (ria_gpu_mcdpsk_acquire_harq_batch, ria_gpu_mcdpsk_decode_frame_batch)
HARQ_COUNTERS = ("rows", "keyed", "stored_rows", "stores", "stored", "combines", "sum_decodes", "recoveries", "delivered_by_combining",
                 "entries_kept", "entries_removed")


def _popcount16(v):
    v = np.asarray(v, np.uint16)
    return sum(((v >> b) & 1).astype(np.int64) for b in range(16))


def harq_tally(result, harq):
    """Counter row (HARQ_COUNTERS) of one call from its result array (MCACQ_RESULT or MCDFRAME_RESULT) and its harq array
    (HARQ_RESULT): rows; rows whose valid header met a cache; rows that stored; store() calls (every codeword that failed
    its own decode: those still failed plus those recovered; ChaseCache::Stats.stores); stores that returned true; combines
    (a store onto an existing sum: stored and its sum decoded; Stats.combines); combined sums decoded; codewords recovered
    (Stats.recoveries); frames delivered through combining (a success with a recovered codeword); entries kept; entries
    removed on success.  Summed over the calls of a connected link the three Stats columns equal the cache's counters.  For
    a disconnected acquire call the harq array describes each window's last candidate that met the cache, so what earlier
    candidates of a window stored shows in the caches' own statistics only."""
    keyed = harq["valid"] != 0
    row = dict(rows=len(harq), keyed=int(keyed.sum()), stored_rows=int((harq["stored_mask"] != 0).sum()),
               stores=int((result["codewords_failed"].astype(np.int64) + _popcount16(harq["recovered_mask"]))[keyed].sum()),
               stored=int(_popcount16(harq["stored_mask"]).sum()), combines=int(_popcount16(harq["stored_mask"] & harq["sum_mask"]).sum()),
               sum_decodes=int(_popcount16(harq["sum_mask"]).sum()), recoveries=int(_popcount16(harq["recovered_mask"]).sum()),
               delivered_by_combining=int(((result["success"] != 0) & (harq["recovered_mask"] != 0)).sum()),
               entries_kept=int((harq["entry"] == capi.HARQ_ENTRY["KEPT"]).sum()),
               entries_removed=int((harq["entry"] == capi.HARQ_ENTRY["REMOVED"]).sum()))
    return np.array([row[k] for k in HARQ_COUNTERS], dtype=np.int64)


# ---- one MC-DPSK window per call (ria_gpu_mcdpsk_window_batch)
_MWIN_DELTAS = (8, -8, 16, -16, 24, -24, 32, -32, 48, -48, 64, -64)
MCDPSK_WINDOW_COUNTERS = ("windows",) + tuple(f"outcome_{k.lower()}" for k in capi.MWIN_OUTCOME) + \
    tuple(f"peek_{k.lower()}" for k in capi.MPEEK_WHAT) + tuple(f"peek_{k.lower()}" for k in capi.MPEEK_BITS) + \
    ("pings", "success", "partial", "delivered", "recovered_alternate") + tuple(f"recovered_{d:+d}" for d in _MWIN_DELTAS)


def mcdpsk_window_tally(res, acq):
    """Counter row (MCDPSK_WINDOW_COUNTERS) of one mcdpsk_window call: windows, windows per outcome, per statement of the CW0
    peek (what CW0 said, then every escalation statement that fired), PINGs, frames decoded in full (success, PINGs not
    counted), results with some codewords only, results the host queues, and - among the decoded frames - those the alternate
    modulation recovered in place and those each timing delta recovered."""
    row = [len(res)] + [int((res["outcome"] == v).sum()) for v in capi.MWIN_OUTCOME.values()]
    what = res["peek"] & capi.MPEEK_WHAT_MASK
    row += [int((what == v).sum()) for v in capi.MPEEK_WHAT.values()]
    row += [int(((res["peek"] & v) != 0).sum()) for v in capi.MPEEK_BITS.values()]
    decoded = res["outcome"] == capi.MWIN_OUTCOME["DECODED"]
    ok = decoded & (acq["success"] != 0)
    row += [int((res["is_ping"] != 0).sum()), int(ok.sum()), int((decoded & ~ok & (acq["codewords_ok"] != 0)).sum()),
            int((res["deliver"] != 0).sum()), int((ok & (acq["delta"] == 0) & (acq["candidates"] > 1)).sum())]
    row += [int((ok & (acq["delta"] == d)).sum()) for d in _MWIN_DELTAS]
    return np.array(row, dtype=np.int64)


def _data_frame(ftype, seq, payload, hs=0x123456, hd=0x654321):
    """a serialized v2 data / connect frame (frame_v2.cpp): 17-byte header with TOTAL_CW at R1/4, LEN and the header CRC,
    the payload, the frame CRC"""
    payload = np.asarray(payload, np.uint8)
    total_cw = -(-(17 + len(payload) + 2) * 8 // 162)
    h = np.zeros(17, np.uint8)
    h[:15] = [0x55, 0x4C, ftype, 0, seq >> 8, seq & 255, hs >> 16, (hs >> 8) & 255, hs & 255, hd >> 16, (hd >> 8) & 255, hd & 255,
              total_cw, len(payload) >> 8, len(payload) & 255]
    c = _crc16(h[:15])
    h[15], h[16] = c >> 8, c & 255
    f = np.concatenate([h, payload])
    c = _crc16(f)
    return np.concatenate([f, np.array([c >> 8, c & 255], np.uint8)])


def _encode_r14(engine, frame, n_cw):
    """encodeFrameWithLDPC at R1/4 (frame_v2.cpp:1098-1130) through ria_gpu_ldpc_encode_host: CW0 = the first 20 bytes,
    CW1+ = 0xD5, index, 18 bytes.  uint8 [81 * n_cw]"""
    info = np.zeros((n_cw, 21), np.uint8)
    info[0, :min(20, len(frame))] = frame[:20]
    off, i = 20, 1
    while off < len(frame):
        info[i, 0], info[i, 1] = 0xD5, i
        chunk = frame[off:off + 18]
        info[i, 2:2 + len(chunk)] = chunk
        off += 18
        i += 1
    assert i == n_cw
    return engine.ldpc_encode(info).reshape(-1)


CONNECT_TYPE = 0x12                             # v2::FrameType::CONNECT
HANDSHAKE_KINDS = ("ping", "connect", "control", "data", "noise")


def make_handshake_windows(engine, n, kind, snr_db, seeds, mix=HANDSHAKE_KINDS, lead=2000, tail=2000, carriers=10, data_cw=3):
    """n disconnected-handshake windows on the engine's device, window i of kind mix[i % len(mix)]: a PING (the whole preamble -
    dual chirp, training, reference symbol - and no data, StreamingEncoder::encodePing), a CONNECT of 3 codewords, a 1-codeword ACK, a data frame of data_cw codewords, noise only.  Built from
    engine.chirp_preamble(), ria_gpu_ldpc_encode_host, the device modulator (DBPSK) and the reference-identical channel (one
    seed per window), peak 0.8 at sample `lead` of a window that holds 3 codewords behind the preamble (data_cw > 3: that many).
    Returns (windows float32 [n, window_len], search_len, kinds: the index into mix of every window)."""
    chirp = engine.chirp_preamble()
    frame_cw = max(3, int(data_cw))
    search_len, window_len = mcdpsk_window_recipe(len(chirp), frame_cw, lead, tail, carriers)
    frames = {"connect": (_data_frame(CONNECT_TYPE, 7, np.arange(25, dtype=np.uint8)), 3),
              "control": (control_frames([40], [ACK])[0], 1),
              "data": (_data_frame(0x30, 9, (np.arange(18 * (data_cw - 1) - 1 if data_cw > 1 else 1) % 251).astype(np.uint8)), int(data_cw))}
    pre = torch.from_numpy(np.ascontiguousarray(chirp, np.float32)).to(engine.device)
    win = torch.zeros((n, window_len), dtype=torch.float32, device=engine.device)
    kinds = np.arange(n) % len(mix)
    for k, name in enumerate(mix):
        idx = torch.from_numpy(np.nonzero(kinds == k)[0]).to(engine.device)
        if name == "noise" or len(idx) == 0:
            continue
        frame, n_cw = frames["control" if name == "ping" else name]
        body = engine.mcdpsk_modulate_batch(_encode_r14(engine, frame, n_cw)[None, :], carriers, 1, 1)[0]
        tx = torch.cat([pre, body[:9 * 512] if name == "ping" else body])       # training (8 symbols) + reference
        tx = tx * (0.8 / tx.abs().max())
        m = min(tx.shape[0], window_len - lead)
        win[idx, lead:lead + m] = tx[:m]
    engine.channel_exact_seeded_(win, kind, snr_db, np.ascontiguousarray(seeds, np.uint32))
    return win, search_len, kinds


# ---- from a capture to its frames (ria_gpu_search_batch + the window calls)
SEARCH_COUNTERS = tuple(f"outcome_{k.lower()}" for k in capi.SEARCH_OUTCOME) + \
    ("invocations", "waits", "rms_skips", "detector_runs", "rejects", "near_misses", "weak_accepts", "replays", "catchups_moderate",
     "catchups_severe")


def search_tally(result):
    """Counter row (SEARCH_COUNTERS) of one RxEngine.search call: streams per outcome, then the sums of the per-stream counters."""
    row = [int((result["outcome"] == v).sum()) for v in capi.SEARCH_OUTCOME.values()]
    row += [int(result[k].sum()) for k in SEARCH_COUNTERS[len(capi.SEARCH_OUTCOME):]]
    return np.array(row, dtype=np.int64)


def _gather_windows(captures, rows, starts, window_len):
    """float32 [len(rows), window_len] on the device: captures[rows[i], starts[i] : starts[i] + window_len]"""
    dev = captures.device
    r = torch.as_tensor(np.asarray(rows, np.int64), device=dev)[:, None]
    c = torch.as_tensor(np.asarray(starts, np.int64), device=dev)[:, None] + torch.arange(window_len, device=dev)[None, :]
    return captures[r, c].contiguous()


def rx_stream(engine, captures, capture_len, mode, control_engine=None, feed_step=0, max_invocations=1 << 20, max_events=256,
              connected=None, carriers=10, modulation="DBPSK", spreading=1):
    """Recordings in, frames out, as a composition of library calls: RxEngine.search on every open stream, then the window
    call of the mode (rx_window on `engine` with control_engine for "OFDM_LTS", mcdpsk_window for the MC-DPSK modes) on the
    window that starts at each SYNC_FOUND stream's search_start, with the parameters the search result names; then the host's
    part as INTEGRATION.md words it - the cursor to search_start + next_pos, last_cfo_ from the window's CFO, the fading hint
    (the SNR hint is the search's own), last_decoded_sync_pos_ on a delivered frame - and again, until every stream is at
    NEED_SAMPLES or LIMIT.  A window holds the window call's documented minimum (search_len + a whole frame + 32 samples for
    OFDM, search_len + an 8-codeword span for MC-DPSK), cut at the capture's end; windows of one length run in one call.

    captures: float32 [n, stride] on the device; capture_len: samples per stream.  feed_step as in RxEngine.search: 0 for a
    recording that is all there.  With feed_step > 0 a window may reach past the samples fed so far (a receiver would wait for
    them before it decodes): after the window call `fed` is moved up to the new cursor, as if the consumed samples had arrived
    meanwhile (not to the window's end: samples nobody consumed would count as backlog).  A connected MC-DPSK (ZC) recording longer than 2.5 x 31 120 samples should be given with
    feed_step 4800: with everything "already arrived" the receiver's backlog catch-up jumps to the recording's end, as the
    reference's would.  Returns, per stream, the list of events (dicts: position = sync_position, outcome = the window call's
    outcome name, frame = the delivered bytes or None).  A window result the host would pass on to another call (BURST,
    TOO_LONG) is an event with that outcome, and the cursor moves past the window's first frame; NEED_SAMPLES from a window
    call ends the stream."""
    n = captures.shape[0]
    m = capi.SEARCH_MODE[mode] if isinstance(mode, str) else int(mode)
    ofdm = m == capi.SEARCH_MODE["OFDM_LTS"]
    chirp = m == capi.SEARCH_MODE["MCDPSK_CHIRP"]
    if connected is None:
        connected = False
    lens = np.empty(n, np.int64)
    lens[:] = capture_len
    state = engine.search_state(n, fed=0 if feed_step else lens)
    bps = {"DBPSK": 1, "DQPSK": 2}[modulation] if isinstance(modulation, str) else int(modulation)
    search_len = capi.SEARCH_MIN_SEARCH[m]
    first_frame = engine.geo.frame_samples if ofdm else mcdpsk_frame_len(1, carriers, bps, spreading)
    full = search_len + (engine.geo.frame_samples + 32 if ofdm else mcdpsk_frame_len(8, carriers, bps, spreading))
    names = {v: k for k, v in (capi.WIN_OUTCOME if ofdm else capi.MWIN_OUTCOME).items()}
    events = [[] for _ in range(n)]
    open_ = np.ones(n, bool)
    while open_.any():
        idx = np.flatnonzero(open_)
        res, st = engine.search(captures[torch.as_tensor(idx, device=captures.device)].contiguous() if len(idx) < n else captures, lens[idx],
                                state[idx], m, feed_step=feed_step, max_invocations=max_invocations, connected=connected, carriers=carriers,
                                modulation=modulation, spreading=spreading)
        state[idx] = st
        found = res["outcome"] == capi.SEARCH_OUTCOME["SYNC_FOUND"]
        open_[idx[~found]] = False
        by_len = {}
        for j in np.flatnonzero(found):
            by_len.setdefault(int(min(full, lens[idx[j]] - res["search_start"][j])), []).append(j)
        for wl, js in by_len.items():
            rows, r = idx[js], res[js]
            w = _gather_windows(captures, rows, r["search_start"], wl)
            conf = np.minimum(r["min_confidence"], r["correlation"])
            if ofdm:
                frames, wres, acq, _, _ = engine.rx_window(control_engine, w, search_len, known_cfo=r["known_cfo_hz"], detect_threshold=r["detect_threshold"],
                                                           min_confidence=conf, abs_base=r["search_start"])
                nbytes, ok, fading = wres["frame"]["frame_bytes"], (wres["frame"]["success"] != 0) | (wres["frame"]["codewords_ok"] != 0), wres["fading_index"]
                cfo, moved = wres["sync_cfo_hz"], (wres["outcome"] == capi.WIN_OUTCOME["DECODED"]) | (wres["outcome"] == capi.WIN_OUTCOME["CONTROL_PROFILE"])
                last = np.where(ok, r["sync_position"], state["last_decoded_sync_pos"][rows])
            else:
                last_in = state["last_decoded_sync_pos"][rows].astype(np.int64)
                rel = np.where(last_in == capi.SEARCH_NO_LAST_SYNC, capi.MWIN_NO_LAST_SYNC, np.clip(last_in - r["search_start"], -2 ** 31 + 1, 2 ** 31 - 1))
                frames, wres, acq, _ = engine.mcdpsk_window(w, search_len, carriers=carriers, modulation=bps, spreading=spreading,
                                                            sync="chirp" if chirp else "zc", disconnected=chirp and not connected,
                                                            known_cfo=r["known_cfo_hz"], detect_threshold=r["detect_threshold"], min_confidence=conf,
                                                            abs_base=r["search_start"], last_decoded_sync=rel)
                nbytes, ok, fading = acq["frame_bytes"], wres["deliver"] != 0, acq["fading_index"]
                cfo, moved = acq["cfo_hz"], wres["outcome"] == capi.MWIN_OUTCOME["DECODED"]
                out_last = wres["last_decoded_sync"].astype(np.int64)
                last = np.where(out_last == capi.MWIN_NO_LAST_SYNC, capi.SEARCH_NO_LAST_SYNC, out_last + r["search_start"])
            frames = frames.cpu().numpy()
            for k, s in enumerate(rows):
                name = names[int(wres["outcome"][k])]
                events[s].append(dict(position=int(r["sync_position"][k]), outcome=name,
                                      frame=frames[k, :int(nbytes[k])].tobytes() if ok[k] else None))
                if moved[k]:
                    state["last_cfo_hz"][s] = cfo[k]
                    state["fading_hint"][s] = fading[k]
                state["last_decoded_sync_pos"][s] = last[k]
                if wres["next_pos"][k] >= 0:
                    state["correlation_pos"][s] = int(r["search_start"][k]) + int(wres["next_pos"][k])
                elif name in ("BURST", "TOO_LONG"):
                    state["correlation_pos"][s] = int(r["sync_position"][k]) + first_frame
                # the samples the window call consumed have arrived (feed_step > 0: a receiver waits for them before it decodes),
                # so the cursor it leaves behind is not ahead of the write position and the next feed does not clamp it back
                state["fed"][s] = max(int(state["fed"][s]), min(int(lens[s]), int(state["correlation_pos"][s])))
                if name == "NEED_SAMPLES" or len(events[s]) >= max_events or state["correlation_pos"][s] >= capi.SEARCH_MAX_CAPTURE:
                    open_[s] = False
    return events


# ---- the MC-DPSK loop with a chase pool, channel interleaving and re-entry (ria_gpu_mcdpsk_stream_batch as a composition)
PENDING_FIELDS = ("pending_total_cw", "need_samples", "pend_search_start", "pend_sync_position", "pend_known_cfo_hz", "pend_detect_threshold",
                  "pend_min_confidence", "pend_correlation")


def mcdpsk_link_stream(engine, captures, capture_len, mode, state=None, feed_step=0, max_invocations=1 << 20, max_events=256, connected=False,
                       carriers=10, modulation="DBPSK", spreading=1, chase=None, cache_id=None, t0_ms=None, channel_interleave=False,
                       interleaver_bits=None):
    """RxEngine.mcdpsk_stream as a composition of RxEngine.search and RxEngine.mcdpsk_window with the host's part between
    them in Python: rx_stream's loop for the two MC-DPSK modes, with the pool (stream s on cache cache_id[s], default s, at
    t0_ms[s] + sync_position * 1000 // sample rate), channel interleaving, and the pending rules - a window that answers
    NEED_SAMPLES leaves the eight pending fields in the state; a stream that comes in pending is not searched first: it gets
    its re-entered window if the samples it waits for are there, and closes unchanged and without an event if not.
    Returns (state (MCSTREAM_STATE), closed (RIA_STREAM_* per stream), events (STREAM_EVENT [n, max_events]), frames uint8
    [n, max_events, 320], harq (HARQ_RESULT [n, max_events])): the records of the one-call form."""
    n = captures.shape[0]
    m = capi.SEARCH_MODE[mode] if isinstance(mode, str) else int(mode)
    assert m != capi.SEARCH_MODE["OFDM_LTS"]
    chirp = m == capi.SEARCH_MODE["MCDPSK_CHIRP"]
    rate = int(engine.cfg.sample_rate)      # the rate of the audio clock
    lens = np.empty(n, np.int64)
    lens[:] = capture_len
    state = (engine.mcdpsk_stream_state(n, fed=0 if feed_step else lens) if state is None else np.array(state, engine.MCSTREAM_STATE)).copy()
    ids = np.arange(n, dtype=np.int32) if cache_id is None else np.broadcast_to(np.asarray(cache_id, np.int32), (n,))
    t0 = np.broadcast_to(np.asarray(0 if t0_ms is None else t0_ms, np.uint64), (n,))
    bps = {"DBPSK": 1, "DQPSK": 2}[modulation] if isinstance(modulation, str) else int(modulation)
    search_len = capi.SEARCH_MIN_SEARCH[m]
    first_frame = mcdpsk_frame_len(1, carriers, bps, spreading)
    full = search_len + mcdpsk_frame_len(8, carriers, bps, spreading)
    ne, row = int(max_events), engine.MCWIN_FRAME_ROW
    events = np.zeros((n, ne), engine.STREAM_EVENT)
    harq = np.zeros((n, ne), engine.HARQ_RESULT)
    frames = np.zeros((n, ne, row), np.uint8)
    n_events = np.zeros(n, np.int64)
    closed = np.zeros(n, np.int32)
    sfields = engine.SEARCH_STATE.names

    def windows(rows, det, wl, pending):
        """one window call on streams `rows` (one window length), det: per row search_start, sync_position, known_cfo_hz,
        detect_threshold, min_confidence, correlation, snr_db; then the host's part"""
        det = {k: det[k].copy() for k in det.dtype.names}       # a field of a record array is strided: torch wants it packed
        w = _gather_windows(captures, rows, det["search_start"], wl)
        last_in = state["last_decoded_sync_pos"][rows].astype(np.int64)
        rel = np.where(last_in == capi.SEARCH_NO_LAST_SYNC, capi.MWIN_NO_LAST_SYNC, np.clip(last_in - det["search_start"], -2 ** 31 + 1, 2 ** 31 - 1))
        conf = np.minimum(det["min_confidence"], det["correlation"])
        with np.errstate(over="ignore"):
            now = t0[rows] + det["sync_position"].astype(np.uint64) * np.uint64(1000) // np.uint64(rate)
        f, wres, acq, hq = engine.mcdpsk_window(w, search_len, carriers=carriers, modulation=bps, spreading=spreading, sync="chirp" if chirp else "zc",
                                                disconnected=chirp and not connected, known_cfo=det["known_cfo_hz"],
                                                detect_threshold=det["detect_threshold"], min_confidence=conf, abs_base=det["search_start"],
                                                last_decoded_sync=rel, pending_total_cw=pending, chase=chase,
                                                cache_id=ids[rows] if chase is not None else -1, now_ms=now,
                                                channel_interleave=channel_interleave, interleaver_bits=interleaver_bits)
        f = f.cpu().numpy()
        need = capi.MWIN_OUTCOME["NEED_SAMPLES"]
        for k, s in enumerate(rows):
            e = events[s, n_events[s]]
            outcome, nxt, start, sync = int(wres["outcome"][k]), int(wres["next_pos"][k]), int(det["search_start"][k]), int(det["sync_position"][k])
            e["sync_position"], e["search_start"], e["window_len"], e["outcome"] = sync, start, wl, outcome
            e["next_pos"] = start + nxt if nxt >= 0 else -1
            e["frame_bytes"], e["need_samples"], e["pending_total_cw"] = acq["frame_bytes"][k], wres["need_samples"][k], wres["pending_total_cw"][k]
            e["delivered"] = wres["deliver"][k] != 0
            for name in ("success", "codewords_ok", "codewords_failed", "frame_type"):
                e[name] = acq[name][k]
            e["correlation"], e["cfo_hz"], e["fading_index"], e["snr_db"] = det["correlation"][k], acq["cfo_hz"][k], acq["fading_index"][k], det["snr_db"][k]
            if e["delivered"]:
                nb = min(int(acq["frame_bytes"][k]), row)
                frames[s, n_events[s], :nb] = f[k, :nb]
            if chase is not None:
                harq[s, n_events[s]] = hq[k]
            if outcome == capi.MWIN_OUTCOME["DECODED"]:
                state["last_cfo_hz"][s], state["fading_hint"][s] = acq["cfo_hz"][k], acq["fading_index"][k]
            out_last = int(wres["last_decoded_sync"][k])
            state["last_decoded_sync_pos"][s] = capi.SEARCH_NO_LAST_SYNC if out_last == capi.MWIN_NO_LAST_SYNC else out_last + start
            if nxt >= 0:
                state["correlation_pos"][s] = start + nxt
            elif outcome == capi.MWIN_OUTCOME["TOO_LONG"]:
                state["correlation_pos"][s] = sync + first_frame
            state["fed"][s] = max(int(state["fed"][s]), min(int(lens[s]), int(state["correlation_pos"][s])))
            keep = outcome == need
            vals = (wres["pending_total_cw"][k], wres["need_samples"][k], start, sync, det["known_cfo_hz"][k], det["detect_threshold"][k], conf[k],
                    det["correlation"][k])
            for name, v in zip(PENDING_FIELDS, vals):
                state[name][s] = v if keep else 0
            n_events[s] += 1
            if keep:
                closed[s] = capi.STREAM_CLOSED["WINDOW_NEED_SAMPLES"]
            elif n_events[s] >= ne:
                closed[s] = capi.STREAM_CLOSED["EVENTS_FULL"]
            elif state["correlation_pos"][s] >= capi.SEARCH_MAX_CAPTURE:
                closed[s] = capi.STREAM_CLOSED["RING_END"]

    det_dtype = np.dtype([("search_start", "<i8"), ("sync_position", "<i8"), ("known_cfo_hz", "<f4"), ("detect_threshold", "<f4"),
                          ("min_confidence", "<f4"), ("correlation", "<f4"), ("snr_db", "<f4")])
    # the streams that wait at a found sync: their window, if its samples are there, ahead of the first search
    pend = np.flatnonzero(state["pending_total_cw"] > 0)
    by_len = {}
    for s in pend:
        sync, need, start = int(state["pend_sync_position"][s]), int(state["need_samples"][s]), int(state["pend_search_start"][s])
        if lens[s] >= sync + need:
            by_len.setdefault(int(min(lens[s] - start, max(full, sync - start + need))), []).append(s)
        else:
            closed[s] = capi.STREAM_CLOSED["WINDOW_NEED_SAMPLES"]
    for wl in sorted(by_len):
        rows = np.asarray(by_len[wl])
        det = np.zeros(len(rows), det_dtype)
        for a, b in (("search_start", "pend_search_start"), ("sync_position", "pend_sync_position"), ("known_cfo_hz", "pend_known_cfo_hz"),
                     ("detect_threshold", "pend_detect_threshold"), ("min_confidence", "pend_min_confidence"), ("correlation", "pend_correlation"),
                     ("snr_db", "snr_hint")):
            det[a] = state[b][rows]
        state["fed"][rows] = np.maximum(state["fed"][rows], state["pend_sync_position"][rows] + state["need_samples"][rows])
        windows(rows, det, wl, state["pending_total_cw"][rows].copy())
    while (closed == 0).any():
        idx = np.flatnonzero(closed == 0)
        sstate = np.zeros(len(idx), engine.SEARCH_STATE)
        for name in sfields:
            sstate[name] = state[name][idx]
        res, st = engine.search(captures[torch.as_tensor(idx, device=captures.device)].contiguous() if len(idx) < n else captures, lens[idx],
                                sstate, m, feed_step=feed_step, max_invocations=max_invocations, connected=connected, carriers=carriers,
                                modulation=modulation, spreading=spreading)
        for name in sfields:
            state[name][idx] = st[name]
        found = res["outcome"] == capi.SEARCH_OUTCOME["SYNC_FOUND"]
        closed[idx[~found]] = res["outcome"][~found]
        by_len = {}
        for j in np.flatnonzero(found):
            by_len.setdefault(int(min(full, lens[idx[j]] - res["search_start"][j])), []).append(j)
        for wl in sorted(by_len):
            js = by_len[wl]
            det = np.zeros(len(js), det_dtype)
            for a, b in (("search_start", "search_start"), ("sync_position", "sync_position"), ("known_cfo_hz", "known_cfo_hz"),
                         ("detect_threshold", "detect_threshold"), ("min_confidence", "min_confidence"), ("correlation", "correlation"),
                         ("snr_db", "sync_snr_db")):
                det[a] = res[b][js]
            windows(idx[js], det, wl, 0)
    return state, closed, events, frames, harq


LINK_STREAM_COUNTERS = tuple(f"outcome_{k.lower()}" for k in capi.MWIN_OUTCOME) + ("delivered", "recovered_by_sum", "stores", "combines")


def link_stream_tally(events, harq):
    """Counter row (LINK_STREAM_COUNTERS) of one mcdpsk_stream / mcdpsk_link_stream call (events STREAM_EVENT [n, max_events],
    harq HARQ_RESULT [n, max_events]; rows past a stream's events are zero and count nowhere: window_len 0): events per window
    outcome, frames delivered, frames a combined sum recovered (success with a codeword of recovered_mask), codewords stored
    and sums combined."""
    live = events["window_len"] > 0
    row = [int(((events["outcome"] == v) & live).sum()) for v in capi.MWIN_OUTCOME.values()]
    row.append(int(((events["delivered"] != 0) & live).sum()))
    row.append(int(((events["success"] != 0) & (harq["recovered_mask"] != 0) & live).sum()))
    row.append(int(_popcount16(harq["stored_mask"][live]).sum()))
    row.append(int(_popcount16(harq["sum_mask"][live]).sum()))
    return np.array(row, dtype=np.int64)


# ---- recordings longer than the ring buffer (ria_gpu_search_ring_batch + the window calls)
RING_COUNTERS = ("overflows", "overflow_dropped", "drift_snaps", "cursor_inits")


def rx_ring(engine, captures, capture_len, mode, control_engine=None, feed_step=4800, max_invocations=1 << 20, max_events=256,
            connected=None, carriers=10, modulation="DBPSK", spreading=1, state=None):
    """rx_stream for recordings of any length: RxEngine.search_ring (the decoder's 960 000-sample ring buffer wraps, with
    feedAudio's drift guard and overflow drop) on every open stream, then the window call of the mode on the window cut from
    the capture by ABSOLUTE index, [abs_search_start, abs_search_start + min(full, capture_len - abs_search_start)), with
    abs_base = abs_search_start and, for MC-DPSK, last_decoded_sync_pos rebased to the window's origin by circular difference;
    then the host's part modulo the ring: the cursor to (search_start + next_pos) % 960000 (behind the first frame of a BURST /
    TOO_LONG window), last_decoded_sync_pos as a ring index, total_fed = max(total_fed, min(capture_len, absolute cursor)).
    A stream whose found span crossed the write position (span_wraps: its window is no contiguous piece of the capture)
    closes with "SPAN_LOST"; one that reaches max_events or whose window call wants samples the capture does not hold closes
    too.  There is no end of the ring to close at.

    feed_step must let the search keep up: with feed_step 0 a recording longer than the ring is "all there" and the decoder
    sees only its last 960 000 samples, as the reference's would.  state: RING_STATE records to continue from (default:
    fresh decoders, nothing fed for feed_step > 0).  Returns (events, state, closed, counters): per stream the list of events
    (dicts: position = the sync's absolute index, search_start = abs_search_start, outcome, frame = the delivered bytes or
    None), the final RING_STATE records, why each stream closed ("NEED_SAMPLES" / "LIMIT" from the search, "WINDOW_NEED_SAMPLES",
    "EVENTS_FULL", "SPAN_LOST") and the search's RING_COUNTERS summed over the legs (int64 [n, 4])."""
    n = captures.shape[0]
    m = capi.SEARCH_MODE[mode] if isinstance(mode, str) else int(mode)
    ofdm = m == capi.SEARCH_MODE["OFDM_LTS"]
    chirp = m == capi.SEARCH_MODE["MCDPSK_CHIRP"]
    connected = bool(connected)
    ring = capi.RING_SAMPLES
    lens = np.empty(n, np.int64)
    lens[:] = capture_len
    state = engine.ring_state(n, total_fed=0 if feed_step else lens) if state is None else np.array(state, engine.RING_STATE)
    bps = {"DBPSK": 1, "DQPSK": 2}[modulation] if isinstance(modulation, str) else int(modulation)
    search_len = capi.SEARCH_MIN_SEARCH[m]
    first_frame = engine.geo.frame_samples if ofdm else mcdpsk_frame_len(1, carriers, bps, spreading)
    full = search_len + (engine.geo.frame_samples + 32 if ofdm else mcdpsk_frame_len(8, carriers, bps, spreading))
    if full > ring - 1:
        raise ValueError("the window of this configuration is longer than the ring buffer")
    names = {v: k for k, v in (capi.WIN_OUTCOME if ofdm else capi.MWIN_OUTCOME).items()}
    search_names = {v: k for k, v in capi.SEARCH_OUTCOME.items()}
    events = [[] for _ in range(n)]
    closed = [None] * n
    counters = np.zeros((n, len(RING_COUNTERS)), np.int64)
    open_ = np.ones(n, bool)
    while open_.any():
        idx = np.flatnonzero(open_)
        res, st = engine.search_ring(captures[torch.as_tensor(idx, device=captures.device)].contiguous() if len(idx) < n else captures, lens[idx],
                                     state[idx], m, feed_step=feed_step, max_invocations=max_invocations, connected=connected, carriers=carriers,
                                     modulation=modulation, spreading=spreading)
        state[idx] = st
        for c, k in enumerate(RING_COUNTERS):
            counters[idx, c] += res[k].astype(np.int64)
        found = res["outcome"] == capi.SEARCH_OUTCOME["SYNC_FOUND"]
        for j in np.flatnonzero(~found):
            open_[idx[j]], closed[idx[j]] = False, search_names[int(res["outcome"][j])]
        by_len = {}
        for j in np.flatnonzero(found):
            if res["span_wraps"][j]:
                open_[idx[j]], closed[idx[j]] = False, "SPAN_LOST"
                continue
            by_len.setdefault(int(min(full, lens[idx[j]] - res["abs_search_start"][j])), []).append(j)
        for wl, js in by_len.items():
            rows, r = idx[js], res[js]
            w = _gather_windows(captures, rows, r["abs_search_start"], wl)
            conf = np.minimum(r["min_confidence"], r["correlation"])
            ss = r["search_start"].astype(np.int64)
            if ofdm:
                frames, wres, acq, _, _ = engine.rx_window(control_engine, w, search_len, known_cfo=r["known_cfo_hz"], detect_threshold=r["detect_threshold"],
                                                           min_confidence=conf, abs_base=r["abs_search_start"])
                nbytes, ok, fading = wres["frame"]["frame_bytes"], (wres["frame"]["success"] != 0) | (wres["frame"]["codewords_ok"] != 0), wres["fading_index"]
                cfo, moved = wres["sync_cfo_hz"], (wres["outcome"] == capi.WIN_OUTCOME["DECODED"]) | (wres["outcome"] == capi.WIN_OUTCOME["CONTROL_PROFILE"])
                last = np.where(ok, r["sync_position"], state["last_decoded_sync_pos"][rows])
            else:
                last_in = state["last_decoded_sync_pos"][rows].astype(np.int64)
                d = (last_in - ss) % ring                    # the circular difference to the window's origin, in -480 000 .. 479 999
                d = np.where(d >= ring // 2, d - ring, d)
                rel = np.where(last_in == capi.SEARCH_NO_LAST_SYNC, capi.MWIN_NO_LAST_SYNC, d)
                frames, wres, acq, _ = engine.mcdpsk_window(w, search_len, carriers=carriers, modulation=bps, spreading=spreading,
                                                            sync="chirp" if chirp else "zc", disconnected=chirp and not connected,
                                                            known_cfo=r["known_cfo_hz"], detect_threshold=r["detect_threshold"], min_confidence=conf,
                                                            abs_base=r["abs_search_start"], last_decoded_sync=rel)
                nbytes, ok, fading = acq["frame_bytes"], wres["deliver"] != 0, acq["fading_index"]
                cfo, moved = acq["cfo_hz"], wres["outcome"] == capi.MWIN_OUTCOME["DECODED"]
                out_last = wres["last_decoded_sync"].astype(np.int64)
                last = np.where(out_last == capi.MWIN_NO_LAST_SYNC, capi.SEARCH_NO_LAST_SYNC, (out_last + ss) % ring)
            frames = frames.cpu().numpy()
            for k, s in enumerate(rows):
                name = names[int(wres["outcome"][k])]
                events[s].append(dict(position=int(r["abs_position"][k]), search_start=int(r["abs_search_start"][k]), outcome=name,
                                      frame=frames[k, :int(nbytes[k])].tobytes() if ok[k] else None))
                if moved[k]:
                    state["last_cfo_hz"][s] = cfo[k]
                    state["fading_hint"][s] = fading[k]
                state["last_decoded_sync_pos"][s] = last[k]
                abs_cursor = None
                if wres["next_pos"][k] >= 0:
                    abs_cursor = int(r["abs_search_start"][k]) + int(wres["next_pos"][k])
                elif name in ("BURST", "TOO_LONG"):
                    abs_cursor = int(r["abs_position"][k]) + first_frame
                if abs_cursor is not None:
                    # the same offset from the span's first sample in ring indices; the consumed samples have arrived
                    state["correlation_pos"][s] = (int(ss[k]) + abs_cursor - int(r["abs_search_start"][k])) % ring
                    state["total_fed"][s] = max(int(state["total_fed"][s]), min(int(lens[s]), abs_cursor))
                if name == "NEED_SAMPLES":
                    open_[s], closed[s] = False, "WINDOW_NEED_SAMPLES"
                elif len(events[s]) >= max_events:
                    open_[s], closed[s] = False, "EVENTS_FULL"
    return events, state, closed, counters


# ---- the MC-DPSK link on recordings longer than the ring buffer (ria_gpu_mcdpsk_ring_batch as a composition)
def mcdpsk_link_ring(engine, captures, capture_len, mode, state=None, feed_step=4800, max_invocations=1 << 20, max_events=256, connected=False,
                     carriers=10, modulation="DBPSK", spreading=1, chase=None, cache_id=None, t0_ms=None, channel_interleave=False,
                     interleaver_bits=None):
    """RxEngine.mcdpsk_ring as a composition of RxEngine.search_ring and RxEngine.mcdpsk_window with the host's part between
    them in Python: rx_ring's loop for the two MC-DPSK modes - windows cut by absolute index, cursor and last decoded position
    on the ring - with what mcdpsk_link_stream adds to rx_stream: the pool (stream s on cache cache_id[s], default s, at
    t0_ms[s] + ABSOLUTE sync position * 1000 // sample rate), channel interleaving, and the pending rules with absolute
    positions in the state.  It is to rx_ring what mcdpsk_link_stream is to rx_stream.  A pending state outside the call's
    domain is a ValueError.  Returns (state (MCRING_STATE), closed (RIA_STREAM_* per stream), events (STREAM_EVENT
    [n, max_events]), frames uint8 [n, max_events, 320], harq (HARQ_RESULT [n, max_events]), counters (RING_COUNTERS summed
    over the legs, int64 [n, 4])): the records of the one-call form; link_stream_tally works on events and harq."""
    n = captures.shape[0]
    m = capi.SEARCH_MODE[mode] if isinstance(mode, str) else int(mode)
    assert m != capi.SEARCH_MODE["OFDM_LTS"]
    chirp = m == capi.SEARCH_MODE["MCDPSK_CHIRP"]
    rate = int(engine.cfg.sample_rate)      # the rate of the audio clock
    ring = capi.RING_SAMPLES
    lens = np.empty(n, np.int64)
    lens[:] = capture_len
    state = (engine.mcdpsk_ring_state(n, total_fed=0 if feed_step else lens) if state is None else np.array(state, engine.MCRING_STATE)).copy()
    ids = np.arange(n, dtype=np.int32) if cache_id is None else np.broadcast_to(np.asarray(cache_id, np.int32), (n,))
    t0 = np.broadcast_to(np.asarray(0 if t0_ms is None else t0_ms, np.uint64), (n,))
    bps = {"DBPSK": 1, "DQPSK": 2}[modulation] if isinstance(modulation, str) else int(modulation)
    search_len = capi.SEARCH_MIN_SEARCH[m]
    first_frame = mcdpsk_frame_len(1, carriers, bps, spreading)
    full = search_len + mcdpsk_frame_len(8, carriers, bps, spreading)
    if full > ring - 1:
        raise ValueError("the window of this configuration is longer than the ring buffer")
    ne, row = int(max_events), engine.MCWIN_FRAME_ROW
    events = np.zeros((n, ne), engine.STREAM_EVENT)
    harq = np.zeros((n, ne), engine.HARQ_RESULT)
    frames = np.zeros((n, ne, row), np.uint8)
    n_events = np.zeros(n, np.int64)
    closed = np.zeros(n, np.int32)
    counters = np.zeros((n, len(RING_COUNTERS)), np.int64)
    rfields = engine.RING_STATE.names

    def windows(rows, det, wl, pending):
        """one window call on streams `rows` (one window length), det: per row abs_search_start, abs_position, known_cfo_hz,
        detect_threshold, min_confidence, correlation, snr_db; then the host's part, modulo the ring"""
        det = {k: det[k].copy() for k in det.dtype.names}
        starts, syncs = det["abs_search_start"], det["abs_position"]
        w = _gather_windows(captures, rows, starts, wl)
        last_in = state["last_decoded_sync_pos"][rows].astype(np.int64)
        d = (last_in - starts) % ring                    # the circular difference to the window's origin, in -480 000 .. 479 999
        d = np.where(d >= ring // 2, d - ring, d)
        rel = np.where(last_in == capi.SEARCH_NO_LAST_SYNC, capi.MWIN_NO_LAST_SYNC, d)
        conf = np.minimum(det["min_confidence"], det["correlation"])
        with np.errstate(over="ignore"):
            now = t0[rows] + syncs.astype(np.uint64) * np.uint64(1000) // np.uint64(rate)
        f, wres, acq, hq = engine.mcdpsk_window(w, search_len, carriers=carriers, modulation=bps, spreading=spreading, sync="chirp" if chirp else "zc",
                                                disconnected=chirp and not connected, known_cfo=det["known_cfo_hz"],
                                                detect_threshold=det["detect_threshold"], min_confidence=conf, abs_base=starts,
                                                last_decoded_sync=rel, pending_total_cw=pending, chase=chase,
                                                cache_id=ids[rows] if chase is not None else -1, now_ms=now,
                                                channel_interleave=channel_interleave, interleaver_bits=interleaver_bits)
        f = f.cpu().numpy()
        need = capi.MWIN_OUTCOME["NEED_SAMPLES"]
        for k, s in enumerate(rows):
            e = events[s, n_events[s]]
            outcome, nxt, start, sync = int(wres["outcome"][k]), int(wres["next_pos"][k]), int(starts[k]), int(syncs[k])
            e["sync_position"], e["search_start"], e["window_len"], e["outcome"] = sync, start, wl, outcome
            e["next_pos"] = start + nxt if nxt >= 0 else -1
            e["frame_bytes"], e["need_samples"], e["pending_total_cw"] = acq["frame_bytes"][k], wres["need_samples"][k], wres["pending_total_cw"][k]
            e["delivered"] = wres["deliver"][k] != 0
            for name in ("success", "codewords_ok", "codewords_failed", "frame_type"):
                e[name] = acq[name][k]
            e["correlation"], e["cfo_hz"], e["fading_index"], e["snr_db"] = det["correlation"][k], acq["cfo_hz"][k], acq["fading_index"][k], det["snr_db"][k]
            if e["delivered"]:
                nb = min(int(acq["frame_bytes"][k]), row)
                frames[s, n_events[s], :nb] = f[k, :nb]
            if chase is not None:
                harq[s, n_events[s]] = hq[k]
            if outcome == capi.MWIN_OUTCOME["DECODED"]:
                state["last_cfo_hz"][s], state["fading_hint"][s] = acq["cfo_hz"][k], acq["fading_index"][k]
            out_last = int(wres["last_decoded_sync"][k])
            state["last_decoded_sync_pos"][s] = capi.SEARCH_NO_LAST_SYNC if out_last == capi.MWIN_NO_LAST_SYNC else (out_last + start) % ring
            abs_cursor = None
            if nxt >= 0:
                abs_cursor = start + nxt
            elif outcome == capi.MWIN_OUTCOME["TOO_LONG"]:
                abs_cursor = sync + first_frame
            if abs_cursor is not None:
                state["correlation_pos"][s] = abs_cursor % ring
                state["total_fed"][s] = max(int(state["total_fed"][s]), min(int(lens[s]), abs_cursor))
            keep = outcome == need
            vals = (wres["pending_total_cw"][k], wres["need_samples"][k], start, sync, det["known_cfo_hz"][k], det["detect_threshold"][k], conf[k],
                    det["correlation"][k])
            for name, v in zip(PENDING_FIELDS, vals):
                state[name][s] = v if keep else 0
            n_events[s] += 1
            if keep:
                closed[s] = capi.RING_STREAM_CLOSED["WINDOW_NEED_SAMPLES"]
            elif n_events[s] >= ne:
                closed[s] = capi.RING_STREAM_CLOSED["EVENTS_FULL"]

    det_dtype = np.dtype([("abs_search_start", "<i8"), ("abs_position", "<i8"), ("known_cfo_hz", "<f4"), ("detect_threshold", "<f4"),
                          ("min_confidence", "<f4"), ("correlation", "<f4"), ("snr_db", "<f4")])
    # the streams that wait at a found sync: their window, if its samples are there, ahead of the first search
    pend = np.flatnonzero(state["pending_total_cw"] > 0)
    by_len = {}
    for s in pend:
        sync, need, start = int(state["pend_sync_position"][s]), int(state["need_samples"][s]), int(state["pend_search_start"][s])
        fed = int(state["total_fed"][s])
        if not (state["pending_total_cw"][s] <= 255 and need >= 0 and 0 <= start < lens[s] and 0 <= sync < lens[s] and lens[s] - start >= search_len and
                sync - start + need <= ring - 1 and fed - start <= ring and start + search_len <= fed):
            raise ValueError(f"stream {s}: pending fields outside the call's domain")
        if lens[s] >= sync + need:
            by_len.setdefault(int(min(lens[s] - start, max(full, sync - start + need))), []).append(s)
        else:
            closed[s] = capi.RING_STREAM_CLOSED["WINDOW_NEED_SAMPLES"]
    for wl in sorted(by_len):
        rows = np.asarray(by_len[wl])
        det = np.zeros(len(rows), det_dtype)
        for a, b in (("abs_search_start", "pend_search_start"), ("abs_position", "pend_sync_position"), ("known_cfo_hz", "pend_known_cfo_hz"),
                     ("detect_threshold", "pend_detect_threshold"), ("min_confidence", "pend_min_confidence"), ("correlation", "pend_correlation"),
                     ("snr_db", "snr_hint")):
            det[a] = state[b][rows]
        state["total_fed"][rows] = np.maximum(state["total_fed"][rows], state["pend_sync_position"][rows].astype(np.int64) + state["need_samples"][rows])
        windows(rows, det, wl, state["pending_total_cw"][rows].copy())
    while (closed == 0).any():
        idx = np.flatnonzero(closed == 0)
        rstate = np.zeros(len(idx), engine.RING_STATE)
        for name in rfields:
            rstate[name] = state[name][idx]
        res, st = engine.search_ring(captures[torch.as_tensor(idx, device=captures.device)].contiguous() if len(idx) < n else captures, lens[idx],
                                     rstate, m, feed_step=feed_step, max_invocations=max_invocations, connected=connected, carriers=carriers,
                                     modulation=modulation, spreading=spreading)
        for name in rfields:
            state[name][idx] = st[name]
        for c, k in enumerate(RING_COUNTERS):
            counters[idx, c] += res[k].astype(np.int64)
        found = res["outcome"] == capi.SEARCH_OUTCOME["SYNC_FOUND"]
        closed[idx[~found]] = res["outcome"][~found]
        by_len = {}
        for j in np.flatnonzero(found):
            if res["span_wraps"][j]:
                closed[idx[j]] = capi.RING_STREAM_CLOSED["SPAN_LOST"]
                continue
            by_len.setdefault(int(min(full, lens[idx[j]] - res["abs_search_start"][j])), []).append(j)
        for wl in sorted(by_len):
            js = by_len[wl]
            det = np.zeros(len(js), det_dtype)
            for a, b in (("abs_search_start", "abs_search_start"), ("abs_position", "abs_position"), ("known_cfo_hz", "known_cfo_hz"),
                         ("detect_threshold", "detect_threshold"), ("min_confidence", "min_confidence"), ("correlation", "correlation"),
                         ("snr_db", "sync_snr_db")):
                det[a] = res[b][js]
            windows(idx[js], det, wl, 0)
    return state, closed, events, frames, harq, counters


# ---- the same loop in one call (ria_gpu_rx_stream_batch)
STREAM_COUNTERS = ("streams", "events", "delivered") + tuple(f"closed_{k.lower()}" for k in capi.STREAM_CLOSED) + \
    ("search_legs",) + SEARCH_COUNTERS[len(capi.SEARCH_OUTCOME):]


def stream_events(results, events, frames):
    """The records of RxEngine.rx_stream / rx_stream_host (results STREAM_RESULT [n], events STREAM_EVENT [n, max_events],
    frames uint8 [n, max_events, row], a tensor or an array) in the form rx_stream returns: per stream the list of events,
    dicts of position, outcome (the window call's outcome name of the result's mode) and frame (the delivered bytes or None)."""
    if isinstance(frames, torch.Tensor):
        frames = frames.cpu().numpy()
    out = []
    for s in range(len(results)):
        ofdm = int(results["mode"][s]) == capi.SEARCH_MODE["OFDM_LTS"]
        names = {v: k for k, v in (capi.WIN_OUTCOME if ofdm else capi.MWIN_OUTCOME).items()}
        out.append([dict(position=int(e["sync_position"]), outcome=names[int(e["outcome"])],
                         frame=frames[s, k, :int(e["frame_bytes"])].tobytes() if e["delivered"] else None)
                    for k, e in enumerate(events[s, :int(results["n_events"][s])])])
    return out


def stream_tally(results, events):
    """Counter row (STREAM_COUNTERS) of one RxEngine.rx_stream call: streams, events, events that delivered a frame, streams
    per reason they closed for, search legs, then the sums of the search counters over the call's legs."""
    n_ev = results["n_events"].astype(np.int64)
    live = np.arange(events.shape[1])[None, :] < n_ev[:, None]
    row = [len(results), int(n_ev.sum()), int(((events["delivered"] != 0) & live).sum())]
    row += [int((results["closed"] == v).sum()) for v in capi.STREAM_CLOSED.values()]
    row += [int(results["search_legs"].sum())] + [int(results[k].sum()) for k in SEARCH_COUNTERS[len(capi.SEARCH_OUTCOME):]]
    return np.array(row, dtype=np.int64)
