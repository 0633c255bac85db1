"""Throughput of ria_gpu_mcdpsk_acquire_batch (RxEngine.mcdpsk_acquire) on one GPU; prints one JSON line.

Workloads (all windows built and channelled on the device, ria_amd.acquire.make_mcdpsk_windows):
  connect_awgn / connect_moderate: disconnected CONNECT windows (dual chirp, DBPSK, 10 carriers, frame_cw 3) at low SNR
  connect_recovery: connect_awgn with the frame 288 samples behind the preamble (timing recovery)
  zc_connected: connected ZC windows of a 1-CW control frame
  host_chain: the connect_awgn windows through the separate calls driven from the host, primary candidate only, with
              the time of each stage (sync_chirp, mcdpsk_demod, ldpc_decode_robust of every codeword)

--harq N: instead, the cost of the HARQ chase cache (ria_gpu_mcdpsk_acquire_harq_batch).  The connect_moderate windows at
  --harq-snr are N transmissions of the same links (window i = link i = cache i of one pool, a new channel seed per
  transmission).  Times the plain call and the HARQ entry without a pool on transmission 0, then the N transmissions into
  the pool (cleared before each repetition), with the HARQ counters of every transmission (ria_amd.acquire.harq_tally: the
  windows' last candidates) and what the transmission added to the caches' own statistics, summed over the pool.  --harq-call-only: one pass of the pool calls alone, for a kernel trace.

--channel-interleave: the link negotiated MC-DPSK channel interleaving.  The data frames (the CONNECT; not the 20-byte ACK)
  are interleaved on the device (ria_gpu_mcdpsk_interleave_batch, width carriers x bits = 10) before they are modulated, and
  every acquire call sets RIA_MACQ_CHANNEL_INTERLEAVE (ria_gpu_mcdpsk_acquire_ci_batch).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps, out


def ci_args(e, a, coded):
    """-> (the coded bytes the windows carry, the keyword arguments of every acquire call)"""
    if not a.channel_interleave:
        return coded, {}
    return e.mcdpsk_interleave(coded, 10).cpu().numpy(), {"channel_interleave": True, "interleaver_bits": 10}


def harq_mode(e, a):
    from mcdpsk_acquire_restatement import CONNECT, data_frame, encode_frame
    from ria_amd.acquire import HARQ_COUNTERS, harq_tally, make_mcdpsk_windows
    from ria_amd.engine import ChasePool
    from ria_amd.srchash import csrc_sha256
    n, N = a.windows, a.harq
    connect, ci = ci_args(e, a, encode_frame(data_frame(CONNECT, 7, np.arange(25, dtype=np.uint8)))[None, :])
    chirp = e.chirp_preamble()
    base = np.arange(1, n + 1, dtype=np.uint32) * np.uint32(2654435761)
    wins = []
    for t in range(N):
        w, sl = make_mcdpsk_windows(e, connect, chirp, n, 3, 2, a.harq_snr, base + np.uint32(7919 * t))
        wins.append(w)
    pool = e.chase_pool(n, max_entries=a.harq_entries)
    out = {"metric": "mcdpsk_acquire_harq_ms", "windows": n, "transmissions": N, "snr_db": a.harq_snr, "channel": "moderate",
           "channel_interleave": bool(a.channel_interleave), "pool_entries": a.harq_entries, "pool_bytes": n * a.harq_entries * 16 * 648 * 4, "source_hash": csrc_sha256()}

    def pass_(record):
        pool.clear()
        torch.cuda.synchronize()
        rows = []
        for t in range(N):
            t0 = time.perf_counter()
            frames, res, hq = e.mcdpsk_acquire(wins[t], sl, 3, chase=pool, now_ms=1000 * t, **ci)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if record:
                rows.append((dt, res, hq))
        return rows
    pass_(False)
    if a.harq_call_only:
        print(json.dumps(out))
        return
    reps = [pass_(True) for _ in range(a.reps)]
    dt, (_, res0) = timed(lambda: e.mcdpsk_acquire(wins[0], sl, 3, **ci), a.reps)
    out["plain_call"] = {"ms": dt * 1e3, "success": int(res0["success"].sum()), "candidates": int(res0["candidates"].sum())}
    dt, (_, res1, _) = timed(lambda: e.mcdpsk_acquire(wins[0], sl, 3, harq_entry=True, **ci), a.reps)
    out["harq_entry_no_pool"] = {"ms": dt * 1e3, "equal_to_plain": bool(res0.tobytes() == res1.tobytes())}
    out["with_pool"] = []
    for t in range(N):
        _, res, hq = reps[-1][t]
        row = {"transmission": t, "ms": float(np.mean([r[t][0] for r in reps])) * 1e3, "success": int(res["success"].sum()),
               "candidates": int(res["candidates"].sum())}
        row.update({k: int(v) for k, v in zip(HARQ_COUNTERS, harq_tally(res, hq))})
        out["with_pool"].append(row)
    # the caches' own counters per transmission, from one more pass (the counters run on through clear(): differences)
    def totals():
        tot = dict.fromkeys(ChasePool.STATS, 0)
        for c in range(n):
            for k, v in pool.stats(c).items():
                tot[k] += v
        return tot
    pool.clear()
    before = totals()
    for t in range(N):
        e.mcdpsk_acquire(wins[t], sl, 3, chase=pool, now_ms=1000 * t, **ci)
        after = totals()
        out["with_pool"][t]["cache_stats"] = {k: after[k] - before[k] for k in ChasePool.STATS}
        before = after
    out["live_entries"] = sum(len(pool.export(c)[0]) for c in range(n))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--harq", type=int, default=0, help="N > 0: time N transmissions of the same links into one chase pool instead")
    ap.add_argument("--harq-snr", type=float, default=-8.0)
    ap.add_argument("--harq-entries", type=int, default=2)
    ap.add_argument("--harq-call-only", action="store_true")
    ap.add_argument("--channel-interleave", action="store_true", help="interleave the data frames and set RIA_MACQ_CHANNEL_INTERLEAVE")
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--snr", type=float, default=0.0)
    ap.add_argument("--zc-snr", type=float, default=15.0)
    a = ap.parse_args()
    from mcdpsk_acquire_restatement import ACK, CONNECT, control_frame, data_frame, encode_frame
    from ria_amd.acquire import make_mcdpsk_windows, mcdpsk_frame_len
    from ria_amd.engine import RxEngine
    from ria_amd.srchash import csrc_sha256
    e = RxEngine("DQPSK", "R1_4", max_batch=64)
    if a.harq > 0:
        return harq_mode(e, a)
    n = a.windows
    seeds = np.arange(1, n + 1, dtype=np.uint32) * np.uint32(2654435761)
    connect, ci = ci_args(e, a, encode_frame(data_frame(CONNECT, 7, np.arange(25, dtype=np.uint8)))[None, :])
    chirp = e.chirp_preamble()
    out = {"metric": "mcdpsk_acquire_windows_per_s", "windows": n, "snr_db": a.snr, "channel_interleave": bool(a.channel_interleave),
           "source_hash": csrc_sha256()}
    for name, kind in (("connect_awgn", 0), ("connect_moderate", 2)):
        w, sl = make_mcdpsk_windows(e, connect, chirp, n, 3, kind, a.snr, seeds)
        dt, (frames, res) = timed(lambda: e.mcdpsk_acquire(w, sl, 3, **ci), a.reps)
        out[name] = {"windows_per_s": n / dt, "ms": dt * 1e3, "success": int(res["success"].sum()),
                     "recovered": int(((res["success"] != 0) & (res["candidates"] > 1)).sum()),
                     "candidates": int(res["candidates"].sum())}
        if kind == 0:
            # the same windows through the separate calls, stage by stage (primary candidate only): detection, demodulation
            # at the detected starts, robust decode of every codeword; windows are gathered between the stages
            fl = mcdpsk_frame_len(3)
            dt_sync, ch = timed(lambda: e.sync_chirp(w[:, :sl].contiguous(), 0.15), a.reps)
            ok = np.nonzero(ch["success"] != 0)[0]
            starts = ch["down_chirp_start"][ok].astype(np.int64) + 28800
            fit = ok[starts + fl <= w.shape[1]]
            starts = ch["down_chirp_start"][fit].astype(np.int64) + 28800
            idx = torch.from_numpy(fit).to(e.device)
            cols = torch.from_numpy(starts).to(e.device)[:, None] + torch.arange(fl, device=e.device)[None, :]
            frames_ = torch.gather(w[idx], 1, cols).contiguous()
            cfo = torch.from_numpy(ch["cfo_hz"][fit].astype(np.float32)).to(e.device)
            dt_demod, (llr, _) = timed(lambda: e.mcdpsk_demod(frames_, 10, 1, 1, cfo_hz=cfo), a.reps)
            rows = llr[:, :3 * 648].reshape(-1, 648).contiguous()
            dt_dec, _ = timed(lambda: e.ldpc_decode_robust(rows), a.reps)
            out["host_chain"] = {"detect_ms": dt_sync * 1e3, "demod_ms": dt_demod * 1e3, "decode_ms": dt_dec * 1e3,
                                 "sum_ms": (dt_sync + dt_demod + dt_dec) * 1e3,
                                 "windows_per_s": n / (dt_sync + dt_demod + dt_dec), "windows_decoded": len(fit)}
            del frames_, llr, rows
        del w
    # windows whose frame sits 288 samples behind the preamble: the primary and the alternate fail, the timing recovery
    # decodes them (at +48 samples in the restatement's AWGN windows)
    w, sl = make_mcdpsk_windows(e, connect, chirp, n, 3, 0, a.snr, seeds, gap=288)
    dt, (frames, res) = timed(lambda: e.mcdpsk_acquire(w, sl, 3, **ci), a.reps)
    out["connect_recovery"] = {"windows_per_s": n / dt, "ms": dt * 1e3, "success": int(res["success"].sum()),
                               "recovered": int(((res["success"] != 0) & (res["candidates"] > 1)).sum()),
                               "candidates": int(res["candidates"].sum())}
    del w
    # connected ZC windows at an SNR where the detector accepts them (at 0 dB the ZC correlation stays below 0.25 and the
    # call is detection only)
    ack = encode_frame(control_frame(ACK, 3))[None, :]
    zc = e.zc_preamble(5)
    w, sl = make_mcdpsk_windows(e, ack, zc, n, 1, 0, a.zc_snr, seeds)
    dt, (frames, res) = timed(lambda: e.mcdpsk_acquire(w, sl, 1, sync="zc", min_confidence=0.25, **ci), a.reps)
    out["zc_connected"] = {"snr_db": a.zc_snr, "windows_per_s": n / dt, "ms": dt * 1e3, "accepted": int(res["accepted"].sum()),
                           "candidates": int(res["candidates"].sum())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
