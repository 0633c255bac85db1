#!/usr/bin/env python3
"""Throughput of ria_gpu_rx_acquire_batch (LTS detection + acceptance + demod/decode + timing recovery in one call) on
QAM16 R1/2 capture windows built by ria_amd.acquire.make_windows, at AWGN 20 dB and at Watterson moderate 12 dB, against
the same windows through sync_lts + rx(offsets=...) called separately (primary candidate only, and with the timing
recovery driven from the host, one rx call per round).  Prints one JSON line; not the contract bench (bench.py is).

Stage times come from device events around calls that reproduce each stage on its own: the detector alone (the strided
sync_lts call the entry point makes), and each round's demod + decode as rx_batch at exactly that round's candidates
(round r holds the windows with more than r candidates, each at its r-th candidate that fits).  'other_ms' is what the
whole call takes beyond their sum: the plan / scatter / next kernels and the per-round host read."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ria_amd.acquire import DETECT_THRESHOLD, SEARCH_LEN, make_windows  # noqa: E402
from ria_amd.engine import RxEngine  # noqa: E402
from ria_amd.sweep import SweepPoint  # noqa: E402

DELTAS = (0, 8, -8, 16, -16, 24, -24, 32, -32)


def timed_ms(fn, reps):
    """median of reps device-event timings of fn(), after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def sync_strided(e, win, search_len, out):
    n, wl = win.shape
    e._check(e.lib.ria_gpu_sync_lts_batch(e.h, C.c_void_p(win.data_ptr()), wl, search_len, n, None, float(DETECT_THRESHOLD),
                                          C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def round_offsets(res, wl, fs, r):
    """(window indices, candidate starts) of round r: windows with more than r candidates, at their r-th fitting one"""
    idx, starts = [], []
    for w in np.nonzero(res["candidates"] > r)[0]:
        fit = [res["sync_start"][w] + d for d in DELTAS if 0 <= res["sync_start"][w] + d and res["sync_start"][w] + d + fs <= wl]
        idx.append(w)
        starts.append(fit[r])
    return np.array(idx, np.int64), np.array(starts, np.int64)


def point(e, name, pt, n, reps):
    win, sent, _ = make_windows(e, 20261016, pt, 0, 0, n)
    wl, fs = win.shape[1], e.geo.frame_samples
    sl = SEARCH_LEN
    info, st, res = e.rx_acquire(win, sl, detect_threshold=DETECT_THRESHOLD)
    torch.cuda.synchronize()
    t_full = timed_ms(lambda: e.rx_acquire(win, sl, detect_threshold=DETECT_THRESHOLD), reps)
    t_primary_call = timed_ms(lambda: e.rx_acquire(win, sl, detect_threshold=DETECT_THRESHOLD, retry=False), reps)
    lts = torch.zeros((n, 32), dtype=torch.uint8, device=e.device)
    t_sync = timed_ms(lambda: sync_strided(e, win, sl, lts), reps)
    flat = win.reshape(-1)
    rounds = []
    for r in range(9):
        idx, starts = round_offsets(res, wl, fs, r)
        if len(idx) == 0:
            break
        offs = (idx * wl + starts).astype(np.uint64)
        meta_flags = (res["burst_interleaved"][idx] if r == 0 else np.zeros(len(idx))).astype(np.uint32)
        rounds.append({"round": r, "windows": int(len(idx)),
                       "ms": round(timed_ms(lambda: e.rx(flat, offsets=offs, cfo_hz=np.zeros(len(idx), np.float32), meta_flags=meta_flags), reps), 3)})

    def separate():   # the baseline: detector, results to the host, offsets, rx_batch on the accepted windows
        sync_strided(e, win, sl, lts)
        r = e._status_array(lts, e.LTS_RESULT)
        ok = (r["detected"] != 0) & (r["correlation"] >= np.float32(0.78)) & (r["start_sample"] + fs <= wl)
        w = np.nonzero(ok)[0]
        e.rx(flat, offsets=(w * wl + r["start_sample"][w]).astype(np.uint64), cfo_hz=np.zeros(len(w), np.float32),
             meta_flags=r["burst_interleaved"][w].astype(np.uint32))
    t_sep = timed_ms(separate, reps)

    def separate_with_recovery():   # the same plus the timing recovery driven from the host: one rx_batch per round
        sync_strided(e, win, sl, lts)
        r = e._status_array(lts, e.LTS_RESULT)
        ok = (r["detected"] != 0) & (r["correlation"] >= np.float32(0.78)) & (r["start_sample"] + fs <= wl)
        w = np.nonzero(ok)[0]
        cand = np.zeros(len(w), np.int64)
        flags = r["burst_interleaved"][w].astype(np.uint32)
        for rnd in range(9):
            if len(w) == 0:
                break
            s0 = r["start_sample"][w] + np.array(DELTAS)[cand]
            _, st_r = e.rx(flat, offsets=(w * wl + s0).astype(np.uint64), cfo_hz=np.zeros(len(w), np.float32), meta_flags=flags)
            failed = ~e.decode_status(st_r)["cw_ok"].any(axis=1)
            nxt = []
            for j in np.nonzero(failed)[0]:
                k = cand[j] + 1
                while k < 9 and not (0 <= r["start_sample"][w[j]] + DELTAS[k] and r["start_sample"][w[j]] + DELTAS[k] + fs <= wl):
                    k += 1
                if k < 9:
                    nxt.append((w[j], k))
            w = np.array([a for a, _ in nxt], np.int64)
            cand = np.array([b for _, b in nxt], np.int64)
            flags = np.zeros(len(w), np.uint32)
    t_sep_rec = timed_ms(separate_with_recovery, reps)
    acc = res["accepted"] != 0
    s = e.decode_status(st)
    good = (s["cw_ok"].all(axis=1) & (s["frame_valid"] != 0) & (info == sent).all(dim=1).cpu().numpy())
    return {"point": name, "channel": pt.channel, "snr_db": pt.snr_db, "windows": n, "window_len": wl, "search_len": sl,
            "detected": int((res["detected"] != 0).sum()), "accepted": int(acc.sum()),
            "entered_recovery": int((acc & (res["candidates"] > 1)).sum()),
            "recovery_share_of_accepted": round(float((acc & (res["candidates"] > 1)).sum()) / max(1, int(acc.sum())), 4),
            "recovered": int((res["delta"] != 0).sum()), "frames_ok": int(good.sum()),
            "decodes_per_window": round(float(res["candidates"].sum()) / n, 4),
            "acquire_ms": round(t_full, 3), "windows_per_s": round(n / t_full * 1e3),
            "acquire_no_retry_ms": round(t_primary_call, 3),
            "separate_calls_ms": round(t_sep, 3), "separate_windows_per_s": round(n / t_sep * 1e3),
            "separate_calls_with_host_recovery_ms": round(t_sep_rec, 3),
            "stages_ms": {"sync": round(t_sync, 3), "rounds": rounds,
                          "other_ms": round(t_full - t_sync - sum(x["ms"] for x in rounds), 3)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    e = RxEngine("QAM16", "R1_2")
    out = {"tool": "bench_acquire", "mode": "QAM16 R1/2", "reps": a.reps,
           "points": [point(e, "awgn20", SweepPoint(0, 20.0), a.windows, a.reps),
                      point(e, "moderate12", SweepPoint(2, 12.0), a.windows, a.reps)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
