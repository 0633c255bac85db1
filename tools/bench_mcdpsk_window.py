"""Throughput of ria_gpu_mcdpsk_window_batch (RxEngine.mcdpsk_window) on one GPU against the hand-composed sequence of the
older calls on the same windows; prints one JSON line and writes it to profiles/bench_mcdpsk_window.json.

The windows are ria_amd.acquire.make_handshake_windows mixes (PING, CONNECT of 3 codewords, 1-codeword ACK, 3-codeword data
frame, noise; dual chirp, DBPSK, 10 carriers), received disconnected.
  window_call  one mcdpsk_window call
  composed     what a host does without it: mcdpsk_acquire at frame_cw 1 with retry off, the headers back on the host, the
               peek rules there (CONNECT guard, the 3-codeword handshake minimum), then mcdpsk_acquire at the codeword count
               every window asks for, one call per distinct count over the gathered windows.  The PING energy test has no
               older call; the composed sequence does without it (its PING windows go through the fallbacks and fail), so it
               is timed a second time without the PING windows' second call (composed_skip_pings), as if the host knew them.
--call-only: one pass of the window call alone, for a kernel trace."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps, out


def composed(e, w, sl, skip=None):
    """-> (success count, second-call windows)"""
    frames, res = e.mcdpsk_acquire(w, sl, 1, retry=False)
    hdr = res["header_total_cw"].astype(np.int64)
    ftype = res["frame_type"]
    # the peek on the host: decodeMCDPSKFrame's guard has rejected a CONNECT that announces < 3 (header 0): the fallback's 3
    need = np.where(hdr > 1, hdr, 3)
    need = np.where(np.isin(ftype, (0x12, 0x13, 0x14)) & (need < 3), 3, need)
    need = np.maximum(need, 3)                      # disconnected: the handshake window
    go = res["accepted"] != 0
    if skip is not None:
        go &= ~skip
    ok, second = 0, 0
    for cw in np.unique(need[go]):
        if cw > 8:
            continue
        idx = np.nonzero(go & (need == cw))[0]
        sub = w[torch.from_numpy(idx).to(e.device)].contiguous()
        _, r2 = e.mcdpsk_acquire(sub, sl, int(cw))
        ok += int(r2["success"].sum())
        second += len(idx)
    return ok, second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--snr", type=float, default=10.0)
    ap.add_argument("--call-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_mcdpsk_window.json"))
    a = ap.parse_args()
    from ria_amd import capi
    from ria_amd.acquire import HANDSHAKE_KINDS, MCDPSK_WINDOW_COUNTERS, make_handshake_windows, mcdpsk_window_tally
    from ria_amd.engine import RxEngine
    from ria_amd.srchash import csrc_sha256
    e = RxEngine("DQPSK", "R1_4", max_batch=64)
    n = a.windows
    seeds = np.arange(1, n + 1, dtype=np.uint32) * np.uint32(2654435761)
    out = {"metric": "mcdpsk_window_windows_per_s", "windows": n, "snr_db": a.snr, "mix": list(HANDSHAKE_KINDS), "source_hash": csrc_sha256()}
    for name, kind in (("awgn", 0), ("moderate", 2)):
        w, sl, kinds = make_handshake_windows(e, n, kind, a.snr, seeds)
        if a.call_only:
            e.mcdpsk_window(w, sl)
            torch.cuda.synchronize()
            continue
        dt, (frames, res, acq, hq) = timed(lambda: e.mcdpsk_window(w, sl), a.reps)
        tally = dict(zip(MCDPSK_WINDOW_COUNTERS, (int(v) for v in mcdpsk_window_tally(res, acq))))
        row = {"window_call": {"windows_per_s": n / dt, "ms": dt * 1e3, "tally": {k: v for k, v in tally.items() if v}}}
        dt2, (ok2, second) = timed(lambda: composed(e, w, sl), a.reps)
        row["composed"] = {"windows_per_s": n / dt2, "ms": dt2 * 1e3, "success": ok2, "second_call_windows": second}
        pings = res["outcome"] == capi.MWIN_OUTCOME["PING"]
        dt3, (ok3, second3) = timed(lambda: composed(e, w, sl, skip=pings), a.reps)
        row["composed_skip_pings"] = {"windows_per_s": n / dt3, "ms": dt3 * 1e3, "success": ok3, "second_call_windows": second3}
        row["window_call_over_composed"] = dt2 / dt
        row["window_call_over_composed_skip_pings"] = dt3 / dt
        out[name] = row
        del w
    print(json.dumps(out))
    if not a.call_only:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
