#!/usr/bin/env python3
"""Throughput of ria_gpu_rx_burst_batch (detection, acceptance, energy gate, CFO chain, burst de-interleave / continuation
and decode in one call) on QAM16 R1/2 burst windows built by ria_amd.acquire.make_burst_windows, for two workloads:
marked, burst-interleaved groups of 4, and unmarked 3-frame bursts (continuation).  Next to each: the same work done by
the separate calls driven from Python, one round per physical frame over the whole batch - sync_lts, then per frame the
fit test and the gate (torch on the device), demod or rx at per-window offsets, a read-back of cfo_hz (and of the decode
status for a continuation), the clamp in numpy - then burst_deinterleave + decode for the groups.  That composition needs
nothing of the one-call entry, so it is the baseline of the commit before it.  Its gate is a torch reduction, not the
reference's serial float32 chain: it is there for its cost, and its rms is not compared bit for bit.
Prints one JSON line and writes it to --out (default profiles/bench_burst.json); not the contract bench (bench.py is).
--call-only runs the entry alone, for a kernel trace in a run of its own; --merge-kernel-stats adds that trace to the file.

Stage times come from device events around calls that reproduce each stage on its own (tools/bench_acquire.py's way): the
detector alone, frame 0 (demod of the group list / rx_acquire of the others), each later round's demod or demod + decode
at exactly that round's windows, and the groups' de-interleave + decode.  'other_ms' is what the whole call takes beyond
their sum: burst_plan / burst_step (the gate) / burst_list / burst_gather / burst_scatter and the per-round host reads."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ria_amd import capi  # noqa: E402
from ria_amd.acquire import BURST_COUNTERS, DETECT_THRESHOLD, SEARCH_LEN, burst_tally, lts_min_confidence, make_burst_windows  # noqa: E402
from ria_amd.engine import RxEngine  # noqa: E402
from ria_amd.sweep import SweepPoint  # noqa: E402

GATE_SKIP, GATE_LEN, GATE_MIN = 1024, 5000, np.float32(0.04)
NON_DATA = (0x10, 0x11, 0x12, 0x13, 0x14, 0x15, 0x16, 0x17, 0x20, 0x21, 0x40)   # control / connect types (frame_v2.hpp:222-228, :348-351)


def _once_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def timed_ms(fn, reps):
    """median of reps device-event timings of fn(), after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    return float(np.median([_once_ms(fn) for _ in range(reps)]))


def timed_pair_ms(fa, fb, reps):
    """fa and fb timed alternately (the machine's load drifts), one warm-up call each -> two (median, min, max)"""
    fa()
    fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(_once_ms(fa))
        tb.append(_once_ms(fb))
    return tuple((float(np.median(t)), float(min(t)), float(max(t))) for t in (ta, tb))


def sync_strided(e, win, search_len, out):
    n, wl = win.shape
    e._check(e.lib.ria_gpu_sync_lts_batch(e.h, C.c_void_p(win.data_ptr()), wl, search_len, n, None, float(DETECT_THRESHOLD),
                                          C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def cfo_next(c, e):
    """the chain step: the reported CFO, at most 2 Hz away from the one used (a NaN drift leaves the report)"""
    d = e - c
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(d) > np.float32(2.0), c + np.copysign(np.float32(2.0), d), e).astype(np.float32)


def gate_pass(win, w, s):
    """fit-tested windows w at block starts s: the energy gate as a torch reduction on the device -> bool per window"""
    first = torch.from_numpy(w * win.shape[1] + s + GATE_SKIP).to(win.device)
    blk = win.reshape(-1)[first[:, None] + torch.arange(GATE_LEN, device=win.device)[None, :]]
    rms = (blk * blk).mean(dim=1).sqrt().cpu().numpy()
    return ~(rms < GATE_MIN)


def accept(e, r, conf, wl, fs):
    return (r["detected"] != 0) & ~(r["correlation"] < conf) & (r["start_sample"] >= 0) & (r["start_sample"] + fs <= wl)


def compose_groups(e, win, sl, N, lts, conf, log=None):
    """groups by the separate calls; log (a list) receives (frame, windows, offsets, cfo) per round for the stage timing"""
    n, wl = win.shape
    fs = e.geo.frame_samples
    flat = win.reshape(-1)
    sync_strided(e, win, sl, lts)
    r = e._status_array(lts, e.LTS_RESULT)
    w = np.nonzero(accept(e, r, conf, wl, fs) & (r["burst_interleaved"] != 0))[0]
    start = r["start_sample"].astype(np.int64)
    cfo = np.zeros(len(w), np.float32)
    rows = []
    for f in range(N):
        if f:
            s = start[w] + f * fs
            keep = s + fs <= wl
            w, cfo, s, rows = w[keep], cfo[keep], s[keep], [x[torch.from_numpy(keep).to(win.device)] for x in rows]
            keep = gate_pass(win, w, s) if len(w) else np.zeros(0, bool)
            w, cfo, rows = w[keep], cfo[keep], [x[torch.from_numpy(keep).to(win.device)] for x in rows]
        if len(w) == 0:
            return None
        offs = (w * wl + start[w] + f * fs).astype(np.uint64)
        if log is not None:
            log.append((f, len(w), offs, cfo.copy(), start[w].astype(np.uint64)))
        llr, st = e.demod(flat, cfo_hz=cfo, abs_pos=start[w].astype(np.uint64), flags=np.full(len(w), 1 if f == 0 else 0, np.uint32), offsets=offs)
        fst = e.frame_status(st)
        keep = fst["n_llr"] != 0
        cfo = cfo_next(cfo, fst["cfo_hz"])
        rows.append(llr)
        if not keep.all():
            w, cfo, rows = w[keep], cfo[keep], [x[torch.from_numpy(keep).to(win.device)] for x in rows]
    phys = torch.stack(rows, dim=1).reshape(len(w) * N, -1).contiguous()
    info, st = e.decode(e.burst_deinterleave(phys, N))
    return w, info, st, phys


def compose_continuation(e, win, sl, conf, log=None):
    """continuation by the separate calls: rx_acquire for frame 0, then one rx per block over the windows still going"""
    n, wl = win.shape
    fs = e.geo.frame_samples
    flat = win.reshape(-1)
    info, st, res, fst = e.rx_acquire(win, sl, detect_threshold=DETECT_THRESHOLD, min_confidence=conf, want_demod_status=True)
    s0 = e.decode_status(st)
    f0 = e.frame_status(fst)
    typ = info[:, 2].cpu().numpy()
    go = (res["accepted"] != 0) & s0["cw_ok"].all(axis=1) & (s0["frame_valid"] != 0) & ~np.isin(typ, NON_DATA) & (res["delta"] == 0)
    w = np.nonzero(go)[0]
    start = res["sync_start"].astype(np.int64)
    cfo = cfo_next(np.zeros(len(w), np.float32), f0["cfo_hz"][w])
    blocks = int((res["accepted"] != 0).sum())
    for k in range(1, capi.BURST_MAX_FRAMES):
        s = start[w] + k * fs
        keep = s + fs <= wl
        w, cfo, s = w[keep], cfo[keep], s[keep]
        if len(w):
            keep = gate_pass(win, w, s)
            w, cfo, s = w[keep], cfo[keep], s[keep]
        if len(w) == 0:
            break
        offs = (w * wl + s).astype(np.uint64)
        if log is not None:
            log.append((k, len(w), offs, cfo.copy(), start[w].astype(np.uint64)))
        _, st_k, _, fst_k = e.rx(flat, offsets=offs, cfo_hz=cfo, abs_pos=start[w].astype(np.uint64), want_llr=True)
        fk = e.frame_status(fst_k)
        sk = e.decode_status(st_k)
        cfo = cfo_next(cfo, fk["cfo_hz"])
        keep = (fk["n_llr"] != 0) & sk["cw_ok"].any(axis=1)
        blocks += int((fk["n_llr"] != 0).sum())
        w, cfo = w[keep], cfo[keep]
    return blocks


def workload(e, name, pt, n, reps, n_frames, interleaved, call_only=False):
    win, sent, _ = make_burst_windows(e, 20261018, pt, 0, 0, n, n_frames, interleaved=interleaved)
    wl, sl, fs = win.shape[1], SEARCH_LEN, e.geo.frame_samples
    conf = lts_min_confidence(e.modulation)
    kw = dict(group_size=max(2, n_frames), detect_threshold=DETECT_THRESHOLD, interleave=interleaved)
    out = e.rx_burst(win, sl, **kw)
    counters = dict(zip(BURST_COUNTERS, (int(v) for v in burst_tally(out, sent))))
    one_call = lambda: e.rx_burst(win, sl, sync=False, **kw)
    if call_only:     # for a kernel trace of the entry alone (rocprofv3 --kernel-trace --stats, a run of its own)
        return {"workload": name, "windows": n, "counters": counters, "one_call_ms_traced": round(timed_ms(one_call, reps), 3)}
    lts = torch.zeros((n, 32), dtype=torch.uint8, device=e.device)
    flat = win.reshape(-1)
    log = []
    if interleaved:
        got = compose_groups(e, win, sl, n_frames, lts, conf, log)
        (t_call, *r_call), (t_comp, *r_comp) = timed_pair_ms(one_call, lambda: compose_groups(e, win, sl, n_frames, lts, conf), reps)
        done = np.nonzero((out["result"]["mode"] == 2) & (out["result"]["frames_decoded"] == n_frames))[0]
        same = got is not None and np.array_equal(got[0], done) and \
            np.array_equal(got[1].cpu().numpy().reshape(len(done), n_frames, -1), out["info"][done, :n_frames])
        logical = int(out["result"]["frames_decoded"].sum())
    else:
        blocks = compose_continuation(e, win, sl, conf, log)
        (t_call, *r_call), (t_comp, *r_comp) = timed_pair_ms(one_call, lambda: compose_continuation(e, win, sl, conf), reps)
        logical = int(out["result"]["frames_decoded"].sum())
        same = blocks == logical
    # stages of the one call, each reproduced on its own
    t_sync = timed_ms(lambda: sync_strided(e, win, sl, lts), reps)
    rounds = []
    if not interleaved:
        rounds.append({"frame": 0, "windows": n, "what": "rx_acquire", "ms": round(timed_ms(
            lambda: e.rx_acquire(win, sl, detect_threshold=DETECT_THRESHOLD, min_confidence=conf), reps) - t_sync, 3)})
    for f, cnt, offs, cfo, pos in log:
        if interleaved:
            fl = np.full(cnt, 1 if f == 0 else 0, np.uint32)
            ms = timed_ms(lambda: e.demod(flat, cfo_hz=cfo, abs_pos=pos, flags=fl, offsets=offs), reps)
            what = "demod"
        else:
            ms = timed_ms(lambda: e.rx(flat, offsets=offs, cfo_hz=cfo, abs_pos=pos), reps)
            what = "demod + decode"
        rounds.append({"frame": f, "windows": cnt, "what": what, "ms": round(ms, 3)})
    t_dec = 0.0
    if interleaved and got is not None:
        t_dec = timed_ms(lambda: e.decode(e.burst_deinterleave(got[3], n_frames)), reps)
    stage_sum = t_sync + sum(x["ms"] for x in rounds) + t_dec
    return {"workload": name, "channel": pt.channel, "snr_db": pt.snr_db, "windows": n, "frames_per_burst": n_frames,
            "interleaved": bool(interleaved), "window_len": wl, "search_len": sl, "counters": counters,
            "one_call_ms": round(t_call, 3), "one_call_ms_min_max": [round(v, 3) for v in r_call], "one_call_windows_per_s": round(n / t_call * 1e3),
            "one_call_logical_frames_per_s": round(logical / t_call * 1e3),
            "composition_ms": round(t_comp, 3), "composition_ms_min_max": [round(v, 3) for v in r_comp], "composition_windows_per_s": round(n / t_comp * 1e3),
            "composition_logical_frames_per_s": round(logical / t_comp * 1e3),
            "composition_agrees": bool(same),
            "stages_ms": {"sync": round(t_sync, 3), "rounds": rounds, "deinterleave_decode": round(t_dec, 3),
                          "other_ms": round(t_call - stage_sum, 3)}}


def merge_kernel_stats(csv_path, json_path):
    """adds the library's kernels of a rocprofv3 --kernel-trace --stats CSV (a --call-only run) to the bench's JSON file"""
    import csv
    with open(json_path) as f:
        out = json.loads(f.readline())
    with open(csv_path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "ria::" in r["Name"]]
    out["kernel_trace"] = {
        "source": "rocprofv3 --kernel-trace --stats of a --call-only run (window building included, composition and stages not)",
        "kernels": [{"name": r["Name"].split("(")[0].replace("void ", ""), "calls": int(r["Calls"]), "total_ms": round(int(r["TotalDurationNs"]) / 1e6, 3),
                     "average_us": round(float(r["AverageNs"]) / 1e3, 2)} for r in rows]}
    with open(json_path, "w") as f:
        f.write(json.dumps(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--channel", type=int, default=2, help="0 AWGN, 2 Watterson moderate")
    ap.add_argument("--snr", type=float, default=20.0)
    ap.add_argument("--call-only", action="store_true", help="only the one call per workload: the run to put under a kernel trace")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_burst.json"))
    ap.add_argument("--merge-kernel-stats", metavar="CSV", help="no run: add the kernels of a rocprofv3 stats CSV to --out")
    a = ap.parse_args()
    if a.merge_kernel_stats:
        return merge_kernel_stats(a.merge_kernel_stats, a.out)
    e = RxEngine("QAM16", "R1_2")
    pt = SweepPoint(a.channel, a.snr)
    out = {"tool": "bench_burst", "mode": "QAM16 R1/2", "reps": a.reps,
           "workloads": [workload(e, "groups_of_4", pt, a.windows, a.reps, 4, True, a.call_only),
                         workload(e, "unmarked_3_frame_bursts", pt, a.windows, a.reps, 3, False, a.call_only)]}
    line = json.dumps(out)
    print(line)
    if a.out and not a.call_only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
