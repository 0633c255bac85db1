"""Throughput of the control hypothesis on one GPU (RxEngine.control_acquire = ria_gpu_control_acquire_batch, and the chain
ria_amd.acquire.rx_acquire_control_first).  Workloads, all windows built and channelled on the device
(ria_amd.acquire.make_control_windows / make_windows):
  control_awgn / control_moderate   ACK / NACK windows at AWGN 20 dB and Watterson moderate 10 dB through control_acquire
  host_chain                        the control_awgn windows through the separate calls driven from the host: sync_lts, the
                                    accepted spans gathered, demod_var, ldpc_decode_robust of the first 648 soft bits, with
                                    the time of each stage
  mixed                             half ACK windows, half QAM16 R1/2 data windows (AWGN 20 dB) through
                                    rx_acquire_control_first, against the same batch through rx_acquire alone, with the
                                    frames each delivers

Prints one JSON line and writes it to --out (default profiles/bench_control.json); not the contract bench (bench.py is)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_control.json"))
    a = ap.parse_args()
    from ria_amd.acquire import (CONTROL_COUNTERS, DETECT_THRESHOLD, control_tally, lts_min_confidence, make_control_windows,
                                 make_windows, rx_acquire_control_first)
    from ria_amd.engine import RxEngine
    from ria_amd.srchash import csrc_sha256
    from ria_amd.sweep import SweepPoint
    ce, de = RxEngine("DQPSK", "R1_4"), RxEngine("QAM16", "R1_2")
    n, search = a.windows, 12000
    span = ce.control_frame_samples(de)
    conf = float(lts_min_confidence(de.modulation))
    out = {"tool": "bench_control", "windows": n, "reps": a.reps, "span_samples": span, "search_len": search, "min_confidence": conf,
           "source_hash": csrc_sha256()}
    for name, pt in (("control_awgn", SweepPoint(0, 20.0)), ("control_moderate", SweepPoint(2, 10.0))):
        w, sent, _ = make_control_windows(ce, 1, pt, 0, 0, n, span, search)
        dt, (frames, res, acq, _) = timed(lambda: ce.control_acquire(w, search, span, min_confidence=conf), a.reps)
        row = {"windows_per_s": n / dt, "ms": dt * 1e3}
        row.update({k: int(v) for k, v in zip(CONTROL_COUNTERS, control_tally(frames, res, acq, sent))})
        out[name] = row
        if name == "control_awgn":
            dt_sync, lts = timed(lambda: ce.sync_lts(w[:, :search].contiguous(), threshold=DETECT_THRESHOLD), a.reps)
            ok = np.nonzero((lts["detected"] != 0) & ~(lts["correlation"] < np.float32(conf)) & (lts["start_sample"] + span <= w.shape[1]))[0]
            t0 = time.perf_counter()
            idx = torch.from_numpy(ok).to(ce.device)
            cols = torch.from_numpy(lts["start_sample"][ok].astype(np.int64)).to(ce.device)[:, None] + torch.arange(span, device=ce.device)[None, :]
            spans = torch.gather(w[idx], 1, cols).contiguous()
            torch.cuda.synchronize()
            dt_gather = time.perf_counter() - t0
            dt_demod, (llr, _) = timed(lambda: ce.demod_var(spans), a.reps)
            rows = llr[:, :648].contiguous()
            dt_dec, (_, okd, _, _) = timed(lambda: ce.ldpc_decode_robust(rows), a.reps)
            total = dt_sync + dt_gather + dt_demod + dt_dec
            out["host_chain"] = {"detect_ms": dt_sync * 1e3, "gather_ms": dt_gather * 1e3, "demod_ms": dt_demod * 1e3, "decode_ms": dt_dec * 1e3,
                                 "sum_ms": total * 1e3, "windows_per_s": n / total, "windows_decoded": int(okd.sum().item())}
            del spans, llr, rows
        del w
    # mixed traffic: even windows carry a control frame, odd windows a data frame; one window length for both
    h = n // 2
    fs = de.geo.frame_samples
    pt = SweepPoint(0, 20.0)
    wd, sent_d, _ = make_windows(de, 2, pt, 0, 0, h, search)
    wc, sent_c, _ = make_control_windows(ce, 3, pt, 0, 0, h, span, search, window_len=search + fs)
    w = torch.stack([wc, wd], dim=1).reshape(2 * h, search + fs).contiguous()
    del wd, wc
    dt1, (info1, st1, acq1) = timed(lambda: de.rx_acquire(w, search), a.reps)
    s1 = de.decode_status(st1)
    ok1 = s1["cw_ok"].all(axis=1) & (s1["frame_valid"] != 0)
    dt2, (frames, res, acq, info2, st2, acq2) = timed(lambda: rx_acquire_control_first(ce, de, w, search, span), a.reps)
    s2 = de.decode_status(st2)
    ok2 = s2["cw_ok"].all(axis=1) & (s2["frame_valid"] != 0)
    same_c = (frames[0::2] == sent_c).all(dim=1).cpu().numpy() & (res["success"][0::2] != 0)
    out["mixed"] = {"windows": 2 * h,
                    "rx_acquire_alone": {"ms": dt1 * 1e3, "windows_per_s": 2 * h / dt1, "data_frames": int(((info1[1::2] == sent_d).all(dim=1).cpu().numpy() & ok1[1::2]).sum()),
                                         "control_frames": 0, "candidates": int(acq1["candidates"].sum())},
                    "control_first": {"ms": dt2 * 1e3, "windows_per_s": 2 * h / dt2, "data_frames": int(((info2[1::2] == sent_d).all(dim=1).cpu().numpy() & ok2[1::2]).sum()),
                                      "control_frames": int(same_c.sum()), "candidates": int(acq2["candidates"].sum()),
                                      "control_tried": int(res["tried"].sum())}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
