"""Time of one connected-mode window call on one GPU: RxEngine.rx_window (ria_gpu_rx_window_batch) against
ria_amd.acquire.rx_acquire_control_first on the same windows in the same session.  Workload: the mixed traffic of
tools/bench_control.py - half ACK / NACK windows, half QAM16 R1/2 data windows - through Watterson moderate at 20 dB, all built
and channelled on the device (ria_amd.acquire.make_mixed_windows).

rx_window does strictly more per data window (the peek span's demodulation and CW0 decodes, decodeFrame's probes, and for a
failing window small-frame recovery and decodeFrame at every timing candidate), so no ratio is expected; the tool reports the
ratio, the tally of the ladder (window_tally) and the share of data windows whose delivered payload differs between the two
calls - pass 2 is demodulated at the peek's CFO estimate, not at the known CFO.

Prints one JSON line and writes it to --out (default profiles/bench_window.json); not the contract bench (bench.py is)."""
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
    ap.add_argument("--snr", type=float, default=20.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_window.json"))
    a = ap.parse_args()
    from ria_amd.acquire import WINDOW_COUNTERS, lts_min_confidence, make_mixed_windows, rx_acquire_control_first, window_tally
    from ria_amd.engine import RxEngine
    from ria_amd.srchash import csrc_sha256
    from ria_amd.sweep import SweepPoint
    ce, de = RxEngine("DQPSK", "R1_4"), RxEngine("QAM16", "R1_2")
    n, search = a.windows, 12000
    conf = float(lts_min_confidence(de.modulation))
    w, sent_c, sent_d, span = make_mixed_windows(ce, de, 2, SweepPoint(2, a.snr), n, search)
    dt1, (cframes, cres, cacq, info, st, dacq) = timed(lambda: rx_acquire_control_first(ce, de, w, search, span, min_confidence=conf), a.reps)
    dt2, (frames, res, acq, _, _) = timed(lambda: de.rx_window(ce, w, search, min_confidence=conf), a.reps)
    s1 = de.decode_status(st)
    ok1 = s1["cw_ok"].all(axis=1) & (s1["frame_valid"] != 0)
    info, frames = info.cpu().numpy(), frames.cpu().numpy()
    sent_c, sent_d = sent_c.cpu().numpy(), sent_d.cpu().numpy()
    ok2 = res["frame"]["success"] != 0
    nb = res["frame"]["frame_bytes"]
    # the reassembled frame is the head of the four codewords' bytes
    good1 = ok1[1::2] & (info[1::2] == sent_d).all(axis=1)
    good2 = np.array([ok2[i] and nb[i] > 0 and np.array_equal(frames[i][:nb[i]], sent_d[i // 2][:nb[i]]) for i in range(1, n, 2)])
    ctl1 = (cres["success"][0::2] != 0) & (cframes.cpu().numpy()[0::2] == sent_c).all(axis=1)
    ctl2 = ok2[0::2] & (frames[0::2, :20] == sent_c).all(axis=1)
    out = {"tool": "bench_window", "windows": n, "reps": a.reps, "channel": "watterson_moderate", "snr_db": a.snr, "span_samples": span,
           "search_len": search, "min_confidence": conf, "source_hash": csrc_sha256(),
           "control_first": {"ms": dt1 * 1e3, "windows_per_s": n / dt1, "data_frames": int(good1.sum()), "control_frames": int(ctl1.sum()),
                             "candidates": int(dacq["candidates"].sum())},
           "rx_window": {"ms": dt2 * 1e3, "windows_per_s": n / dt2, "data_frames": int(good2.sum()), "control_frames": int(ctl2.sum()),
                         "candidates": int(acq["candidates"][1::2].sum()),
                         "tally": {k: int(v) for k, v in zip(WINDOW_COUNTERS, window_tally(res, acq))}},
           "time_ratio_window_over_control_first": dt2 / dt1,
           "data_windows_delivered_by_one_call_only": int((good1 != good2).sum()),
           "share_of_data_windows_whose_delivery_differs": float((good1 != good2).mean())}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
