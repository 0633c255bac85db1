"""Time of RxEngine.rx_stream (ria_gpu_rx_stream_batch) on one GPU against the composition it replaces,
ria_amd.acquire.rx_stream, in the same session.

Workload: tools/bench_search.py's captures - N captures of a few seconds, each holding K frames, the first behind silence, the
others behind noise - in its three modes (connected OFDM light sync, connected MC-DPSK ZC, the MC-DPSK dual chirp), with
feed_step 0 and 4800.  A walk is the whole receive loop: search, the window call of the mode on every stream that found a
sync, the state update, until every stream waits for samples.  The OFDM captures hold decodable frames; the MC-DPSK ones hold
random coded bytes behind real preambles, so their windows run detection, the energy test, the peek and the decode ladder and
deliver nothing.

The comparator is what a user could do before the call existed: rx_stream drives the same library calls from Python, copies
the open streams' captures per round, gathers windows with torch indexing, downloads every record and frame and walks the rows
in a Python loop.  Both walks' events are compared.  The walks alternate; the first pair warms both up; medians of --reps.

Prints one JSON line and writes it to --out (default profiles/bench_stream.json); not the contract bench (bench.py is)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_stream.json"))
    a = ap.parse_args()
    assert a.reps >= 3, "medians of at least three"
    from bench_search import build_captures
    from ria_amd import capi
    from ria_amd.acquire import STREAM_COUNTERS, rx_stream, stream_events, stream_tally
    from ria_amd.engine import RxEngine
    from ria_amd.srchash import csrc_sha256
    eng, ctrl = RxEngine("DQPSK", "R1_4"), RxEngine("DQPSK", "R1_4")
    out = {"tool": "bench_stream", "streams": a.streams, "seconds": a.seconds, "frames_per_capture": a.frames, "reps": a.reps,
           "source_hash": csrc_sha256(), "counters": list(STREAM_COUNTERS), "points": []}
    for mode, secs in (("OFDM_LTS", a.seconds), ("MCDPSK_ZC", a.seconds), ("MCDPSK_CHIRP", max(a.seconds, 8.0))):
        x, fl, starts = build_captures(eng, mode, a.streams, secs, a.frames, 7)
        length = x.shape[1]
        kw = dict(carriers=10, modulation="DQPSK" if mode == "MCDPSK_ZC" else "DBPSK", spreading=1,
                  control_engine=ctrl if mode == "OFDM_LTS" else None, max_events=16)
        for fs in (0, 4800):
            call_ms, comp_ms = [], []
            for rep in range(a.reps + 1):
                torch.cuda.synchronize()
                t = time.perf_counter()
                st, res, ev, frames = eng.rx_stream(x, length, mode, feed_step=fs, **kw)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                want = rx_stream(eng, x, length, mode, feed_step=fs, **kw)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if rep:
                    call_ms.append((t1 - t) * 1e3)
                    comp_ms.append((t2 - t1) * 1e3)
            got = stream_events(res, ev, frames)
            rounds = int(res["search_legs"].max())
            call_med, comp_med = float(np.median(call_ms)), float(np.median(comp_ms))
            out["points"].append({
                "mode": mode, "feed_step": fs, "capture_samples": int(length), "frame_samples": int(fl), "frames_sent": int(starts.size),
                "call": {"ms_per_walk": call_ms, "median_ms": call_med, "streams_per_s": a.streams / (call_med / 1e3), "host_rounds": rounds,
                         # per round: the found list and the open count; beside the search's and the window calls' own
                         "own_device_to_host_reads_at_most": 2 * rounds, "tally": stream_tally(res, ev).tolist(),
                         "events_full": int((res["closed"] == capi.STREAM_CLOSED["EVENTS_FULL"]).sum())},
                "composition": {"ms_per_walk": comp_ms, "median_ms": comp_med, "streams_per_s": a.streams / (comp_med / 1e3),
                                "events": sum(len(e) for e in want), "delivered": sum(e["frame"] is not None for s in want for e in s)},
                "streams_with_identical_events": int(sum(p == q for p, q in zip(got, want))),
                "time_ratio_composition_over_call": comp_med / call_med})
        del x
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
