"""Time of RxEngine.rx_ring (ria_gpu_rx_ring_batch) and RxEngine.search_ring (ria_gpu_search_ring_batch) on one GPU, in one
session, alternating with what each is compared to, medians of --reps walks after a warm-up pair:

  ring    rx_ring on --ring-streams captures of --ring-seconds (default 256 of 60 s, three laps) per mode, feed_step 4800,
          against the composition ria_amd.acquire.rx_ring, the only other way to get these results: call ms, rounds,
          composition / call, and whether both gave the same events.
  stream  rx_ring against RxEngine.rx_stream (ria_gpu_rx_stream_batch) on tools/bench_stream.py's captures of a few seconds,
          where both calls are valid: the cost of the closed-form indexing and the larger records.
  short   search_ring against RxEngine.search (ria_gpu_search_batch) on tools/bench_search.py's captures of a few seconds, where both calls
          are valid and give the same syncs: the cost of reading the capture through the ring's closed form.  Alternating,
          medians of --reps walks after a warm-up pair.
  long    on captures longer than the ring buffer (--long-seconds, default 30 s = 1.5 laps), which only the ring call takes:
          ms per walk, search calls and detector rounds.  There is no comparator in the library for these.

A walk is tools/bench_search.py's: search; every stream that found a sync moves its cursor behind that frame (the last decoded
position set, the consumed samples counted as fed) and searches on; until every stream waits for samples.  feed_step 4800.

Prints one JSON line and writes it to --out (default profiles/bench_ring.json); not the contract bench (bench.py is)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
RING = 960000


def ring_walk(eng, x, mode, feed_step, frame_len, cfg, as_search=False):
    """as_search: move the cursor exactly as bench_search.library_walk does (captures that never wrap), so that both walks
    are the same walk; else behind the frame modulo the ring, with the consumed samples counted as fed"""
    n, length = x.shape
    st = eng.ring_state(n, total_fed=0 if feed_step else length)
    open_ = np.ones(n, bool)
    found, calls, runs, rounds = [[] for _ in range(n)], 0, 0, 0
    while open_.any():
        idx = np.flatnonzero(open_)
        res, out = eng.search_ring(x if len(idx) == n else x[torch.as_tensor(idx, device=x.device)].contiguous(), length, st[idx], mode, feed_step=feed_step, **cfg)
        calls += 1
        runs += int(res["detector_runs"].sum())
        rounds += int(res["detector_runs"].max()) + 1
        ok = res["outcome"] == 1
        behind = res["abs_position"][ok] + frame_len
        if as_search:
            out["correlation_pos"][ok] = np.minimum(behind, RING - 1)
        else:
            out["correlation_pos"][ok] = behind % RING
            out["total_fed"][ok] = np.maximum(out["total_fed"][ok], np.minimum(behind, length))
        out["last_decoded_sync_pos"][ok] = res["sync_position"][ok]
        st[idx] = out
        for j in np.flatnonzero(ok):
            found[idx[j]].append(int(res["abs_position"][j]))
        open_[idx[~ok]] = False
    return found, calls, runs, rounds


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def ring_and_stream(a, eng, ctrl, out):
    from bench_search import build_captures
    from ria_amd.acquire import rx_ring, stream_events
    out["ring"], out["stream"] = [], []
    for mode in ("OFDM_LTS", "MCDPSK_ZC", "MCDPSK_CHIRP"):
        kw = dict(carriers=10, modulation="DQPSK" if mode == "MCDPSK_ZC" else "DBPSK", spreading=1,
                  control_engine=ctrl if mode == "OFDM_LTS" else None, max_events=16)
        x, fl, starts = build_captures(eng, mode, a.ring_streams, a.ring_seconds, max(a.frames, 3), 11)
        length = x.shape[1]
        call_ms, comp_ms = [], []
        for rep in range(a.reps + 1):
            t_call, (st, res, ev, frames) = timed(lambda: eng.rx_ring(x, length, mode, feed_step=4800, **kw))
            t_comp, want = timed(lambda: rx_ring(eng, x, length, mode, feed_step=4800, **kw))
            if rep:
                call_ms.append(t_call)
                comp_ms.append(t_comp)
        got = stream_events(res, ev, frames)
        ref = [[{k: e[k] for k in ("position", "outcome", "frame")} for e in evs] for evs in want[0]]
        c, m = float(np.median(call_ms)), float(np.median(comp_ms))
        out["ring"].append({"mode": mode, "streams": a.ring_streams, "capture_samples": int(length), "frames_sent": int(starts.size),
                            "call_ms": call_ms, "composition_ms": comp_ms, "call_median_ms": c, "composition_median_ms": m,
                            "time_ratio_composition_over_call": m / c, "rounds": int(res["search_legs"].max()),
                            "events": int(res["n_events"].sum()), "delivered": int(sum(e["frame"] is not None for s_ in got for e in s_)),
                            "events_behind_the_wrap": int(sum(e["position"] >= RING for s_ in got for e in s_)),
                            "streams_with_identical_events": int(sum(p == q for p, q in zip(got, ref))),
                            "streams_with_identical_state": int(sum(st[i].tobytes() == want[1][i].tobytes() for i in range(len(st))))})
        del x
        x, fl, starts = build_captures(eng, mode, a.streams, max(a.seconds, 8.0) if mode == "MCDPSK_CHIRP" else a.seconds, a.frames, 7)
        length = x.shape[1]
        for fs in (0, 4800):
            old_ms, new_ms = [], []
            for rep in range(a.reps + 1):
                t_old, o = timed(lambda: eng.rx_stream(x, length, mode, feed_step=fs, **kw))
                t_new, r = timed(lambda: eng.rx_ring(x, length, mode, feed_step=fs, **kw))
                if rep:
                    old_ms.append(t_old)
                    new_ms.append(t_new)
            om, rm = float(np.median(old_ms)), float(np.median(new_ms))
            out["stream"].append({"mode": mode, "feed_step": fs, "streams": a.streams, "capture_samples": int(length), "rx_stream_ms": old_ms,
                                  "rx_ring_ms": new_ms, "rx_stream_median_ms": om, "rx_ring_median_ms": rm, "time_ratio_ring_over_stream": rm / om,
                                  "events": int(r[1]["n_events"].sum()), "identical_event_records": bool(o[2].tobytes() == r[2].tobytes())})
        del x


def main():
    from bench_search import build_captures, library_walk
    ap = argparse.ArgumentParser()
    ap.add_argument("--ring-streams", type=int, default=256)
    ap.add_argument("--ring-seconds", type=float, default=60.0)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--long-streams", type=int, default=64)
    ap.add_argument("--long-seconds", type=float, default=30.0)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_ring.json"))
    a = ap.parse_args()
    from ria_amd.engine import RxEngine
    from ria_amd.srchash import csrc_sha256
    eng, ctrl = RxEngine("DQPSK", "R1_4"), RxEngine("DQPSK", "R1_4")
    out = {"tool": "bench_ring", "ring_streams": a.ring_streams, "ring_seconds": a.ring_seconds, "streams": a.streams, "seconds": a.seconds, "long_streams": a.long_streams, "long_seconds": a.long_seconds,
           "frames_per_capture": a.frames, "reps": a.reps, "feed_step": 4800, "source_hash": csrc_sha256(), "short": [], "long": []}
    ring_and_stream(a, eng, ctrl, out)
    for mode in ("OFDM_LTS", "MCDPSK_ZC", "MCDPSK_CHIRP"):
        cfg = dict(carriers=10, modulation="DQPSK" if mode == "MCDPSK_ZC" else "DBPSK", spreading=1)
        x, fl, starts = build_captures(eng, mode, a.streams, max(a.seconds, 8.0) if mode == "MCDPSK_CHIRP" else a.seconds, a.frames, 7)
        old_ms, new_ms = [], []
        for rep in range(a.reps + 1):                 # alternating; the first pair warms both up
            t_old, (f_old, _, _, _) = timed(lambda: library_walk(eng, x, mode, 4800, fl, cfg))
            t_new, (f_new, calls, runs, rounds) = timed(lambda: ring_walk(eng, x, mode, 4800, fl, cfg, as_search=True))
            if rep:
                old_ms.append(t_old)
                new_ms.append(t_new)
        o, r = float(np.median(old_ms)), float(np.median(new_ms))
        out["short"].append({"mode": mode, "capture_samples": int(x.shape[1]), "search_ms": old_ms, "search_ring_ms": new_ms, "search_median_ms": o,
                             "search_ring_median_ms": r, "time_ratio_ring_over_search": r / o, "search_calls": calls, "rounds": rounds, "detector_runs": runs,
                             "syncs": sum(len(v) for v in f_new), "streams_with_identical_syncs": int(sum(p == q for p, q in zip(f_old, f_new)))})
        del x
        x, fl, starts = build_captures(eng, mode, a.long_streams, a.long_seconds, max(a.frames, 3), 11)
        ms = []
        for rep in range(a.reps + 1):
            t_new, (f_new, calls, runs, rounds) = timed(lambda: ring_walk(eng, x, mode, 4800, fl, cfg))
            if rep:
                ms.append(t_new)
        near = sum(int(any(abs(p - s) < 62000 for p in f_new[i])) for i in range(a.long_streams) for s in starts[i])
        out["long"].append({"mode": mode, "capture_samples": int(x.shape[1]), "search_ring_ms": ms, "median_ms": float(np.median(ms)),
                            "streams_per_s": a.long_streams / (float(np.median(ms)) / 1e3), "search_calls": calls, "rounds": rounds, "detector_runs": runs,
                            "frames_sent": int(starts.size), "frames_with_a_sync": near, "syncs_behind_the_wrap": sum(int(p >= RING) for v in f_new for p in v)})
        del x
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
