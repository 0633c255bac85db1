"""Time of RxEngine.mcdpsk_ring (ria_gpu_mcdpsk_ring_batch) on one GPU, in one session, alternating with what it is compared
to, medians of --reps runs after a warm-up pair:

  link   mcdpsk_ring on --streams captures of --seconds (default 256 of 60 s, three laps: tools/bench_ring.py's ring walk)
         per MC-DPSK mode, feed_step 4800, with a chase pool (one cache per stream) and channel interleaving, against the
         composition ria_amd.acquire.mcdpsk_link_ring - before this call the only way to do this job: call ms, composition ms,
         composition / call, rounds, and whether both gave the same events, state and chase records.
  plain  mcdpsk_ring with no pool and no flag against RxEngine.rx_ring (ria_gpu_rx_ring_batch) on the same captures, where
         the two calls give the same records: what the up-front check, the contiguous state copy and the new gather cost.

Nothing here is a speed claim or a threshold.  Prints one JSON line and writes it to --out (default
profiles/bench_mcdpsk_ring.json); not the contract bench (bench.py is)."""
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


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def main():
    from bench_search import build_captures
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_mcdpsk_ring.json"))
    a = ap.parse_args()
    from ria_amd.acquire import mcdpsk_link_ring
    from ria_amd.engine import RxEngine
    from ria_amd.srchash import csrc_sha256
    eng = RxEngine("DQPSK", "R1_4")
    out = {"tool": "bench_mcdpsk_ring", "streams": a.streams, "seconds": a.seconds, "frames_per_capture": a.frames, "reps": a.reps, "feed_step": 4800,
           "source_hash": csrc_sha256(), "link": [], "plain": []}
    n = a.streams
    for mode in ("MCDPSK_ZC", "MCDPSK_CHIRP"):
        kw = dict(carriers=10, modulation="DQPSK" if mode == "MCDPSK_ZC" else "DBPSK", spreading=1, max_events=16)
        bits = 10 * (2 if mode == "MCDPSK_ZC" else 1)
        x, fl, starts = build_captures(eng, mode, n, a.seconds, a.frames, 11)
        length = x.shape[1]
        t0 = np.arange(n, dtype=np.uint64) * np.uint64(1000)
        call_ms, comp_ms = [], []
        for rep in range(a.reps + 1):                 # alternating; the first pair warms both up.  A fresh pool per run: the same work every time
            pool = eng.chase_pool(n)
            t_call, got = timed(lambda: eng.mcdpsk_ring(x, length, mode, feed_step=4800, chase=pool, t0_ms=t0, channel_interleave=True,
                                                        interleaver_bits=bits, **kw))
            pool.close()
            pool = eng.chase_pool(n)
            t_comp, want = timed(lambda: mcdpsk_link_ring(eng, x, length, mode, feed_step=4800, chase=pool, t0_ms=t0, channel_interleave=True,
                                                          interleaver_bits=bits, **kw))
            pool.close()
            if rep:
                call_ms.append(t_call)
                comp_ms.append(t_comp)
        st, res, ev, frames, hq = got
        c, m = float(np.median(call_ms)), float(np.median(comp_ms))
        live = ev["window_len"] > 0
        out["link"].append({"mode": mode, "streams": n, "capture_samples": int(length), "frames_sent": int(starts.size), "interleaver_bits": bits,
                            "call_ms": call_ms, "composition_ms": comp_ms, "call_median_ms": c, "composition_median_ms": m,
                            "time_ratio_composition_over_call": m / c, "rounds": int(res["search_legs"].max()), "events": int(res["n_events"].sum()),
                            "delivered": int((ev["delivered"][live] != 0).sum()), "events_behind_the_wrap": int((ev["sync_position"][live] >= RING).sum()),
                            "codewords_stored": int(sum(bin(int(v)).count("1") for v in hq["stored_mask"][live])),
                            "identical_state": bool(st.tobytes() == want[0].tobytes()), "identical_events": bool(ev.tobytes() == want[2].tobytes()),
                            "identical_frames": bool(np.array_equal(frames.cpu().numpy(), want[3])),
                            "identical_chase_masks": bool(all(np.array_equal(hq[f], want[4][f]) for f in ("stored_mask", "sum_mask", "recovered_mask")))})
        new_ms, old_ms = [], []
        for rep in range(a.reps + 1):
            t_old, o = timed(lambda: eng.rx_ring(x, length, mode, feed_step=4800, **kw))
            t_new, r = timed(lambda: eng.mcdpsk_ring(x, length, mode, feed_step=4800, **kw))
            if rep:
                old_ms.append(t_old)
                new_ms.append(t_new)
        om, nm = float(np.median(old_ms)), float(np.median(new_ms))
        out["plain"].append({"mode": mode, "streams": n, "capture_samples": int(length), "rx_ring_ms": old_ms, "mcdpsk_ring_ms": new_ms,
                             "rx_ring_median_ms": om, "mcdpsk_ring_median_ms": nm, "time_ratio_mcdpsk_ring_over_rx_ring": nm / om,
                             "events": int(r[1]["n_events"].sum()), "identical_event_records": bool(o[2].tobytes() == r[2].tobytes()),
                             "identical_results": bool(o[1].tobytes() == r[1].tobytes())})
        del x
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
