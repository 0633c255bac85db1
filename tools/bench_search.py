"""Time of RxEngine.search (ria_gpu_search_batch) on one GPU against the same walk driven from the host, in the same session.

Workload: N captures of a few seconds, each holding K frames - the first behind silence, the others behind the channel's noise
- in the three modes (connected OFDM light sync, connected MC-DPSK ZC, the MC-DPSK dual chirp), with feed_step 0 (the recording
is all there) and 4800 (it arrives in 100 ms chunks, one invocation per chunk).  A walk is: search; every stream that found
a sync moves its cursor behind that frame (last_decoded_sync_pos set) and searches on; until every stream waits for samples.

The comparator is what a user could do before the call existed: the rules of searchForSync in numpy on the host, one
invocation of every open stream per round, the RMS by torch, and one sync_lts / sync_zc / sync_chirp call per round on the
windows gathered by torch (ZC: one call per distinct threshold of the round).  Its RMS is torch's tree sum, not the reference's
chain, and it leaves out the near-miss / weak-accept bookkeeping's counters; the syncs both walks find are compared.

Prints one JSON line and writes it to --out (default profiles/bench_search.json); not the contract bench (bench.py is)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = np.float32


def build_captures(eng, mode, n, seconds, k_frames, seed):
    """float32 [n, seconds * 48000] on the device, the frame length, and the frame starts [n, k]"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    length = int(seconds * 48000)
    if mode == "OFDM_LTS":
        frames = eng.tx(eng.make_frames(seed, 0, n * k_frames)).reshape(n, k_frames, -1)
    else:
        zc = mode == "MCDPSK_ZC"
        pre = torch.from_numpy(eng.zc_preamble(5) if zc else eng.chirp_preamble()).to(eng.device)
        data = torch.randint(0, 256, (n * k_frames, 81), generator=g, dtype=torch.uint8)
        body = eng.mcdpsk_modulate_batch(data.to(eng.device), 10, 2 if zc else 1, 1)
        body = body * (0.8 / body.abs().amax(dim=1, keepdim=True))
        frames = torch.cat([(pre * (0.8 / pre.abs().max())).expand(n * k_frames, -1), body], dim=1).reshape(n, k_frames, -1)
    fl = frames.shape[2]
    gap = (length - k_frames * fl) // (k_frames + 1)
    assert gap > 9600, "capture too short for its frames"
    x = torch.zeros((n, length), dtype=torch.float32, device=eng.device)
    starts = np.zeros((n, k_frames), np.int64)
    for s in range(n):
        for k in range(k_frames):
            starts[s, k] = gap + k * (fl + gap) + (s * 977) % 4800
    torch.manual_seed(seed)
    noise = torch.randn((n, length), dtype=torch.float32, device=eng.device) * 0.012
    first_end = torch.as_tensor(starts[:, 0] + fl, device=eng.device)[:, None]
    x += noise * (torch.arange(length, device=eng.device)[None, :] >= first_end)      # silence up to the end of the first frame
    for k in range(k_frames):
        idx = torch.as_tensor(starts[:, k], device=eng.device)[:, None] + torch.arange(fl, device=eng.device)[None, :]
        x.scatter_add_(1, idx, frames[:, k, :].contiguous())
    return x.contiguous(), fl, starts


def library_walk(eng, x, mode, feed_step, frame_len, cfg):
    n, length = x.shape
    st = eng.search_state(n, fed=0 if feed_step else length)
    open_ = np.ones(n, bool)
    found, calls, runs, rounds = [[] for _ in range(n)], 0, 0, 0
    while open_.any():
        idx = np.flatnonzero(open_)
        res, out = eng.search(x if len(idx) == n else x[torch.as_tensor(idx, device=x.device)].contiguous(), length, st[idx], mode, feed_step=feed_step, **cfg)
        calls += 1
        runs += int(res["detector_runs"].sum())
        rounds += int(res["detector_runs"].max()) + 1          # walk -> list -> detect rounds of the call, and the walk that ends it
        ok = res["outcome"] == 1
        out["correlation_pos"][ok] = np.minimum(res["sync_position"][ok] + frame_len, 959999)
        out["last_decoded_sync_pos"][ok] = res["sync_position"][ok]
        st[idx] = out
        for j in np.flatnonzero(ok):
            found[idx[j]].append(int(res["sync_position"][j]))
        open_[idx[~ok]] = False
    return found, calls, runs, rounds


def _conf(zc_mode, streak, snr_hint):
    """light_sync_min_confidence of the two light-sync classes the bench uses (differential OFDM, ZC), vectorised"""
    if zc_mode:
        relax = np.where(streak >= 4, np.minimum(F(0.15), F(0.025) * (streak - 3).astype(F)), F(0)).astype(F)
        return np.maximum(F(0.25), F(0.40) - relax).astype(F)
    conf = np.where(snr_hint < F(10), F(0.62), np.where(snr_hint < F(14), F(0.65), np.where(snr_hint < F(18), F(0.68), F(0.72)))).astype(F)
    relax = np.where(streak >= 8, np.minimum(F(0.12), F(0.015) * (streak - 7).astype(F)), F(0)).astype(F)
    return np.where(streak >= 8, np.maximum(F(0.56), conf - relax), conf).astype(F)


def host_walk(eng, x, mode, feed_step, frame_len):
    """searchForSync driven from the host: numpy rules, torch gathers, one detector batch per round -> (syncs, rounds, detector runs)"""
    from ria_amd.acquire import _gather_windows
    n, length = x.shape
    zc, chirp = mode == "MCDPSK_ZC", mode == "MCDPSK_CHIRP"
    m = {"OFDM_LTS": 67304, "MCDPSK_ZC": 31120, "MCDPSK_CHIRP": 120000}[mode]
    cur, fed = np.zeros(n, np.int64), np.full(n, 0 if feed_step else length, np.int64)
    floor, streak, snr = np.full(n, 0.001, F), np.zeros(n, np.int64), np.zeros(n, F)
    last_cfo, last = np.zeros(n, F), np.full(n, -1, np.int64)
    open_ = np.ones(n, bool)
    found, rounds, runs = [[] for _ in range(n)], 0, 0

    def feed(ix):
        cnt = np.minimum(feed_step, length - fed[ix])
        ix = ix[cnt > 0]
        ahead = cur[ix] > fed[ix]
        cur[ix[ahead]], streak[ix[ahead]] = fed[ix[ahead]], 0
        fed[ix] += np.minimum(feed_step, length - fed[ix])

    while open_.any():
        rounds += 1
        ix = np.flatnonzero(open_)
        wait = (fed[ix] < m) | (cur[ix] > fed[ix]) | (fed[ix] - cur[ix] < m)
        stuck = ix[wait & (np.minimum(feed_step, length - fed[ix]) <= 0)]
        open_[stuck] = False
        feed(ix[wait])
        ix = ix[~wait]
        if not len(ix):
            continue
        if zc:
            uns = fed[ix] - cur[ix]
            sc = uns * 10 // m
            sev, mod_ = sc > 25, (sc > 15) & (sc <= 25)
            cur[ix[sev]] = fed[ix[sev]] - m - 4800
            cur[ix[mod_]] += np.maximum(np.minimum((uns[mod_] - m) // 2, 24000), 4800)
        seg = _gather_windows(x, ix, cur[ix], 1000)
        rms = (seg * seg).mean(dim=1).sqrt().cpu().numpy().astype(F)
        nf = np.maximum(F(0.001), floor[ix])
        floor[ix] = np.where(rms < nf * F(3), F(0.98) * nf + F(0.02) * rms, F(0.995) * nf + F(0.005) * rms).astype(F)
        if chirp:
            gate = np.clip(floor[ix] * F(1.8), F(0.014), F(0.030))
            gate = np.where(streak[ix] >= 8, np.maximum(F(0.010), gate - np.minimum(F(0.008), F(0.001) * (streak[ix] - 7).astype(F))), gate)
        else:
            gate = np.clip(floor[ix] * F(2.2), F(0.015), F(0.040))
            gate = np.where(streak[ix] >= 8, np.maximum(F(0.012), gate - np.minimum(F(0.010), F(0.001) * (streak[ix] - 7).astype(F))), gate)
        skip = rms < gate
        cur[ix[skip]] += 4800
        feed(ix[skip])
        ix = ix[~skip]
        if not len(ix):
            continue
        back = 19200 if zc else 9600
        ss = np.maximum(cur[ix] - back, 0)
        cur[ix] += 1200 if zc else 4800
        conf = _conf(not (mode == "OFDM_LTS"), streak[ix], snr[ix])
        w = _gather_windows(x, ix, ss, m)
        runs += len(ix)
        if chirp:
            d = eng.sync_chirp(w, 0.15)
            det, start, corr, cfo = d["success"] != 0, d["down_chirp_start"] + 28800, np.maximum(d["up_correlation"], d["down_correlation"]), d["cfo_hz"]
        elif zc:
            det, start, corr, cfo = np.zeros(len(ix), bool), np.zeros(len(ix), np.int64), np.zeros(len(ix), F), np.zeros(len(ix), F)
            known = torch.from_numpy(last_cfo[ix]).to(x.device)
            for thr in np.unique(conf):
                sel = np.flatnonzero(conf == thr)
                t = torch.as_tensor(sel, device=x.device)
                d = eng.sync_zc(w[t].contiguous(), float(thr), 12, known[t].contiguous())
                det[sel], start[sel], corr[sel], cfo[sel] = d["detected"] != 0, d["start_sample"], d["correlation"], d["cfo_hz"]
            miss = ~det
            up = miss & (corr >= np.maximum(F(0.20), F(0.30) - (F(0.40) - conf)))
            streak[ix[up]] += 1
            down = miss & ~up & (streak[ix] > 0)
            streak[ix[down]] -= 1
        else:
            d = eng.sync_lts(w, torch.from_numpy(last_cfo[ix]).to(x.device), 0.15)
            det, start, corr, cfo = d["detected"] != 0, d["start_sample"], d["correlation"], last_cfo[ix]
        if not chirp:
            low = det & (corr < conf)
            weak = low & (streak[ix] >= 3) & (corr >= np.maximum(F(0.30) if zc else F(0.55), conf - F(0.08)))
            rej = low & ~weak
            streak[ix[rej]] += 1
            det = det & ~rej
            streak[ix[det & weak]] = np.maximum(1, streak[ix[det & weak]] // 2)
            streak[ix[det & ~weak]] = 0
        pos = ss + start
        replay = det & (last[ix] >= 0) & (np.abs(pos - last[ix]) < 200)
        cur[ix[replay]] = pos[replay] + 14400
        acc = det & ~replay
        for j in np.flatnonzero(acc):
            found[ix[j]].append(int(pos[j]))
        a = ix[acc]
        known = last_cfo[a]
        take = (np.abs(known) > F(0.01)) & (np.abs(cfo[acc] - known) > F(1.0)) & (not chirp)
        last_cfo[a] = np.where(take, known, cfo[acc])
        snr[a] = np.clip((corr[acc] - F(0.15)) / F(0.03), F(-5), F(30))
        cur[a] = np.minimum(pos[acc] + frame_len, 959999)       # the walk: behind the frame, as after a decode
        last[a] = pos[acc]
        feed(ix[~acc])
    return found, rounds, runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_search.json"))
    a = ap.parse_args()
    from ria_amd.engine import RxEngine
    from ria_amd.srchash import csrc_sha256
    eng = RxEngine("DQPSK", "R1_4")
    out = {"tool": "bench_search", "streams": a.streams, "seconds": a.seconds, "frames_per_capture": a.frames, "reps": a.reps,
           "source_hash": csrc_sha256(), "points": []}
    for mode, secs in (("OFDM_LTS", a.seconds), ("MCDPSK_ZC", a.seconds), ("MCDPSK_CHIRP", max(a.seconds, 8.0))):
        x, fl, starts = build_captures(eng, mode, a.streams, secs, a.frames, 7)
        cfg = dict(carriers=10, modulation="DQPSK" if mode == "MCDPSK_ZC" else "DBPSK", spreading=1)
        for fs in (0, 4800):
            lib_ms, host_ms = [], []
            for rep in range(a.reps + 1):                 # alternating; the first pair warms both up
                torch.cuda.synchronize()
                t = time.perf_counter()
                f1, calls, runs1, lrounds = library_walk(eng, x, mode, fs, fl, cfg)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                f2, rounds, runs2 = host_walk(eng, x, mode, fs, fl)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if rep:
                    lib_ms.append((t1 - t) * 1e3)
                    host_ms.append((t2 - t1) * 1e3)
            sent = int(starts.size)
            lib_med, host_med = float(np.median(lib_ms)), float(np.median(host_ms))
            out["points"].append({"mode": mode, "feed_step": fs, "capture_samples": int(x.shape[1]), "frame_samples": int(fl),
                                  "library": {"ms_per_walk": lib_ms, "median_ms": lib_med, "streams_per_s": a.streams / (lib_med / 1e3), "search_calls": calls, "rounds": lrounds,
                                              "detector_runs": runs1, "syncs": sum(len(v) for v in f1)},
                                  "host_driven": {"ms_per_walk": host_ms, "median_ms": host_med, "streams_per_s": a.streams / (host_med / 1e3), "rounds": rounds,
                                                  "detector_runs": runs2, "syncs": sum(len(v) for v in f2)},
                                  "frames_sent": sent, "streams_with_identical_syncs": int(sum(p == q for p, q in zip(f1, f2))),
                                  "time_ratio_host_over_library": host_med / lib_med})
        del x
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
