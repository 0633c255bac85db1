"""Time of RxEngine.mcdpsk_stream (ria_gpu_mcdpsk_stream_batch) on one GPU against the composition it replaces,
ria_amd.acquire.mcdpsk_link_stream (RxEngine.search + RxEngine.mcdpsk_window with the host's part in Python, one host round
trip per window), in the same run, each with a chase pool and with none.

Workload: N recordings of a connected MC-DPSK link (ZC preamble, 20 carriers DQPSK), each holding a data frame of --codewords
codewords and its retransmission, built on the device: ria_gpu_ldpc_encode_host for the coded bytes, the device interleaver
with --interleave, the device modulator, the reference-identical channel (AWGN at --snr-db, one seed per recording), and a
burst of Gaussian noise of standard deviation --burst on the second codeword of both receptions, so that a reception on its own
loses that codeword and the two together may recover it.  feed_step 4800: the recording arrives in 100 ms chunks.

Prints one JSON line and writes it to --out (default profiles/bench_mcdpsk_stream.json); not the contract bench (bench.py is)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CARRIERS, BPS = 20, 2
LEAD, GAP, TAIL = 14000, 9000, 40000


def build_recordings(eng, n, codewords, snr_db, burst, interleave, seed):
    """float32 [n, length] on the device, the frames' bytes and the two receptions' first samples"""
    from ria_amd.acquire import _data_frame, _encode_r14, mcdpsk_frame_len
    pre = torch.from_numpy(eng.zc_preamble(5)).to(eng.device)
    coded, sent = [], []
    for s in range(n):
        payload = ((np.arange(18 * (codewords - 1) - 1) * 7 + s) % 251).astype(np.uint8)
        frame = _data_frame(0x30, s & 0xFFFF, payload)
        sent.append(bytes(frame))
        coded.append(_encode_r14(eng, frame, codewords))
    coded = torch.from_numpy(np.stack(coded)).to(eng.device)
    if interleave:
        coded = eng.mcdpsk_interleave(coded, CARRIERS * BPS)
    body = eng.mcdpsk_modulate_batch(coded, CARRIERS, BPS, 1)
    tx = torch.cat([pre[None, :].expand(n, -1), body], dim=1)
    tx = tx * (0.8 / tx.abs().amax(dim=1, keepdim=True))
    fl = tx.shape[1]
    assert fl <= len(pre) + mcdpsk_frame_len(codewords, CARRIERS, BPS, 1)      # the modulator packs the bits: the last symbols of the span lie in the gap
    at = [LEAD, LEAD + fl + GAP]
    x = torch.zeros((n, at[1] + fl + TAIL), dtype=torch.float32, device=eng.device)
    for a in at:
        x[:, a:a + fl] = tx
    eng.channel_exact_seeded_(x, 0, snr_db, np.arange(seed, seed + n, dtype=np.uint32))
    if burst > 0:
        per = CARRIERS * BPS
        first, last = -(-648 // per) + 1, 2 * 648 // per - 1          # the symbols that carry bits of codeword 1 only
        torch.manual_seed(seed)
        for a in at:
            lo, hi = a + len(pre) + (9 + first) * 512, a + len(pre) + (9 + last) * 512
            x[:, lo:hi] += torch.randn((n, hi - lo), dtype=torch.float32, device=eng.device) * burst
    return x.contiguous(), sent, at


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--codewords", type=int, default=3)
    ap.add_argument("--snr-db", type=float, default=25.0)
    ap.add_argument("--burst", type=float, default=0.3)
    ap.add_argument("--interleave", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_mcdpsk_stream.json"))
    a = ap.parse_args()
    from ria_amd.acquire import LINK_STREAM_COUNTERS, link_stream_tally, mcdpsk_link_stream
    from ria_amd.engine import RxEngine
    from ria_amd.srchash import csrc_sha256
    eng = RxEngine("DQPSK", "R1_4")
    n = a.streams
    x, sent, at = build_recordings(eng, n, a.codewords, a.snr_db, a.burst, a.interleave, 7)
    lens = np.full(n, x.shape[1], np.int64)
    kw = dict(feed_step=4800, max_events=4, carriers=CARRIERS, modulation="DQPSK", spreading=1, channel_interleave=a.interleave)
    out = {"tool": "bench_mcdpsk_stream", "streams": n, "codewords": a.codewords, "snr_db": a.snr_db, "burst_sigma": a.burst,
           "interleave": bool(a.interleave), "recording_samples": int(x.shape[1]), "reps": a.reps, "source_hash": csrc_sha256(), "points": []}
    for with_pool in (True, False):
        call_ms, comp_ms = [], []
        for rep in range(a.reps + 1):                 # alternating; the first pair warms both up
            pools = [eng.chase_pool(n), eng.chase_pool(n)] if with_pool else [None, None]
            try:
                torch.cuda.synchronize()
                t = time.perf_counter()
                st, res, ev, frames, hq = eng.mcdpsk_stream(x, lens, "MCDPSK_ZC", chase=pools[0], **kw)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                cst, cclosed, cev, cframes, chq = mcdpsk_link_stream(eng, x, lens, "MCDPSK_ZC", chase=pools[1], **kw)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
            finally:
                for p in pools:
                    if p is not None:
                        p.close()
            if rep:
                call_ms.append((t1 - t) * 1e3)
                comp_ms.append((t2 - t1) * 1e3)
        fr = frames.cpu().numpy()
        whole = sum(any(e["success"] and fr[s, k, :len(sent[s])].tobytes() == sent[s] for k, e in enumerate(ev[s, :res["n_events"][s]])) for s in range(n))
        identical = bool(np.array_equal(ev.view(np.uint8), cev.view(np.uint8)) and np.array_equal(fr, cframes) and
                         np.array_equal(st.view(np.uint8), cst.view(np.uint8)) and np.array_equal(res["closed"], cclosed))
        call_med, comp_med = float(np.median(call_ms)), float(np.median(comp_ms))
        out["points"].append({"pool": with_pool,
                              "one_call": {"ms": call_ms, "median_ms": call_med, "streams_per_s": n / (call_med / 1e3)},
                              "composition": {"ms": comp_ms, "median_ms": comp_med, "streams_per_s": n / (comp_med / 1e3)},
                              "time_ratio_composition_over_call": comp_med / call_med, "records_identical": identical,
                              "streams_with_the_whole_frame": int(whole), "search_legs": int(res["search_legs"].max()),
                              "tally": dict(zip(LINK_STREAM_COUNTERS, (int(v) for v in link_stream_tally(ev, hq))))})
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
