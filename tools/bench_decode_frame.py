#!/usr/bin/env python3
"""Cost of decodeFrame's control-frame hypotheses on the GPU: ria_gpu_decode_frame_batch (RxEngine.decode_frame) on rows
of QAM16 R1/2 soft bits that come from the device chain make_frames -> tx -> channel -> demod, for three sets: AWGN
20 dB, Watterson moderate 20 dB, and the AWGN set with every second row replaced by a clean R1/4 ACK.  Timed alternately,
median of --reps runs each:
  (a) decode_frame
  (b) decode (ria_gpu_decode_batch) on the same rows: (a) - (b) is what the hypotheses cost
  (c) the composition a user can write from the separate calls: a second R1/4 engine's ldpc_decode on the gathered CW0
      rows, ldpc_decode at the rate on them, the classification (magic, control / data-header CRC, total_cw) in torch, a
      read-back of the selection, decode on the selected rows.  It has neither the salvage nor the legacy stage: its
      results are compared with (a) only on the rows it covers.
Stage times come from device events around calls that reproduce each stage on its own (tools/bench_burst.py's way): the
R1/4 probe over all rows, the rate probe over the rows it leaves, decodeFixedFrame over the rows selected, the two robust
decoders over the rows it fails; 'other_ms' is what the whole call takes beyond their sum (lists, gather, legacy, finish,
the two host reads).
Prints one JSON line and writes it to --out (default profiles/bench_decode_frame.json); not the contract bench."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ria_amd import capi  # noqa: E402
from ria_amd.acquire import DFRAME_COUNTERS, dframe_tally  # noqa: E402
from ria_amd.engine import RxEngine  # noqa: E402

CONTROL_TYPES = (0x10, 0x11, 0x16, 0x17, 0x20, 0x21, 0x15, 0x40)


def crc16(data, init=0xFFFF):
    crc = init
    for b in bytes(data):
        crc ^= b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def crc16_torch(d, table):
    """CRC-16/CCITT-FALSE of every row of d (uint8 [n, L]) on the device -> int64 [n]"""
    crc = torch.full((d.shape[0],), 0xFFFF, dtype=torch.int64, device=d.device)
    for i in range(d.shape[1]):
        crc = ((crc << 8) & 0xFFFF) ^ table[(crc >> 8) ^ d[:, i].long()]
    return crc


def _once_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def timed_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    return float(np.median([_once_ms(fn) for _ in range(reps)]))


def timed_round_ms(fns, reps):
    """the forms timed alternately (the machine's load drifts), one warm-up call each -> (median, min, max) per form"""
    for f in fns:
        f()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            t[k].append(_once_ms(f))
    return [(float(np.median(x)), float(min(x)), float(max(x))) for x in t]


def ack_row(e14, seq, amp=4.0):
    d = np.zeros(21, np.uint8)
    d[:12] = [0x55, 0x4C, 0x20, 0, seq >> 8, seq & 255, 0x12, 0x34, 0x56, 0x65, 0x43, 0x21]
    c = crc16(d[:18])
    d[18], d[19] = c >> 8, c & 255
    bits = np.unpackbits(e14.ldpc_encode(d[None, :]).reshape(-1))[:648]
    return (amp * (1.0 - 2.0 * bits)).astype(np.float32)


def compose(e, e14, llr, table, keep=None):
    """form (c) -> (selected row indices, info, status) and, in keep (a dict), the intermediate tensors"""
    cw0 = llr[:, :648].contiguous()
    o14, ok14, _ = e14.ldpc_decode(cw0, e14.geo.ldpc_max_iterations, 0.75)
    o, ok, _ = e.ldpc_decode(cw0, e.geo.ldpc_max_iterations, 0.75)
    ctl_types = torch.tensor(CONTROL_TYPES, device=llr.device, dtype=torch.uint8)

    def classify(b, good):
        magic = (good != 0) & (b[:, 0] == 0x55) & (b[:, 1] == 0x4C)
        is_ctl = (b[:, 2:3] == ctl_types[None, :]).any(dim=1)
        ctl_ok = crc16_torch(b[:, :18], table) == ((b[:, 18].long() << 8) | b[:, 19].long())
        hdr_ok = crc16_torch(b[:, :15], table) == ((b[:, 15].long() << 8) | b[:, 16].long())
        total = torch.where(is_ctl, torch.ones_like(b[:, 12].long()), b[:, 12].long())
        valid = magic & torch.where(is_ctl, ctl_ok, hdr_ok)
        return magic, valid, total

    _, v14, t14 = classify(o14, ok14)
    hit14 = v14 & (t14 == 1)
    magic, valid, total = classify(o, ok)
    hit0 = ~hit14 & valid & (total == 1)
    fixed = ~hit14 & ~hit0 & (~magic | (valid & (total == 4)))
    sel = torch.nonzero(fixed).reshape(-1)                  # sizes the next call: a device-to-host read
    info, st = e.decode(llr[sel][:, :2592].contiguous()) if len(sel) else (None, None)
    if keep is not None:
        keep.update(hit14=hit14, hit0=hit0, sel=sel, info=info, st=st)
    return sel, info, st


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--seed", type=int, default=20240607)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_decode_frame.json"))
    args = ap.parse_args()
    n = args.rows
    e = RxEngine("QAM16", "R1_2", device=0, max_batch=n)
    e14 = RxEngine("DQPSK", "R1_4", device=0, max_batch=64)
    tab = np.zeros(256, np.int64)
    for b in range(256):
        tab[b] = crc16(bytes([b]), init=0)
    table = torch.from_numpy(tab).cuda()

    def soft_bits(kind, seed):
        x = e.tx(e.make_frames(seed, 0, n))
        e.channel_exact_(x, kind, 20.0, seed)
        return e.demod(x, want_status=False)[0]

    sets = {"awgn_20db": soft_bits(0, args.seed), "watterson_moderate_20db": soft_bits(2, args.seed + 1)}
    half = sets["awgn_20db"].clone()
    acks = np.stack([ack_row(e14, s) for s in range(64)])
    rng = np.random.default_rng(args.seed)
    rows = (4.0 * rng.standard_normal((n // 2, half.shape[1]))).astype(np.float32)     # noise behind the ACK
    rows[:, :648] = acks[np.arange(n // 2) % 64]
    half[1::2] = torch.from_numpy(rows).cuda()[: half[1::2].shape[0]]
    sets["awgn_20db_half_acks"] = half
    out = {"bench": "decode_frame", "mode": "QAM16 R1/2", "rows": n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "sets": {}}
    for name, llr in sets.items():
        frames, res, st = e.decode_frame(llr)
        torch.cuda.synchronize()
        status = e.decode_status(st)
        keep = {}
        compose(e, e14, llr, table, keep)
        torch.cuda.synchronize()
        # (c) covers the R1/4 hit, the CW0 hit and the fixed frame: on those rows it must say what (a) says
        path = torch.from_numpy(res["path"].astype(np.int64)).cuda()
        sel = keep["sel"]
        agree = bool(((path == 1) == keep["hit14"]).all().item()) and bool(((path == 2) == keep["hit0"]).all().item())
        ran_fixed = torch.from_numpy(((res["stages"] >> 2) & 1).astype(bool)).cuda()
        agree = agree and bool((torch.nonzero(ran_fixed).reshape(-1) == sel).all().item()) if len(sel) == int(ran_fixed.sum().item()) else False
        if agree and len(sel):
            agree = bool((e.decode_status(keep["st"])["cw_ok"] == status["cw_ok"][sel.cpu().numpy()]).all())
        ta, tb, tc = timed_round_ms([lambda: e.decode_frame(llr), lambda: e.decode(llr),
                                     lambda: compose(e, e14, llr, table)], args.reps)
        cw0 = llr[:, :648].contiguous()
        open1 = cw0[torch.from_numpy(((res["stages"] >> 1) & 1).astype(bool)).cuda()].contiguous()
        fixed_rows = llr[sel][:, :2592].contiguous() if len(sel) else None
        stage = {"r14_probe_ms": timed_ms(lambda: e14.ldpc_decode(cw0, 50, 0.75), args.reps),
                 "rate_probe_ms": timed_ms(lambda: e.ldpc_decode(open1, e.geo.ldpc_max_iterations, 0.75), args.reps) if len(open1) else 0.0,
                 "fixed_ms": timed_ms(lambda: e.decode(fixed_rows), args.reps) if fixed_rows is not None else 0.0}
        salv = cw0[torch.from_numpy(((res["stages"] >> 3) & 1).astype(bool)).cuda()].contiguous()
        stage["salvage_ms"] = timed_ms(lambda: (e14.ldpc_decode_robust(salv), e.ldpc_decode_robust(salv)), args.reps) if len(salv) else 0.0
        stage["other_ms"] = ta[0] - sum(stage.values())
        ran = ((res["stages"] >> 2) & 1).astype(bool)
        out["sets"][name] = {
            "decode_frame_ms": dict(zip(("median", "min", "max"), ta)), "decode_ms": dict(zip(("median", "min", "max"), tb)),
            "composition_ms": dict(zip(("median", "min", "max"), tc)), "hypotheses_ms": ta[0] - tb[0],
            "stage_ms": stage, "tally": dict(zip(DFRAME_COUNTERS, (int(v) for v in dframe_tally(res)))),
            "probe_codeword_iterations": int(res["iters_r14"].astype(np.int64).sum() + res["iters_cw0"].astype(np.int64).sum()),
            "fixed_codeword_iterations_reported": int(status["iterations"][ran].astype(np.int64).sum()),
            "composition_agrees_on_its_rows": agree,
        }
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
