#!/usr/bin/env python3
"""Developer aid (CPU only, oracle only): the first decodes (factor 0.9375) decodeFixedFrame never reads on the bench
workload (QAM16 R1/2, Watterson moderate, 20 dB), i.e. what fast_primary_kernel skips when it walks a frame's codewords in
order.  Once a codeword goes to the cascade the reference's decoder object stays at 0.875, so every later codeword of the
frame makes its first decode at 0.875 and its 0.9375 decode is unread - unless phase 0 rescues a codeword in between,
which puts the decoder back to 0.9375 (fast_late_kernel then makes that decode).  The stream is the one of
tools/count_lazy_factors.py.  DESIGN.md section 4 (32) quotes the output.

    python tools/count_unread_first_decodes.py [--classes] [n_frames] [first_frame] [seed] [channel] [snr_db] [mod] [rate]

--classes also runs the whole decode of every frame that has a skipped slot (slow: the cascade on the CPU) and lists the
frames by class; tests/test_gpu_frame_walk.py pins its sample from that list and asserts the classes with walk()."""
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pyoracle as po  # noqa: E402
import count_lazy_factors as clf  # noqa: E402


def walk(O, llr, rate, bps, mod=po.QAM16, flags=3):
    """One frame -> what the frame walk does with it under `flags` (bit 0: phase 0, bit 1: perturbation cascade):
    first_fail   codeword of the first failing 0.9375 decode, None: none fails
    skipped[cw]  the 0.9375 decode fast_primary_kernel does not make (a codeword behind first_fail, cascade flag set)
    late[cw]     of those, the ones the chain reads after all (the decoder is back at 0.9375 behind a phase-0 rescue)
    d0[cw]       (converged, iterations run) of the 0.9375 decode, made or not (a decode that converges in iteration i ran i + 1)
    fill_back    skipped 0.9375 decodes a fallback trial could read: the fallback substitutes factors clf.FORDER only"""
    g = O.geom(mod, rate)
    mi = g.max_iter
    table = O.gather_table(bps, True)
    memo = {}

    def dec(cw, f):
        if (cw, f) not in memo:
            memo[(cw, f)] = O.ldpc_decode(rate, llr[table[cw * 648:(cw + 1) * 648]], mi, clf.FACTORS[f])
        return memo[(cw, f)]

    d0 = [(bool(dec(cw, 0)[0]), int(dec(cw, 0)[2]) + int(bool(dec(cw, 0)[0]))) for cw in range(4)]
    first_fail = next((cw for cw in range(4) if not d0[cw][0]), None)
    perturb, phase0 = bool(flags & 2), bool(flags & 1)
    skipped = [perturb and first_fail is not None and cw > first_fail for cw in range(4)]
    late, rescued, cascade = [False] * 4, [0] * 4, [False] * 4
    f = 0
    for cw in range(4):          # the chain (fast_chain_walk): which slot the decoder reads first
        if f == 0 and skipped[cw]:
            late[cw] = True
        if dec(cw, f)[0]:
            continue
        ts = 5
        if phase0:
            ts = next((t for t in range(1, 5) if dec(cw, t)[0]), 5)
            f = 0
        if ts < 5:
            rescued[cw] = ts
        elif perturb:
            cascade[cw] = True
            f = 1
    fill_back = sum(1 for i in range(16) if clf.FORDER[i >> 2] == 0 and skipped[i & 3])
    return {"first_fail": first_fail, "skipped": skipped, "late": late, "d0": d0, "rescued": rescued, "cascade": cascade,
            "fill_back": fill_back}


def frame_classes(w):
    """the classes of tests/test_gpu_frame_walk.py a frame belongs to, from walk() alone"""
    c = set()
    c.add("no failure" if w["first_fail"] is None else f"first failure at cw {w['first_fail']}")
    for cw in range(4):
        if w["skipped"][cw]:
            c.add("converging behind failing" if w["d0"][cw][0] else "failing behind failing")
        if w["late"][cw]:
            c.add("late decode")
    return c


def _threads(work, n, nt=16):
    th = [threading.Thread(target=work, args=(k * n // nt, (k + 1) * n // nt)) for k in range(nt)]
    [t.start() for t in th]; [t.join() for t in th]


def main():
    a = sys.argv[1:]
    classes = bool(a) and a[0] == "--classes"
    a = a[1:] if classes else a
    n = int(a[0]) if len(a) > 0 else 3000
    first = int(a[1]) if len(a) > 1 else 0
    seed = int(a[2]) if len(a) > 2 else 20261004
    kind = int(a[3]) if len(a) > 3 else 2
    snr = float(a[4]) if len(a) > 4 else 20.0
    mod = getattr(po, a[5]) if len(a) > 5 else po.QAM16
    rate = getattr(po, a[6]) if len(a) > 6 else po.R1_2
    O = po.Oracle()
    bps = O.geom(mod, rate).bits_per_symbol
    ws, llrs = [None] * n, [None] * n

    def work(lo, hi):
        for q in range(lo, hi):
            llr, _ = O.rx_process(mod, rate, clf.frame_sample(O, mod, rate, first + q, seed, kind, snr))
            ws[q] = walk(O, llr, rate, bps, mod)
            if classes and any(ws[q]["skipped"]):
                llrs[q] = llr
    work(0, 1)
    _threads(work, n)
    it_all = sum(w["d0"][cw][1] for w in ws for cw in range(4))
    sk = [w["d0"][cw] for w in ws for cw in range(4) if w["skipped"][cw]]
    late = sum(sum(w["late"]) for w in ws)
    it_late = sum(w["d0"][cw][1] for w in ws for cw in range(4) if w["late"][cw])
    fill_back = sum(w["fill_back"] for w in ws)
    print(f"frames {n} first {first} seed {seed} channel {kind} snr {snr}")
    print(f"first decodes at 0.9375: {4 * n} decodes / {it_all} iterations")
    print(f"behind a codeword whose 0.9375 decode failed: {len(sk)} codewords / {sum(i for _, i in sk)} iterations "
          f"({100.0 * sum(i for _, i in sk) / max(it_all, 1):.0f} %): {sum(1 for ok, _ in sk if not ok)} fail, {sum(1 for ok, _ in sk if ok)} converge")
    print(f"read after all behind a phase-0 rescue (late decodes): {late} codewords / {it_late} iterations")
    print(f"skipped 0.9375 decodes a fallback trial reads (the fallback substitutes factors {[clf.FACTORS[t] for t in clf.FORDER]} only): {fill_back}")
    per = 100000.0 / n
    print(f"per 100 000 frames: {(sum(i for _, i in sk) - it_late) * per / 1e6:.2f} M of {it_all * per / 1e6:.2f} M first-decode iterations are not run, "
          f"{len(sk) * per:.0f} codewords ({100.0 * len(sk) / (4 * n):.0f} %) are not set up")
    by = {}
    for q, w in enumerate(ws):
        for c in frame_classes(w):
            by.setdefault(c, []).append(first + q)
    if classes:
        todo = [q for q in range(n) if llrs[q] is not None]
        cls = {}

        def full(lo, hi):
            for k in range(lo, hi):
                cls[todo[k]] = clf.classify(O, llrs[todo[k]], rate, bps, mod)
        _threads(full, len(todo))
        for q in todo:
            if cls[q]["flagged"] and cls[q]["stage"] in (2, 3):
                by.setdefault("flagged for the fallback with a skipped slot 0", []).append(first + q)
    for c in sorted(by):
        print(f"  {c}: {len(by[c])} frames, first {by[c][:12]}")


if __name__ == "__main__":
    main()
