#!/usr/bin/env python3
"""Developer aid (CPU only, oracle only): how many of the fallback stage's re-decodes (frame_v2.cpp:1836-1866, the units of
recovery_fill_kernel) can change a verifying trial, by the rule of ria_amd/csrc/fallback_relevance.hpp restated here in
Python: codeword 0 always; codeword c >= 1 only if the header in codeword 0 parses and the codewords before c do not
already supply the whole frame.  Same frames and method as tools/count_lazy_factors.py (frame_sample, classify): numpy
payloads of the largest size on the bench workload's channel, not bench.py's own frames; the fill set assumes that phase 0
skips every factor behind a listed codeword's first converging one.  DESIGN.md section 4 (28) quotes its output.

    python tools/count_fallback_relevance.py [n_frames] [first_frame] [seed] [channel] [snr_db] [mod] [rate]"""
import os
import sys
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import count_lazy_factors as clf  # noqa: E402
from count_lazy_factors import po  # noqa: E402

CONTROL_TYPES = (0x10, 0x11, 0x16, 0x17, 0x20, 0x21, 0x15, 0x40)


def relevant_codewords(O, data, bpc):
    """(header parses, [relevant] per codeword) of four codewords' current bytes"""
    crc = lambda d, n: O.lib.ro_crc16(po.up(np.ascontiguousarray(d[:n])), n)  # noqa: E731
    cw = data.reshape(4, bpc)
    d = cw[0]
    hdr = d[0] == 0x55 and d[1] == 0x4C
    if hdr and int(d[2]) in CONTROL_TYPES:
        hdr, expected = crc(d, 18) == (int(d[18]) << 8 | int(d[19])), 20
    elif hdr:
        hdr, expected = crc(d, 15) == (int(d[15]) << 8 | int(d[16])), 17 + (int(d[13]) << 8 | int(d[14])) + 2
    if not hdr:
        return False, [True, False, False, False]
    rel, n = [], 0
    for i in range(4):
        rel.append(i == 0 or n < expected)
        n += bpc - (2 if i != 0 and cw[i][0] == 0xD5 else 0)
    return True, rel


def count_frame(O, mod, rate, idx, seed, kind, snr):
    g = O.geom(mod, rate)
    bps, bpc, mi = g.bits_per_symbol, g.bytes_per_cw, g.max_iter
    llr, _ = O.rx_process(mod, rate, clf.frame_sample(O, mod, rate, idx, seed, kind, snr))
    r = clf.classify(O, llr, rate, bps, mod)
    if r["stage"] not in (2, 3):
        return None
    table = O.gather_table(bps, True)
    d3 = O.decode_fixed_frame(llr, rate, True, bps, flags=3)[0]
    hdr, rel = relevant_codewords(O, d3, bpc)
    units = its = p_units = p_its = 0
    for cw in range(4):
        for t in range(1, 5):
            if r["listed"][cw] and t <= min(r["tstar"][cw], 4):
                continue                      # phase 0 has it
            if (cw, t) not in r["memo"]:
                r["memo"][(cw, t)] = O.ldpc_decode(rate, llr[table[cw * 648:(cw + 1) * 648]], mi, clf.FACTORS[t])
            it = r["memo"][(cw, t)][2]
            units += 1; its += it
            if not rel[cw]:
                p_units += 1; p_its += it
    return {"hdr": hdr, "units": units, "its": its, "p_units": p_units, "p_its": p_its,
            "stage1_reach": r["stage"] == 2 and r["s2_ambiguous"]}


def main():
    a = sys.argv[1:]
    n = int(a[0]) if len(a) > 0 else 3200
    first = int(a[1]) if len(a) > 1 else 0
    seed = int(a[2]) if len(a) > 2 else 20261004
    kind = int(a[3]) if len(a) > 3 else 2
    snr = float(a[4]) if len(a) > 4 else 20.0
    mod = getattr(po, a[5]) if len(a) > 5 else po.QAM16
    rate = getattr(po, a[6]) if len(a) > 6 else po.R1_2
    O = po.Oracle()
    count_frame(O, mod, rate, first, seed, kind, snr)     # static tables before threading
    rows = [None] * n
    nt = min(16, len(os.sched_getaffinity(0)))

    def work(k):
        for q in range(k, n, nt):
            rows[q] = count_frame(O, mod, rate, first + q, seed, kind, snr)
    th = [threading.Thread(target=work, args=(k,)) for k in range(nt)]
    [t.start() for t in th]; [t.join() for t in th]
    fb = [r for r in rows if r is not None]
    tot = lambda k: sum(r[k] for r in fb)  # noqa: E731
    pct = lambda x, y: f"{100.0 * x / max(y, 1):.1f} %"  # noqa: E731
    print(f"frames {n} first {first} seed {seed} channel {kind} snr {snr}")
    print("| quantity | value |\n|---|---|")
    print(f"| frames reaching the fallback | {len(fb)} |")
    print(f"| of which header invalid | {sum(not r['hdr'] for r in fb)} ({pct(sum(not r['hdr'] for r in fb), len(fb))}) |")
    print(f"| of which repaired by a substitution of at most 4 bits (stage 1 may take them first) | {sum(r['stage1_reach'] for r in fb)} |")
    print(f"| fill units | {tot('units')} |")
    print(f"| fill iterations | {tot('its')} |")
    print(f"| units prunable by the two rules | {tot('p_units')} ({pct(tot('p_units'), tot('units'))}) |")
    print(f"| iterations prunable | {tot('p_its')} ({pct(tot('p_its'), tot('its'))}) |")
    per = 100000.0 / n
    print(f"per 100 000 frames: fill {tot('its') * per / 1e6:.1f} M iterations in {tot('units') * per:.0f} units, "
          f"prunable {tot('p_its') * per / 1e6:.1f} M in {tot('p_units') * per:.0f} units, of about 150 M")


if __name__ == "__main__":
    main()
