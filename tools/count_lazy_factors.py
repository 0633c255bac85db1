#!/usr/bin/env python3
"""Developer aid (CPU only, oracle only): how many (codeword, factor) decodes of the min-sum factor table
decodeFixedFrame really reads on the bench workload (QAM16 R1/2, Watterson moderate, 20 dB, bench seed),
against what fast_phase0_kernel + recovery_fill_kernel compute eagerly.  The payloads are numpy draws, not bench.py's
make_frames: the same workload statistically, not the bench's own frames.  DESIGN.md section 4 quotes its output.

    python tools/count_lazy_factors.py [--scan] [n_frames] [first_frame] [seed] [channel] [snr_db] [mod] [rate]

Also used to pick the sample of tests/test_gpu_lazy_factors.py (classify())."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyoracle as po  # noqa: E402

FACTORS = (0.9375, 0.875, 0.75, 0.625, 0.5)
FORDER = (2, 3, 4, 1)     # stage-2 substitution order: 0.75, 0.625, 0.5, 0.875 (frame_v2.cpp:1837)


def frame_sample(O, mod, rate, idx, seed, kind, snr):
    """Frame idx of the stream: a random payload of the largest size drawn from (seed, idx), peak 0.8, and the channel
    seed (seed + idx) bench.py gives frame idx - any subset of the stream can be regenerated on its own"""
    rng = np.random.default_rng([seed, idx])
    cap = 4 * O.geom(mod, rate).bytes_per_cw - 19
    s, _, _ = O.tx_frame(mod, rate, rng.integers(0, 256, cap, dtype=np.uint8), idx & 0xFFFF)
    x = s * np.float32(0.8 / np.abs(s).max())
    return O.channel(kind, snr, (seed + idx) & 0xFFFFFFFF, x)


def frame_samples(O, mod, rate, n, first, seed, kind, snr):
    for f in range(n):
        yield frame_sample(O, mod, rate, first + f, seed, kind, snr)


def scan(O, mod, rate, n, first, seed, kind, snr):
    """Cheap search for the rare cases (no cascade is run): a first decode that fails and converges at factor 2..4, and
    a frame of four first-try codewords that only the fallback stage repairs"""
    g = O.geom(mod, rate)
    bpc, mi, bps = g.bytes_per_cw, g.max_iter, g.bits_per_symbol
    table = O.gather_table(bps, True)
    for idx in range(first, first + n):
        llr, _ = O.rx_process(mod, rate, frame_sample(O, mod, rate, idx, seed, kind, snr))
        cwl = [llr[table[cw * 648:(cw + 1) * 648]] for cw in range(4)]
        d0 = [O.ldpc_decode(rate, cwl[cw], mi, FACTORS[0]) for cw in range(4)]
        for cw in range(4):
            if not d0[cw][0]:
                ts = next((t for t in range(1, 5) if O.ldpc_decode(rate, cwl[cw], mi, FACTORS[t])[0]), 5)
                if ts < 5:
                    print(f"frame {idx}: cw{cw} fails first, t*={ts}", flush=True)
        if all(d[0] for d in d0):
            data = np.concatenate([d[1][:bpc] for d in d0])
            if not verify(O, data, bpc):
                for i in range(16):
                    c, t = i & 3, FORDER[i >> 2]
                    ok, by, _ = O.ldpc_decode(rate, cwl[c], mi, FACTORS[t])
                    if ok and not np.array_equal(by[:bpc], data[c * bpc:(c + 1) * bpc]):
                        tr = data.copy(); tr[c * bpc:(c + 1) * bpc] = by[:bpc]
                        if verify(O, tr, bpc):
                            d7, ok7, _, _ = O.decode_fixed_frame(llr, rate, True, bps, flags=7)
                            print(f"frame {idx}: substitution {i} passes, stage {2 if np.array_equal(d7, tr) else 1} repairs", flush=True)
                            break


def verify(O, data, bpc):
    """Frame check of four codewords' bytes: restates ro_reassemble + ro_verify_frame of oracle/ria_oracle.c, which are
    static there and not exported (their only caller, ro_decode_fixed_frame, does not say which stage repaired a frame)"""
    crc = lambda d, n: O.lib.ro_crc16(po.up(np.ascontiguousarray(d[:n])), n)  # noqa: E731
    cw = data.reshape(4, bpc)
    d = cw[0]
    if d[0] != 0x55 or d[1] != 0x4C:
        return False
    ctl = int(d[2]) in (0x10, 0x11, 0x16, 0x17, 0x20, 0x21, 0x15, 0x40)
    if ctl:
        return crc(d, 18) == (int(d[18]) << 8 | int(d[19]))
    plen = int(d[13]) << 8 | int(d[14])
    if crc(d, 15) != (int(d[15]) << 8 | int(d[16])):
        return False
    expected, parts, n = 17 + plen + 2, [], 0
    for i in range(4):
        rem = expected - n
        if rem == 0:
            break
        src = cw[i] if (i == 0 or cw[i][0] != 0xD5) else cw[i][2:]
        c = min(rem, len(src))
        parts.append(src[:c]); n += c
    fr = np.concatenate(parts)
    if len(fr) < expected:
        return False
    return crc(fr, expected - 2) == (int(fr[expected - 2]) << 8 | int(fr[expected - 1]))


def classify(O, llr, rate, bps, mod=po.QAM16):
    """One frame -> dict: per codeword the factor-table facts the walk reads, and the recovery outcome."""
    g = O.geom(mod, rate)
    bpc, mi = g.bytes_per_cw, g.max_iter
    table = O.gather_table(bps, True)
    d3, ok3, it3, att3 = O.decode_fixed_frame(llr, rate, True, bps, flags=3)
    d7, ok7, it7, att7 = O.decode_fixed_frame(llr, rate, True, bps, flags=7)
    memo = {}

    def dec(cw, f):
        if (cw, f) not in memo:
            memo[(cw, f)] = O.ldpc_decode(rate, llr[table[cw * 648:(cw + 1) * 648]], mi, FACTORS[f])
        return memo[(cw, f)]

    r = {"listed": [False] * 4, "tstar": [0] * 4, "inherit": [None] * 4, "cascade": [False] * 4}
    listed, f = False, 0
    for cw in range(4):
        listed = not dec(cw, 0)[0] or listed
        r["listed"][cw] = listed
        if listed:      # first converging factor 1..4 (5: none) - what a lazy phase 0 runs for this codeword
            r["tstar"][cw] = next((t for t in range(1, 5) if dec(cw, t)[0]), 5)
        if f == 1:
            r["inherit"][cw] = bool(dec(cw, 1)[0])
        if dec(cw, f)[0]:
            continue
        f = 0
        if r["tstar"][cw] == 5:
            r["cascade"][cw] = True
            f = 1
    r["memo"] = memo
    r["full"] = (d7, ok7, it7, att7)
    r["first_fails"] = [not dec(cw, 0)[0] for cw in range(4)]
    r["flagged"] = bool(ok3.all()) and not verify(O, d3, bpc)
    r["stage"], r["s2_index"], r["s2_ambiguous"] = 0, -1, False
    if r["flagged"]:
        # stage 2 replayed on the codewords stage 1 leaves untouched when it fails
        s2 = -1
        for i in range(16):
            at, c = i >> 2, i & 3
            ok, by, _ = dec(c, FORDER[at])
            if ok and not np.array_equal(by[:bpc], d3[c * bpc:(c + 1) * bpc]):
                t = d3.copy(); t[c * bpc:(c + 1) * bpc] = by[:bpc]
                if verify(O, t, bpc):
                    s2, s2d = i, t
                    break
        if not ok7.all():
            r["stage"] = 3           # neither stage repairs it
        elif s2 >= 0 and np.array_equal(s2d, d7):
            nbits = int(np.unpackbits(d3 ^ d7).sum())
            r["stage"], r["s2_index"], r["s2_ambiguous"] = 2, s2, nbits <= 4   # <= 4 flipped bits: stage 1 could have done it
        else:
            r["stage"] = 1
    return r


def main():
    a = sys.argv[1:]
    do_scan = bool(a) and a[0] == "--scan"
    a = a[1:] if do_scan else a
    n = int(a[0]) if len(a) > 0 else 3000
    first = int(a[1]) if len(a) > 1 else 0
    seed = int(a[2]) if len(a) > 2 else 20261004
    kind = int(a[3]) if len(a) > 3 else 2
    snr = float(a[4]) if len(a) > 4 else 20.0
    mod = getattr(po, a[5]) if len(a) > 5 else po.QAM16
    rate = getattr(po, a[6]) if len(a) > 6 else po.R1_2
    O = po.Oracle()
    if do_scan:
        return scan(O, mod, rate, n, first, seed, kind, snr)
    bps = O.geom(mod, rate).bits_per_symbol
    eager = [0, 0]; lazy = [0, 0]; fill_e = [0, 0]; fill_l = [0, 0]
    n_listed = n_flag = 0
    stages = [0, 0, 0, 0]; s2_hist = [0] * 16; amb = 0
    tstar_hist = [0] * 6; inherit = [0, 0]; casc = 0; fi = -1
    for y in frame_samples(O, mod, rate, n, first, seed, kind, snr):
        llr, _ = O.rx_process(mod, rate, y)
        r = classify(O, llr, rate, bps, mod)
        g = O.geom(mod, rate)
        mi = g.max_iter
        table = O.gather_table(bps, True)

        def it(cw, f):
            if (cw, f) not in r["memo"]:
                r["memo"][(cw, f)] = O.ldpc_decode(rate, llr[table[cw * 648:(cw + 1) * 648]], mi, FACTORS[f])
            return r["memo"][(cw, f)][2]

        fi += 1
        rare = [f"cw{cw} t*={r['tstar'][cw]}" for cw in range(4) if r["listed"][cw] and not r["memo"][(cw, 0)][0] and r["tstar"][cw] < 5]
        if r["stage"] == 2:
            rare.append(f"stage 2 repairs at index {r['s2_index']}")
        if rare:
            print(f"  frame {first + fi}: " + ", ".join(rare))
        have = set()
        for cw in range(4):
            if not r["listed"][cw]:
                continue
            n_listed += 1
            ts = r["tstar"][cw]
            tstar_hist[ts] += 1
            for t in range(1, 5):
                eager[0] += 1; eager[1] += it(cw, t)
                if t <= min(ts, 4):
                    lazy[0] += 1; lazy[1] += it(cw, t); have.add((cw, t))
            casc += int(r["cascade"][cw])
            if r["inherit"][cw] is not None:
                inherit[int(r["inherit"][cw])] += 1
        if r["flagged"]:
            n_flag += 1
            stages[r["stage"]] += 1
            amb += int(r["s2_ambiguous"])
            if r["stage"] in (2, 3):
                last = r["s2_index"] if r["stage"] == 2 else 15
                if r["stage"] == 2:
                    s2_hist[last] += 1
                for i in range(16):
                    cw, t = i & 3, FORDER[i >> 2]
                    if not r["listed"][cw]:
                        fill_e[0] += 1; fill_e[1] += it(cw, t)
                    if i <= last and (cw, t) not in have:
                        fill_l[0] += 1; fill_l[1] += it(cw, t)
    print(f"frames {n} first {first} seed {seed} channel {kind} snr {snr}")
    print(f"listed codewords {n_listed}: first converging factor t* histogram (1..4, 5 = none) {tstar_hist[1:]}, cascade {casc}")
    print(f"  first decode at inherited 0.875 (f == 1): converged {inherit[1]}, failed {inherit[0]}")
    print(f"(a) eager: phase 0 {eager[0]} decodes / {eager[1]} iterations; fill {fill_e[0]} / {fill_e[1]}")
    print(f"(b) lazy : phase 0 {lazy[0]} decodes / {lazy[1]} iterations; fill {fill_l[0]} / {fill_l[1]}")
    print(f"(c) flagged {n_flag}: stage 1 repairs {stages[1]}, stage 2 repairs {stages[2]} (of which {amb} within stage 1's reach), "
          f"unrepaired {stages[3]}; stage-2 index histogram {s2_hist}")
    per = 100000.0 / n
    print(f"per 100 000 frames: phase 0 saves {(eager[1] - lazy[1]) * per / 1e6:.2f} M iterations, "
          f"fill saves {(fill_e[1] - fill_l[1]) * per / 1e6:.2f} M, of about 150 M")


if __name__ == "__main__":
    main()
