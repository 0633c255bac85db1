#!/usr/bin/env python3
"""Developer aid (CPU only, reads the oracle, changes nothing in it): how many failing LDPC decodes of the bench workload
(QAM16 R1/2, Watterson moderate, 20 dB, bench seed) reach a message state they have been in before - from there on they
repeat themselves and cannot converge - and what a given schedule of state copies would save (the repeated-state exit
of fast_decode).  The decoder arithmetic and the cascade walk of ro_decode_fixed_frame are
restated in tools/state_repeats_helper.c with the per-iteration message vector kept; tests/test_state_repeats_cpu.py pins
both against the oracle.  Payloads are numpy draws as in tools/count_lazy_factors.py: the bench's statistics, not its frames.

    python tools/count_state_repeats.py [--scan] [n_frames] [first_frame] [seed] [channel] [snr_db] [mod] [rate]

--scan prints, per frame, the kinds of decode tests/test_gpu_state_exit.py wants in its sample (kinds())."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
import pyoracle as po  # noqa: E402
import count_lazy_factors as clf  # noqa: E402

EXIT_FIRST, EXIT_STRIDE = 22, 24      # kExitFirst, kExitStride of ria_amd/csrc/ldpc_fast.hip.h
STAGES = ("first decodes", "phase 0", "cascade")


class Result(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("ok", "iters", "rep_t", "rep_p")]


class Rec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("cw", "stage", "idx", "needed", "ok", "iters", "rep_t", "rep_p")]


_lib = None


def helper():
    """the helper and the oracle's sources as one library (the oracle's own flags), rebuilt when a source is newer"""
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(HERE, "libstate_repeats.so")
    orc = os.path.join(ROOT, "oracle")
    srcs = [os.path.join(HERE, "state_repeats_helper.c"), os.path.join(orc, "ria_oracle.c"), os.path.join(orc, "ria_oracle_sync.c")]
    deps = srcs + [os.path.join(orc, "ria_oracle.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        tmp = f"{so}.tmp.{os.getpid()}"
        subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                               "-I" + orc, "-o", tmp] + srcs + ["-lm"])
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.sr_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    L.sr_walk_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.ro_ldpc_build.argtypes = [C.c_void_p, C.c_int]
    _lib = L
    return L


_codes = {}


def decode(rate, llr, max_iter, factor):
    """the restated decoder: (ok, info bytes, iterations, rep_t, rep_p) - the first three as Oracle.ldpc_decode"""
    L = helper()
    if rate not in _codes:
        c = po.Ldpc()
        L.ro_ldpc_build(C.byref(c), rate)
        _codes[rate] = c
    c = _codes[rate]
    llr = np.ascontiguousarray(llr, np.float32)
    assert len(llr) == 648
    out = np.zeros(81, np.uint8)
    r = Result()
    L.sr_decode(C.byref(c), po.fp(llr), max_iter, factor, po.up(out), C.byref(r))
    return bool(r.ok), out[:(c.k + 7) // 8].copy(), r.iters, r.rep_t, r.rep_p


def walk(llr, rate, bps, max_iter, every=False):
    """cascade walk of one frame (phase 0 and perturbation flags set): (ok[4], iterations[4], attempts[4], records)
    records: dicts cw, stage (0 first decode, 1 factor, 2 cascade attempt), idx, needed, ok, iters, rep_t, rep_p"""
    L = helper()
    llr = np.ascontiguousarray(llr, np.float32)
    ok = np.zeros(4, np.uint8); it = np.zeros(4, np.int32); att = np.zeros(4, np.int32)
    rec = (Rec * 256)()
    n = L.sr_walk_frame(po.fp(llr), rate, bps, max_iter, int(every), po.up(ok), po.ip(it), po.ip(att), rec, 256)
    assert n <= 256
    return ok, it, att, [{f: getattr(rec[i], f) for f, _ in Rec._fields_} for i in range(n)]


def exit_iteration(r, max_iter, first=EXIT_FIRST, stride=EXIT_STRIDE):
    """Iteration at which a decode with copies at first, first + stride, ... (each compared with the one before) ends, or
    None.  A decode whose first repeat is state(rep_t) == state(rep_t - rep_p) has the pre-period mu = rep_t - rep_p and
    the period rep_p; the comparison at iteration c sees state(c) == state(c - stride) iff c - stride >= mu and the
    period divides the stride."""
    if r["ok"] or r["rep_t"] < 0 or stride % r["rep_p"]:
        return None
    mu = r["rep_t"] - r["rep_p"]
    c = first + stride
    while c < max_iter:
        if c - stride >= mu:
            return c
        c += stride
    return None


def gpu_decodes(recs):
    """The walk's records (every=True) as the decodes of the GPU's retry kernels: key (kernel, cw, idx) -> (record, certain).
    Phase 0 decodes factor t = 1..4 of every listed codeword (one at or behind the frame's first failed first decode):
    certainly up to its first converging factor, the later ones depending on timing.  The first decode at the inherited
    0.875 is phase 0's t = 1.  The cascade certainly runs the attempts up to the winner, the later ones depending on timing."""
    out = {}
    listed = False
    for cw in range(4):
        first = next(r for r in recs if r["cw"] == cw and r["stage"] == 0)
        listed = listed or not first["ok"]
        fac = {r["idx"]: r for r in recs if r["cw"] == cw and r["stage"] == 1}
        if listed and fac:
            tstar = next((t for t in range(1, 5) if fac[t]["ok"]), 4)
            for t, r in fac.items():
                out[("phase0", cw, t)] = (r, t <= tstar)
        for r in recs:
            if r["cw"] == cw and r["stage"] == 2:
                out[("cascade", cw, r["idx"])] = (r, bool(r["needed"]))
    return out


def kinds(recs, max_iter):
    """which of the cases of tests/test_gpu_state_exit.py the NEEDED decodes of a frame hold (phase 0 and cascade)"""
    k = set()
    for (kern, _, _), (r, certain) in gpu_decodes(recs).items():
        if not certain:
            continue
        if r["ok"]:
            if EXIT_FIRST < r["iters"] <= EXIT_FIRST + EXIT_STRIDE:
                k.add("converges 23..46")
            elif r["iters"] > EXIT_FIRST + EXIT_STRIDE:
                k.add("converges after 46")
            continue
        x = exit_iteration(r, max_iter)
        if x == EXIT_FIRST + EXIT_STRIDE:
            k.add("exit at 46")
        elif x is not None:
            k.add(f"exit at {x}")
        elif r["rep_t"] < 0:
            k.add("no repeat")
        elif r["rep_p"] == 48:
            k.add("period 48")
        else:
            k.add("repeat not found")
    return k


def frame_llr(O, mod, rate, idx, seed, kind, snr):
    return O.rx_process(mod, rate, clf.frame_sample(O, mod, rate, idx, seed, kind, snr))[0]


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
    g = O.geom(mod, rate)
    bps, mi = g.bits_per_symbol, g.max_iter
    helper()
    results = [None] * n
    nt = min(16, len(os.sched_getaffinity(0)))

    def work(k):
        for q in range(k, n, nt):
            results[q] = walk(frame_llr(O, mod, rate, first + q, seed, kind, snr), rate, bps, mi, every=do_scan)[3]
    frame_llr(O, mod, rate, first, seed, kind, snr)      # static tables before threading
    th = [threading.Thread(target=work, args=(k,)) for k in range(nt)]
    [t.start() for t in th]; [t.join() for t in th]
    if do_scan:
        for q, recs in enumerate(results):
            k = kinds(recs, mi)
            rare = k & {"converges 23..46", "converges after 46", "period 48"} | {x for x in k if x.startswith("exit at")}
            if rare:
                print(f"frame {first + q}: " + ", ".join(sorted(rare)), flush=True)
        return
    schedules = [(22, 24, 2), (22, 24, 3), (20, 24, 3), (24, 24, 3), (16, 24, 3), (22, 12, 5)]
    print(f"frames {n} first {first} seed {seed} channel {kind} snr {snr} max_iter {mi}")
    tot_it = [0, 0, 0]; fail_it = [0, 0, 0]
    for st in range(3):
        rs = [r for recs in results for r in recs if r["stage"] == st and r["needed"]]
        failed = [r for r in rs if not r["ok"]]
        rep = [r for r in failed if r["rep_t"] >= 0]
        per = {}
        for r in rep:
            per[r["rep_p"]] = per.get(r["rep_p"], 0) + 1
        # iterations a decode runs: converged after `iters` iterations has run iters + 1 check passes
        tot_it[st] = sum(r["iters"] + (1 if r["ok"] else 0) for r in rs)
        fail_it[st] = sum(r["iters"] for r in failed)
        mu = sorted(r["rep_t"] - r["rep_p"] for r in rep)
        pct = (lambda p: mu[min(len(mu) - 1, int(p * len(mu)))]) if mu else (lambda p: -1)
        ex = [exit_iteration(r, mi) for r in failed]
        found = sum(x is not None for x in ex)
        saved = sum(mi - (x + 1) for x in ex if x is not None)
        every = sum(mi - (r["rep_t"] + 1) for r in rep)
        print(f"{STAGES[st]}: {len(rs)} decodes / {tot_it[st]} iterations, failed {len(failed)} ({100.0 * fail_it[st] / max(tot_it[st], 1):.1f} % of the "
              f"iterations), with an exact repeat before iteration {mi}: {len(rep)}")
        print("    periods " + ", ".join(f"{p}: {c}" for p, c in sorted(per.items(), key=lambda kv: -kv[1])[:8])
              + f"; cycle entered at iteration (10 / 50 / 90 %) {pct(0.1)} / {pct(0.5)} / {pct(0.9)}")
        print(f"    copies at {EXIT_FIRST} + {EXIT_STRIDE} i: {found} exits ({sum(x == EXIT_FIRST + EXIT_STRIDE for x in ex)} at the first comparison), "
              f"{saved} iterations = {100.0 * saved / max(tot_it[st], 1):.1f} %; a comparison in every iteration: {every} = {100.0 * every / max(tot_it[st], 1):.1f} %")
    scale = 100000.0 / n
    print(f"per 100 000 frames: first decodes {tot_it[0] * scale / 1e6:.1f} M iterations, phase 0 {tot_it[1] * scale / 1e6:.1f} M, cascade {tot_it[2] * scale / 1e6:.1f} M")
    for f0, stride, cnt in schedules:
        sv = [0, 0, 0]; nx = [0, 0, 0]
        for st in (1, 2):
            for recs in results:
                for r in recs:
                    if r["stage"] == st and r["needed"] and not r["ok"]:
                        x = exit_iteration(r, min(mi, f0 + stride * (cnt - 1) + 1), f0, stride)
                        if x is not None:
                            sv[st] += mi - (x + 1); nx[st] += 1
        at = ", ".join(str(f0 + stride * i) for i in range(cnt) if f0 + stride * i < mi)
        print(f"copies at {at}: phase 0 {nx[1] * scale / 1e3:.0f} k exits / {100.0 * sv[1] / max(tot_it[1], 1):.1f} % of its iterations, "
              f"cascade {nx[2] * scale / 1e3:.0f} k exits / {100.0 * sv[2] / max(tot_it[2], 1):.1f} %, together "
              f"{100.0 * (sv[1] + sv[2]) / max(tot_it[1] + tot_it[2], 1):.1f} % of phase 0 + cascade")


if __name__ == "__main__":
    main()
