"""CPU: the HARQ chase cache without a GPU.

(a) the ABI of the chase pool and the two HARQ calls: symbols, record sizes, argument validation that needs no device;
(b) the Python ChaseCache of tests/mcdpsk_harq_restatement.py reproduces every cache sum the reference recorded
    (tests/golden/harq_trials.npz), so it can stand for the reference's cache in the GPU tests;
(c) ria_amd/csrc/chase_policy.hpp, the policy the kernels run, built into a stand-alone program (tests/helpers/
    chase_policy_check.cpp) and driven through scripted operation sequences against that Python cache - plainly, and again
    under AddressSanitizer and UBSan;
(d) the ordering trap: "store all failures, then mark all successes" gives a miss where the reference combines."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import pyoracle as po
from mcdpsk_harq_restatement import STATS, ChaseCache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- (a)
def test_harq_abi_symbols_sizes_and_null_arguments():
    from ria_amd import capi
    L = capi.load()
    for name in ("ria_gpu_chase_default_config", "ria_gpu_chase_create", "ria_gpu_chase_destroy", "ria_gpu_chase_clear", "ria_gpu_chase_stats",
                 "ria_gpu_chase_export", "ria_gpu_mcdpsk_decode_frame_batch", "ria_gpu_mcdpsk_acquire_harq_batch"):
        assert getattr(L, name) is not None and name in capi.EXPORTS
    assert C.sizeof(capi.ChaseConfig) == 32 and C.sizeof(capi.ChaseStats) == 56 and C.sizeof(capi.ChaseEntry) == 80
    assert C.sizeof(capi.McDframeResult) == 16 and C.sizeof(capi.McHarqResult) == 32
    assert capi.ChaseEntry.combine_count.offset == 32 and capi.ChaseEntry.has_sum.offset == 64
    assert capi.McHarqResult.stored_mask.offset == 12 and capi.McHarqResult.cache_id.offset == 20
    from ria_amd.engine import ChasePool, RxEngine
    assert ChasePool.ENTRY.itemsize == 80 and RxEngine.HARQ_RESULT.itemsize == 32 and RxEngine.MCDFRAME_RESULT.itemsize == 16
    cfg = capi.ChaseConfig()
    L.ria_gpu_chase_default_config(C.byref(cfg))
    assert (cfg.n_caches, cfg.max_entries, cfg.ttl_ms) == (1, 16, 30000)
    p = C.c_void_p()
    assert L.ria_gpu_chase_create(None, C.byref(cfg), C.byref(p)) == -1 and not p
    L.ria_gpu_chase_destroy(None)
    st = capi.ChaseStats()
    assert L.ria_gpu_chase_clear(None, None, 0, None) == -1
    assert L.ria_gpu_chase_stats(None, 0, C.byref(st)) == -1
    assert L.ria_gpu_chase_export(None, 0, None, None) == -1
    assert L.ria_gpu_mcdpsk_decode_frame_batch(None, None, 648, None, 0, None, None, None, None, 20, None, None, None) == -1
    assert L.ria_gpu_mcdpsk_acquire_harq_batch(None, None, None, 0, 0, 0, 0, 1, None, 0, None, None, None, 0, None, None, None, None, None) == -1


# ---- (b)
def test_python_cache_reproduces_the_reference_sums(oracle, golden):
    """The chain of tests/test_oracle_golden.py (modulate, channel, demodulate, robust decode; on failure store and, from the
    second reception on, decode the sum) with the Python ChaseCache: the checksum of every sum equals the one recorded from
    the reference's ChaseCache."""
    import gen_golden
    g = golden("harq_trials")
    sums = 0
    for case, n in ((0, 6), (6, 6), (9, 6)):
        nc, bps, sp, kind, snr = gen_golden.HARQ_CASES[case]
        info, seeds = gen_golden.harq_inputs(case, n)
        for i in range(n):
            tx = oracle.mcdpsk_modulate(nc, bps, sp, oracle.ldpc_encode(po.R1_4, info[i]))
            cache, key = ChaseCache(), (i, 0x123456, 0x654321)
            for t in range(seeds.shape[1]):
                llr, _ = oracle.mcdpsk_demod(nc, bps, sp, oracle.channel(kind, snr, int(seeds[i, t]), tx))
                soft = np.ascontiguousarray(llr[:648])
                assert zlib.crc32(soft.tobytes()) == g[f"llr_crc_{case}"][i, t]
                ok, _, _, _ = oracle.robust_decode(po.R1_4, soft)
                if not ok:
                    assert cache.store(key, 1, soft, 2, 0x30, 1000 * t)
                    acc = cache.get_combined(key, 1)
                    assert zlib.crc32(acc.tobytes()) == g[f"acc_crc_{case}"][i, t], (case, i, t)
                    assert cache.get_combine_count(key, 1) == t + 1
                    sums += 1
                    if t:
                        ok, _, _, _ = oracle.robust_decode(po.R1_4, acc)
                if ok:
                    assert g[f"tx_to_success_{case}"][i] == t + 1
                    break
            else:
                assert g[f"tx_to_success_{case}"][i] == 0
    assert sums >= 8


# ---- (c)
K = [(s, 0x123456, 0x654321) for s in range(40)]


def scripts():
    """name -> list of operations (op, args...)"""
    S = {}
    # fill to max_entries, then the oldest goes; touching an entry makes it young
    ops = [("cfg", 4, 30000)]
    for j in range(4):
        ops.append(("store", K[j], 1, 3, 0x30, 100 + j, 1.0 + j))
    ops += [("dump",), ("store", K[0], 2, 3, 0x30, 110, 0.5), ("store", K[4], 1, 3, 0x30, 111, 2.0), ("dump",),
            ("get", K[1], 1), ("get", K[0], 1), ("get", K[0], 2), ("store", K[5], 1, 3, 0x30, 112, 3.0), ("dump",)]
    S["fill_and_evict"] = ops
    # equal times: the entry touched first goes
    S["tie"] = [("cfg", 3, 30000), ("store", K[2], 1, 3, 0x30, 50, 1.0), ("store", K[1], 1, 3, 0x30, 50, 1.0), ("store", K[0], 1, 3, 0x30, 50, 1.0),
                ("store", K[2], 2, 3, 0x30, 50, 1.0), ("store", K[3], 1, 3, 0x30, 50, 1.0), ("dump",), ("get", K[1], 1), ("get", K[2], 1),
                ("store", K[4], 1, 3, 0x30, 50, 1.0), ("dump",), ("get", K[0], 1)]
    # expiry at exactly ttl (kept) and ttl + 1 (gone); a clock that runs backwards expires nothing
    S["expiry"] = [("cfg", 16, 1000), ("store", K[0], 1, 3, 0x30, 5000, 1.0), ("store", K[1], 1, 3, 0x30, 5000, 1.0),
                   ("store", K[2], 1, 3, 0x30, 6000, 1.0), ("dump",), ("store", K[3], 1, 3, 0x30, 6001, 1.0), ("dump",),
                   ("store", K[4], 1, 3, 0x30, 10, 1.0), ("dump",), ("get", K[0], 1), ("get", K[2], 1), ("count", K[0], 1)]
    # the fifth store is refused while the sum is still returned
    ops = [("cfg", 16, 30000)]
    for j in range(6):
        ops += [("store", K[7], 2, 3, 0x31, 10 * j, 0.1 * (j + 1)), ("get", K[7], 2), ("count", K[7], 2)]
    S["max_combines"] = ops + [("dump",)]
    # markDecoded: on no entry a no-op; after it the store is refused and getCombined misses; all decoded erases the entry
    S["mark"] = [("cfg", 16, 30000), ("mark", K[0], 1), ("dump",), ("store", K[0], 2, 3, 0x30, 1, 1.0), ("store", K[0], 1, 3, 0x30, 2, 1.5),
                 ("mark", K[0], 1), ("recover",), ("store", K[0], 1, 3, 0x30, 3, 2.0), ("get", K[0], 1), ("count", K[0], 1), ("dump",),
                 ("mark", K[0], 7), ("mark", K[0], -1), ("mark", K[0], 2), ("dump",), ("mark", K[0], 0), ("dump",), ("get", K[0], 2),
                 ("store", K[0], 2, 3, 0x30, 4, 1.0), ("get", K[0], 2), ("dump",)]
    # argument checks: cw_index against total_cw and against the entry's, total_cw 0 and 17, negative index
    S["arguments"] = [("cfg", 16, 30000), ("store", K[0], 0, 0, 0x30, 1, 1.0), ("store", K[0], 1, 17, 0x30, 1, 1.0), ("store", K[0], 16, 17, 0x30, 1, 1.0),
                      ("store", K[0], -1, 3, 0x30, 1, 1.0), ("store", K[0], 3, 3, 0x30, 1, 1.0), ("dump",), ("store", K[0], 15, 16, 0x30, 1, 1.0),
                      ("store", K[1], 1, 2, 0x30, 2, 1.0), ("store", K[1], 2, 3, 0x30, 3, 1.0), ("store", K[1], 1, 3, 0x30, 4, 1.0), ("get", K[1], 2),
                      ("get", K[1], -1), ("get", K[1], 1), ("get", K[9], 1), ("count", K[1], 2), ("count", K[9], 0), ("count", K[1], -1), ("dump",),
                      ("remove", K[1]), ("remove", K[9]), ("dump",), ("clear",), ("dump",), ("store", K[0], 1, 3, 0x30, 9, 1.0), ("dump",)]
    # max_entries 1: every new key evicts
    S["single_entry"] = [("cfg", 1, 30000), ("store", K[0], 1, 3, 0x30, 1, 1.0), ("store", K[1], 1, 3, 0x30, 2, 1.0), ("store", K[1], 1, 3, 0x30, 3, 1.0),
                         ("store", K[0], 1, 3, 0x30, 4, 1.0), ("get", K[1], 1), ("get", K[0], 1), ("dump",)]
    # a seeded random walk over few keys in a small cache
    rng = np.random.default_rng(20260101)
    ops, now = [("cfg", 3, 40)], 0
    for _ in range(600):
        now += int(rng.integers(0, 12))
        k, cw = K[int(rng.integers(0, 6))], int(rng.integers(0, 4))
        op = rng.choice(["store", "store", "store", "get", "count", "mark", "remove", "dump"], p=[0.3, 0.2, 0.1, 0.15, 0.05, 0.1, 0.04, 0.06])
        if op == "store":
            ops.append(("store", k, cw, int(rng.integers(2, 5)), 0x30, now, float(np.float32(rng.standard_normal()))))
        elif op in ("get", "count", "mark"):
            ops.append((op, k, cw))
        elif op == "remove":
            ops.append(("remove", k))
        else:
            ops.append(("dump",))
    S["random_walk"] = ops + [("dump",)]
    # time: ttl 0 (the same now keeps, now + 1 expires), ttl INT64_MAX, now stepping 2^63 - 1 -> 2^63 -> 2^64 - 1 -> 0, and
    # last_access 0 against now 2^63, where (int64)(now - last_access) and an unbounded subtraction disagree; the steps are
    # those of tests/mcdpsk_harq_domain_inputs.py, which the GPU domain test runs through the kernels
    from mcdpsk_harq_domain_inputs import time_script
    for name, (max_entries, ttl, steps) in time_script().items():
        ops = [("cfg", max_entries, ttl)]
        for s, now in steps:
            ops += [("store", K[s], 1, 3, 0x30, now, 1.0), ("dump",)]
        S[name] = ops
    return S


def script_text(ops):
    out = []
    for op in ops:
        words = [op[0]]
        for a in op[1:]:
            if isinstance(a, tuple):
                words += [str(v) for v in a]
            elif isinstance(a, float):
                words.append(repr(float(np.float32(a))))
            else:
                words.append(str(a))
        out.append(" ".join(words))
    return "\n".join(out) + "\n"


def python_transcript(ops):
    cache, out = None, []
    for op in ops:
        name, a = op[0], op[1:]
        if name == "cfg":
            cache = ChaseCache(a[0], a[1])
        elif name == "store":
            key, cw, total, ftype, now, v = a
            out.append("store %d" % cache.store(key, cw, np.full(648, v, np.float32), total, ftype, now))
        elif name == "get":
            s = cache.get_combined(a[0], a[1])
            assert s is None or (s == s[0]).all()
            out.append("get %d %08x" % (s is not None, 0 if s is None else int(s[:1].view(np.uint32)[0])))
        elif name == "count":
            out.append("count %d" % cache.get_combine_count(a[0], a[1]))
        elif name == "mark":
            cache.mark_decoded(a[0], a[1])
        elif name == "remove":
            cache.remove_entry(a[0])
        elif name == "clear":
            cache.clear()
        elif name == "recover":
            cache.increment_recoveries()
        elif name == "dump":
            out.append("stats " + " ".join(str(cache.stats[k]) for k in STATS))
            out.append("size %d" % cache.size())
            for k in sorted(cache.cache):
                e = cache.cache[k]
                out.append("entry %d %d %d total %d type %d last %d order %d : " % (k + (e.total_cw, e.frame_type, e.last_access, e.order)) +
                           " ".join("%d/%d/%d" % (e.count[i], e.decoded[i], e.soft[i] is not None) for i in range(e.total_cw)))
    return out + ["done"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def policy_exe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chase") / "chase_policy_check")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "helpers", "chase_policy_check.cpp")])
    return exe


def test_policy_header_matches_the_python_cache(policy_exe, tmp_path):
    S = scripts()
    for name, ops in S.items():
        path = str(tmp_path / (name + ".txt"))
        with open(path, "w") as f:
            f.write(script_text(ops))
        out = subprocess.run([policy_exe, path], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (name, out.stdout[-2000:], out.stderr[-4000:])
        got, want = [l.rstrip() for l in out.stdout.strip().split("\n")], [l.rstrip() for l in python_transcript(ops)]
        assert got == want, (name, next((i, g, w) for i, (g, w) in enumerate(zip(got + [""], want + [""])) if g != w))
    # the scripts do what their names say (on the Python cache)
    t = python_transcript(S["fill_and_evict"])
    assert [l for l in t if l.startswith(("stats", "size"))] == ["stats 0 0 4 0 0 0 0", "size 4", "stats 0 0 6 0 1 0 0", "size 4", "stats 2 1 7 0 2 0 0", "size 4"]
    assert [l.split()[1] for l in t if l.startswith("entry")][-4:] == ["0", "3", "4", "5"]        # 1 went first, then 2: 0 was touched
    t = python_transcript(S["tie"])
    assert [l.split()[1] for l in t if l.startswith("entry")] == ["0", "2", "3", "2", "3", "4"]   # equal times: 1, then 0, go
    t = python_transcript(S["expiry"])
    assert [l for l in t if l.startswith(("stats", "size"))] == ["stats 0 0 3 0 0 0 0", "size 3", "stats 0 0 4 0 0 2 0", "size 2", "stats 0 0 5 0 0 2 0", "size 3"]
    t = python_transcript(S["max_combines"])
    assert [l for l in t if l.startswith("store")] == ["store 1"] * 4 + ["store 0"] * 2 and t.count("count 4") == 3
    assert t[10:12] == t[13:15] == t[16:18] and t[10].startswith("get 1") and "stats 6 0 6 3 0 0 0" in t
    from mcdpsk_harq_domain_inputs import TIME_SIZES
    for name, sizes in TIME_SIZES.items():
        t = python_transcript(S[name])
        assert [int(l.split()[1]) for l in t if l.startswith("size")] == sizes, name
    assert [l.split()[6] for l in python_transcript(S["time_ttl0"]) if l.startswith("stats")] == ["0", "0", "2", "2", "2", "5"]   # entries_expired


# ---- (d)
class _Scripted:
    """robust_decode that fails the rows whose first soft bit is negative (the payload never reaches the test)"""

    def __init__(self, d0):
        self.d0 = d0

    def robust_decode(self, rate, llr):
        if llr[0] < 0:
            return False, np.zeros(21, np.uint8), 50, 5
        if llr[1] == 0:
            return True, np.concatenate([self.d0, [0]]).astype(np.uint8), 1, 1
        return True, np.concatenate([[0xD5, int(llr[1])], np.zeros(19, np.uint8)]).astype(np.uint8), 1, 1


def test_ordering_trap_wrong_order_misses():
    """Reception 1: CW1 decodes, CW2 fails.  Reception 2: CW1 fails.  The reference marks CW1 in a cache without an entry (a
    no-op), so reception 2's CW1 is stored; with "store all failures, then mark all successes" it is refused and
    getCombined misses."""
    from mcdpsk_acquire_restatement import data_frame
    from mcdpsk_harq_restatement import decode_mcdpsk_frame
    d0 = data_frame(0x30, 5, np.arange(25, dtype=np.uint8))[:20]

    def rows(ok1, ok2):
        x = np.ones(3 * 648, np.float32)
        x[1] = 0
        x[648], x[649] = (1 if ok1 else -1), 1
        x[1296], x[1297] = (1 if ok2 else -1), 2
        return x
    chk = _Scripted(d0)
    for wrong, stored, misses in ((False, 1 << 1, 0), (True, 0, 1)):
        cache = ChaseCache()
        r, hq = decode_mcdpsk_frame(chk, rows(True, False), cache, 0, wrong_order=wrong)
        assert (r["codewords_ok"], r["codewords_failed"], hq["stored_mask"]) == (2, 1, 1 << 2)
        base = cache.stats["cache_misses"]
        r, hq = decode_mcdpsk_frame(chk, rows(False, True), cache, 1, wrong_order=wrong)
        assert hq["stored_mask"] == stored and cache.stats["cache_misses"] - base == misses, (wrong, hq, cache.stats)
