"""Rows, the pool-and-restatement pair and the scenarios of the HARQ chase pool's domain tests: shared by
tests/test_mcdpsk_harq_domain_cpu.py (which runs every scenario on the restatement alone and asserts that it reaches what it
is about), tests/test_gpu_mcdpsk_harq_domain.py (which runs them on the device) and tests/test_gpu_mcdpsk_harq.py.

Everything is a function of small integers (key, per-codeword amplitudes at unit noise, seed, n_llr, cache id, now_ms), so
nothing large is committed.  The robust decoder at R1/4 can converge on noise: the seeds below were searched on the CPU and
are pinned; the claims_* functions state, as assertions, what each scenario must do.

Test infrastructure only (not collected: no test_ prefix)."""
import numpy as np

from mcdpsk_acquire_restatement import ACK, control_frame, data_frame, encode_frame, oracle
from mcdpsk_ci_restatement import decode_mcdpsk_frame_ci, interleave_bytes
from mcdpsk_harq_restatement import STATS, ChaseCache, cache_snapshot, canon, decode_mcdpsk_frame, empty_harq

RES_FIELDS = ("success", "codewords_ok", "codewords_failed", "frame_type", "header_total_cw")
CI_FIELDS = ("cw0_deinterleaved", "ci_tried")
HARQ_FIELDS = ("valid", "seq", "src_hash", "dst_hash", "stored_mask", "sum_mask", "recovered_mask", "max_combine", "entry")
GOOD, WEAK2, WEAK3, DEAD = 2.0, 0.6, 0.42, 0.12   # codeword amplitudes at unit noise: decodes / sum of 2 decodes / of 3 / never
NONE, KEPT, REMOVED = 0, 1, 2                      # RIA_HARQ_ENTRY_*
U64 = 2 ** 64
INT64_MAX = 2 ** 63 - 1
N = 648


# ---- the checker: the oracle's robust decoder, remembered by input (a pure function of 648 floats), so that a codeword
# that many rows of a scenario share is decoded once
class Memo:
    def __init__(self, checker):
        self.checker, self.seen, self.calls = checker, {}, 0

    def robust_decode(self, rate, llr):
        llr = np.ascontiguousarray(llr, np.float32)
        k = (int(rate), llr.tobytes())
        if k not in self.seen:
            self.calls += 1
            self.seen[k] = self.checker.robust_decode(rate, llr)
        return self.seen[k]

    def __getattr__(self, name):
        return getattr(self.checker, name)


_memo = None


def checker():
    global _memo
    if _memo is None:
        _memo = Memo(oracle())
    return _memo


# ---- rows
def frame_of(seq, total_cw, ftype=0x30):
    """a data frame that fills exactly total_cw codewords (20 bytes in CW0, 18 in each of the others)"""
    n = 1 + 18 * (total_cw - 1)
    return data_frame(ftype, seq, ((np.arange(n) * 7 + seq) % 256).astype(np.uint8), total_cw=total_cw)


def row(seq, amps, seed, stride=3 * N, frame=None, il=None):
    """coded bits of a frame (default: the 3-codeword data frame of sequence number seq), codeword c scaled by amps[c], plus
    seeded unit Gaussian noise; noise alone behind the frame.  il: every codeword through ChannelInterleaver(il, 648)"""
    if frame is None:
        frame = data_frame(0x30, seq, np.arange(25, dtype=np.uint8))
    coded = encode_frame(frame)
    if il is not None:
        coded = interleave_bytes(coded, il)
    bits = np.unpackbits(coded).astype(np.float64)
    x = np.random.default_rng(seed).standard_normal(max(stride, len(bits)))
    x[:len(bits)] += np.repeat(np.asarray(amps, np.float64)[:len(bits) // N], N) * (1.0 - 2.0 * bits)
    return x[:stride].astype(np.float32)


def same_floats(got, want):
    """bit-equal, except that where the restatement holds a NaN the device holds a NaN (sign and payload not compared)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.isnan(got[nan]).all()) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def restate(llr, cache, now, B=None):
    """one row through the restatement -> (DecodeResult dict, harq dict)"""
    if B is None:
        r, h = decode_mcdpsk_frame(checker(), llr, cache, now)
    else:
        r, h = decode_mcdpsk_frame_ci(checker(), llr, B, cache, now)
    return r, h or empty_harq()


# ---- a pool on the device and the restatement's caches beside it
class Links:
    """A pool on the device and the restatement's caches beside it; call() runs one batch through both and compares"""

    def __init__(self, eng, n_caches, max_entries=16, ttl_ms=30000):
        from ria_amd.acquire import HARQ_COUNTERS
        self.eng, self.pool = eng, eng.chase_pool(n_caches, max_entries, ttl_ms)
        self.caches = [ChaseCache(max_entries, ttl_ms) for _ in range(n_caches)]
        self.counters = HARQ_COUNTERS
        self.tally = np.zeros(len(HARQ_COUNTERS), np.int64)

    def check_tally(self):
        """ria_amd.acquire.harq_tally summed over the calls against the sum of the caches' counters"""
        t = dict(zip(self.counters, self.tally))
        for k in ("stores", "combines", "recoveries"):
            assert t[k] == sum(c.stats[k] for c in self.caches), (k, t)
        return t

    def call(self, rows, ids, now, n_llr=None, compare=None, B=None):
        """compare: the cache ids to compare after the call (None: all).  B: through the channel-interleaving call"""
        import torch
        from ria_amd.acquire import harq_tally
        rows = np.stack(rows)
        n, stride = rows.shape
        n_llr = [stride] * n if n_llr is None else n_llr
        now = np.broadcast_to(np.asarray(now, np.uint64), (n,))
        kw = {} if B is None else dict(channel_interleave=True, interleaver_bits=B)
        frames, res, hq = self.eng.mcdpsk_decode_frame(torch.from_numpy(rows).to(self.eng.device), n_llr=n_llr, chase=self.pool, cache_id=ids,
                                                       now_ms=now, **kw)
        frames = frames.cpu().numpy()
        self.tally += harq_tally(res, hq)
        out = []
        for i in range(n):
            r, h = restate(rows[i, :max(0, min(n_llr[i], stride))], self.caches[ids[i]] if ids[i] >= 0 else None, int(now[i]), B)
            for f in RES_FIELDS + (CI_FIELDS if B is not None else ()):
                assert int(res[f][i]) == int(r[f]), (i, f, res[f][i], r[f])
            nb = len(r["frame"])
            assert int(res["frame_bytes"][i]) == nb and np.array_equal(frames[i, :nb], r["frame"]) and not frames[i, nb:].any(), i
            for f in HARQ_FIELDS:
                assert int(hq[f][i]) == int(h[f]), (i, f, hq[f][i], h[f])
            assert int(hq["cache_id"][i]) == (ids[i] if h["valid"] else 0), i
            out.append((r, h))
        self.compare_caches(compare)
        return out

    def clear(self, ids=None):
        self.pool.clear(ids)
        for c in (range(len(self.caches)) if ids is None else ids):
            if 0 <= c < len(self.caches):
                self.caches[c].clear()

    def compare_caches(self, ids=None):
        for c in (range(len(self.caches)) if ids is None else ids):
            compare_cache(self.pool, c, self.caches[c])

    def run(self, scn):
        """a Scenario's calls, one after the other -> what replay() returns"""
        hist, snaps = [], []
        for k in scn.calls:
            if k.clear is not None:
                self.clear(None if k.clear == "all" else k.clear)
                self.compare_caches()
            hist.append(self.call(k.rows, k.ids, k.now, k.n_llr, B=k.B))
            snaps.append([(dict(c.stats), cache_snapshot(c)) for c in self.caches])
        return hist, self.caches, snaps

    def close(self):
        self.pool.close()


def compare_cache(pool, c, cache):
    """counters, live entries and sums of cache c of the pool against the restatement's cache"""
    assert pool.stats(c) == cache.stats, (c, pool.stats(c), cache.stats)
    ent, sums = pool.export(c)
    want = cache_snapshot(cache)
    assert sorted((int(e["seq"]), int(e["src_hash"]), int(e["dst_hash"])) for e in ent) == sorted(want), c
    for e, s in zip(ent, sums):
        w = want[(int(e["seq"]), int(e["src_hash"]), int(e["dst_hash"]))]
        assert (int(e["total_cw"]), int(e["frame_type"]), int(e["last_access_ms"]), int(e["order"]), int(e["used"])) == \
               (w["total_cw"], w["frame_type"], w["last_access"], w["order"], 1), (c, e, w)
        assert e["combine_count"].tolist() == w["count"] and e["decoded"].tolist() == w["decoded"] and e["has_sum"].tolist() == w["has_sum"], (c, e, w)
        assert not e["reserved"].any(), (c, e)
        assert same_floats(s, w["sums"]), c


# ---- scenarios
class Call:
    def __init__(self, rows, ids, now, n_llr=None, clear=None, B=None):
        self.rows, self.ids, self.now, self.n_llr, self.clear, self.B = rows, ids, now, n_llr, clear, B


class Scenario:
    def __init__(self, n_caches, max_entries, ttl_ms, calls):
        self.n_caches, self.max_entries, self.ttl_ms, self.calls = n_caches, max_entries, ttl_ms, calls

    def links(self, eng):
        return Links(eng, self.n_caches, self.max_entries, self.ttl_ms)


def replay(scn):
    """the scenario on the restatement alone -> (hist[call][row] = (DecodeResult dict, harq dict), the caches, a snapshot
    of every cache after every call)"""
    caches = [ChaseCache(scn.max_entries, scn.ttl_ms) for _ in range(scn.n_caches)]
    hist, snaps = [], []
    for k in scn.calls:
        if k.clear is not None:
            for c in (range(scn.n_caches) if k.clear == "all" else k.clear):
                if 0 <= c < scn.n_caches:
                    caches[c].clear()
        n = len(k.rows)
        now = np.broadcast_to(np.asarray(k.now, np.uint64), (n,))
        out = []
        for i in range(n):
            stride = len(k.rows[i])
            nl = stride if k.n_llr is None else max(0, min(k.n_llr[i], stride))
            out.append(restate(k.rows[i][:nl], caches[k.ids[i]] if k.ids[i] >= 0 else None, int(now[i]), k.B))
        hist.append(out)
        snaps.append([(dict(c.stats), cache_snapshot(c)) for c in caches])
    return hist, caches, snaps


def keys_of(snap):
    return sorted(k[0] for k in snap[1])


# ---- (a) sixteen codewords
S16 = 16 * N
FILL_BLOCKS = 15


def fill_row(k):
    """key 200 + k of the cache that is filled: CW0 of its 16-codeword frame, and behind it 15 noise blocks that never
    decode; key k takes the blocks in an order of its own (rotated by k), so that every slot holds different floats while
    the restatement decodes 15 blocks in all"""
    x = row(200 + k, (GOOD,) + (0.0,) * 15, 7000 + k, stride=S16, frame=frame_of(200 + k, 16))
    blocks = np.random.default_rng(7100).standard_normal((FILL_BLOCKS, N)).astype(np.float32)
    for c in range(1, 16):
        x[c * N:(c + 1) * N] = blocks[(c - 1 + k) % FILL_BLOCKS]
    return x


SIXTEEN_SEEDS = (3, 4)        # pinned: claims_sixteen holds with them


def sixteen():
    """A pool of 3 caches, 16 calls.  Cache 0: 16-codeword frames over several receptions (key 100: every codeword weak
    twice, then whole; key 101: weak three times; key 102: the odd codewords fail first, the even ones next, then all of
    them weak).  Cache 2: filled with 16 keys of 16 codewords.  Cache 1: only rows that n_llr cuts at 15 codewords and at
    16 * 648 - 1 soft bits, which never reach the cache."""
    s0, s1 = SIXTEEN_SEEDS
    W2, W3, G = (GOOD,) + (WEAK2,) * 15, (GOOD,) + (WEAK3,) * 15, (GOOD,) * 16
    odd = (GOOD,) + tuple(DEAD if c % 2 else GOOD for c in range(1, 16))
    even = (GOOD,) + tuple(GOOD if c % 2 else DEAD for c in range(1, 16))
    link = [(100, W2, s0), (100, W2, s0 + 100), (100, G, 11), (101, W3, s1), (101, W3, s1 + 100), (101, W3, s1 + 200), (101, W3, s1 + 300),
            (102, odd, 20), (102, even, 21), (102, odd, 22), (102, even, 23), (102, G, 24), (103, W2, s0 + 200), (103, W2, s0 + 300),
            (103, G, 12), (104, odd, 25)]
    calls = []
    for t in range(16):
        seq, amps, seed = link[t]
        rows, ids, n_llr = [row(seq, amps, seed, stride=S16, frame=frame_of(seq, 16)), fill_row(t)], [0, 2], [S16, S16]
        if t in (3, 9):
            rows.append(row(150 + t, (GOOD,) + (DEAD,) * 15, 30 + t, stride=S16, frame=frame_of(150 + t, 16)))
            ids.append(1)
            n_llr.append(15 * N if t == 3 else S16 - 1)
        calls.append(Call(rows, ids, 1000 * t, n_llr))
    return Scenario(3, 16, 30000, calls)


def claims_sixteen(hist, caches, snaps):
    stored = summed = recovered = 0
    for out in hist:
        stored |= out[0][1]["stored_mask"]
        summed |= out[0][1]["sum_mask"]
        recovered |= out[0][1]["recovered_mask"]
    assert stored == summed == recovered == 0xFFFE, (hex(stored), hex(summed), hex(recovered))   # every index 1 .. 15, bit 15 included
    assert any(out[0][1]["max_combine"] == 3 and out[0][1]["recovered_mask"] for out in hist)
    for t, out in enumerate(hist):                                        # the cache that is filled
        assert out[1][1]["stored_mask"] == 0xFFFE and out[1][1]["entry"] == KEPT, t
        assert len(snaps[t][2][1]) == t + 1
    full = snaps[15][2][1]
    assert len(full) == 16 and all(e["has_sum"] == [0] + [1] * 15 for e in full.values())
    assert snaps[15][2][0]["entries_evicted"] == 0 and snaps[15][2][0]["stores"] == 240
    for t in (3, 9):                                                      # the cut rows: a header, 16 asked for, 15 there
        r, h = hist[t][2]
        assert (r["header_total_cw"], r["codewords_ok"], r["success"], len(r["frame"]), h["valid"], h["entry"]) == (16, 1, 0, 20, 1, NONE)
    assert all(s[1][0] == dict.fromkeys(STATS, 0) and not s[1][1] for s in snaps)


# ---- (b) slot reuse
def slot_reuse(max_entries):
    """One cache of max_entries 1 or 2, ttl 1000.  Keys leave by eviction, by expiry, by full success and by clear; each time
    a key with another total_cw lands in the slot and fails codewords that had a sum in the old entry: its first store must
    copy, its second add.  max_entries 2 runs the same steps with a second key (T = 4) kept alive in the other slot."""
    st = 5 * N
    D = DEAD
    steps = [(300, 5, (GOOD, D, D, GOOD, D), 0), (301, 3, (GOOD, D, D), 10), (301, 3, (GOOD, D, D), 20),      # 301 evicts 300
             (302, 5, (GOOD, D, GOOD, D, D), 2000), (302, 5, (GOOD,) * 5, 2010),                              # 301 expired; 302 removed on success
             (303, 2, (GOOD, D), 2020), (303, 2, (GOOD, D), 2030),                                            # after the removal
             (304, 4, (GOOD, D, D, D), 2040, "all"), (304, 4, (GOOD, D, D, D), 2050)]                         # after clear
    calls = []
    for j, s in enumerate(steps):
        seq, T, amps, now = s[:4]
        if max_entries == 2 and j not in (3, 4):    # the neighbour: touched before every step but the expiry, so it is never the oldest
            calls.append(Call([row(390, (GOOD, D, GOOD, D), 8100 + j, stride=st, frame=frame_of(390, 4))], [0], now - 5 if now else 0))
        calls.append(Call([row(seq, amps, 8000 + j, stride=st, frame=frame_of(seq, T))], [0], now, clear=s[4] if len(s) > 4 else None))
    return Scenario(1, max_entries, 1000, calls)


def claims_slot_reuse(max_entries, scn, hist, caches, snaps):
    idx = [i for i, k in enumerate(scn.calls) if 300 <= k_seq(hist[i]) <= 304]
    assert len(idx) == 9
    h = [hist[i][0][1] for i in idx]
    sn = [snaps[i][0] for i in idx]
    ent = lambda j, seq: sn[j][1][(seq, 0x123456, 0x654321)]
    assert [x["stored_mask"] for x in h] == [0b10110, 0b110, 0b110, 0b11010, 0, 0b10, 0b10, 0b1110, 0b1110]
    assert [x["sum_mask"] for x in h] == [0, 0, 0b110, 0, 0, 0, 0b10, 0, 0b1110]
    assert [x["max_combine"] for x in h] == [1, 1, 2, 1, 0, 1, 2, 1, 2]          # counts start fresh in a used slot
    assert h[4]["entry"] == REMOVED and all(x["recovered_mask"] == 0 for x in h)
    assert sn[1][0]["entries_evicted"] - sn[0][0]["entries_evicted"] == 1 and 300 not in keys_of(sn[1])
    assert sn[3][0]["entries_expired"] == max_entries and keys_of(sn[3]) == [302]
    assert keys_of(sn[4]) == [] and ent(5, 303)["total_cw"] == 2 and ent(7, 304)["total_cw"] == 4
    assert ent(1, 301)["has_sum"][:5] == [0, 1, 1, 0, 0] and ent(1, 301)["decoded"] == [0] * 16 and not ent(1, 301)["sums"][3:].any()
    assert ent(3, 302)["decoded"][:5] == [0, 0, 1, 0, 0] and ent(5, 303)["decoded"] == [0] * 16
    for j, seq, src in ((1, 301, 1), (3, 302, 3), (5, 303, 5), (7, 304, 7)):      # the first store in a used slot is a copy of the row
        assert np.array_equal(ent(j, seq)["sums"][1], scn.calls[idx[j]].rows[0][N:2 * N])
    if max_entries == 2:
        assert all(390 in keys_of(snaps[i][0]) for i in range(len(hist)) if i not in (idx[3], idx[4], idx[7]))


def k_seq(out):
    return out[0][1]["seq"]


# ---- (c) one key, changing header
def changing_header():
    """Two caches, ttl 1000, the key of sequence number 400 throughout.  Cache 0: total_cw 3 (type 0x30) at 0; total_cw 5 (type
    0x31) at 400, codewords 1 and 2 add, 3 and 4 are refused, miss and count 0; the same at 500 with codewords 1 and 2 whole:
    only refused stores, which still refresh last_access; total_cw 2 at 1500 = last + ttl: the entry is kept (and its
    codeword 1 is decoded, so the store is refused); at 2501 it is expired and a fresh entry of total_cw 2 begins.
    Cache 1: the same first row, nothing in between, and at 1001 the entry is expired."""
    st, D = 5 * N, DEAD
    f3, f5, f2 = frame_of(400, 3), frame_of(400, 5, 0x31), frame_of(400, 2)
    r0 = row(400, (GOOD, D, D), 9000, stride=st, frame=f3)
    calls = [Call([r0, r0], [0, 1], 0),
             Call([row(400, (GOOD, D, D, D, D), 9001, stride=st, frame=f5)], [0], 400),
             Call([row(400, (GOOD, GOOD, GOOD, D, D), 9002, stride=st, frame=f5)], [0], 500),
             Call([row(400, (GOOD, D), 9003, stride=st, frame=f2), row(400, (GOOD, D), 9004, stride=st, frame=f2)], [0, 1], [1500, 1001]),
             Call([row(400, (GOOD, D), 9005, stride=st, frame=f2)], [0], 2501)]
    return Scenario(2, 16, 1000, calls)


def claims_changing_header(hist, caches, snaps):
    key = (400, 0x123456, 0x654321)
    h = [hist[t][0][1] for t in range(5)]
    r = [hist[t][0][0] for t in range(5)]
    assert [x["header_total_cw"] for x in r] == [3, 5, 5, 2, 2] and [x["frame_type"] for x in r] == [0x30, 0x31, 0x31, 0x30, 0x30]
    assert [x["stored_mask"] for x in h] == [0b110, 0b110, 0, 0, 0b10] and [x["sum_mask"] for x in h] == [0, 0b110, 0, 0, 0]
    assert [x["max_combine"] for x in h] == [1, 2, 0, 2, 1]      # call 2: only codewords 3 and 4 fail, their count is 0; call 3: a decoded codeword keeps its count
    st = [snaps[t][0][0] for t in range(5)]
    assert st[1]["cache_misses"] - st[0]["cache_misses"] == 2 and st[2]["cache_misses"] - st[1]["cache_misses"] == 2   # the refused codewords miss
    assert st[2]["stores"] - st[1]["stores"] == 2 and st[2]["combines"] == st[1]["combines"] == 2
    e = [snaps[t][0][1][key] for t in range(5)]
    assert [(x["total_cw"], x["frame_type"]) for x in e] == [(3, 0x30)] * 4 + [(2, 0x30)]       # the entry keeps its first header
    assert [x["last_access"] for x in e] == [0, 400, 500, 1500, 2501]                           # 500: refused stores alone
    assert e[2]["decoded"][:3] == [0, 1, 1] and e[3]["count"][:3] == [0, 2, 2]
    assert [s["entries_expired"] for s in st] == [0, 0, 0, 0, 1]                                # kept at last + ttl, gone at 2501
    assert h[3]["stored_mask"] == 0 and st[3]["cache_misses"] - st[2]["cache_misses"] == 1
    # cache 1, without the touch: expired at 1001
    assert snaps[3][1][0]["entries_expired"] == 1 and snaps[3][1][1][key]["total_cw"] == 2 and hist[3][1][1]["stored_mask"] == 0b10


# ---- (d) time
def time_script():
    """the "time" scripts of tests/test_mcdpsk_harq_cpu.py as (max_entries, ttl, [(sequence number, now)]): one store per step"""
    return {"time_ttl0": (16, 0, [(0, 5), (1, 5), (2, 6), (3, 6), (4, 5), (5, 7)]),
            "time_ttl_max": (16, INT64_MAX, [(0, 0), (1, 2 ** 63 - 1), (2, 2 ** 63), (3, U64 - 1), (4, 0), (5, 2 ** 63)]),
            "time": (16, 1000, [(0, 2 ** 63 - 1), (1, 2 ** 63 - 1), (2, 2 ** 63), (3, U64 - 1), (4, 0), (5, 1000), (6, 1001),
                                (7, 0), (8, 2 ** 63), (9, 2 ** 63 + 1001), (10, 5), (11, U64 - 1)])}


TIME_SIZES = {"time_ttl0": [1, 2, 1, 2, 3, 1], "time_ttl_max": [1, 2, 3, 4, 5, 6],
              # 2^63: both kept (1 ms old).  2^64 - 1: 2^63 is 2^63 - 1 ms old and goes, 2^63 - 1 is INT64_MIN "old" and stays.
              # 0: one ms after 2^64 - 1.  1000: 0 is exactly ttl old, 2^64 - 1 is 1001 and goes.  1001: 0 goes.  0: earlier than
              # every last_access, nothing goes.  2^63 against last_access 0: the difference is INT64_MIN, it stays (an unbounded
              # subtraction would expire it); 1000 and 1001 go.  2^63 + 1001: 2^63 - 1 (twice) and 2^63 go.  5: 2^63 + 1001 goes,
              # 0 stays.  2^64 - 1 = 5 - 6: nothing goes.
              "time": [1, 2, 3, 3, 4, 4, 4, 5, 4, 2, 2, 3]}


def time_scenario(name):
    """a time script through the kernels, one row per call, one codeword stored per call"""
    max_entries, ttl, steps = time_script()[name]
    calls = [Call([row(500 + s, (GOOD, DEAD), 9100 + s, stride=2 * N, frame=frame_of(500 + s, 2))], [0], now) for s, now in steps]
    return Scenario(1, max_entries, ttl, calls)


def claims_time(name, hist, caches, snaps):
    assert [len(s[0][1]) for s in snaps] == TIME_SIZES[name], [len(s[0][1]) for s in snaps]
    assert all(out[0][1]["stored_mask"] == 2 for out in hist)
    assert snaps[-1][0][0]["entries_evicted"] == 0


def four_times():
    """four caches, two calls; the second has four different now_ms: row 0 later than ttl (expires), row 1 exactly ttl (kept),
    row 2 earlier than its cache's last_access (kept), row 3 at 2^64 - 1 (the difference is negative: kept)"""
    rows = lambda base: [row(520 + i, (GOOD, DEAD, GOOD), base + i) for i in range(4)]
    return Scenario(4, 16, 1000, [Call(rows(9200), [2, 0, 3, 1], 5000), Call(rows(9210), [2, 0, 3, 1], [6001, 6000, 10, U64 - 1])])


def claims_four_times(hist, caches, snaps):
    assert [snaps[1][c][0]["entries_expired"] for c in (2, 0, 3, 1)] == [1, 0, 0, 0]
    assert [snaps[1][c][0]["combines"] for c in (2, 0, 3, 1)] == [0, 1, 1, 1]
    assert [list(snaps[1][c][1].values())[0]["last_access"] for c in (2, 0, 3, 1)] == [6001, 6000, 10, U64 - 1]


def tie():
    """max_entries 2, every call at now_ms 50: A, B, A again (its order now follows B's), then C evicts B; a cache that
    ignored the order would take A, the first slot"""
    seqs = (540, 541, 540, 542)
    return Scenario(1, 2, 30000, [Call([row(s, (GOOD, DEAD, GOOD), 9300 + j)], [0], 50) for j, s in enumerate(seqs)])


def claims_tie(hist, caches, snaps):
    assert [keys_of(s[0]) for s in snaps] == [[540], [540, 541], [540, 541], [540, 542]]
    assert snaps[3][0][0]["entries_evicted"] == 1 and snaps[2][0][0]["combines"] == 1


# ---- (e) special values in sums
F = np.float32
INF, NAN, FMAX = F(np.inf), F(np.nan), np.finfo(np.float32).max
DMIN, DMAX = np.uint32(1).view(np.float32), np.uint32(0x007FFFFF).view(np.float32)      # the smallest and the largest denormal
# position in the codeword -> the value in receptions 0 .. 3
SPECIALS = {3: (INF, -INF, F(1), F(1)),             # inf + -inf = NaN, and it stays
            50: (FMAX, FMAX, FMAX, -FMAX),          # FLT_MAX + FLT_MAX = inf
            101: (DMIN, DMIN, DMIN, DMIN),          # denormal + denormal, not flushed
            152: (DMAX, -DMAX, F(0), F(0)),         # denormal + -denormal = +0
            203: (F(-0.0), F(-0.0), F(-0.0), F(-0.0)),   # -0.0 + -0.0 = -0.0
            254: (NAN, F(1), F(1), F(1)),
            305: (-FMAX, -FMAX, F(1), INF),         # -inf, then -inf + inf = NaN
            356: (F(1e30), F(1e30), F(1e30), F(1e30)),   # beyond the decoder's clamp
            407: (F(-1e30), F(1e30), DMIN, -DMIN),
            458: (DMAX, DMAX, DMAX, DMAX),          # denormals that add up to a normal number
            509: (-INF, -INF, -INF, -INF),
            560: (F(-1e30), F(-1e30), F(-1e30), F(-1e30))}
SPECIAL_SEEDS = (1, 0)


def special_row(seq, amps, seed, t, cws):
    x = row(seq, amps, seed)
    for c in cws:
        for p, v in SPECIALS.items():
            x[c * N + p] = v[t]
    return x


def special_values():
    """Three caches, four receptions.  Row 0: codeword 1 weak with the special values in it, received until the sum decodes.
    Row 1: codeword 2 dead with them, four times (its sums never decode).  Row 2: both codewords dead with them."""
    s0, s1 = SPECIAL_SEEDS
    calls = []
    for t in range(4):
        rows = [special_row(600, (GOOD, WEAK2, GOOD), 9400 + 10 * s0 + t, t, (1,)), special_row(601, (GOOD, GOOD, DEAD), 9500 + 10 * s1 + t, t, (2,)),
                special_row(602, (GOOD, DEAD, DEAD), 9600 + t, t, (1, 2))]
        calls.append(Call(rows, [0, 1, 2], 100 * t))
    return Scenario(3, 16, 30000, calls)


def claims_special_values(hist, caches, snaps):
    with np.errstate(all="ignore"):
        want = {p: [np.cumsum(np.asarray(v, np.float32), dtype=np.float32)[t] for t in range(4)] for p, v in SPECIALS.items()}
    # the sums hold what the rows are built for (cache 1, codeword 2, after receptions 2 and 4)
    e = lambda t: list(snaps[t][1][1].values())[0]["sums"][2]
    bits = lambda v: int(np.float32(v).view(np.uint32))
    assert np.isnan(e(1)[3]) and np.isnan(e(3)[3]) and bits(e(1)[50]) == bits(INF) and bits(e(3)[50]) == bits(INF)
    assert bits(e(1)[101]) == 2 and bits(e(3)[101]) == 4                          # denormal sums, kept
    assert bits(e(1)[152]) == 0 and bits(e(1)[203]) == 0x80000000 and bits(e(3)[203]) == 0x80000000
    assert np.isnan(e(3)[254]) and bits(e(1)[305]) == bits(-INF) and np.isnan(e(3)[305])
    assert bits(e(1)[407]) == 0 and bits(e(2)[407]) == 1 and bits(e(3)[407]) == 0
    assert bits(e(1)[458]) == 0x00FFFFFE and bits(e(1)[509]) == bits(-INF)
    for p in SPECIALS:
        for t in range(4):
            assert same_floats(e(t)[p], want[p][t]), (p, t)
    # a recovery from a sum with special values, and such sums that do not recover
    rec = [t for t in range(4) if hist[t][0][1]["recovered_mask"] == 2]
    assert rec and rec[0] >= 1 and hist[rec[0]][0][0]["success"] == 1
    assert [hist[t][1][1]["sum_mask"] for t in range(4)] == [0, 4, 4, 4] and all(hist[t][1][1]["recovered_mask"] == 0 for t in range(4))
    assert [hist[t][2][1]["sum_mask"] for t in range(4)] == [0, 6, 6, 6] and hist[3][2][1]["max_combine"] == 4
    x = canon(e(3))
    assert np.isfinite(x).all() and x[3] == F(1e30) and x[50] == F(1e30) and bits(x[203]) == 0


# ---- (f) sizes: a dozen row histories tiled over a big batch
def histories(T):
    """per-codeword amplitudes of the histories of a T-codeword frame: twelve that are tiled, then the few that are placed
    by hand (noise, a control frame, a row that n_llr cuts).  With T = 2 every tiled history fails its codeword in both
    receptions, so that all but a handful of rows list a sum in the second call."""
    G, W, D = GOOD, WEAK2, DEAD
    if T == 3:
        return [(G, W, G), (G, G, W), (G, D, G), (G, D, D), (G, W, W), (G, G, D), (G, W, D), (G, D, W), (G, D, D), (G, W, W), (G, G, G), (G, D, G),
                None, "ack", "cut"]
    return [(G, W), (G, D), (G, W), (G, D), (G, W), (G, W), (G, D), (G, W), (G, D), (G, W), (G, D), (G, W), None]


TILED = {3: dict(n=1100, placed={100: 12, 1023: 13, 1030: 14}, off=(5, 1024, 1099)),
         2: dict(n=16388, placed={16385: 12}, off=(7, 16386))}


def history_rows(T, t):
    """reception t of the histories of histories(T): rows [k, T * 648] and their n_llr"""
    rows, n_llr = [], []
    for j, a in enumerate(histories(T)):
        seed = 9700 + 100 * T + 20 * t + j
        if a is None:
            rows.append(np.random.default_rng(seed).standard_normal(T * N).astype(np.float32))
        elif a == "ack":
            rows.append(row(0, (GOOD,), seed, stride=T * N, frame=control_frame(ACK, 700 + j)))
        else:
            rows.append(row(700 + j, (GOOD,) * T if a == "cut" else a, seed, stride=T * N, frame=frame_of(700 + j, T)))
        n_llr.append(T * N - 1 if a == "cut" else T * N)
    return np.stack(rows), n_llr


def tiled_map(T, n=None):
    """the history of each of the batch's rows: the twelve in turn, and the placed ones"""
    n = TILED[T]["n"] if n is None else n
    m = np.arange(n) % 12
    for i, j in TILED[T]["placed"].items():
        if i < n:
            m[i] = j
    return m


def tiled_ids(T, n=None, n_caches=None):
    """a fixed permutation of the cache ids that is not the identity, with the chase of a few rows off"""
    n = TILED[T]["n"] if n is None else n
    n_caches = n if n_caches is None else n_caches
    ids = (np.arange(n, dtype=np.int64) * 7919 + 11) % n_caches
    assert n <= n_caches and len(set(ids.tolist())) == n and not np.array_equal(ids, np.arange(n))
    for i in TILED[T]["off"]:
        if i < n:
            ids[i] = -1
    return ids.astype(np.int32)


class Tiled:
    """the restatement of a tiled batch: once per history and reception, with a cache (max_entries 1) and without"""

    def __init__(self, T):
        self.T, self.k = T, len(histories(T))
        self.caches = [ChaseCache(1, 30000) for _ in range(self.k)]

    def step(self, t):
        """reception t -> (rows [k, T * 648], n_llr, want[with cache][history] = (r, h))"""
        rows, n_llr = history_rows(self.T, t)
        off = [restate(rows[j][:n_llr[j]], None, 0) for j in range(self.k)]
        on = [restate(rows[j][:n_llr[j]], self.caches[j], 1000 * t) for j in range(self.k)]
        return rows, n_llr, (off, on)


def claims_tiled(T, want0, want1):
    """what the two receptions of the histories must hold -> (round-B rows, sums listed in the second call) of the batch"""
    first, second = [h for _, h in want0[1]], [h for _, h in want1[1]]
    assert not any(h["sum_mask"] for h in first)
    assert sum(1 for h in second[:12] if h["recovered_mask"]) >= 3 and sum(1 for h in second[:12] if h["sum_mask"] and not h["recovered_mask"]) >= 3
    assert first[12]["valid"] == 0 and want0[1][12][0]["codewords_ok"] == 0                   # noise
    if T == 3:
        assert first[10]["valid"] == 1 and first[10]["stored_mask"] == 0 and want0[1][10][0]["success"] == 1
        assert want0[1][13][0]["header_total_cw"] == 1 and want0[1][14][0]["header_total_cw"] == 3 and len(want0[1][14][0]["frame"]) == 20
    else:
        assert all(h["stored_mask"] == 2 for h in first[:12]) and all(h["sum_mask"] == 2 for h in second[:12])
    m, ids = tiled_map(T), tiled_ids(T)
    rows_b = sum((T - 1) for i in range(len(m)) if want0[1][m[i]][0]["header_total_cw"] == T and m[i] != 14)
    sums = sum(bin(second[m[i]]["sum_mask"]).count("1") for i in range(len(m)) if ids[i] >= 0)
    return rows_b, sums


# ---- (h) ria_gpu_chase_combine_batch
def combine_inputs(n):
    """n codeword slots: counts 0 .. 4 in turn, every third of the rest decoded, Gaussian sums and soft bits with the special
    values of (e) laid over them -> (acc, count, decoded, soft)"""
    rng = np.random.default_rng(9900 + n)
    acc, soft = rng.standard_normal((n, N)).astype(np.float32), rng.standard_normal((n, N)).astype(np.float32)
    count = (np.arange(n) % 5).astype(np.int32)
    decoded = ((np.arange(n) // 5) % 3 == 2).astype(np.uint8)
    for p, v in SPECIALS.items():
        for k in range(4):
            acc[k::8, p + k], soft[k::8, p + k] = v[k], v[(k + 1) % 4]
            acc[k + 4::8, p + k], soft[k + 4::8, p + k] = v[(k + 1) % 4], v[k]
    return acc, count, decoded, soft


def combine_expect(acc, count, decoded, soft):
    """ChaseCache::store's arithmetic: refused when decoded or at MAX_COMBINES, a copy at count 0, else one float add"""
    stored = (decoded == 0) & (count < 4) if decoded is not None else count < 4
    with np.errstate(all="ignore"):
        out = np.where(stored[:, None], np.where((count == 0)[:, None], soft, acc + soft), acc).astype(np.float32)
    return out, np.where(stored, count + 1, count).astype(np.int32), stored.astype(np.uint8)


# ---- (i) interleaved sums
CI_WIDTHS = (1, 215, 216, 647, 648)      # findCoprimeStep changes branch at 3 * B >= 648: 215 | 216
CI_SEEDS = {1: 1, 215: 0, 216: 0, 647: 0, 648: 0}


def interleaved(B):
    """Two caches, three receptions through the channel-interleaving call at width B.  Cache 0: a 3-codeword frame,
    interleaved, codeword 1 weak until the sum recovers it, codeword 2 dead.  Cache 1: a 16-codeword frame, interleaved,
    codewords 5 and 15 weak, then whole."""
    s = CI_SEEDS[B]
    W16 = tuple(WEAK2 if c in (5, 15) else GOOD for c in range(16))
    calls = []
    for t in range(3):
        a3 = (GOOD, WEAK2 if t < 2 else GOOD, DEAD)
        rows = [row(800, a3, 9800 + 10 * s + t, stride=S16, il=B), row(801, W16 if t < 2 else (GOOD,) * 16, 9850 + 10 * s + t, stride=S16, frame=frame_of(801, 16), il=B)]
        calls.append(Call(rows, [0, 1], 1000 * t, n_llr=[3 * N, S16], B=B))
    return Scenario(2, 16, 30000, calls)


def claims_interleaved(B, hist, caches, snaps):
    r = lambda t, i: hist[t][i][0]
    h = lambda t, i: hist[t][i][1]
    assert all(r(t, i)["cw0_deinterleaved"] == 1 for t in range(3) for i in range(2))
    assert h(0, 0)["stored_mask"] == 6 and h(1, 0)["sum_mask"] == 6 and h(1, 0)["recovered_mask"] == 2 and h(2, 0)["sum_mask"] == 4
    assert h(0, 1)["stored_mask"] == 0x8020 and h(1, 1)["recovered_mask"] == 0x8020 and r(1, 1)["success"] == 1 and h(1, 1)["entry"] == REMOVED
    assert r(2, 1)["success"] == 1 and len(r(2, 1)["frame"]) == 290
