"""GPU tests of the device-resident HARQ chase pool over its input domain: ria_gpu_chase_create .. _export and the chase stages
of ria_gpu_mcdpsk_decode_frame_batch / _ci_batch (ria_amd/csrc/mcdpsk_harq_kernels.hip.h), and ria_gpu_chase_combine_batch,
against the CPU restatement (tests/mcdpsk_harq_restatement.py on the oracle's robust decoder).  Every comparison is
bit-exact: the DecodeResult fields, the frame bytes, the harq record, the seven counters of a cache and its exported entries
and sums.  The one relaxation is the header's: where the restatement's sum is NaN the device's is NaN, sign and payload not
compared.

The scenarios are those of tests/mcdpsk_harq_domain_inputs.py; what each of them reaches is asserted on the restatement in
tests/test_mcdpsk_harq_domain_cpu.py, and again here on what the device was compared with."""
import ctypes as C

import numpy as np
import pytest
import torch

import mcdpsk_harq_domain_inputs as I
from mcdpsk_harq_domain_inputs import DEAD, GOOD, HARQ_FIELDS, N, RES_FIELDS, Links, compare_cache, row
from mcdpsk_harq_restatement import STATS

pytestmark = pytest.mark.gpu
ZERO_STATS = dict.fromkeys(STATS, 0)


@pytest.fixture(scope="module")
def eng():
    from ria_amd.engine import RxEngine
    e = RxEngine("DQPSK", "R1_4", max_batch=64)
    yield e
    e.close()


def run(eng, scn):
    """the scenario through the device and the restatement, compared call by call -> (hist, caches, snaps) as replay() gives"""
    L = scn.links(eng)
    try:
        return L.run(scn)
    finally:
        L.close()


# ---- a. sixteen codewords
def test_sixteen_codewords_three_caches_and_a_full_cache(eng):
    """llr_stride 16 * 648, frame_row 320: every codeword index 1 .. 15 stored, summed and recovered (bit 15 in the three
    masks), cache 2 filled to 16 entries x 16 codewords (the last float of its sum area), cache 1 used only by rows that n_llr
    cuts (at 15 codewords and at 16 * 648 - 1) and all-zero to the end, the neighbours compared after every call"""
    I.claims_sixteen(*run(eng, I.sixteen()))


# ---- b. slot reuse
@pytest.mark.parametrize("max_entries", [1, 2])
def test_a_new_key_in_a_used_slot_copies_first(eng, max_entries):
    """after an eviction, an expiry, a removal on full success and a clear: another total_cw in the slot, the first store of a
    codeword that had a sum in the old entry is a copy, the export is zero where has_sum is 0, counts and flags start fresh"""
    scn = I.slot_reuse(max_entries)
    I.claims_slot_reuse(max_entries, scn, *run(eng, scn))


# ---- c. one key, changing header
def test_one_key_with_a_changing_header(eng):
    """total_cw 3, then 5, then 2 and another frame type under one key: refused stores, misses and zero counts; the entry keeps
    its first header; refused stores alone refresh last_access (kept at last + ttl, expired 1 ms later without them)"""
    I.claims_changing_header(*run(eng, I.changing_header()))


# ---- d. time
@pytest.mark.parametrize("name", sorted(I.TIME_SIZES))
def test_time_scripts_through_the_kernels(eng, name):
    """ttl 0, ttl INT64_MAX, now_ms around 2^63 and 2^64 - 1: the scripts that tests/test_mcdpsk_harq_cpu.py runs on
    chase_policy.hpp, one row per call"""
    I.claims_time(name, *run(eng, I.time_scenario(name)))


def test_four_times_in_one_call_and_the_order_tie_break(eng):
    I.claims_four_times(*run(eng, I.four_times()))
    I.claims_tie(*run(eng, I.tie()))


# ---- e. special values
def test_special_values_are_summed_raw_and_decoded_canonical(eng):
    """NaN, +-inf, +-FLT_MAX, +-1e30, the smallest and largest denormal and -0.0 in failing codewords, received four times:
    inf + -inf, overflow to inf, denormal sums, +0 and -0.0 in the exported sums, bit for bit; the decodes of the sums are the
    restatement's on canon(sum)"""
    I.claims_special_values(*run(eng, I.special_values()))


# ---- f. sizes
def tiled_call(eng, pool, rows_k, n_llr_k, m, ids, now):
    rows = torch.from_numpy(rows_k)[torch.from_numpy(m)].contiguous().to(eng.device)
    frames, res, hq = eng.mcdpsk_decode_frame(rows, n_llr=np.ascontiguousarray(np.asarray(n_llr_k, np.int32)[m]), chase=pool, cache_id=ids, now_ms=now)
    return frames.cpu().numpy(), res, hq


def check_tiled(frames, res, hq, want, m, ids):
    """every row's outputs against its history's, with a cache or without"""
    seen = 0
    for on in (0, 1):
        for j, (r, h) in enumerate(want[on]):
            sel = (m == j) & ((ids >= 0) == bool(on))
            if not sel.any():
                continue
            seen += int(sel.sum())
            for f in RES_FIELDS:
                assert (res[f][sel] == int(r[f])).all(), (on, j, f)
            nb = len(r["frame"])
            assert (res["frame_bytes"][sel] == nb).all() and (frames[sel, :nb] == r["frame"]).all() and not frames[sel, nb:].any(), (on, j)
            for f in HARQ_FIELDS:
                assert (hq[f][sel] == int(h[f])).all(), (on, j, f)
            assert (hq["cache_id"][sel] == (ids[sel] if h["valid"] else 0)).all(), (on, j)
    assert seen == len(m)


def tiled_batch(eng, T, near):
    """two receptions of the tiled batch of T-codeword rows; the caches of the rows listed in `near` compared after each"""
    n = I.TILED[T]["n"]
    m, ids = I.tiled_map(T), I.tiled_ids(T)
    tl = I.Tiled(T)
    pool = eng.chase_pool(n, 1, 30000)
    wants = []
    try:
        for t in range(2):
            rows_k, n_llr_k, want = tl.step(t)
            frames, res, hq = tiled_call(eng, pool, rows_k, n_llr_k, m, ids, 1000 * t)
            check_tiled(frames, res, hq, want, m, ids)
            wants.append(want)
            for i in near:
                if ids[i] >= 0:
                    compare_cache(pool, int(ids[i]), tl.caches[m[i]])
            unused = sorted(set(range(n)) - set(ids.tolist()))
            assert len(unused) == len(I.TILED[T]["off"]) and all(pool.stats(c) == ZERO_STATS and pool.export(c)[0].size == 0 for c in unused)
    finally:
        pool.close()
    return I.claims_tiled(T, wants[0], wants[1])


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_one_to_five_rows(eng, n):
    """four waves per block: a block of one, three, four waves and a second block"""
    L = Links(eng, 8, 1)
    tl = I.Tiled(3)
    order = [3, 0, 10, 4, 6][:n]                       # histories that store, recover, decode at once
    for t in range(2):
        rows_k, n_llr_k, _ = tl.step(t)
        L.call([rows_k[j] for j in order], [7, 2, 5, 0, 3][:n], 1000 * t, n_llr=[n_llr_k[j] for j in order])
    assert sum(c.stats["stores"] for c in L.caches) >= n
    L.close()


def test_1100_rows_of_three_codewords(eng):
    """more than 2048 round-B rows: three chunks of the one-block scan with a carried count, flagged and unflagged rows on
    both sides of 1024 and 2048, a list of more than 1024 sums"""
    near = list(range(12)) + list(range(505, 520)) + list(range(1016, 1034)) + list(range(1088, 1100))
    rows_b, sums = tiled_batch(eng, 3, near)
    assert rows_b > 2048 and sums > 1024


def test_16388_rows_of_two_codewords(eng):
    """the smallest batch at which the 4096-block stride loops of the store, resolve and finish stages run twice; a pool of
    16 388 caches of one entry; the second call gathers more than 16 384 sums"""
    near = list(range(12)) + list(range(4090, 4102)) + list(range(16376, 16388))
    rows_b, sums = tiled_batch(eng, 2, near)
    assert rows_b > 16384 and sums > 16384


def test_workspaces_grow_between_calls_on_one_handle():
    """a fresh handle: five rows, then the 1100-row batch (both receptions), then five rows again, on pools of that handle:
    every call equals the restatement, as the calls on the module's handle do"""
    from ria_amd.engine import RxEngine
    e = RxEngine("DQPSK", "R1_4", max_batch=64)
    try:
        L = Links(e, 8, 1)
        small = I.Tiled(3)
        order, ids = [3, 0, 10, 4, 6], [7, 2, 5, 0, 3]
        rows_k, n_llr_k, _ = small.step(0)
        L.call([rows_k[j] for j in order], ids, 0, n_llr=[n_llr_k[j] for j in order])
        tiled_batch(e, 3, list(range(12)) + list(range(1020, 1030)))
        rows_k, n_llr_k, _ = small.step(1)
        out = L.call([rows_k[j] for j in order], ids, 1000, n_llr=[n_llr_k[j] for j in order])
        assert any(h["sum_mask"] for _, h in out)
        L.close()
    finally:
        e.close()


# ---- g. refusals
def stored_links(eng, n_caches):
    """a pool with something in caches 0, 1 and the last one"""
    L = Links(eng, n_caches)
    L.call([row(900 + i, (GOOD, DEAD, GOOD), 9950 + i) for i in range(3)], [0, 1, n_caches - 1], 5, compare=[0, 1, n_caches - 1])
    assert all(L.caches[c].size() == 1 for c in (0, 1, n_caches - 1))
    return L


def test_refused_calls_leave_every_cache_unchanged(eng):
    """a duplicate id whose rows sit in different claim blocks (rows 0 and 300), id == n_caches, a pool of another handle:
    RIA_ERR_INVALID, and every cache as before.  Negative ids other than -1 turn chase off for the row, as -1 does."""
    from ria_amd.capi import RiaError
    from ria_amd.engine import RxEngine
    n = 301
    L = stored_links(eng, n)
    base = np.stack([row(900 + i, (GOOD, DEAD, DEAD), 9960 + i) for i in range(3)])
    rows = torch.from_numpy(base[np.arange(n) % 3]).to(eng.device)
    dup = np.arange(n, dtype=np.int32)
    dup[300] = 0
    top = np.arange(n, dtype=np.int32)
    top[150] = n
    for ids in (dup, top):
        with pytest.raises(RiaError, match="status -1"):
            eng.mcdpsk_decode_frame(rows, chase=L.pool, cache_id=ids, now_ms=9)
        L.compare_caches()
    e2 = RxEngine("DQPSK", "R1_4", max_batch=64)
    try:
        other = e2.chase_pool(n)
        with pytest.raises(RiaError, match="status -1"):
            eng.mcdpsk_decode_frame(rows, chase=other, cache_id=np.arange(n, dtype=np.int32), now_ms=9)
        assert all(other.stats(c) == ZERO_STATS for c in (0, 1, 300))
        L.compare_caches()
        other.close()
    finally:
        e2.close()
    # negative ids: chase off
    neg = [-2, -2, -2 ** 31]
    f0, r0, _ = eng.mcdpsk_decode_frame(rows[:3].contiguous())
    f1, r1, h1 = eng.mcdpsk_decode_frame(rows[:3].contiguous(), chase=L.pool, cache_id=neg, now_ms=9)
    assert torch.equal(f0, f1) and r0.tobytes() == r1.tobytes() and not h1.view(np.uint8).any() and [int(v) for v in r0["codewords_failed"]] == [2, 2, 2]
    L.compare_caches()
    L.call(list(base), [0, -5, 300], 9, compare=[0, 1, 300])         # through the restatement too: the row without a cache fails alone
    assert L.caches[0].stats["combines"] == 1 and L.caches[300].stats["combines"] == 1 and L.caches[1].stats["stores"] == 1
    L.close()


def test_clear_stats_and_export_arguments(eng):
    from ria_amd.capi import RiaError, ChaseEntry, ChaseStats
    lib = eng.lib
    L = stored_links(eng, 4)
    ids = torch.tensor([1, 1, 9, -1, -7, 4, 1], dtype=torch.int32, device=eng.device)        # repeated and out of range
    one = torch.tensor([0], dtype=torch.int32, device=eng.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.ria_gpu_chase_clear(L.pool.p, C.c_void_p(one.data_ptr()), 0, stream) == 0           # n 0: nothing
    L.compare_caches()
    assert lib.ria_gpu_chase_clear(L.pool.p, C.c_void_p(one.data_ptr()), -1, stream) == -1         # n < 0 with a list
    L.pool.clear([])
    L.compare_caches()
    assert lib.ria_gpu_chase_clear(L.pool.p, C.c_void_p(ids.data_ptr()), ids.numel(), stream) == 0
    L.caches[1].clear()
    L.compare_caches()
    assert L.caches[0].size() == 1 and L.caches[3].size() == 1 and L.pool.export(1)[0].size == 0
    assert lib.ria_gpu_chase_clear(L.pool.p, None, -3, stream) == 0                                # NULL list: every cache, n ignored
    for c in L.caches:
        c.clear()
    L.compare_caches()
    assert all(c.stats["stores"] == 1 for c in (L.caches[0], L.caches[3]))                         # counters stay
    # on a stream, between two calls
    s = torch.cuda.Stream()
    rows = [row(910 + i, (GOOD, DEAD, GOOD), 9970 + i) for i in range(2)]
    with torch.cuda.stream(s):
        L.call(rows, [2, 3], 20)
        L.clear([3])
        out = L.call(rows, [2, 3], 30)
    assert [h["sum_mask"] for _, h in out] == [2, 0]
    # stats and export: ids outside the pool, NULL outputs
    st = ChaseStats()
    for c in (-1, 4, 2 ** 31 - 1):
        assert lib.ria_gpu_chase_stats(L.pool.p, c, C.byref(st)) == -1 and lib.ria_gpu_chase_export(L.pool.p, c, None, None) == -1
        with pytest.raises(RiaError):
            L.pool.stats(c)
    assert lib.ria_gpu_chase_stats(L.pool.p, 0, None) == -1
    assert lib.ria_gpu_chase_export(L.pool.p, 2, None, None) == 1 and lib.ria_gpu_chase_export(L.pool.p, 1, None, None) == 0   # the count is still returned
    ent = (ChaseEntry * 16)()
    assert lib.ria_gpu_chase_export(L.pool.p, 2, C.cast(ent, C.c_void_p), None) == 1 and ent[0].seq == 910 and ent[0].combine_count[1] == 2
    L.compare_caches()
    L.close()


# ---- h. ria_gpu_chase_combine_batch
@pytest.mark.parametrize("n", [0, 1, 4097])
def test_chase_combine_batch(eng, n):
    """counts preset to 0 .. 4, decoded flags, the special values of (e), with and without decoded_dev and stored_out_dev,
    against ChaseCache::store's arithmetic in NumPy"""
    from ria_amd.engine import _ptr, _stream_ptr
    acc, count, decoded, soft = I.combine_inputs(n)
    dev = lambda x: torch.from_numpy(x.copy()).to(eng.device)
    for use_decoded in (True, False):
        want_acc, want_count, want_stored = I.combine_expect(acc, count, decoded if use_decoded else None, soft)
        a, c = dev(acc), dev(count)
        stored = eng.chase_combine(a, c, dev(soft), dev(decoded) if use_decoded else None).cpu().numpy()
        assert I.same_floats(a.cpu().numpy(), want_acc) and np.array_equal(c.cpu().numpy(), want_count) and np.array_equal(stored, want_stored)
        a2, c2, d2, s2 = dev(acc), dev(count), dev(decoded), dev(soft)    # stored_out_dev NULL
        eng._check(eng.lib.ria_gpu_chase_combine_batch(eng.h, _ptr(a2), _ptr(c2), _ptr(d2) if use_decoded else None, _ptr(s2), n, None, _stream_ptr()))
        assert I.same_floats(a2.cpu().numpy(), want_acc) and np.array_equal(c2.cpu().numpy(), want_count)
    if n > 1:
        assert want_stored.any() and not want_stored.all()


def test_chase_combine_counts_outside_0_to_4(eng):
    """what the call does with a count it never produces: above 4 refused like 4, below 0 added like 1 .. 3 (include/ria_gpu.h)"""
    acc, _, _, soft = I.combine_inputs(6)
    count = np.array([5, 2 ** 31 - 1, -1, -3, -2 ** 31, 4], np.int32)
    a, c = torch.from_numpy(acc.copy()).to(eng.device), torch.from_numpy(count.copy()).to(eng.device)
    stored = eng.chase_combine(a, c, torch.from_numpy(soft).to(eng.device)).cpu().numpy()
    with np.errstate(all="ignore"):
        want = np.where(np.array([0, 0, 1, 1, 1, 0], bool)[:, None], acc + soft, acc).astype(np.float32)
    assert stored.tolist() == [0, 0, 1, 1, 1, 0] and c.cpu().numpy().tolist() == [5, 2 ** 31 - 1, 0, -2, -2 ** 31 + 1, 4]
    assert I.same_floats(a.cpu().numpy(), want)


# ---- i. interleaved sums
@pytest.mark.parametrize("B", I.CI_WIDTHS)
def test_interleaved_sums(eng, B):
    """ria_gpu_mcdpsk_decode_frame_ci_batch at the widths where findCoprimeStep changes branch (215 | 216) and at its ends, a
    3-codeword and a 16-codeword frame: the exported sums are raw, the gathered sums decode as the restatement's
    de-interleaved ones"""
    scn = I.interleaved(B)
    hist, caches, snaps = run(eng, scn)
    I.claims_interleaved(B, hist, caches, snaps)
    e = list(snaps[0][0][1].values())[0]
    assert np.array_equal(e["sums"][1].view(np.uint32), scn.calls[0].rows[0][N:2 * N].view(np.uint32))      # raw, as received
