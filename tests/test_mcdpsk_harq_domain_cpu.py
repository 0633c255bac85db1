"""CPU: every scenario of tests/mcdpsk_harq_domain_inputs.py on the restatement alone (tests/mcdpsk_harq_restatement.py on the
oracle's robust decoder), asserting that it reaches what tests/test_gpu_mcdpsk_harq_domain.py runs it for: which codeword is
stored, summed and recovered in which call, which key is evicted or expired, which sum holds a NaN.  The R1/4 robust decoder
can converge on noise, so a seed that stops producing its scenario fails here, on the CPU, and not quietly on the GPU."""
import numpy as np
import pytest

import mcdpsk_harq_domain_inputs as I
from mcdpsk_harq_restatement import ChaseCache, age_ms, canon


def test_age_is_the_difference_modulo_2_64_read_as_int64():
    M = 2 ** 63
    assert [age_ms(n, l) for n, l in ((5, 3), (3, 5), (M, 0), (M - 1, 0), (0, M), (0, 2 ** 64 - 1), (2 ** 64 - 1, 0), (M + 1, 1))] == \
           [2, -2, -M, M - 1, -M, 1, -1, -M]
    c = ChaseCache(16, 1000)
    key = (1, 2, 3)
    assert c.store(key, 1, np.zeros(648, np.float32), 3, 0x30, 0)
    assert c.store((2, 2, 3), 1, np.zeros(648, np.float32), 3, 0x30, M) and c.size() == 2        # INT64_MIN is not above ttl
    assert c.store((3, 2, 3), 1, np.zeros(648, np.float32), 3, 0x30, M - 1) and c.size() == 2     # 2^63 - 1 is: the first entry goes


def test_canon_is_the_decoders_input_mapping():
    from ldpc_domain_inputs import canon as ldpc_canon
    x = np.array([np.nan, -np.nan, np.inf, -np.inf, 3e38, -3e38, 1e30, -0.0, 0.0, I.DMIN, -I.DMAX, 1.5], np.float32)
    assert np.array_equal(canon(x).view(np.uint32), ldpc_canon(x).view(np.uint32))
    want = np.array([1e30, 1e30, 1e30, -1e30, 1e30, -1e30, 1e30, 0.0, 0.0, I.DMIN, -I.DMAX, 1.5], np.float32)
    assert np.array_equal(canon(x).view(np.uint32), want.view(np.uint32))


def test_sixteen_codewords():
    I.claims_sixteen(*I.replay(I.sixteen()))


@pytest.mark.parametrize("max_entries", [1, 2])
def test_slot_reuse(max_entries):
    scn = I.slot_reuse(max_entries)
    I.claims_slot_reuse(max_entries, scn, *I.replay(scn))


def test_changing_header():
    I.claims_changing_header(*I.replay(I.changing_header()))


@pytest.mark.parametrize("name", sorted(I.TIME_SIZES))
def test_time_scripts(name):
    I.claims_time(name, *I.replay(I.time_scenario(name)))


def test_four_times_in_one_call_and_the_tie():
    I.claims_four_times(*I.replay(I.four_times()))
    I.claims_tie(*I.replay(I.tie()))


def test_special_values():
    I.claims_special_values(*I.replay(I.special_values()))


@pytest.mark.parametrize("T", [3, 2])
def test_tiled_histories(T):
    """the two big batches: what their histories do, how many round-B rows the batch has and how many sums its second call
    lists"""
    tl = I.Tiled(T)
    _, _, w0 = tl.step(0)
    _, _, w1 = tl.step(1)
    rows_b, sums = I.claims_tiled(T, w0, w1)
    m, ids = I.tiled_map(T), I.tiled_ids(T)
    if T == 3:
        assert len(m) == 1100 and rows_b > 2048 and sums > 1024             # three scan chunks, a list longer than one chunk
        flagged = np.repeat([bool(w1[1][j][1]["sum_mask"]) for j in m], 1)
        for lo, hi in ((1000, 1024), (1024, 1100)):                        # codeword rows 2000 .. 2200: on both sides of 2048
            assert flagged[lo:hi].any() and not flagged[lo:hi].all()
        assert flagged[:500].any() and not flagged[:500].all() and flagged[520:1000].any() and not flagged[520:1000].all()   # and of 1024
    else:
        assert len(m) == 16388 and rows_b > 16384 and sums > 16384          # the 4096-block stride loops run twice
        assert ids[16387] >= 0 and m[16387] < 12 and ids[16384] >= 0
    assert (ids < 0).sum() == len(I.TILED[T]["off"])


@pytest.mark.parametrize("B", I.CI_WIDTHS)
def test_interleaved_sums(B):
    I.claims_interleaved(B, *I.replay(I.interleaved(B)))
    from mcdpsk_ci_restatement import coprime_step
    assert [coprime_step(b) for b in I.CI_WIDTHS] == [5, 647, 325, 325, 325]      # both branches of findCoprimeStep


def test_combine_expectation_is_store_arithmetic():
    """combine_expect against ChaseCache.store, slot by slot"""
    acc, count, decoded, soft = I.combine_inputs(40)
    out, cnt, stored = I.combine_expect(acc, count, decoded, soft)
    for i in range(40):
        c = ChaseCache()
        key = (i, 1, 2)
        if count[i]:
            c.store(key, 1, acc[i], 2, 0x30, 0)
            c.cache[key].count[1] = int(count[i])
        if decoded[i]:
            c.store(key, 0, acc[i], 2, 0x30, 0)
            c.cache[key].decoded[1] = True
        with np.errstate(all="ignore"):
            ok = c.store(key, 1, soft[i], 2, 0x30, 0)
        assert ok == bool(stored[i]), i
        if ok:
            assert I.same_floats(c.cache[key].soft[1], out[i]) and c.cache[key].count[1] == cnt[i], i
        else:
            assert I.same_floats(out[i], acc[i]) and cnt[i] == count[i]
    assert stored.sum() not in (0, 40) and {0, 1, 2, 3, 4} <= set(count.tolist())
