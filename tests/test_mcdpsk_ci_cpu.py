"""CPU: MC-DPSK channel interleaving without a GPU.

(a) the permutation of tests/mcdpsk_ci_restatement.py against the reference's recorded tables, and its inverse;
(b) with the mode off the restatement is mcdpsk_harq_restatement.decode_mcdpsk_frame;
(c) the ABI of the three new calls: symbols, prototypes in the header, a NULL handle;
(d) the row and window recipes of tests/test_gpu_mcdpsk_ci.py do, on the restatement, what that file says they do (the
    robust decoder at R1/4 can converge on noise, so this is asserted and not assumed)."""
import os

import numpy as np
import pytest

import pyoracle as po
import mcdpsk_ci_inputs as I
from mcdpsk_acquire_restatement import ACK, CONNECT, control_frame, data_frame, encode_frame, window
from mcdpsk_ci_restatement import acquire_window_ci, coprime_step, decode_mcdpsk_frame_ci, deinterleave, interleave_bytes, permutation
from mcdpsk_harq_restatement import ChaseCache, cache_snapshot, decode_mcdpsk_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- (a)
def test_permutation_equals_the_recorded_tables_and_inverts(golden):
    g = golden("channel_interleaver")
    x = np.arange(648, dtype=np.float32)
    for B in (10, 20):
        assert np.array_equal(deinterleave(x, B).astype(np.int64), g[f"inv_{B}"])       # deinterleave(x)[i] = x[(i * step) % 648]
    assert (coprime_step(10), coprime_step(20)) == (31, 61)
    rng = np.random.default_rng(7)
    for B in (1, 10, 20, 40, 215, 216, 648):
        p = permutation(B)
        assert sorted(p.tolist()) == list(range(648)), B
        coded = rng.integers(0, 256, (5, 81), dtype=np.uint8)
        soft = 1.0 - 2.0 * np.unpackbits(interleave_bytes(coded, B), axis=1).astype(np.float32)
        for r in range(5):
            assert np.array_equal(deinterleave(soft[r], B), 1.0 - 2.0 * np.unpackbits(coded[r]).astype(np.float32)), B
    assert np.array_equal(interleave_bytes(coded.reshape(-1), 20), interleave_bytes(coded, 20).reshape(-1))
    assert not np.array_equal(interleave_bytes(coded, 10), interleave_bytes(coded, 20))


# ---- (b)
def test_mode_off_is_the_harq_restatement(oracle):
    rows, n_llr, ids, _ = I.decode_rows(10)
    rows = rows + [I.row(I.data3(5), (I.GOOD, I.DEAD, I.GOOD), 900 + t) for t in range(2)]
    n_llr = n_llr + [1944, 1944]
    ids = ids + [0, 0]
    a, b = [ChaseCache() for _ in range(10)], [ChaseCache() for _ in range(10)]
    for i, (x, n) in enumerate(zip(rows, n_llr)):
        r0, h0 = decode_mcdpsk_frame(oracle, x[:n], a[ids[i]] if ids[i] >= 0 else None, 10 * i)
        r1, h1 = decode_mcdpsk_frame_ci(oracle, x[:n], None, b[ids[i]] if ids[i] >= 0 else None, 10 * i)
        assert (r1.pop("cw0_deinterleaved"), r1.pop("ci_tried")) == (0, 0)
        assert np.array_equal(r0.pop("frame"), r1.pop("frame")) and r0 == r1 and h0 == h1, i
    for ca, cb in zip(a, b):
        sa, sb = cache_snapshot(ca), cache_snapshot(cb)
        assert ca.stats == cb.stats and sa.keys() == sb.keys()
        assert all(np.array_equal(sa[k]["sums"], sb[k]["sums"]) for k in sa)
    assert a[0].stats["combines"] == 1


# ---- (c)
def test_ci_abi_symbols_prototypes_and_null_handle():
    from ria_amd import capi
    L = capi.load()
    header = open(os.path.join(ROOT, "include", "ria_gpu.h")).read()
    for name in ("ria_gpu_mcdpsk_decode_frame_ci_batch", "ria_gpu_mcdpsk_acquire_ci_batch", "ria_gpu_mcdpsk_interleave_batch"):
        assert getattr(L, name) is not None and name in capi.EXPORTS and ("int %s(" % name) in header
    assert L.ria_gpu_mcdpsk_decode_frame_ci_batch(None, None, 648, None, 0, None, None, None, None, 20, None, None, 8, 10, None) == -1
    assert L.ria_gpu_mcdpsk_acquire_ci_batch(None, None, None, 0, 0, 0, 0, 1, None, 8, None, None, None, 0, None, None, None, None, 10, None) == -1
    assert L.ria_gpu_mcdpsk_interleave_batch(None, 10, None, 0, None, None) == -1
    from ria_amd.engine import RxEngine
    for f in ("mcdpsk_interleave", "mcdpsk_decode_frame", "mcdpsk_acquire"):
        assert hasattr(RxEngine, f)


# ---- (d)
@pytest.mark.parametrize("B", [10, 20])
def test_decode_rows_do_what_they_are_meant_to(oracle, B):
    rows, n_llr, ids, want = I.decode_rows(B)
    for i, (x, n) in enumerate(zip(rows, n_llr)):
        r, _ = decode_mcdpsk_frame_ci(oracle, x[:n], B, ChaseCache() if ids[i] >= 0 else None, 0)
        assert I.outcome(r) == want[i], (i, I.outcome(r), want[i])
    base, order = I.boundary_rows(B)
    assert [I.outcome(decode_mcdpsk_frame_ci(oracle, x, B)[0]) for x in base] == I.BOUNDARY_WANT
    assert len(order) == 1030 and set(order[:1024]) == set(range(8)) and set(order[1024:]) >= {0, 1, 2, 3}


@pytest.mark.parametrize("B", [10, 20])
def test_chase_rows_do_what_they_are_meant_to(oracle, B):
    caches = [ChaseCache() for _ in range(4)]
    hist = []
    for t, (rows, ids) in enumerate(I.chase_calls(B)):
        hist.append([decode_mcdpsk_frame_ci(oracle, x, B, caches[c], 1000 * t) for x, c in zip(rows, ids)])
        if t == 0:       # the sums are the raw soft bits, not the de-interleaved ones
            assert all(r["cw0_deinterleaved"] for r, _ in hist[0])
            e = next(iter(caches[0].cache.values()))
            assert np.array_equal(e.soft[1], rows[0][648:1296]) and not np.array_equal(e.soft[1], deinterleave(rows[0][648:1296], B))
    r = lambda t, l: hist[t][l][0]
    h = lambda t, l: hist[t][l][1]
    assert [r(t, 0)["success"] for t in range(2)] == [0, 1] and h(1, 0)["recovered_mask"] == 2 and h(1, 0)["max_combine"] == 2 and h(1, 0)["entry"] == 2
    assert [r(t, 1)["success"] for t in range(3)] == [0, 0, 1] and h(2, 1)["recovered_mask"] == 4 and h(2, 1)["max_combine"] == 3
    assert (r(0, 2)["codewords_ok"], h(0, 2)["stored_mask"]) == (2, 4) and (r(1, 2)["codewords_ok"], h(1, 2)["stored_mask"]) == (2, 2)   # the trap
    assert h(2, 2)["stored_mask"] == 2 and h(2, 2)["sum_mask"] == 2 and h(3, 2)["entry"] == 2
    # link 3: reception 1 interleaved, reception 2 plain under the same key: the raw sum is decoded as it is
    assert (r(0, 3)["cw0_deinterleaved"], h(0, 3)["stored_mask"]) == (1, 2)
    assert (r(1, 3)["cw0_deinterleaved"], r(1, 3)["ci_tried"], h(1, 3)["sum_mask"], h(1, 3)["recovered_mask"], h(1, 3)["max_combine"]) == (0, 0, 2, 0, 2)
    assert r(2, 3)["success"] == 1 and h(2, 3)["entry"] == 2


def test_acquire_windows_do_what_they_are_meant_to(oracle):
    zc, hs = I.zc_windows(oracle), I.handshake_windows(oracle)
    cache = ChaseCache()
    out = [acquire_window_ci(oracle, x, I.ZC_SEARCH, 3, 20, cache if i == 3 else None, 0, bps=2, chirp=False, min_confidence=0.25)
           for i, x in enumerate(zc[0])]
    assert [(r["success"], r["cw0_deinterleaved"], r["ci_tried"]) for r, _ in out[:3]] == [(1, 1, 1), (1, 0, 0), (0, 0, 0)]
    assert out[0][0]["header_total_cw"] == 3 and out[1][0]["frame_type"] == ACK and out[2][0]["accepted"] == 0
    assert (out[3][0]["success"], out[3][0]["codewords_failed"], out[3][1]["stored_mask"]) == (0, 1, 4)
    r, h = acquire_window_ci(oracle, zc[1][3], I.ZC_SEARCH, 3, 20, cache, 1000, bps=2, chirp=False, min_confidence=0.25)
    assert (r["success"], r["cw0_deinterleaved"], h["recovered_mask"], h["entry"]) == (1, 1, 4, 2)
    rs = [acquire_window_ci(oracle, x, I.CHIRP_SEARCH, 3, 20, None, 0, bps=1, chirp=True)[0] for x in hs]
    assert [(r["success"], r["cw0_deinterleaved"], r["frame_type"]) for r in rs] == [(1, 1, CONNECT)] * 3
    assert (rs[0]["delta"], rs[0]["candidates"]) == (0, 1)
    assert rs[1]["delta"] != 0 and rs[1]["candidates"] > 2 and rs[1]["modulation"] == po.DBPSK       # a timing-recovery candidate
    assert (rs[2]["delta"], rs[2]["candidates"], rs[2]["modulation"]) == (0, 2, po.DQPSK)            # the alternate modulation, B = 20
