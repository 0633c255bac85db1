"""The HIP OFDM demodulator against the oracle over the demodulator's whole input domain (tests/demod_domain_inputs.py):
ria_gpu_demod_batch and ria_gpu_rx_batch, bit for bit in every LLR and status field, in every batch layout and through
both implementations of the demodulator (the split pipeline and the one-wave-per-frame demod_frames_kernel).
The oracle is pinned to the compiled reference on the same inputs by tests/test_demod_domain_cpu.py.

NaN rule: where an LLR is NaN the position must agree; the sign and payload of a NaN are not compared.  The same holds for
the float status words: IEEE 754 leaves the sign and payload of a NaN that an operation generates to the implementation
(x86 SSE writes 0xFFC00000, gfx950 0x7FC00000), so a NaN noise variance of the reference is a NaN here, in the same frame."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import demod_domain_inputs as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_engines, _gpu, _orc = {}, {}, {}


def engine(mode):
    from ria_amd.engine import RxEngine
    if mode not in _engines:
        _engines[mode] = RxEngine(*D.ENGINE[mode])
    return _engines[mode]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def demod(e, F, idx=None):
    """-> (llr float32 [n, llrs_per_frame], status structured [n]) of the frames idx (all) in row layout"""
    idx = np.arange(len(F["x"])) if idx is None else np.asarray(idx)
    llr, st = e.demod(dev(F["x"][idx]), cfo_hz=F["cfo"][idx], abs_pos=F["pos"][idx], flags=F["flags"][idx])
    return llr.cpu().numpy(), e.frame_status(st).copy()


def gpu_answers(golden, oracle, mode, fam):
    """the default path's answers on the whole set in row layout (computed once, never modified)"""
    if (mode, fam) not in _gpu:
        F = D.family(oracle, mode, fam)
        assert D.digest(F) == str(golden("demod_domain")[f"sha_{mode}_{fam}"]), f"{mode} {fam}: generator drifted"
        _gpu[(mode, fam)] = demod(engine(mode), F)
    return _gpu[(mode, fam)]


def oracle_answers(oracle, mode, fam):
    if (mode, fam) not in _orc:
        _orc[(mode, fam)] = D.oracle_answers(oracle, mode, D.family(oracle, mode, fam))
    return _orc[(mode, fam)]


def assert_same(what, labels, llr_a, st_a, llr_b, st_b, idx=None):
    """two GPU results must be identical: LLR bits under the NaN rule, status words in every byte"""
    for f in range(len(llr_a)):
        name = labels[f if idx is None else idx[f]]
        if not D.same_bits(llr_a[f], llr_b[f]):
            d = np.nonzero(llr_a[f].view(np.uint32) != llr_b[f].view(np.uint32))[0]
            raise AssertionError(f"{what} frame {f} ({name}): {len(d)} LLRs differ, first at {d[0]}: {llr_a[f][d[0]]!r} vs {llr_b[f][d[0]]!r}")
        assert st_a[f:f + 1].tobytes() == st_b[f:f + 1].tobytes(), f"{what} frame {f} ({name}): status {st_a[f]} vs {st_b[f]}"


@pytest.mark.parametrize("mode,fam", D.CASES)
def test_demodulator_equals_the_oracle(golden, oracle, mode, fam):
    F = D.family(oracle, mode, fam)
    llr, st = gpu_answers(golden, oracle, mode, fam)
    lo, ao, so, _ = oracle_answers(oracle, mode, fam)
    bad = []
    for f in range(len(lo)):
        msg = []
        if st["n_llr"][f] != len(lo[f]):
            msg.append(f"n_llr {st['n_llr'][f]} oracle {len(lo[f])}")
        elif not D.same_bits(llr[f][:len(lo[f])], lo[f]):
            d = np.nonzero((llr[f][:len(lo[f])].view(np.uint32) != lo[f].view(np.uint32)) & ~(np.isnan(llr[f][:len(lo[f])]) & np.isnan(lo[f])))[0]
            msg.append(f"{len(d)} of {len(lo[f])} LLRs differ, first at {d[0]}: gpu {llr[f][d[0]]!r} oracle {lo[f][d[0]]!r}")
        for c, k in enumerate(D.AUX):
            if np.float32(st[k][f]).view(np.uint32) != ao[f, c] and not (np.isnan(st[k][f]) and np.isnan(ao[f, c:c + 1].view(np.float32)[0])):
                msg.append(f"{k} gpu {st[k][f]!r} oracle {ao[f, c:c + 1].view(np.float32)[0]!r}")
        if not np.allclose(st["snr_db"][f], so[f], rtol=1e-5, atol=1e-5, equal_nan=True):   # display value, log10f not bit-pinned
            msg.append(f"snr_db gpu {st['snr_db'][f]!r} oracle {so[f]!r}")
        if msg:
            bad.append(f"frame {f} ({F['labels'][f]}): " + "; ".join(msg))
    for b in bad:
        print(b)
    assert not bad, f"{mode} {fam}: {len(bad)} of {len(lo)} frames differ from the oracle, first: {bad[0]}"


@pytest.mark.parametrize("mode,fam", D.CASES)
def test_fused_call_gives_the_same_llrs_and_decodes_them_as_the_oracle(golden, oracle, mode, fam):
    """ria_gpu_rx_batch: its LLRs and demodulator status equal ria_gpu_demod_batch's; cw_ok, iterations, attempts,
    frame_valid and the bytes equal the oracle's decodeFixedFrame (CRC recovery included) of those LLRs"""
    e = engine(mode)
    F = D.family(oracle, mode, fam)
    llr0, st0 = gpu_answers(golden, oracle, mode, fam)
    info, st, llr, fst = e.rx(dev(F["x"]), cfo_hz=F["cfo"], abs_pos=F["pos"], meta_flags=F["flags"], want_llr=True)
    info, s, llr, fst = info.cpu().numpy(), e.decode_status(st).copy(), llr.cpu().numpy(), e.frame_status(fst).copy()
    assert_same(f"{mode} {fam} rx_batch vs demod_batch", F["labels"], llr, fst, llr0, st0)
    rate, bps = D.MODES[mode][1], e.geo.bits_per_symbol
    with ThreadPoolExecutor(16) as ex:
        ans = list(ex.map(lambda x: oracle.decode_fixed_frame(x, rate, True, bps, flags=7), list(llr)))
    for f, (d, ok, it, att) in enumerate(ans):
        what = f"{mode} {fam} frame {f} ({F['labels'][f]})"
        assert np.array_equal(s["cw_ok"][f], ok), f"{what}: cw_ok {s['cw_ok'][f]} oracle {ok}"
        assert np.array_equal(s["iterations"][f], it.astype(np.uint16)), f"{what}: iterations {s['iterations'][f]} oracle {it}"
        assert np.array_equal(s["attempts"][f], att.astype(np.uint8)), f"{what}: attempts {s['attempts'][f]} oracle {att}"
        assert np.array_equal(info[f], d), f"{what}: bytes"
        assert bool(s["frame_valid"][f]) == bool(ok.all()), f"{what}: frame_valid {s['frame_valid'][f]} with cw_ok {ok}"


@pytest.mark.parametrize("mode,fam", D.CASES)
def test_batch_position_does_not_change_a_frame(golden, oracle, mode, fam):
    e = engine(mode)
    F = D.family(oracle, mode, fam)
    llr0, st0 = gpu_answers(golden, oracle, mode, fam)
    n = len(llr0)
    rng = np.random.default_rng(5150 + n)
    sets = [rng.permutation(n), np.arange(n)] + [np.array([f]) for f in (0, n // 2, n - 1)] + \
        [np.resize(np.arange(s, n), 7) for s in (0, max(n - 7, 0))]
    for idx in sets:
        llr, st = demod(e, F, idx)
        assert_same(f"{mode} {fam} batch of {len(idx)} starting with frame {idx[0]}", F["labels"], llr, st, llr0[idx], st0[idx], idx)


@pytest.mark.parametrize("mode,fam", [c for c in D.CASES if c[1] in ("nonfinite", "level")])
def test_frame_offsets_into_one_capture(golden, oracle, mode, fam):
    """frames at odd sample offsets of one capture, 1 to 36 NaN samples between them and NaN behind the last one:
    ria_gpu_demod_batch and ria_gpu_rx_batch give what they give for the row layout"""
    e = engine(mode)
    F = D.family(oracle, mode, fam)
    llr0, st0 = gpu_answers(golden, oracle, mode, fam)
    n, fs = F["x"].shape
    rng = np.random.default_rng(6160 + n)
    gaps = np.concatenate([[1 + 2 * int(rng.integers(0, 18))], 2 * rng.integers(1, 19, n - 1)])      # every offset odd
    offs = np.cumsum(gaps + np.concatenate([[0], np.full(n - 1, fs)])).astype(np.uint64)
    assert (offs % 2 == 1).all() and gaps.min() >= 1 and gaps.max() <= 36
    cap = np.full(int(offs[-1]) + fs + 40, np.nan, np.float32)
    for f in range(n):
        cap[int(offs[f]):int(offs[f]) + fs] = F["x"][f]
    c = dev(cap)
    llr, st = e.demod(c, cfo_hz=F["cfo"], abs_pos=F["pos"], flags=F["flags"], offsets=offs)
    assert_same(f"{mode} {fam} demod_batch with offsets", F["labels"], llr.cpu().numpy(), e.frame_status(st), llr0, st0)
    i0, s0 = e.rx(dev(F["x"]), cfo_hz=F["cfo"], abs_pos=F["pos"], meta_flags=F["flags"])
    i1, s1, llr, fst = e.rx(c, cfo_hz=F["cfo"], abs_pos=F["pos"], meta_flags=F["flags"], want_llr=True, offsets=offs)
    assert_same(f"{mode} {fam} rx_batch with offsets", F["labels"], llr.cpu().numpy(), e.frame_status(fst), llr0, st0)
    assert np.array_equal(i1.cpu().numpy(), i0.cpu().numpy()) and np.array_equal(s1.cpu().numpy(), s0.cpu().numpy())


FUSED_MODES = ("QAM16_R1_2", "DQPSK_R1_4", "D8PSK_R1_2")


def test_one_wave_per_frame_kernel_equals_the_default_path(golden, oracle, tmp_path):
    """demod_frames_kernel (RIA_DEMOD_FUSED=1, read once per process: a fresh child selects it) against the split
    pipeline of this process on every family of three modes: LLR bits and status words identical"""
    from ria_amd import capi
    assert capi.load().ria_gpu_demod_variant() == 0, "this process must run the split pipeline"
    out = str(tmp_path / "fused.npz")
    env = dict(os.environ, RIA_DEMOD_FUSED="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "demod_fused_child.py"), out, *FUSED_MODES],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    n_cases = 0
    for mode, fam in D.CASES:
        if mode not in FUSED_MODES:
            continue
        F = D.family(oracle, mode, fam)
        llr0, st0 = gpu_answers(golden, oracle, mode, fam)
        st = got[f"st_{mode}_{fam}"].view(engine(mode).FRAME_STATUS).reshape(-1)
        assert_same(f"{mode} {fam} one wave per frame", F["labels"], got[f"llr_{mode}_{fam}"].view(np.float32), st, llr0, st0)
        n_cases += 1
    assert n_cases == 19


def test_level_family_through_the_multi_stream_path(golden, oracle):
    """ria_gpu_rx_batch cuts a batch of 4096 or more frames into parts on internal streams (RIA_OPT_SPLIT_PARTS):
    the level family tiled to 4096 + 9 frames with 1 part and with 3 parts equals the small batch frame by frame"""
    mode, fam = "QAM16_R1_2", "level"
    e = engine(mode)
    F = D.family(oracle, mode, fam)
    llr0, st0 = gpu_answers(golden, oracle, mode, fam)
    i0, s0 = e.rx(dev(F["x"]), cfo_hz=F["cfo"], abs_pos=F["pos"], meta_flags=F["flags"])
    i0, s0 = i0.cpu().numpy(), s0.cpu().numpy()
    n = len(llr0)
    idx = np.random.default_rng(7170).permutation(np.resize(np.arange(n), 4096 + 9))
    x = dev(F["x"])[dev(idx)].contiguous()
    try:
        for parts in (1, 3):
            e.set_split_parts(parts)
            info, st, llr, fst = e.rx(x, cfo_hz=F["cfo"][idx], abs_pos=F["pos"][idx], meta_flags=F["flags"][idx], want_llr=True)
            llr, fst = llr.cpu().numpy(), e.frame_status(fst)
            same = np.array([D.same_bits(llr[k], llr0[idx[k]]) for k in range(len(idx))])
            assert same.all(), f"{parts} parts: LLRs of {int((~same).sum())} frames differ, first {np.nonzero(~same)[0][0]}"
            assert fst.tobytes() == st0[idx].tobytes(), f"{parts} parts: demodulator status"
            assert np.array_equal(info.cpu().numpy(), i0[idx]) and np.array_equal(st.cpu().numpy(), s0[idx]), f"{parts} parts: decode"
    finally:
        e.set_split_parts(0)
