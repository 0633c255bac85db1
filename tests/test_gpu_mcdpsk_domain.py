"""The HIP MC-DPSK demodulator and modulator against the oracle over their input domain (tests/mcdpsk_domain_inputs.py):
ria_gpu_mcdpsk_demod_batch, ria_gpu_mcdpsk_demod_host, ria_gpu_mcdpsk_modulate_batch and ria_gpu_mcdpsk_modulate_host, bit for
bit in every LLR, every status word and every audio sample, in every batch layout.  The oracle is pinned to the compiled
reference on the same inputs by tests/test_mcdpsk_domain_cpu.py; for training_cfo_residual and valid_symbols, which the
reference exposes no getter for, the oracle is the reference.

NaN rule: where a float word is NaN the position must agree; the sign and payload of a NaN are not compared (IEEE 754 leaves
them to the implementation: x86 SSE generates 0xFFC00000, gfx950 0x7FC00000)."""
import ctypes as C

import numpy as np
import pytest

import mcdpsk_domain_inputs as M
import pyoracle as po

pytestmark = pytest.mark.gpu

IDS = [M.key(c, f) for c, f in M.CASES]
_state, _gpu, _orc = {}, {}, {}
FLOAT_WORDS = M.AUX + ("training_cfo_residual",)


def engine(fresh=False):
    from ria_amd.engine import RxEngine
    if fresh:
        return RxEngine("QAM16", "R1_2")
    if "e" not in _state:
        _state["e"] = RxEngine("QAM16", "R1_2")
    return _state["e"]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def n_llr_of(cfg):
    return max(1, cfg[3] // cfg[2]) * cfg[0] * cfg[1]


def raw_demod(e, cfg, x, fs, n, stride=None, cfo=None, ph=None, llr=None, llr_stride=None):
    """ria_gpu_mcdpsk_demod_batch with every argument spelt out -> (rc, llr tensor, status structured array)"""
    import torch
    from ria_amd import capi
    from ria_amd.engine import _ptr, _stream_ptr
    llr_stride = n_llr_of(cfg) if llr_stride is None else llr_stride
    if llr is None:
        llr = torch.full((n, llr_stride), -77.0, dtype=torch.float32, device="cuda")
    st = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    c = capi.McdpskConfig(cfg[0], cfg[1], cfg[2], 0)
    rc = e.lib.ria_gpu_mcdpsk_demod_batch(e.h, C.byref(c), _ptr(x), fs if stride is None else stride, fs, n, _ptr(cfo), _ptr(ph),
                                          _ptr(llr), llr_stride, _ptr(st), _stream_ptr())
    torch.cuda.synchronize()
    return rc, llr, e._status_array(st, e.MCDPSK_STATUS).copy()


def demod(e, cfg, F, idx=None):
    """-> (llr float32 [n, n_llr], status [n]) of the frames idx (all) as one contiguous batch with CFO and phase arrays"""
    idx = np.arange(len(F["x"])) if idx is None else np.asarray(idx)
    rc, llr, st = raw_demod(e, cfg, dev(F["x"][idx]), F["x"].shape[1], len(idx), cfo=dev(F["cfo"][idx]), ph=dev(F["phase0"][idx]))
    assert rc == 0, e.lib.ria_gpu_last_error(e.h).decode()
    return llr.cpu().numpy(), st


def gpu_answers(golden, oracle, cfg, fam):
    """the answers on the whole family as one batch (computed once, never modified)"""
    if (cfg, fam) not in _gpu:
        F = M.family(oracle, cfg, fam)
        assert M.digest(F) == str(golden("mcdpsk_domain")[f"sha_{M.key(cfg, fam)}"]), f"{M.key(cfg, fam)}: generator drifted"
        _gpu[(cfg, fam)] = demod(engine(), cfg, F)
    return _gpu[(cfg, fam)]


def oracle_answers(oracle, cfg, fam):
    if (cfg, fam) not in _orc:
        _orc[(cfg, fam)] = M.oracle_answers(oracle, cfg, M.family(oracle, cfg, fam))
    return _orc[(cfg, fam)]


def same_word(a, b):
    a, b = np.float32(a), np.float32(b)
    return a.view(np.uint32) == b.view(np.uint32) or (np.isnan(a) and np.isnan(b))


def differences(cfg, F, llr, st, lo, ao, ro, vo):
    """one line per frame that differs from the oracle's (llr list, aux bits, residual, valid)"""
    bad = []
    for f in range(len(lo)):
        msg = []
        if st["n_llr"][f] != len(lo[f]):
            msg.append(f"n_llr {st['n_llr'][f]} oracle {len(lo[f])}")
        elif not M.same_bits(llr[f][:len(lo[f])], lo[f]):
            g = llr[f][:len(lo[f])]
            d = np.nonzero((g.view(np.uint32) != lo[f].view(np.uint32)) & ~(np.isnan(g) & np.isnan(lo[f])))[0]
            msg.append(f"{len(d)} of {len(lo[f])} LLRs differ, first at {d[0]}: gpu {g[d[0]]!r} oracle {lo[f][d[0]]!r}")
        for c, k in enumerate(M.AUX):
            if not same_word(st[k][f], ao[f, c:c + 1].view(np.float32)[0]):
                msg.append(f"{k} gpu {st[k][f]!r} oracle {ao[f, c:c + 1].view(np.float32)[0]!r}")
        if not same_word(st["training_cfo_residual"][f], ro[f]):
            msg.append(f"training_cfo_residual gpu {st['training_cfo_residual'][f]!r} oracle {ro[f]!r}")
        if st["valid_symbols"][f] != vo[f]:
            msg.append(f"valid_symbols gpu {st['valid_symbols'][f]} oracle {vo[f]}")
        if st["reserved"][f] != 0:
            msg.append(f"reserved {st['reserved'][f]}")
        if msg:
            bad.append(f"frame {f} ({F['labels'][f]}): " + "; ".join(msg))
    return bad


def assert_same(what, labels, llr_a, st_a, llr_b, st_b, idx=None):
    """two GPU results must be identical: LLR bits and float status words under the NaN rule, the integer words exactly"""
    for f in range(len(llr_a)):
        name = labels[f if idx is None else idx[f]]
        if not M.same_bits(llr_a[f], llr_b[f]):
            d = np.nonzero(llr_a[f].view(np.uint32) != llr_b[f].view(np.uint32))[0]
            raise AssertionError(f"{what} frame {f} ({name}): {len(d)} LLRs differ, first at {d[0]}: {llr_a[f][d[0]]!r} vs {llr_b[f][d[0]]!r}")
        for k in FLOAT_WORDS:
            assert same_word(st_a[k][f], st_b[k][f]), f"{what} frame {f} ({name}): {k} {st_a[k][f]!r} vs {st_b[k][f]!r}"
        for k in ("n_llr", "valid_symbols", "reserved"):
            assert st_a[k][f] == st_b[k][f], f"{what} frame {f} ({name}): {k} {st_a[k][f]} vs {st_b[k][f]}"


@pytest.mark.parametrize("cfg,fam", M.CASES, ids=IDS)
def test_demodulator_equals_the_oracle(golden, oracle, cfg, fam):
    F = M.family(oracle, cfg, fam)
    llr, st = gpu_answers(golden, oracle, cfg, fam)
    bad = differences(cfg, F, llr, st, *oracle_answers(oracle, cfg, fam)[:4])
    for b in bad:
        print(b)
    assert not bad, f"{M.key(cfg, fam)}: {len(bad)} of {len(F['x'])} frames differ from the oracle, first: {bad[0]}"


@pytest.mark.parametrize("cfg,fam", [c for c in M.CASES if c[1] != "shape"], ids=[i for i in IDS if not i.endswith("shape")])
def test_batch_position_does_not_change_a_frame(golden, oracle, cfg, fam):
    e = engine()
    F = M.family(oracle, cfg, fam)
    llr0, st0 = gpu_answers(golden, oracle, cfg, fam)
    n = len(llr0)
    rng = np.random.default_rng(5250 + n)
    sets = [rng.permutation(n)] + [np.array([f]) for f in (0, n // 2, n - 1)] + [np.resize(np.arange(s, n), 7) for s in (0, max(n - 7, 0))]
    for idx in sets:
        llr, st = demod(e, cfg, F, idx)
        assert_same(f"{M.key(cfg, fam)} batch of {len(idx)} starting with frame {idx[0]}", F["labels"], llr, st, llr0[idx], st0[idx], idx)


@pytest.mark.parametrize("cfg,fam", [(M.MAIN[0], "cfo"), (M.MAIN[1], "nonfinite"), (M.SHAPES[-1], "shape")],
                         ids=[M.key(M.MAIN[0], "cfo"), M.key(M.MAIN[1], "nonfinite"), M.key(M.SHAPES[-1], "shape")])
def test_strides_above_the_frame_and_the_llr_count(golden, oracle, cfg, fam):
    """frames `stride` apart with NaN between them and behind the last one, LLR rows llr_stride apart: the answers are those
    of the contiguous batch and the slack of every LLR row keeps what it held"""
    import torch
    e = engine()
    F = M.family(oracle, cfg, fam)
    llr0, st0 = gpu_answers(golden, oracle, cfg, fam)
    n, fs = F["x"].shape
    stride, ls, nl = fs + 37, n_llr_of(cfg) + 13, n_llr_of(cfg)
    cap = np.full(n * stride, np.nan, np.float32)
    for f in range(n):
        cap[f * stride:f * stride + fs] = F["x"][f]
    llr = torch.full((n, ls), 12345.0, dtype=torch.float32, device="cuda")
    rc, llr, st = raw_demod(e, cfg, dev(cap), fs, n, stride=stride, cfo=dev(F["cfo"]), ph=dev(F["phase0"]), llr=llr, llr_stride=ls)
    assert rc == 0, e.lib.ria_gpu_last_error(e.h).decode()
    llr = llr.cpu().numpy()
    assert_same(f"{M.key(cfg, fam)} with stride {stride} and llr_stride {ls}", F["labels"], llr[:, :nl], st, llr0, st0)
    assert (llr[:, nl:] == 12345.0).all(), "the slack behind the LLRs was written"


@pytest.mark.parametrize("cfg", M.MAIN + (M.SHAPES[0],), ids=lambda c: "c%d_b%d_s%d_n%d_x%d" % c)
def test_null_cfo_and_phase_are_arrays_of_zeros(golden, oracle, cfg):
    e = engine()
    fam = "level" if cfg in M.MAIN else "shape"
    F = M.family(oracle, cfg, fam)
    assert not F["cfo"].any() and not F["phase0"].any()
    llr0, st0 = gpu_answers(golden, oracle, cfg, fam)
    n, fs = F["x"].shape
    x = dev(F["x"])
    for cfo, ph in ((None, None), (dev(F["cfo"]), None), (None, dev(F["phase0"]))):
        rc, llr, st = raw_demod(e, cfg, x, fs, n, cfo=cfo, ph=ph)
        assert rc == 0, e.lib.ria_gpu_last_error(e.h).decode()
        assert_same(f"{M.key(cfg, fam)} cfo {'NULL' if cfo is None else 'zeros'} phase0 {'NULL' if ph is None else 'zeros'}", F["labels"],
                    llr.cpu().numpy(), st, llr0, st0)


def test_a_batch_that_needs_two_workspace_chunks(golden, oracle):
    """the per-handle workspace holds at most 256 MiB; with CFO arrays each frame takes 2 * frame_samples floats of it for
    the corrected samples alone, so n frames with n * 2 * frame_samples * 4 > 256 MiB cannot be one chunk: the cfo family of
    the shortest configuration tiled to that count (and twice the family more, so that every frame of it also lies in the
    second chunk) equals the small batch frame by frame"""
    e = engine(fresh=True)
    cfg, fam = M.SHORT, "cfo"
    F = M.family(oracle, cfg, fam)
    llr0, st0 = gpu_answers(golden, oracle, cfg, fam)
    m, fs = F["x"].shape
    n = (256 << 20) // (2 * fs * 4) + 1 + 2 * m
    assert n * 2 * fs * 4 > (256 << 20) and fs == 5120
    idx = np.resize(np.arange(m), n)
    x = dev(F["x"])[dev(idx)].contiguous()
    rc, llr, st = raw_demod(e, cfg, x, fs, n, cfo=dev(F["cfo"][idx]), ph=dev(F["phase0"][idx]))
    assert rc == 0, e.lib.ria_gpu_last_error(e.h).decode()
    llr = llr.cpu().numpy()
    same = np.array([M.same_bits(llr[k], llr0[idx[k]]) for k in range(n)])
    assert same.all(), f"LLRs of {int((~same).sum())} frames differ, first {np.nonzero(~same)[0][0]}"
    assert_same("two chunks", F["labels"], llr[-3 * m:], st[-3 * m:], llr0[idx[-3 * m:]], st0[idx[-3 * m:]], idx[-3 * m:])
    for k in FLOAT_WORDS + ("n_llr", "valid_symbols"):
        a, b = st[k], st0[k][idx]
        differ = ~((a == b) | ((a != a) & (b != b)))
        assert not differ.any(), f"two chunks: {k} of {int(differ.sum())} frames differs, first {np.nonzero(differ)[0][0]}"
    e.close()


def test_one_handle_through_calls_of_different_shapes(golden, oracle):
    """the mixer cache per carrier count, the dynamic-LDS opt-in and the workspace growth are set once per handle: calls of
    different carrier counts and frame lengths following each other (small, large, small again; with and without CFO arrays)
    on one handle equal what each gives as the first call of a fresh handle"""
    big = [c for c in M.SHAPES if c[0] == 20][-1]
    seq = [(M.SHAPES[0], "shape", False), (M.SHORT, "cfo", True), (big, "shape", True), (M.SHAPES[0], "shape", True), (M.MAIN[0], "cfo", True),
           (M.SHAPES[2], "shape", False), (big, "shape", False), (M.SHORT, "cfo", True), (M.MAIN[1], "level", False)]

    def call(e, cfg, fam, with_cfo):
        F = M.family(oracle, cfg, fam)
        n, fs = F["x"].shape
        assert with_cfo or not F["cfo"].any()
        rc, llr, st = raw_demod(e, cfg, dev(F["x"]), fs, n, cfo=dev(F["cfo"]) if with_cfo else None, ph=dev(F["phase0"]) if with_cfo else None)
        assert rc == 0, e.lib.ria_gpu_last_error(e.h).decode()
        return llr.cpu().numpy(), st

    first = {}
    for step in dict.fromkeys(seq):
        e = engine(fresh=True)
        first[step] = call(e, *step)
        e.close()
    e = engine(fresh=True)
    for k, step in enumerate(seq):
        llr, st = call(e, *step)
        assert_same(f"call {k} ({M.key(*step[:2])}) on one handle", M.family(oracle, *step[:2])["labels"], llr, st, *first[step])
        llr0, st0 = gpu_answers(golden, oracle, *step[:2])
        assert_same(f"call {k} ({M.key(*step[:2])}) against the shared handle", M.family(oracle, *step[:2])["labels"], llr, st, llr0, st0)
    e.close()


def test_host_call_equals_the_batch_call(golden, oracle):
    from ria_amd import capi
    e = engine()
    k = 0
    for cfg, fam, frames in ((M.MAIN[0], "level", (0, 7, 20, 33)), (M.MAIN[1], "cfo", (3, 6, 13, 22)), (M.MAIN[0], "nonfinite", (1, 11, 19, 37, 38, 39))):
        F = M.family(oracle, cfg, fam)
        llr0, st0 = gpu_answers(golden, oracle, cfg, fam)
        c = capi.McdpskConfig(cfg[0], cfg[1], cfg[2], 0)
        for f in frames:
            x = np.ascontiguousarray(F["x"][f])
            llr = np.full(n_llr_of(cfg) + 5, -3.0, np.float32)
            st = np.zeros(1, e.MCDPSK_STATUS)
            rc = e.lib.ria_gpu_mcdpsk_demod_host(e.h, C.byref(c), x.ctypes.data, len(x), float(F["cfo"][f]), float(F["phase0"][f]),
                                                 llr.ctypes.data, len(llr), st.ctypes.data)
            assert rc == 0, e.lib.ria_gpu_last_error(e.h).decode()
            assert_same(f"{M.key(cfg, fam)} host call", F["labels"], llr[None, :-5], st, llr0[f:f + 1], st0[f:f + 1], [f])
            assert (llr[-5:] == -3.0).all()
            k += 1
    assert k >= 12


def test_lds_limit_at_20_carriers(oracle):
    """one workgroup stages a whole frame: the longest frame whose LDS need (the layout in the kernel's comments) is within
    160 KiB equals the oracle; one symbol more is RIA_ERR_UNSUPPORTED with a message and writes nothing"""
    import torch
    e = engine(fresh=True)
    n_sym = 4
    while M.lds_bytes(20, n_sym + 1) <= 160 * 1024:
        n_sym += 1
    assert M.lds_bytes(20, n_sym) <= 160 * 1024 < M.lds_bytes(20, n_sym + 1) and n_sym > 800
    cfg = (20, 2, 1, n_sym - 3, 0)
    F = M.shape(oracle, cfg, np.random.default_rng(4711))
    F = {k: v[:1] for k, v in F.items()}
    rc, llr, st = raw_demod(e, cfg, dev(F["x"]), F["x"].shape[1], 1, cfo=dev(F["cfo"]), ph=dev(F["phase0"]))
    assert rc == 0, e.lib.ria_gpu_last_error(e.h).decode()
    bad = differences(cfg, F, llr.cpu().numpy(), st, *M.oracle_answers(oracle, cfg, F)[:4])
    assert not bad, bad[0]
    over = (20, 2, 1, n_sym - 2, 0)
    x = torch.zeros((1, M.frame_samples(over)), dtype=torch.float32, device="cuda")
    rc, llr, st = raw_demod(e, over, x, x.shape[1], 1)
    assert rc == -4 and len(e.lib.ria_gpu_last_error(e.h).decode()) > 10, rc
    assert (llr.cpu().numpy() == -77.0).all() and not st.view(np.uint8).any(), "a refused call wrote its outputs"
    e.close()


# ---------------------------------------------------------------------------------------------- modulator
def modulate_batch(e, case, data, out_stride=None, fill=None):
    """ria_gpu_mcdpsk_modulate_batch on rows of bytes -> (rc, float32 [n, out_stride])"""
    import torch
    from ria_amd import capi
    from ria_amd.engine import _ptr, _stream_ptr
    nc, bps, sp, nb = case[:4]
    n, fs = len(data), po.mcdpsk_frame_samples(nc, bps, sp, nb)
    out_stride = fs if out_stride is None else out_stride
    d = dev(np.concatenate([np.ascontiguousarray(data, np.uint8).reshape(-1), np.zeros(1, np.uint8)]))     # never a null pointer
    out = torch.full((n, out_stride), 0.0 if fill is None else fill, dtype=torch.float32, device="cuda")
    c = capi.McdpskConfig(nc, bps, sp, 0)
    rc = e.lib.ria_gpu_mcdpsk_modulate_batch(e.h, C.byref(c), _ptr(d), nb, n, _ptr(out), out_stride, _stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def test_modulator_equals_the_host_builder_the_oracle_and_the_recorded_audio(golden, oracle):
    """every case of mcdpsk_domain_inputs.MOD_CASES (carriers x bits x spreading, byte counts 0 .. 2045 with 1 and
    carriers * bits - 1 bits of padding, all-zero, all-one and random bytes, 600-symbol chains, the largest byte count of the
    64 KB rule): device == host builder == oracle == the reference's recorded digest, with 9 floats of slack behind each frame"""
    from ria_amd import capi
    e = engine()
    fx = golden("mcdpsk_domain")
    assert len(fx["mod_dig"]) == len(M.MOD_CASES)
    for i, case in enumerate(M.MOD_CASES):
        nc, bps, sp, nb = case[:4]
        data = M.mod_data(case, i)
        want = oracle.mcdpsk_modulate(nc, bps, sp, data)
        fs = len(want)
        assert M.audio_digest(want) == bytes(fx["mod_dig"][i]).hex(), f"case {i} {case}: the oracle left the recorded audio"
        rc, out = modulate_batch(e, case, data[None], out_stride=fs + 9, fill=-5.0)
        assert rc == 0, (case, e.lib.ria_gpu_last_error(e.h).decode())
        d = np.nonzero(out[0, :fs].view(np.uint32) != want.view(np.uint32))[0]
        assert not len(d), f"case {i} {case}: {len(d)} of {fs} samples differ from the oracle, first at {d[0]}: {out[0, d[0]]!r} vs {want[d[0]]!r}"
        assert (out[0, fs:] == -5.0).all(), f"case {i} {case}: the slack behind the frame was written"
        host = np.zeros(fs + 1, np.float32)
        c = capi.McdpskConfig(nc, bps, sp, 0)
        buf = np.concatenate([data, np.zeros(1, np.uint8)])
        assert e.lib.ria_gpu_mcdpsk_modulate_host(e.h, C.byref(c), buf.ctypes.data, nb, host.ctypes.data, len(host)) == fs, case
        assert np.array_equal(host[:fs].view(np.uint32), want.view(np.uint32)), f"case {i} {case}: host builder"


def test_modulator_batch_whose_rows_differ(oracle):
    e = engine()
    rng = np.random.default_rng(31337)
    for case in ((10, 1, 1, 81), (13, 2, 2, 20), (3, 1, 4, 7)):
        data = rng.integers(0, 256, (37, case[3]), dtype=np.uint8)
        data[5], data[6] = 0, 255
        rc, out = modulate_batch(e, case, data)
        assert rc == 0
        for f in range(len(data)):
            assert np.array_equal(out[f].view(np.uint32), oracle.mcdpsk_modulate(*case[:3], data[f]).view(np.uint32)), (case, f)


def test_modulator_lds_limit(oracle):
    """the transmitted symbols of a frame are parked in 64 KiB of LDS: 8190 (symbol, carrier) pairs.  The largest byte count is
    in MOD_CASES; the first one with a symbol more is RIA_ERR_UNSUPPORTED with a message and writes nothing"""
    e = engine()
    last = M.MOD_CASES[-1]
    nc, bps, sp, nb = last[:4]
    n_sym = -(-8 * nb // (nc * bps))
    assert n_sym * nc * 8 + 16 <= 64 * 1024 < (n_sym + 1) * nc * 8 + 16
    over = (nc, bps, sp, nb + 1, "zero")
    rc, out = modulate_batch(e, over, np.zeros((1, nb + 1), np.uint8), fill=-5.0)
    assert rc == -4 and len(e.lib.ria_gpu_last_error(e.h).decode()) > 10, rc
    assert (out == -5.0).all()


@pytest.mark.parametrize("cfg", [(10, 1, 1, 65, 0), (10, 2, 1, 33, 0), (13, 2, 2, 12, 0), (1, 1, 4, 64, 0), (20, 1, 1, 6, 0)], ids=lambda c: "c%d_b%d_s%d_n%d_x%d" % c)
def test_round_trip_on_the_device_gives_the_oracles_llrs(oracle, cfg):
    import torch
    e = engine()
    nc, bps, sp, num_rx, _ = cfg
    nb = (num_rx // sp) * nc * bps // 8
    data = np.random.default_rng(808 + nc).integers(0, 256, (5, nb), dtype=np.uint8)
    rc, out = modulate_batch(e, (nc, bps, sp, nb), data)
    assert rc == 0
    fs = out.shape[1]
    got = (fs - M.PRE) // 512
    rcfg = (nc, bps, sp, got, 0)
    rc, llr, st = raw_demod(e, rcfg, torch.from_numpy(out).cuda(), fs, len(data))
    assert rc == 0, e.lib.ria_gpu_last_error(e.h).decode()
    F = {"x": np.stack([oracle.mcdpsk_modulate(nc, bps, sp, d) for d in data]), "cfo": np.zeros(5, np.float32), "phase0": np.zeros(5, np.float32),
         "labels": [f"row {f}" for f in range(5)]}
    bad = differences(rcfg, F, llr.cpu().numpy(), st, *M.oracle_answers(oracle, rcfg, F)[:4])
    assert not bad, bad[0]
    bits = np.unpackbits(data, axis=1)
    hard = (llr.cpu().numpy()[:, :bits.shape[1]] < 0).astype(np.uint8)
    if bps == 1:
        assert np.array_equal(hard, bits), "a clean DBPSK round trip returns the bits"
