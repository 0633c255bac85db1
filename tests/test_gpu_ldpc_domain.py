"""The HIP LDPC decoders against the reference over the decoder's whole input domain (tests/ldpc_domain_inputs.py):
ria_gpu_ldpc_decode_batch, ria_gpu_ldpc_decode_robust_batch and ria_gpu_decode_batch, bit for bit in every field.
Reference answers come live from oracle/_ref where it is built, else from tests/golden/ldpc_domain.npz."""
import numpy as np
import pytest

import ldpc_domain_inputs as L
import pyoracle as po

pytestmark = pytest.mark.gpu

RATE_NAME = {v: k for k, v in L.RATES.items()}
_engines, _answers = {}, {}


def engine(mod, rn):
    from ria_amd.engine import RxEngine
    if (mod, rn) not in _engines:
        _engines[(mod, rn)] = RxEngine(mod, rn)
    return _engines[(mod, rn)]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def answers(golden, oracle, rn, fam, canon=False):
    """the reference's answers for one family at one rate: live from the compiled reference, else the fixture"""
    key = (rn, fam, canon)
    if key not in _answers:
        rate = L.RATES[rn]
        X = L.family(oracle, rate, fam)
        fx = golden("ldpc_domain")
        assert L.digest(X) == str(fx[f"sha_{fam}_{rn}"]), f"{fam} {rn}: generator drifted"
        tag = f"_canon_{fam}_{rn}" if canon else f"_{fam}_{rn}"
        if po.Ref.available():
            R = po.Ref()
            Y = L.canon(X) if canon else X
            a = {**L.decode_answers(R, rate, Y), **L.robust_answers(R, rate, Y)}
            if fam == "waterfall":
                rows, factors = L.boundary_rows(rate, X, a)
                a.update(bnd_rows=rows, bnd_factors=factors, **L.boundary_answers(R, rate, X, rows, factors))
        else:
            names = ("res", "bytes", "rob", "rob_bytes") + (("bnd_rows", "bnd_factors", "bnd_res", "bnd_bytes") if fam == "waterfall" else ())
            a = {k: fx[k + tag] for k in names}
        _answers[key] = a
    return _answers[key]


def gpu_single(e, X, mi, f):
    out, ok, it = e.ldpc_decode(dev(X), mi, f)
    return out.cpu().numpy(), ok.cpu().numpy().astype(np.int32), it.cpu().numpy().astype(np.int32)


def gpu_robust(e, X):
    out, ok, it, tr = e.ldpc_decode_robust(dev(X))
    return out.cpu().numpy(), np.stack([ok.cpu().numpy(), tr.cpu().numpy(), it.cpu().numpy()], 1).astype(np.int32)


def check_single(e, X, a, what):
    for c, (f, mi) in enumerate(L.CONFIGS):
        out, ok, it = gpu_single(e, X, mi, f)
        bad = np.nonzero((ok != a["res"][:, c, 0]) | (it != a["res"][:, c, 1]) | (out != a["bytes"][:, c]).any(1))[0]
        assert len(bad) == 0, (f"{what} factor {f} max_iter {mi}: {len(bad)} rows differ, first {bad[0]}: gpu ok/it "
                               f"{ok[bad[0]]}/{it[bad[0]]} ref {a['res'][bad[0], c]}")


@pytest.mark.parametrize("fam", L.FAMILIES)
@pytest.mark.parametrize("rn", list(L.RATES))
def test_single_decoder_equals_the_reference(golden, oracle, rn, fam):
    e = engine("QAM16", rn)
    X = L.family(oracle, L.RATES[rn], fam)
    a = answers(golden, oracle, rn, fam)
    check_single(e, X, a, f"{rn} {fam}")
    # max_iterations 0: the hard bits of the input, ok 0, iterations 0
    out, ok, it = gpu_single(e, X, 0, 0.9375)
    k = e.geo.ldpc_k
    assert not ok.any() and not it.any() and np.array_equal(out, np.packbits((X[:, :k] < 0).astype(np.uint8), axis=1))
    if fam == "waterfall":   # iteration boundary: t*, t*+1, t*+2 of every converged row
        rows, factors = a["bnd_rows"], a["bnd_factors"]
        assert len(rows) >= 60
        for f in np.unique(factors):
            sel = np.nonzero(factors == f)[0]
            for mi in np.unique(rows[sel, 1]):
                s2 = sel[rows[sel, 1] == mi]
                out, ok, it = gpu_single(e, X[rows[s2, 0]], int(mi), float(f))
                assert np.array_equal(ok, a["bnd_res"][s2, 0]) and np.array_equal(it, a["bnd_res"][s2, 1]), (rn, f, mi)
                assert np.array_equal(out, a["bnd_bytes"][s2]), (rn, f, mi)


@pytest.mark.parametrize("fam", L.FAMILIES)
@pytest.mark.parametrize("rn", list(L.RATES))
def test_robust_decoder_equals_the_reference(golden, oracle, rn, fam):
    e = engine("QAM16", rn)
    X = L.family(oracle, L.RATES[rn], fam)
    a = answers(golden, oracle, rn, fam)
    out, rti = gpu_robust(e, X)
    assert np.array_equal(rti, a["rob"]), f"{rn} {fam}: ok / tries / iterations"
    assert np.array_equal(out, a["rob_bytes"]), f"{rn} {fam}: bytes"


@pytest.mark.parametrize("rn", list(L.RATES))
def test_out_of_contract_inputs_as_the_header_states(golden, oracle, rn):
    """NaN, +-inf and |x| > 1e30: the GPU decodes canon(x) (include/ria_gpu.h).  Rows where the reference on the raw
    input agrees are asserted against the raw answers too; every row must equal the reference on canon(x)."""
    e = engine("QAM16", rn)
    X = L.family(oracle, L.RATES[rn], L.OOC)
    raw, can = answers(golden, oracle, rn, L.OOC), answers(golden, oracle, rn, L.OOC, canon=True)
    check_single(e, X, can, f"{rn} out of contract vs reference(canon(x))")
    out, rti = gpu_robust(e, X)
    assert np.array_equal(rti, can["rob"]) and np.array_equal(out, can["rob_bytes"])
    # the mapping is the whole difference: where canon(x) == x bit for bit the raw answers are the same
    same = (L.canon(X).view(np.uint32) == X.view(np.uint32)).all(1)
    assert np.array_equal(raw["res"][same], can["res"][same]) and np.array_equal(raw["bytes"][same], can["bytes"][same])


BATCH_SIZES = (1, 63, 64, 65, 16384, 16385, 3 * 16384 + 7)


@pytest.mark.parametrize("rn", ["R1_4", "R1_2", "R5_6"])
def test_batch_size_and_position_do_not_change_a_row(golden, oracle, rn):
    """n_cw beyond the 16384-block grid: one wave decodes several codewords in turn.  Every row of a large, shuffled
    batch tiled from reference-checked rows equals its own single-row result."""
    e = engine("QAM16", rn)
    rate = L.RATES[rn]
    base = np.concatenate([L.family(oracle, rate, f) for f in L.FAMILIES])
    a = {f: answers(golden, oracle, rn, f) for f in L.FAMILIES}
    c = L.CONFIGS.index((0.9375, 80))
    ref_res = np.concatenate([a[f]["res"][:, c] for f in L.FAMILIES])
    ref_bytes = np.concatenate([a[f]["bytes"][:, c] for f in L.FAMILIES])
    ref_rob = np.concatenate([a[f]["rob"] for f in L.FAMILIES])
    ref_rob_bytes = np.concatenate([a[f]["rob_bytes"] for f in L.FAMILIES])
    rng = np.random.default_rng(4040 + rate)
    for n in BATCH_SIZES:
        idx = rng.permutation(np.resize(np.arange(len(base)), max(n, len(base))))[:n]
        out, ok, it = gpu_single(e, base[idx], 80, 0.9375)
        assert np.array_equal(ok, ref_res[idx, 0]) and np.array_equal(it, ref_res[idx, 1]), f"{rn} n={n}"
        assert np.array_equal(out, ref_bytes[idx]), f"{rn} n={n}"
        out, rti = gpu_robust(e, base[idx])
        assert np.array_equal(rti, ref_rob[idx]) and np.array_equal(out, ref_rob_bytes[idx]), f"{rn} robust n={n}"


def check_frame_family(golden, oracle, monkeypatch, mod, rate, shape, n, seed):
    """decodeFixedFrame on one set of ldpc_domain_inputs.frames: bytes and cw_ok against the reference, iterations, attempts
    and frame_valid against the oracle, device recovery against the host recovery, with and without the channel
    de-interleaver.  (tests/test_gpu_frame_rates.py runs the sets at all six code rates through it.)"""
    from ria_amd import capi
    rn = RATE_NAME[rate]
    e = engine(mod, rn)
    key = L.set_key(mod, rate, shape)
    fx = golden("ldpc_domain")
    g = oracle.geom(getattr(po, mod), rate)
    bpc, bps = g.bytes_per_cw, g.bits_per_symbol
    for ch in (True, False):
        llr, _ = L.frames(oracle, mod, rate, shape, n, seed, ch_deint=ch)
        if ch:
            assert L.digest(llr) == str(fx[f"sha_frm_{key}"]), key
            ref = L.frame_answers(po.Ref(), mod, rate, llr) if po.Ref.available() else \
                {"ok": fx[f"frm_ok_{key}"], "data": fx[f"frm_data_{key}"]}
        flag_ch = 0 if ch else capi.DECODE_NO_CHANNEL_DEINTERLEAVE
        x = dev(llr)
        res = {}
        for name, flags in (("full", capi.DECODE_FULL), ("raw", capi.DECODE_PHASE0 | capi.DECODE_PERTURB)):
            monkeypatch.delenv("RIA_RECOVERY_HOST", raising=False)
            d, st = e.decode(x, flags=flags | flag_ch)
            res[name] = (d.cpu().numpy(), e.decode_status(st).copy())
            for f in range(n):
                do, oko, it, att = oracle.decode_fixed_frame(llr[f], rate, ch, bps, flags=flags)
                d_f, s = res[name][0][f], res[name][1]
                assert np.array_equal(s["cw_ok"][f], oko), (key, ch, name, f)
                assert np.array_equal(d_f, do), (key, ch, name, f)
                assert np.array_equal(s["iterations"][f], it.astype(np.uint16)), (key, ch, name, f)
                assert np.array_equal(s["attempts"][f], att.astype(np.uint8)), (key, ch, name, f)
        d, s = res["full"]
        assert not s["needs_recovery"].any()
        assert np.array_equal(s["cw_ok"], ref["ok"]), (key, ch)
        assert np.array_equal(d * np.repeat(s["cw_ok"] != 0, bpc, axis=1), ref["data"]), (key, ch)
        assert np.array_equal(s["frame_valid"] != 0, ref["ok"].all(1)), (key, ch)
        monkeypatch.setenv("RIA_RECOVERY_HOST", "1")
        dh, sth = e.decode(x, flags=capi.DECODE_FULL | flag_ch)
        monkeypatch.delenv("RIA_RECOVERY_HOST", raising=False)
        sth = e.decode_status(sth)
        assert np.array_equal(dh.cpu().numpy(), d), (key, ch)
        for k in ("cw_ok", "frame_valid", "needs_recovery", "iterations", "attempts"):
            assert np.array_equal(sth[k], s[k]), (key, ch, k)
        if shape == "recovery":
            flagged = int(res["raw"][1]["needs_recovery"].sum())
            assert flagged >= 20, f"{key}: only {flagged} frames flagged for the CRC recovery"


@pytest.mark.parametrize("mod,rate,shape,n,seed", L.FRAME_SETS)
def test_decode_fixed_frame_families(golden, oracle, monkeypatch, mod, rate, shape, n, seed):
    """decodeFixedFrame on real frames mapped to the erasure / ties / clamp / tiny shapes and on frames that converge to a
    wrong codeword (CRC recovery with suspects tied on |LLR|, a search that exhausts without a repair): bytes and cw_ok
    against the reference, iterations, attempts and frame_valid against the oracle, device recovery against the host
    recovery, with and without the channel de-interleaver."""
    check_frame_family(golden, oracle, monkeypatch, mod, rate, shape, n, seed)
