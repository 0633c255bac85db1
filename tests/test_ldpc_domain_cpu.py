"""The oracle's LDPC decoders against the reference's answers over the decoder's whole input domain
(tests/ldpc_domain_inputs.py, answers in tests/golden/ldpc_domain.npz).  CPU only."""
import numpy as np
import pytest

import ldpc_domain_inputs as L
import pyoracle as po


@pytest.fixture(scope="module")
def fx(golden):
    return golden("ldpc_domain")


@pytest.mark.parametrize("fam", L.FAMILIES + (L.OOC,))
@pytest.mark.parametrize("rn", list(L.RATES))
def test_family_inputs_hash_to_the_recorded_values(oracle, fx, rn, fam):
    assert L.digest(L.family(oracle, L.RATES[rn], fam)) == str(fx[f"sha_{fam}_{rn}"]), f"{fam} {rn}: generator drifted"


def test_frame_inputs_hash_to_the_recorded_values(oracle, fx):
    for mod, rate, shape, n, seed in L.FRAME_SETS:
        key = f"{mod}_{[k for k, v in L.RATES.items() if v == rate][0]}_{shape}"
        assert L.digest(L.frames(oracle, mod, rate, shape, n, seed)[0]) == str(fx[f"sha_frm_{key}"]), key


def test_configs_are_the_recorded_ones(fx):
    assert np.array_equal(fx["configs"], np.array(L.CONFIGS, np.float32))


@pytest.mark.parametrize("fam", L.FAMILIES)
@pytest.mark.parametrize("rn", list(L.RATES))
def test_oracle_decoders_equal_the_reference(oracle, fx, rn, fam):
    rate, key = L.RATES[rn], f"{fam}_{rn}"
    X = L.family(oracle, rate, fam)
    a = L.decode_answers(oracle, rate, X)
    for c, (f, mi) in enumerate(L.CONFIGS):
        assert np.array_equal(a["res"][:, c], fx[f"res_{key}"][:, c]), f"{key} factor {f} max_iter {mi}: ok / iterations"
        assert np.array_equal(a["bytes"][:, c], fx[f"bytes_{key}"][:, c]), f"{key} factor {f} max_iter {mi}: bytes"
    r = L.robust_answers(oracle, rate, X)
    assert np.array_equal(r["rob"], fx[f"rob_{key}"]) and np.array_equal(r["rob_bytes"], fx[f"rob_bytes_{key}"]), key
    if fam == "waterfall":
        rows, factors = L.boundary_rows(rate, X, a)
        assert np.array_equal(rows, fx[f"bnd_rows_{key}"]) and np.array_equal(factors, fx[f"bnd_factors_{key}"])
        b = L.boundary_answers(oracle, rate, X, rows, factors)
        assert np.array_equal(b["bnd_res"], fx[f"bnd_res_{key}"]) and np.array_equal(b["bnd_bytes"], fx[f"bnd_bytes_{key}"])
        # at t* the codeword fails, at t* + 1 it converges on its last allowed iteration, at t* + 2 with one to spare
        res = b["bnd_res"].reshape(-1, 3, 2)
        t = rows[0::3, 1]
        assert (res[:, 0, 0] == 0).all() and (res[:, 0, 1] == t).all()
        assert (res[:, 1:, 0] == 1).all() and (res[:, 1, 1] == t).all() and (res[:, 2, 1] == t).all()
        assert len(t) >= 20 and (t >= 1).sum() >= 10


@pytest.mark.parametrize("mod,rate,shape,n,seed", L.FRAME_SETS)
def test_oracle_decode_fixed_frame_equals_the_reference(oracle, fx, mod, rate, shape, n, seed):
    key = f"{mod}_{[k for k, v in L.RATES.items() if v == rate][0]}_{shape}"
    llr, _ = L.frames(oracle, mod, rate, shape, n, seed)
    a = L.frame_answers(oracle, mod, rate, llr)
    assert np.array_equal(a["ok"], fx[f"frm_ok_{key}"]), key
    assert np.array_equal(a["data"], fx[f"frm_data_{key}"]), key


def test_max_iterations_zero_is_the_hard_decision_of_the_input(oracle, fx):
    """max_iterations 0: no iteration runs; ok 0, lastIterations 0 and the bytes are the hard bits (x < 0) of the input,
    -0.0 and NaN giving 0"""
    for rn, rate in L.RATES.items():
        k = oracle.code(rate).k
        for fam in L.FAMILIES + (L.OOC,):
            X = L.family(oracle, rate, fam)
            for f in L.FACTORS:
                c = L.CONFIGS.index((f, 0))
                assert not fx[f"res_{fam}_{rn}"][:, c].any(), (rn, fam, f)
                hard = np.packbits((X[:, :k] < 0).astype(np.uint8), axis=1)
                assert np.array_equal(fx[f"bytes_{fam}_{rn}"][:, c], hard), (rn, fam, f)
