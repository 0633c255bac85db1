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
    for mod, rate, shape, n, seed in L.ALL_FRAME_SETS:
        key = L.set_key(mod, rate, shape)
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


@pytest.mark.parametrize("mod,rate,shape,n,seed", L.ALL_FRAME_SETS)
def test_oracle_decode_fixed_frame_equals_the_reference(oracle, fx, mod, rate, shape, n, seed):
    key = L.set_key(mod, rate, shape)
    llr, _ = L.frames(oracle, mod, rate, shape, n, seed)
    a = L.frame_answers(oracle, mod, rate, llr)
    assert np.array_equal(a["ok"], fx[f"frm_ok_{key}"]), key
    assert np.array_equal(a["data"], fx[f"frm_data_{key}"]), key


def test_frame_modes_cover_every_rate_and_symbol_size(oracle):
    assert {r for _, r in L.ALL_FRAME_MODES} == set(L.RATES.values())
    assert sorted(oracle.geom(getattr(po, m), r).bits_per_symbol for m, r in L.ALL_FRAME_MODES) == [53, 106, 153, 188, 245, 306, 376]
    assert sorted(oracle.geom(getattr(po, m), r).bytes_per_cw for m, r in L.ALL_FRAME_MODES) == [20, 27, 40, 54, 54, 60, 67]
    assert L.ALL_FRAME_SETS[:len(L.FRAME_SETS)] == L.FRAME_SETS and len(L.FRAME_SETS) == 10


MAX_ATTEMPTS = 1 + 4 + 15 + 5 + 3 + 3 + 5 + 3       # the first decode, phase 0, phases 1..6


@pytest.mark.parametrize("mod,rate,shape,n,seed", L.NEW_NOISE_SETS)
def test_noise_sets_hold_every_kind_of_frame(oracle, mod, rate, shape, n, seed):
    """each set of the four noise shapes at a new mode, from the oracle's answers: frames that decode at once, codewords a
    retry rescues, and a codeword the whole cascade fails"""
    bps = oracle.geom(getattr(po, mod), rate).bits_per_symbol
    llr, _ = L.frames(oracle, mod, rate, shape, n, seed)
    r = L._pool_map(lambda x: oracle.decode_fixed_frame(x, rate, True, bps, flags=3), list(llr))
    at_once = sum(bool(ok.all() and (att == 1).all()) for _, ok, _, att in r)
    rescued = sum(bool(((ok != 0) & (att > 1)).any()) for _, ok, _, att in r)
    failed = sum(bool(((ok == 0) & (att == MAX_ATTEMPTS)).any()) for _, ok, _, att in r)
    assert max(int(att.max()) for _, _, _, att in r) == MAX_ATTEMPTS
    assert at_once >= 2 and rescued >= 2 and failed >= 1, (at_once, rescued, failed)


@pytest.mark.parametrize("mod,rate,stage,n,seed", L.STAGE_SETS)
def test_stage_sets_are_repaired_by_their_step(oracle, mod, rate, stage, n, seed):
    """each frame of a recovery set: the cascade gives four good codewords holding wrong bytes, the recovery gives the sent
    bytes back, and the oracle names the set's step - or an earlier, wrong syndrome match wins (counted per set)"""
    llr, infos = L.frames(oracle, mod, rate, stage, n, seed)
    cl = L.recovery_classes(oracle, mod, rate, llr, infos)
    repaired = sum(c == (stage, "repaired") for c in cl)
    wrong = sum(k == "wrong" for _, k in cl)
    assert repaired >= 4 and repaired + wrong == n, cl
    assert (repaired, wrong) == L.STAGE_COUNTS[L.fill_key(mod, rate)][L.STAGES.index(stage)], cl
    # the wrong codeword rotates over the frame where the step allows it
    d3 = [oracle.decode_fixed_frame(x, rate, True, oracle.geom(getattr(po, mod), rate).bits_per_symbol, flags=3)[0] for x in llr]
    bpc = infos.shape[1] // 4
    hit = {int(np.nonzero((d != i).reshape(4, bpc).any(1))[0][0]) for d, i in zip(d3, infos)}
    assert hit == ({0} if stage in ("hdr1", "hdr2") else {2, 3} if stage == "crc" else {0, 1, 2, 3}), hit


# modes where the search of 20 000 candidates (L.FILL_SEARCH) found no frame the fallback step repairs: no fill set
FILL_EMPTY_MODES = ("QAM16_R1_2",)


def test_fill_sets_are_repaired_by_the_fallback(oracle):
    """every frame of every fill set: the cascade gives four good codewords with wrong bytes, no search step repairs them,
    and the fallback's re-decode gives the sent bytes back; every mode but the listed ones has at least two"""
    assert list(L.FILL_SEARCH) == [L.fill_key(m, r) for m, r in L.ALL_FRAME_MODES]
    for key, (searched, hits, kept) in L.FILL_SEARCH.items():
        assert searched == 20000 and len(kept) == min(hits, 4) and list(kept) == sorted(set(kept)), key
        assert (hits == 0) if key in FILL_EMPTY_MODES else (len(kept) >= 2), key
    assert [(m, n) for m, _, _, n, _ in L.FILL_SETS] == \
        [(m, len(L.FILL_SEARCH[L.fill_key(m, r)][2])) for m, r in L.ALL_FRAME_MODES if L.fill_key(m, r) not in FILL_EMPTY_MODES]
    for mod, rate, shape, n, seed in L.FILL_SETS:
        llr, infos = L.frames(oracle, mod, rate, shape, n, seed)
        assert L.recovery_classes(oracle, mod, rate, llr, infos) == [(L.FILL, "repaired")] * n, (mod, rate)


def test_fill_search_gives_the_kept_frames(oracle):
    """the search itself, repeated up to the second kept candidate of the mode where that comes earliest: its hits are the
    first two kept frames (the whole 20 000 per mode are too long for a test)"""
    i, (mod, rate) = min(((i, m) for i, m in enumerate(L.ALL_FRAME_MODES) if L.FILL_SEARCH[L.fill_key(*m)][2]),
                         key=lambda a: L.FILL_SEARCH[L.fill_key(*a[1])][2][1])
    kept = L.FILL_SEARCH[L.fill_key(mod, rate)][2]
    assert kept[1] < 1000
    _, hits = L.find_fill_frames(oracle, mod, rate, 1700 + i, budget=kept[1] + 1)
    assert tuple(hits) == kept[:2]


@pytest.mark.parametrize("mod,rate", L.ALL_FRAME_MODES)
def test_wrong_bytes_over_a_clean_channel(oracle, mod, rate):
    """the frames tests/test_gpu_frame_rates.py transmits with wrong bytes, through the oracle's own encoder, modulator and
    demodulator: the header, single-bit and CRC-field steps repair theirs, the two-bit frames are given up (L.TX_COUNTS)"""
    m = getattr(po, mod)
    bps = oracle.geom(m, rate).bits_per_symbol
    send, meant = L.wrong_bytes(oracle, mod, rate)

    def one(b):
        s = oracle.modulate(m, rate, oracle.encode_fixed_frame(b, rate, True, bps))
        llr, _ = oracle.rx_process(m, rate, s * np.float32(0.8 / np.abs(s).max()))
        return oracle.decode_fixed_frame_stage(llr, rate, True, bps)
    r = L._pool_map(one, list(send))
    assert L.tx_counts([x[4] for x in r], np.stack([x[0] for x in r]), meant) == L.TX_COUNTS[L.fill_key(mod, rate)]


@pytest.mark.parametrize("mod,rate,shape,n,seed", L.BEYOND_SETS)
def test_beyond_sets_are_not_repaired(oracle, mod, rate, shape, n, seed):
    """five wrong bits: the recovery gives up, or a wrong match of an earlier step validates other bytes"""
    llr, infos = L.frames(oracle, mod, rate, shape, n, seed)
    cl = L.recovery_classes(oracle, mod, rate, llr, infos)
    assert cl.count(("failed", "unrepaired")) >= 5 and all(k in ("unrepaired", "wrong") for _, k in cl), cl


def test_old_recovery_sets_exhaust_the_search(oracle, fx):
    """the two "recovery" sets from before the sets above stay as they are: the search exhausts without a repair (their two
    true bits sit among about 52 suspects tied at |LLR| 1, of which 30 are searched), but for one frame each where a wrong
    match validates other bytes.  No frame gives the sent bytes back."""
    want = {"QAM16": {("failed", "unrepaired"): 23, ("pair", "wrong"): 1}, "DQPSK": {("failed", "unrepaired"): 23, ("quad", "wrong"): 1}}
    for mod, rate, shape, n, seed in L.FRAME_SETS:
        if shape == "recovery":
            llr, infos = L.frames(oracle, mod, rate, shape, n, seed)
            assert L.digest(llr) == str(fx[f"sha_frm_{L.set_key(mod, rate, shape)}"])
            cl = L.recovery_classes(oracle, mod, rate, llr, infos)
            assert {c: cl.count(c) for c in set(cl)} == want[mod], mod


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
