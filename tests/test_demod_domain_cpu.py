"""The oracle's OFDM demodulator against the reference's answers over the demodulator's input domain
(tests/demod_domain_inputs.py, answers in tests/golden/demod_domain.npz).  CPU only."""
import numpy as np
import pytest

import demod_domain_inputs as D
import pyoracle as po


@pytest.fixture(scope="module")
def fx(golden):
    return golden("demod_domain")


_ans = {}


def oracle_answers(oracle, mode, fam):
    if (mode, fam) not in _ans:
        _ans[(mode, fam)] = D.oracle_answers(oracle, mode, D.family(oracle, mode, fam))
    return _ans[(mode, fam)]


def check_against_fixture(fx, key, labels, llr, aux, snr):
    assert len(llr) == len(fx[f"n_llr_{key}"])
    assert np.array_equal(np.array([len(l) for l in llr], np.int32), fx[f"n_llr_{key}"]), f"{key}: LLR counts"
    for f in range(len(llr)):
        for c, name in enumerate(D.AUX):
            assert aux[f, c] == fx[f"aux_{key}"][f, c] or (np.isnan(aux[f, c:c + 1].view(np.float32))[0] and np.isnan(fx[f"aux_{key}"][f, c:c + 1].view(np.float32))[0]), \
                f"{key} frame {f} ({labels[f]}): {name} {aux[f, c:c + 1].view(np.float32)[0]!r} recorded {fx[f'aux_{key}'][f, c:c + 1].view(np.float32)[0]!r}"
        assert D.llr_digest(llr[f]) == bytes(fx[f"dig_{key}"][f]).hex(), f"{key} frame {f} ({labels[f]}): LLR digest"
    assert D.same_bits(llr[0], fx[f"llr0_{key}"].view(np.float32)), f"{key}: full LLR row of frame 0"
    assert np.allclose(snr, fx[f"snr_{key}"], rtol=1e-5, atol=1e-5, equal_nan=True), f"{key}: snr_db"


@pytest.mark.parametrize("mode,fam", D.CASES)
def test_inputs_hash_to_the_recorded_values(oracle, fx, mode, fam):
    assert D.digest(D.family(oracle, mode, fam)) == str(fx[f"sha_{mode}_{fam}"]), f"{mode} {fam}: generator drifted"


@pytest.mark.parametrize("mode,fam", D.CASES)
def test_oracle_demodulator_equals_the_reference(oracle, fx, mode, fam):
    F = D.family(oracle, mode, fam)
    llr, aux, snr, _ = oracle_answers(oracle, mode, fam)
    check_against_fixture(fx, f"{mode}_{fam}", F["labels"], llr, aux, snr)


@pytest.mark.skipif(not po.Ref.available(), reason="oracle/_ref is not built here")
@pytest.mark.parametrize("mode,fam", D.CASES)
def test_live_reference_equals_the_recorded_answers(oracle, fx, mode, fam):
    F = D.family(oracle, mode, fam)
    llr, aux, snr = D.reference_answers(po.Ref(), mode, F)
    check_against_fixture(fx, f"{mode}_{fam}", F["labels"], llr, aux, snr)


@pytest.mark.parametrize("mode,fam", D.CASES)
def test_reference_llrs_are_finite(oracle, fx, mode, fam):
    """every family but nonfinite: no NaN and no inf in the LLRs; nonfinite: at most 1 % NaN.  Counted on the oracle's
    LLRs, which test_oracle_demodulator_equals_the_reference pins to the reference's digests."""
    llr = np.concatenate(oracle_answers(oracle, mode, fam)[0])
    if fam == "nonfinite":
        assert np.isnan(llr).sum() <= 0.01 * llr.size, f"{int(np.isnan(llr).sum())} of {llr.size} LLRs are NaN"
    else:
        assert np.isfinite(llr).all(), f"{int((~np.isfinite(llr)).sum())} of {llr.size} LLRs are not finite"


@pytest.mark.parametrize("mode", [m for m, f in D.CASES if f == "residual"])
def test_residual_frames_lie_on_both_sides_of_both_limits(oracle, mode):
    """channel_equalizer.cpp:327: the training symbols are transformed again when 0.3 Hz < |residual| < 5 Hz.  A frame
    takes the re-run when the corrected CFO differs from the CFO told.  Per sign: two frames under 0.3 Hz and two over
    5 Hz that do not take it, two just over 0.3 Hz and two just under 5 Hz that do."""
    F = D.family(oracle, mode, "residual")
    taken = oracle_answers(oracle, mode, "residual")[1][:, 0].view(np.float32) != F["cfo"]
    k, groups = 0, {}
    for r in D.RESIDUALS:
        for sg in ((1,) if r == 0 else (1, -1)):
            band = "zero" if r == 0 else "under 0.3" if r < 0.3 else "over 0.3" if r < 1 else "mid" if r < 3 else "under 5" if r < 5 else \
                "over 5" if r < 10 else "far"
            groups.setdefault((band, sg), []).append(bool(taken[k]))
            k += 1
    for sg in (1, -1):
        for band, want in (("under 0.3", False), ("over 0.3", True), ("under 5", True), ("over 5", False)):
            got = groups[(band, sg)]
            assert len(got) >= 2 and all(t == want for t in got), f"{mode} sign {sg} {band} Hz: re-run taken {got}"
    assert groups[("zero", 1)] == [False] and not any(groups[("far", 1)] + groups[("far", -1)])


def test_notch_frames_on_d8psk_lie_on_both_sides_of_the_two_pass_gate(oracle):
    fad = oracle_answers(oracle, "D8PSK_R1_2", "notch")[1][:, 1].view(np.float32)
    assert (fad > 0.30).sum() >= 3 and (fad <= 0.30).sum() >= 3, fad


def test_level_frames_put_carriers_on_both_sides_of_the_channel_gate(oracle):
    """|H| > 0.01 (channel_equalizer.cpp:316, :352, :607): the three searched scales of each base frame leave some
    carriers above and some below; the smallest level leaves none above, 1e6 none below"""
    for mode in D.MODES:
        F = D.family(oracle, mode, "level")
        h = oracle_answers(oracle, mode, "level")[3]
        mag = np.hypot(h[:, 0::2].astype(np.float64), h[:, 1::2].astype(np.float64))
        above = (mag > 0.01).sum(1)
        mixed = [f for f, lab in enumerate(F["labels"]) if "across" in lab]
        assert len(mixed) == 6 and all(0 < above[f] < 59 for f in mixed), (mode, above[mixed])
        assert above[0] == 0 and above[D.LEVELS.index(1e6)] == 59, (mode, above[0], above[D.LEVELS.index(1e6)])


def test_meta_stays_inside_the_short_wrap(oracle):
    """the GPU tests pass only metadata whose initial-phase wrap is short (include/ria_gpu.h bounds the product)"""
    for mode, fam in D.CASES:
        F = D.family(oracle, mode, fam)
        ip = 2.0 * np.pi * F["cfo"].astype(np.float64) * F["pos"].astype(np.float64) / 48000.0
        assert np.isfinite(F["cfo"]).all() and (np.abs(ip) <= D.MAX_WRAP_RAD).all(), (mode, fam)
    F = D.family(oracle, "QAM16_R1_2", "meta")
    assert len(F["x"]) >= 40 and int(F["pos"].max()) == 2 ** 36 and (F["flags"] > 1).sum() >= 5


def test_every_branch_condition_of_the_demodulator_is_taken(oracle):
    """counted by the oracle itself (ro_branch_counts): the data-dependent thresholds the kernels share with it are crossed
    by frames of QAM16 R1/2 (snv < 1e-6 exists on the differential path only: DQPSK level), the D8PSK two-pass gate by
    D8PSK notch frames on both sides, the 1-bit demapper's sp < 1e-6 by DBPSK silence; the recipe of the other suites
    (the AWGN base frame at peak 0.8) crosses none of the magnitude thresholds.
    Two conditions cannot be met by any frame here, by arithmetic: mag > 1e-6 is only tested after both |H| > 0.01, so
    mag >= 1e-4 unless it is NaN; and the per-carrier noise nv / (|H|^2 + nv) never exceeds 1, so its clamp at 100 only
    ever sees the 100 the code itself assigns."""
    hit = np.zeros(len(D.BRANCHES), np.int64)
    for fam in D.FAMILIES:
        hit += (D.branch_counts(oracle, "QAM16_R1_2", D.family(oracle, "QAM16_R1_2", fam)) > 0).sum(0)
    hit = dict(zip(D.BRANCHES, hit))
    for name in ("H_SMALL", "CNT_SMALL", "RERUN", "SNR_LOW", "SNR_HIGH", "HM_SMALL", "CNV_LOW"):
        assert hit[name] >= 2, f"{name}: taken by {hit[name]} QAM16 R1/2 frames"
    assert hit["DEN_SMALL"] >= 1 and hit["MAG_SMALL"] == 0 and hit["CNV_HIGH"] == 0, hit
    snv = D.branch_counts(oracle, "DQPSK_R1_4", D.family(oracle, "DQPSK_R1_4", "level"))[:, D.BRANCHES.index("SNV_SMALL")]
    assert (snv > 0).sum() >= 2 and (snv == 0).sum() >= 2, snv
    two = D.branch_counts(oracle, "D8PSK_R1_2", D.family(oracle, "D8PSK_R1_2", "notch"))[:, D.BRANCHES.index("D8PSK_TWO_PASS")]
    # the gate is tested at every data symbol on the tracked fading index: frames with every symbol through it, frames with some
    assert (two == two.max()).sum() >= 3 and (two < two.max()).sum() >= 3, two
    sp = D.branch_counts(oracle, "DBPSK_R1_4", D.family(oracle, "DBPSK_R1_4", "silence"))[:, D.BRANCHES.index("SP_SMALL")]
    assert (sp > 0).sum() >= 3, sp
    x = D.base_frames(oracle, "QAM16_R1_2")[0][None]
    base = D.branch_counts(oracle, "QAM16_R1_2", {"x": x, "cfo": np.zeros(1, np.float32), "pos": np.zeros(1, np.uint64), "flags": np.zeros(1, np.uint32)})
    for name in ("H_SMALL", "MAG_SMALL", "CNT_SMALL", "SNV_SMALL", "DEN_SMALL", "SP_SMALL"):
        assert base[0, D.BRANCHES.index(name)] == 0, name
