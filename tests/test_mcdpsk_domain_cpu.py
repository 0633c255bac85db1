"""The oracle's MC-DPSK demodulator and modulator against the reference's answers over their input domain
(tests/mcdpsk_domain_inputs.py, answers in tests/golden/mcdpsk_domain.npz).  CPU only.

The reference has no getter for the training CFO residual and the number of valid data symbols: for those two words the
oracle is the reference, and this file checks them against float64 arithmetic and against the way the tail family is built."""
import numpy as np
import pytest

import mcdpsk_domain_inputs as M
import pyoracle as po

IDS = [M.key(c, f) for c, f in M.CASES]


@pytest.fixture(scope="module")
def fx(golden):
    return golden("mcdpsk_domain")


_ans = {}


def oracle_answers(oracle, cfg, fam):
    if (cfg, fam) not in _ans:
        _ans[(cfg, fam)] = M.oracle_answers(oracle, cfg, M.family(oracle, cfg, fam))
    return _ans[(cfg, fam)]


def check_against_fixture(fx, key, labels, llr, aux):
    assert np.array_equal(np.array([len(l) for l in llr], np.int32), fx[f"n_llr_{key}"]), f"{key}: LLR counts"
    want = fx[f"aux_{key}"]
    for f in range(len(llr)):
        for c, name in enumerate(M.AUX):
            a, w = aux[f, c:c + 1].view(np.float32)[0], want[f, c:c + 1].view(np.float32)[0]
            assert aux[f, c] == want[f, c] or (np.isnan(a) and np.isnan(w)), f"{key} frame {f} ({labels[f]}): {name} {a!r} recorded {w!r}"
        assert M.llr_digest(llr[f]) == bytes(fx[f"dig_{key}"][f]).hex(), f"{key} frame {f} ({labels[f]}): LLR digest"
    assert M.same_bits(llr[0], fx[f"llr0_{key}"].view(np.float32)), f"{key}: full LLR row of frame 0"


@pytest.mark.parametrize("cfg,fam", M.CASES, ids=IDS)
def test_inputs_hash_to_the_recorded_values(oracle, fx, cfg, fam):
    assert M.digest(M.family(oracle, cfg, fam)) == str(fx[f"sha_{M.key(cfg, fam)}"]), f"{M.key(cfg, fam)}: generator drifted"


@pytest.mark.parametrize("cfg,fam", M.CASES, ids=IDS)
def test_oracle_demodulator_equals_the_reference(oracle, fx, cfg, fam):
    llr, aux = oracle_answers(oracle, cfg, fam)[:2]
    check_against_fixture(fx, M.key(cfg, fam), M.family(oracle, cfg, fam)["labels"], llr, aux)


@pytest.mark.skipif(not po.Ref.available(), reason="oracle/_ref is not built here")
@pytest.mark.parametrize("cfg,fam", M.CASES, ids=IDS)
def test_live_reference_equals_the_recorded_answers(oracle, fx, cfg, fam):
    F = M.family(oracle, cfg, fam)
    llr, aux = M.reference_answers(po.Ref(), cfg, F)
    check_against_fixture(fx, M.key(cfg, fam), F["labels"], llr, aux)


def test_the_existing_entry_gives_the_same_answers(oracle):
    """ro_mcdpsk_demod keeps its signature and results: it is ro_mcdpsk_demod_ex without the two new words"""
    for cfg, fam in ((M.MAIN[0], "cfo"), (M.MAIN[1], "nonfinite"), (M.SHAPES[-1], "shape")):
        F = M.family(oracle, cfg, fam)
        llr, aux = oracle_answers(oracle, cfg, fam)[:2]
        for f in range(len(llr)):
            l, a = oracle.mcdpsk_demod(cfg[0], cfg[1], cfg[2], F["x"][f], float(F["cfo"][f]), float(F["phase0"][f]))
            assert M.same_bits(l, llr[f]) and M.same_bits(a, aux[f].view(np.float32))


def test_modulator_oracle_equals_the_recorded_audio(oracle, fx):
    assert np.array_equal(fx["mod_cases"], np.array([c[:4] + (("random", "zero", "one").index(c[4]),) for c in M.MOD_CASES], np.int32))
    for i, c in enumerate(M.MOD_CASES):
        x = oracle.mcdpsk_modulate(*c[:3], M.mod_data(c, i))
        assert len(x) == po.mcdpsk_frame_samples(*c[:4]), c
        assert M.audio_digest(x) == bytes(fx["mod_dig"][i]).hex(), f"modulator case {i} {c}"
    sizes = {c[3] for c in M.MOD_CASES if c[:3] == (10, 1, 1)}
    assert {0, 1, 20, 81} <= sizes and any(c[3] * 8 // (c[0] * c[1]) >= 600 for c in M.MOD_CASES)
    assert any((-8 * c[3]) % (c[0] * c[1]) == 1 for c in M.MOD_CASES) and any((-8 * c[3]) % (c[0] * c[1]) == c[0] * c[1] - 1 and c[3] for c in M.MOD_CASES)


@pytest.mark.skipif(not po.Ref.available(), reason="oracle/_ref is not built here")
def test_modulator_live_reference_equals_the_recorded_audio(fx):
    R = po.Ref()
    for i, c in enumerate(M.MOD_CASES):
        assert M.audio_digest(R.mcdpsk_modulate(*c[:3], M.mod_data(c, i))) == bytes(fx["mod_dig"][i]).hex(), f"modulator case {i} {c}"


def test_one_carrier_is_the_centre_frequency(oracle):
    """getCarrierFreqs (multi_carrier_dpsk.hpp:66-78): one carrier sits on (500 + 2500) / 2 Hz; include/ria_gpu.h takes 1..20"""
    x = oracle.mcdpsk_modulate(1, 1, 1, np.zeros(1, np.uint8))[8 * 512:9 * 512].astype(np.float64)
    assert np.argmax(np.abs(np.fft.rfft(x))) == 16            # 1500 Hz = bin 16 of 512 at 48 kHz
    import os
    with open(os.path.join(os.path.dirname(po.HERE), "include", "ria_gpu.h")) as f:
        assert "int32_t num_carriers;      /* 1..20" in f.read()


def test_every_condition_of_the_demodulator_is_taken_on_both_sides(oracle):
    """counted by the oracle itself (ro_mcdpsk_branch_counts), over every frame of the suite: each data-dependent condition
    the kernels share with it is true in at least two frames and false in at least two.
    Two sides cannot be met, by arithmetic, and are asserted to be zero:
      * 20 < scale: the noise variance is at least 0.01f, 1 / 0.01f rounds to 100.0f exactly (the quotient 100.0000022 is
        nearer to 100 than to the next float, 100.0000076), its root is 10 and scale = 2 * 10 = 20, which is not above 20;
      * gmean <= 1e-4 with a finite mean: gmean is the mean of the carrier means above 1e-4.  It is met only through
        `mean <= 1e-4` being false for a NaN or infinite mean while no carrier counts (gmean 0): nonfinite frames only."""
    true, false = np.zeros(len(po.MBC), np.int64), np.zeros(len(po.MBC), np.int64)
    gdead_finite = 0
    for cfg, fam in M.CASES:
        bc = oracle_answers(oracle, cfg, fam)[4]
        true += (bc[:, 0::2] > 0).sum(0); false += (bc[:, 1::2] > 0).sum(0)
        if fam != "nonfinite":
            gdead_finite += int(bc[:, 2 * po.MBC.index("GMEAN_DEAD")].sum())
    for i, name in enumerate(po.MBC):
        if name == "SCALE_CAP":
            assert true[i] == 0 and false[i] >= 2, (name, true[i], false[i])
        elif name.endswith("_EDGE"):         # searched for in the level family: two frames per base frame and threshold
            assert true[i] >= 4 and false[i] >= 2, f"{name}: on the threshold in {true[i]} frames"
        else:
            assert true[i] >= 2 and false[i] >= 2, f"{name}: true in {true[i]} frames, false in {false[i]}"
    assert gdead_finite == 0


def test_carrier_ratios_sit_next_to_their_thresholds(oracle):
    """the NEAR frames of the carrier family put one carrier's mean 1.5 % under and over 0.10, 0.20, 0.35 and 1.25 of the mean
    over the carriers (every other carrier of the AWGN base frame stays between 0.35 and 1.25): the oracle's weight rule takes
    the side the label names, so a threshold moved by 3 % changes an LLR"""
    cfg = M.MAIN[0]
    F = M.family(oracle, cfg, "carrier")
    bc = oracle_answers(oracle, cfg, "carrier")[4]
    col = {n + s: 2 * i + j for i, n in enumerate(po.MBC) for j, s in enumerate(("_T", "_F"))}
    seen = 0
    for f, lab in enumerate(F["labels"]):
        if "at a mean ratio of" not in lab:
            continue
        r = float(lab.split()[-1])
        got = (bc[f, col["MW_FLOOR_F"]], bc[f, col["RATIO_020_T"]], bc[f, col["RATIO_035_T"]], bc[f, col["RATIO_CAP_F"]])
        assert got == (int(r <= 0.10), int(r < 0.20), int(0.20 <= r < 0.35), int(r >= 1.25)), (lab, got)
        seen += 1
    assert seen == len(M.NEAR) == 8


def test_base_frames_cross_none_of_the_magnitude_gates(oracle):
    """the recipe of the other suites (AWGN 20 dB at peak 0.8) stays on one side of every magnitude gate"""
    for cfg in M.MAIN:
        x = M.base_frames(oracle, cfg)[0]
        oracle.mcdpsk_demod_ex(cfg[0], cfg[1], cfg[2], x)
        bc = dict(zip([n + s for n in po.MBC for s in ("_T", "_F")], oracle.mcdpsk_branch_counts()))
        for side in ("REF_AMP_F", "SYM_MAG_F", "REF_MAG_F", "TRIM_LOW_T", "MEAN_OK_F", "MEAN_DEAD_T", "GMEAN_DEAD_T", "TFI_MEAN_T", "FFI_MEAN_T",
                     "LLR_HI_F", "LLR_LO_F", "CFO_GATE_T"):
            assert bc[side] == 0, (cfg, side, bc[side])


@pytest.mark.parametrize("cfg,fam", M.CASES, ids=IDS)
def test_reference_llrs_are_finite(oracle, cfg, fam):
    """every family, nonfinite included: the reference clamps with std::max(-20, std::min(20, x)), which turns a NaN soft bit
    into +20, so no LLR is NaN or infinite whatever the samples are.  Counted on the oracle's LLRs, which
    test_oracle_demodulator_equals_the_reference pins to the reference's digests."""
    llr = np.concatenate(oracle_answers(oracle, cfg, fam)[0])
    assert np.isfinite(llr).all() and np.abs(llr).max() <= 20.0


@pytest.mark.parametrize("cfg", M.MAIN, ids=[M.key(c, "nonfinite") for c in M.MAIN])
def test_nonfinite_frames_have_the_structure_the_reference_gives_them(oracle, cfg):
    """what the recorded reference does, which is not "NaN from the poisoned symbol on":
      * training symbols 2..7 and the tail behind the last whole symbol are never read: every word equals the untouched frame's;
      * training symbol 0 reaches only the residual (NaN for NaN / inf; a finite other value for FLT_MAX);
      * a NaN or infinite reference symbol leaves only finite LLRs (NaN fails `a > 0.001`; inf / inf is NaN and clamps to +20);
      * a NaN in data symbol k fails `mag > 0.0001`, so the chain continues from (1, 0): the row is not forced to +20;
      * +-inf in data symbol k makes the normalised symbol NaN: the LLRs of symbols k and k + 1 are +20 on every carrier (a
        NaN soft bit through the clamp), and symbol k + 2 differs from its own predecessor again, so later LLRs are not."""
    F = M.family(oracle, cfg, "nonfinite")
    llr, aux, res, valid, _ = oracle_answers(oracle, cfg, "nonfinite")
    per, nds = cfg[0] * cfg[1], cfg[3]
    lab = {l: f for f, l in enumerate(F["labels"])}
    assert F["labels"][0] == "untouched" and np.isfinite(res[0]) and valid[0] == nds and not (llr[0] == 20.0).all()
    for v in ("NaN", "+inf", "-inf", "+FLT_MAX", "-FLT_MAX"):
        for where in ("training symbol 4", "the ignored tail"):
            f = lab[f"{v} in {where}"]
            assert M.same_bits(llr[f], llr[0]) and np.array_equal(aux[f], aux[0]) and res[f].view(np.uint32) == res[0].view(np.uint32) and valid[f] == nds
        f = lab[f"{v} in training symbol 0"]
        assert M.same_bits(llr[f], llr[0]) and np.array_equal(aux[f], aux[0]) and valid[f] == nds
        assert np.isnan(res[f]) if "FLT" not in v else (np.isfinite(res[f]) and res[f] != res[0])
        for _, _, k in [p for p in M.nonfinite_places(cfg) if p[2] is not None]:
            f = lab[f"{v} in data symbol {k}"]
            hit = llr[f][k * per:(k + 2) * per]
            if "inf" in v:
                before, after = llr[f][:k * per], llr[f][(k + 2) * per:]
                assert (hit == 20.0).all() and (k > 0 or len(after)) and len(hit), F["labels"][f]
                assert not (len(before) and (before == 20.0).all()) and not (len(after) and (after == 20.0).all()), F["labels"][f]
            if v == "NaN":
                assert not (hit == 20.0).all() and valid[f] == nds, F["labels"][f]
    assert not (llr[lab["data symbol 3 all NaN"]][3 * per:5 * per] == 20.0).all()
    assert np.isnan(aux[lab["cfo_hz NaN"], 0:1].view(np.float32)[0]) and M.same_bits(llr[lab["cfo_hz NaN"]], llr[0])
    for l in ("cfo_hz +inf", "phase0 NaN with cfo_hz 2"):                 # every corrected sample is NaN
        assert np.isnan(res[lab[l]]) and valid[lab[l]] == nds and aux[lab[l], 0] == 0


def test_valid_symbols_follow_the_tail_family(oracle):
    """the tail family sets the last k symbols' totals to a multiple of ref_mag: below 0.2 they are trimmed, down to four
    symbols; above they are kept; with silent first symbols (ref_mag <= 0.001) or fewer than four symbols nothing is trimmed"""
    for cfg in M.MAIN + M.TAIL_SHORT:
        F = M.family(oracle, cfg, "tail")
        valid, nds = oracle_answers(oracle, cfg, "tail")[3], cfg[3]
        for f, lab in enumerate(F["labels"]):
            if "last" in lab and "at" in lab:
                k = 1 if "the last at" in lab else int(lab.split("last ")[1].split()[0])
                fac = float(lab.split(" at ")[1].split()[0])
                want = max(min(4, nds), nds - k) if fac < 0.2 and nds >= 4 else nds
            else:
                want = nds
            assert valid[f] == want, (cfg, lab, valid[f], want)


def test_training_residual_equals_float64_arithmetic(oracle):
    """processTraining (:473-505) on frames that get no CFO correction, in float64: the float32 correlations are sums of 512
    products (relative error below 512 * 2^-24 = 3e-5 of the sum of magnitudes), so the mean phase is within 1e-4 rad and
    the residual, phase / (2 pi 512 / 48000) = 14.9 Hz per rad, within 0.01 Hz"""
    n = 0
    for cfg in M.MAIN:
        nc = cfg[0]
        mix = np.exp(-2j * np.pi * np.outer(np.arange(512), M.freqs(nc)) / 48000.0)
        for fam in ("weak", "cfo", "tail"):
            F = M.family(oracle, cfg, fam)
            res = oracle_answers(oracle, cfg, fam)[2]
            for f in range(len(res)):
                if abs(F["cfo"][f]) > np.float32(0.1):
                    continue
                y = F["x"][f][:1024].astype(np.float64).reshape(2, 512) @ mix
                er = y[1] * np.conj(y[0]) * np.exp(-1j * np.arange(nc) * np.pi / 2)
                want = np.angle(er).mean() / (2 * np.pi * 512 / 48000.0)
                if np.abs(np.abs(np.angle(er)) - np.pi).min() < 1e-3:      # a carrier on the branch cut of atan2: not comparable
                    continue
                assert abs(res[f] - want) < 0.01, (cfg, F["labels"][f], res[f], want)
                n += 1
    assert n >= 80
