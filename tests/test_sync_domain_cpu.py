"""The oracle's four acquisition detectors against the reference's answers over their input domain
(tests/sync_domain_inputs.py, answers in tests/golden/sync_domain.npz), and the conditions that keep a family from
degenerating, checked on the reference's recorded answers.  CPU only."""
import numpy as np
import pytest

import pyoracle as po
import sync_domain_inputs as S


@pytest.fixture(scope="module")
def fx(golden):
    return golden("sync_domain")


def mismatches(det, F, got, exp):
    nf = len(S.FIELDS[det])
    return [f"buffer {i} ({F['labels'][i]}): {name} {got[i, c]!r} reference {exp[i, c]!r}"
            for i in range(len(exp)) for c, name in enumerate(S.FIELDS[det]) if not S.same_bits(got[i, c:c + 1], exp[i, c:c + 1])] + \
           [f"buffer {i}: unused words not zero" for i in range(len(exp)) if got[i, nf:].any() or exp[i, nf:].any()]


@pytest.mark.parametrize("det,fam", S.CASES)
def test_inputs_hash_to_the_recorded_values(oracle, fx, det, fam):
    assert S.digest(S.family(oracle, det, fam)) == str(fx[f"sha_{det}_{fam}"]), f"{det} {fam}: generator drifted"


@pytest.mark.parametrize("det,fam", S.CASES)
def test_oracle_detector_equals_the_reference(oracle, fx, det, fam):
    F = S.family(oracle, det, fam)
    bad = mismatches(det, F, S.answers(oracle, det, F), fx[f"ans_{det}_{fam}"])
    assert not bad, f"{det} {fam}: {len(bad)} fields differ\n" + "\n".join(bad[:10])


@pytest.mark.skipif(not po.Ref.available(), reason="oracle/_ref is not built here")
@pytest.mark.parametrize("det,fam", S.CASES)
def test_live_reference_equals_the_recorded_answers(oracle, fx, det, fam):
    F = S.family(oracle, det, fam)
    bad = mismatches(det, F, S.answers(po.Ref(), det, F), fx[f"ans_{det}_{fam}"])
    assert not bad, f"{det} {fam}: {len(bad)} fields differ\n" + "\n".join(bad[:10])


@pytest.mark.parametrize("det", S.DETECTORS)
def test_position_buffers_with_a_whole_preamble_are_detected(oracle, fx, det):
    F = S.family(oracle, det, "position")
    a = fx[f"ans_{det}_position"]
    whole = F["whole"]
    assert whole.sum() >= 12 and (~whole).sum() >= 1
    assert (a[whole, 0] == 1).sum() >= 0.75 * whole.sum(), (det, a[whole, 0])


@pytest.mark.parametrize("det", ("zc", "chirp", "lts"))
def test_threshold_buffers_flip_on_the_reported_correlation(oracle, fx, det):
    """ZC and LTS detect with correlation > threshold: detected one float below the reported correlation, not on it.
    Chirp rejects with correlation < threshold on the transform path and accepts with >= on the time-domain path: detected
    on the up (down) correlation, not one float above it."""
    F = S.family(oracle, det, "threshold")
    a = fx[f"ans_{det}_threshold"]
    thr = F["thr"]
    col = {"zc": (3,), "chirp": (4, 5), "lts": (2,)}[det]
    flips = 0
    for i in range(1, len(thr) - 1):
        if not (np.array_equal(F["x"][i - 1], F["x"][i]) and np.array_equal(F["x"][i], F["x"][i + 1])):
            continue
        if not (np.nextafter(thr[i], np.float32(-1)) == thr[i - 1] and np.nextafter(thr[i], np.float32(2)) == thr[i + 1]):
            continue
        # the triple sits on the correlation the detector compares: the run on it reports it (chirp: the smaller of its two)
        on = a[i]
        c = on[col[0]] if det != "chirp" else min(on[4], on[5])
        if np.float32(c).view(np.uint32) != thr[i].view(np.uint32):
            continue
        d = a[i - 1:i + 2, 0]
        assert (d[0], d[2]) == (1, 0), (det, F["labels"][i], d)
        assert d[1] == (0 if det in ("zc", "lts") else 1), (det, F["labels"][i], d)
        flips += 1
    assert flips >= 3, (det, flips)
    edge = {t: a[[i for i in range(len(thr)) if (np.isnan(t) and np.isnan(thr[i])) or thr[i] == t], 0] for t in S.EDGE_THR}
    assert ((edge[-1.0] == 1).all() if det != "chirp" else (edge[-1.0] == 1).any()) and (edge[2.0] == 0).all() and (edge[np.inf] == 0).all()
    # a NaN threshold: `corr > NaN` never detects; the chirp transform path's `corr < NaN` never rejects
    assert (edge[np.nan] == 0).all() if det != "chirp" else (edge[np.nan] == 1).any()


def test_zc_threshold_family_crosses_the_internal_levels(oracle, fx):
    """combined metric below and above 0.25 (zc_sync.hpp:280), the SNR clamp at 0.01 (:628-633).  The clamp at 0.99 cannot be
    reached: by Cauchy-Schwarz the correlation of real samples with the complex reference stays near 1/sqrt(2)."""
    a = fx["ans_zc_threshold"]
    det = a[:, 0] == 1
    corr = a[det, 3]
    assert (corr < 0.25).sum() >= 2 and (corr >= 0.25).sum() >= 2 and (corr <= 0.01).sum() >= 1 and corr.max() < 0.99, corr
    assert (a[det, 5] == -10.0).any() and ((a[det, 5] > -10.0) & (a[det, 5] < 30.0)).any()


@pytest.mark.parametrize("det", S.DETECTORS)
def test_level_has_detecting_and_non_detecting_scales(oracle, fx, det):
    F = S.family(oracle, det, "level")
    a = fx[f"ans_{det}_level"]
    assert (a[:, 0] == 1).sum() >= 4 and (a[:, 0] == 0).sum() >= 4, (det, a[:, 0])
    gates = [i for i, lab in enumerate(F["labels"]) if "the " in lab]
    assert len(gates) >= 6


@pytest.mark.parametrize("det", S.DETECTORS)
def test_nonfinite_and_meta_families_hold_what_they_say(oracle, det):
    F = S.family(oracle, det, "nonfinite")
    kinds = [(np.isnan(x).sum(), np.isposinf(x).sum(), np.isneginf(x).sum(), (np.abs(x) == S.FLT_MAX).sum()) for x in F["x"]]
    assert sum(k[0] == 1 for k in kinds) >= 5 and sum(k[1] == 1 for k in kinds) >= 5 and sum(k[2] == 1 for k in kinds) >= 5
    assert sum(k[3] >= 1 for k in kinds) >= 3 and any(k[0] == len(x) for k, x in zip(kinds, F["x"]))
    if det != "chirp":
        M = S.family(oracle, det, "meta")
        assert np.isnan(M["p"]).any() and np.isinf(M["p"]).any()
    if det == "zc":
        assert set(M["mask"].tolist()) == set(range(16))


_bc = {}


def branch_hits(oracle, det, fam):
    """buffers of a family on which the oracle found each condition true / false at least once -> int [len(S.BRANCHES)]"""
    if (det, fam) not in _bc:
        _bc[(det, fam)] = (S.branch_counts(oracle, det, S.family(oracle, det, fam)) > 0).sum(0)
    return _bc[(det, fam)]


# ZC_SNR_HIGH: corr >= 0.99 is out of reach of real samples (Cauchy-Schwarz); everything else goes both ways
UNREACHABLE = ("ZC_SNR_HIGH_T",)


@pytest.mark.parametrize("det", S.DETECTORS)
def test_every_branch_condition_of_a_detector_goes_both_ways(oracle, det):
    """counted by the oracle itself (ro_sync_branch_counts), which test_oracle_detector_equals_the_reference pins to the
    reference on the same buffers: every data-dependent condition is true on at least one buffer and false on at least one"""
    hit = sum(branch_hits(oracle, det, fam) for d, fam in S.CASES if d == det)
    for i, name in enumerate(S.BRANCHES):
        if name.startswith(S.PREFIX[det]) and not name.endswith("_TIE"):
            assert (hit[i] == 0) == (name in UNREACHABLE), f"{name}: {hit[i]} buffers"


@pytest.mark.parametrize("det", ("zc", "chirp", "cox"))   # the LTS metric adds 1e-10 to its denominator: it has no gate
def test_level_scales_sit_on_both_sides_of_the_denominator_gate(oracle, det):
    name = {"zc": "ZC_DENOM", "chirp": "CH_DENOM", "cox": "COX_NORM"}[det]
    F = S.family(oracle, det, "level")
    c = S.branch_counts(oracle, det, F)
    t, f = c[:, S.BRANCHES.index(name + "_T")], c[:, S.BRANCHES.index(name + "_F")]
    for b in (0, 1) if det != "chirp" else (0,):
        lo = [i for i, lab in enumerate(F["labels"]) if lab.startswith(f"base{b}") and "below the denominator gate" in lab]
        hi = [i for i, lab in enumerate(F["labels"]) if lab.startswith(f"base{b}") and "above the denominator gate" in lab]
        assert len(lo) == 1 and len(hi) == 1
        # below: no window passes the gate (ZC, chirp: _T counts passes; Cox: _T counts failures); above: the preamble's do
        passes = (lambda i: f[i]) if det == "cox" else (lambda i: t[i])
        assert passes(lo[0]) == 0 and passes(hi[0]) > 0, (det, b, passes(lo[0]), passes(hi[0]))


@pytest.mark.parametrize("det", S.DETECTORS)
def test_ties_family_holds_lags_with_bit_equal_metric(oracle, det):
    """a maximum search of the oracle met a lag whose metric equals the running maximum bit for bit: the first-maximum rule
    decided the position"""
    tie = S.branch_counts(oracle, det, S.family(oracle, det, "ties"))[:, S.BRANCHES.index(S.PREFIX[det] + "TIE")]
    assert (tie > 0).sum() >= 1, (det, tie)


def test_zc_buffers_lie_on_both_sides_of_the_earlier_repetition_ratio(oracle):
    """zc_sync.hpp:268: the four searched buffers put the earlier repetition below and above 0.4 of the peak, the two middle
    ones as close as the search came"""
    F = S.family(oracle, "zc", "threshold")
    idx = [i for i, lab in enumerate(F["labels"]) if "earlier repetition" in lab]
    c = S.branch_counts(oracle, "zc", {k: ([v[i] for i in idx] if isinstance(v, list) else v[idx]) for k, v in F.items()})
    t, f = c[:, S.BRANCHES.index("ZC_EARLIER_T")], c[:, S.BRANCHES.index("ZC_EARLIER_F")]
    assert t.tolist() == [0, 0, 1, 1] and f.tolist() == [1, 1, 0, 0], (t, f)
