"""The oracle's channel (channel, channel_cfo) and transmitter offset (apply_tx_cfo) against the compiled reference over
their input domain (tests/channel_domain_inputs.py; recorded answers in tests/golden/channel_domain.npz), and the conditions
on the expected answers that tests/test_gpu_channel_domain.py relies on.  CPU only.  Every comparison is equality of float32
bit patterns; where the expected value is NaN the other side is NaN."""
import numpy as np
import pytest

import pyoracle as po
import channel_domain_inputs as D

needs_ref = pytest.mark.skipif(not po.Ref.available(), reason="oracle/_ref is not built here")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("channel_domain")


@pytest.fixture(scope="module")
def mine(oracle):
    return D.answers(oracle, oracle)


@pytest.fixture(scope="module")
def theirs(oracle):
    return D.answers(po.Ref(), oracle)


def test_inputs_hash_to_the_recorded_value(oracle, fx):
    assert D.digest(oracle) == str(fx["sha"]), "generator drifted"


def test_families_and_sizes(oracle):
    ch, tx = D.rows(oracle)
    assert D.DELAYS == [24, 48, 96] and D.DELAY == (0, 24, 48, 96, 24)
    assert {d + k for d in D.DELAYS for k in (0, 1, 2)} <= set(D.LENGTHS)
    assert {r["family"] for r in ch} == {"lengths", "levels", "snr", "seeds", "batch", "stride", "cfo", "random", "grow", "bench"}
    assert {r["family"] for r in tx} == {"lengths", "offsets", "accumulators", "continue", "chunks", "samples", "nonfinite"}
    for r in ch:
        assert len(r["x"]) <= 600 or r["family"] == "bench" or r["cls"] == "nan1", (r["family"], r["label"])
    assert [len(r["x"]) for r in D.select(ch, "bench")] == [18432] * 3
    assert len(D.select(ch, "grow")) == 4097 and len(D.select(ch, "batch", kind=3)) == 130
    # the tx_cfo chunk rule, from the sizes its comment states: 102 transforms of 131072 points fit 256 MiB
    assert D.txcfo_chunk(131072, 1000) == (256 << 20) // (2 * 131072 * 8 + 131072 * 4) == 102
    assert D.txcfo_chunk(2, 32769) == 32768 and D.txcfo_chunk(2, 7) == 7


def check_equal(rows, A, B, skip=()):
    bad = []
    for r in rows:
        k = (r["family"], r["label"])
        if r["cls"] in skip:
            continue
        m = D.explain(r, A[k][0], B[k][0]) or D.explain(r, [A[k][1]], [B[k][1]], "actual CFO / accumulator")
        if m:
            bad.append(m)
    assert not bad, f"{len(bad)} rows differ:\n" + "\n".join(bad[:10])


@needs_ref
def test_oracle_equals_the_compiled_reference_on_every_row(oracle, mine, theirs):
    """where a row differs the fix goes into oracle/ria_oracle.c.  tx_cfo buffers with a NaN or infinite sample are outside
    bit identity (the reference's butterflies recover infinities in std::complex's operator*, the restatement and the kernel
    multiply by hand): both sides give no finite sample there"""
    ch, tx = D.rows(oracle)
    check_equal(ch, mine[0], theirs[0])
    check_equal(tx, mine[1], theirs[1], skip=("nan_sample",))
    for r in tx:
        if r["cls"] == "nan_sample":
            k = (r["family"], r["label"])
            assert not np.isfinite(theirs[1][k][0]).any() and not np.isfinite(mine[1][k][0]).any(), k
            assert D.word(theirs[1][k][1]) == D.word(mine[1][k][1]), "the accumulator does not depend on the samples"


def recorded(fx, oracle):
    rc, rt = D.recorded_rows(oracle)
    assert [f"{r['family']}|{r['label']}" for r in rc] == list(fx["c_labels"]) and [f"{r['family']}|{r['label']}" for r in rt] == list(fx["t_labels"])
    A = {(r["family"], r["label"]): (fx[f"c_{i}"], fx["c_actual"][i]) for i, r in enumerate(rc)}
    B = {(r["family"], r["label"]): (fx[f"t_{i}"], fx["t_phase"][i]) for i, r in enumerate(rt)}
    return rc, rt, A, B


def test_oracle_equals_the_recorded_answers(oracle, fx, mine):
    rc, rt, A, B = recorded(fx, oracle)
    assert len(rc) >= 5 * 7 and len(rt) >= 15
    check_equal(rc, mine[0], A)
    check_equal(rt, mine[1], B, skip=("nan_sample",))


@needs_ref
def test_live_reference_equals_the_recorded_answers(oracle, fx, theirs):
    rc, rt, A, B = recorded(fx, oracle)
    check_equal(rc, theirs[0], A)
    check_equal(rt, theirs[1], B)


# ---------------------------------------------------------------------------------------------- what the GPU test relies on
@pytest.fixture(scope="module")
def expect(oracle, mine):
    """the reference's answers where it is built; else the restatement's (pinned to it by the tests above)"""
    return D.answers(po.Ref(), oracle) if po.Ref.available() else mine


def test_rows_labelled_finite_have_no_nan(oracle, expect):
    ch, tx = D.rows(oracle)
    for part, E in ((ch, expect[0]), (tx, expect[1])):
        n = 0
        for r in part:
            if r["cls"] == "finite":
                y, a = E[(r["family"], r["label"])]
                assert not np.isnan(y).any(), (r["family"], r["label"])
                n += 1
        assert n > 100


def test_one_nan_sample_without_cfo_gives_nans_at_its_index_and_one_delay_line_later(oracle, expect):
    rows = [r for r in D.rows(oracle)[0] if r["cls"] == "nan1"]
    assert len(rows) == 5
    for r in rows:
        p, d = r["nan_at"], D.DELAY[r["kind"]]
        assert p >= 0.9 * len(r["x"]) and np.isnan(r["x"][p]) and int(np.isnan(r["x"]).sum()) == 1
        want = [p] + ([p + d + 1] if d and p + d + 1 < len(r["x"]) else [])
        assert np.nonzero(np.isnan(expect[0][(r["family"], r["label"])][0]))[0].tolist() == want, r["label"]
    assert sum(r["nan_at"] + D.DELAY[r["kind"]] + 1 < len(r["x"]) for r in rows if D.DELAY[r["kind"]]) == 4, "the delayed NaN is inside every multipath row"


def test_one_nan_sample_under_cfo_leaves_everything_before_it(oracle, expect):
    rows = [r for r in D.rows(oracle)[0] if r["cls"] == "nan_cfo"]
    assert len(rows) == 5
    for r in rows:
        p, y = r["nan_at"], expect[0][(r["family"], r["label"])][0]
        assert p >= 0.9 * len(r["x"]) and not np.isnan(y[:p]).any() and np.isnan(y[p:]).all(), r["label"]


def test_rows_labelled_nonfinite_have_no_finite_sample(oracle, expect):
    """snr NaN and -inf, the rows whose signal power overflows, the infinite samples.  An infinite or NaN channel CFO is
    not among them: applyCFO rotates sample 0 by the phase 0, which is finite, and the phase is infinite (its cosine NaN)
    from sample 1 on (rows labelled tail)"""
    ch = D.rows(oracle)[0]
    seen = set()
    for r in ch:
        y = expect[0][(r["family"], r["label"])][0]
        if r["cls"] == "nonfinite":
            assert not np.isfinite(y).any(), r["label"]
            seen.add(r["family"])
        if r["cls"] == "tail":
            assert np.isfinite(y[0]) and np.isnan(y[1:]).all(), r["label"]
            assert not np.isfinite(r["cfo"]) and not np.isnan(r["cfo"])
            seen.add("tail")
    assert seen == {"levels", "snr", "tail"}
    big = [r for r in D.select(ch, "levels") if "3e+19" in r["label"] or "3.4028" in r["label"]]
    assert len(big) == 10 and all(np.isinf(expect[0][(r["family"], r["label"])][0]).all() for r in big), "sigma +inf: every output is +-inf"
    for r in D.select(ch, "cfo"):
        if np.isnan(r["cfo"]):                           # |NaN| > 0.001 is false: the offset is not applied
            z = [q for q in D.select(ch, "cfo", kind=r["kind"]) if len(q["x"]) == len(r["x"]) and D.word(q["cfo"]) == 0 and q["seed"] == r["seed"]][0]
            assert np.array_equal(D.bits(expect[0][(r["family"], r["label"])][0]), D.bits(expect[0][(z["family"], z["label"])][0]))


def test_snr_rows(oracle, expect):
    ch = D.rows(oracle)[0]
    for kind in D.KINDS:
        E = {r["snr"] if not np.isnan(r["snr"]) else "nan": expect[0][(r["family"], r["label"])][0] for r in D.select(ch, "snr", kind=kind)}
        assert len(E) == len(D.SNRS) - 1, "-0.0 == 0.0 as a key"
        assert np.array_equal(D.bits(E[D.INF]), D.bits(E[1e30])), "sigma 0 both ways"
        # 800 dB: powf gives the denormal 1e-40, not 0; on these samples the noise is below half an ulp (the impulse rows show it)
        assert np.array_equal(D.bits(E[800.0]), D.bits(E[D.INF]))
        assert np.isnan(E["nan"]).all() and not np.isfinite(E[-D.INF]).any()
        assert np.isfinite(E[-300.0]).all() and np.abs(E[-300.0]).max() > 1e12


def test_the_two_gates_go_opposite_ways_at_0001(oracle, expect):
    """exactly +-0.001f: the channel compares |cfo| > 0.001f (not applied), applyTxCFO |cfo| < 0.001f (not copied)"""
    ch, tx = D.rows(oracle)
    g, up = float(D.CFO_GATE), float(np.nextafter(D.CFO_GATE, D.F(1)))
    for kind in D.KINDS:
        E = {D.word(r["cfo"]): expect[0][(r["family"], r["label"])][0] for r in D.select(ch, "cfo", kind=kind) if len(r["x"]) == 320}
        b = D.word
        assert np.array_equal(D.bits(E[b(g)]), D.bits(E[b(0.0)])) and np.array_equal(D.bits(E[b(-g)]), D.bits(E[b(0.0)])), kind
        assert not np.array_equal(D.bits(E[b(up)]), D.bits(E[b(0.0)])), kind
    T = {D.word(r["cfo"]): (r, expect[1][(r["family"], r["label"])]) for r in D.select(tx, "offsets") if "below" not in r["label"]}
    for v in (g, -g):
        r, (y, p) = T[D.word(v)]
        assert not np.array_equal(D.bits(y), D.bits(r["x"])) and D.word(p) != D.word(r["phase"]), v
    for v in (0.0, -0.0, float(np.nextafter(D.CFO_GATE, D.F(0)))):
        r, (y, p) = T[D.word(v)]
        assert np.array_equal(D.bits(y), D.bits(r["x"])) and D.word(p) == D.word(r["phase"]), v
    for r in tx:
        if r.get("copy"):
            y, p = expect[1][(r["family"], r["label"])]
            assert np.array_equal(D.bits(y), D.bits(r["x"])) and D.word(p) == D.word(r["phase"]), r["label"]


def test_impulse_rows_show_the_delayed_tap_at_delay_plus_1(oracle, expect):
    rows = [r for r in D.rows(oracle)[0] if r.get("impulse")]
    assert len(rows) == 5
    for r in rows:
        y, d = expect[0][(r["family"], r["label"])][0], D.DELAY[r["kind"]]
        assert r["snr"] == 800.0 and np.nonzero(r["x"])[0].tolist() == [0]
        big = np.nonzero(np.abs(y) > 1e-3)[0].tolist()
        assert big == ([0, d + 1] if d else [0]), (r["label"], big)
        assert np.abs(np.delete(y, big)).max() < 1e-37, "everything else is the denormal noise"


def test_continuation_rows_walk_one_phase_sequence(oracle, expect):
    tx = D.by_label(D.rows(oracle)[1], "continue")
    for cfo in (50.0, -2400.0):
        a, b, w = (expect[1][("continue", f"{s} cfo {cfo}")] for s in ("first call", "second call", "one walk"))
        assert D.word(b[1]) == D.word(w[1]) and D.word(a[1]) != D.word(b[1]), cfo
        assert len(tx[f"first call cfo {cfo}"]["x"]) == 200 and len(tx[f"second call cfo {cfo}"]["x"]) == 250, "both transformed at 256 points"
