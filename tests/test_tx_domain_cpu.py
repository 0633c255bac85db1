"""The oracle's transmit chain (encode_fixed_frame, modulate, make_frame) against the reference's answers over the
transmit chain's input domain (tests/tx_domain_inputs.py, answers in tests/golden/tx_domain.npz), the conditions the input
sets must meet, and the plain restatements of make_frames and of the peak rule the GPU tests compare with.  CPU only.
Every comparison is equality of bytes or of float32 bit patterns."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pyoracle as po
import tx_domain_inputs as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE_NAMES = list(T.MODES)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("tx_domain")


def check_against_fixture(fx, mode, S, coded, samples):
    labels = S["info_labels"] + S["coded_labels"]
    assert coded.shape == fx[f"coded_{mode}"].shape and len(samples) == len(fx[f"dig_{mode}"]) == len(labels)
    for f in range(len(coded)):
        assert np.array_equal(coded[f], fx[f"coded_{mode}"][f]), f"{mode} info row {f} ({labels[f]}): coded bytes"
    for f, s in enumerate(samples):
        assert T.sample_digest(s) == bytes(fx[f"dig_{mode}"][f]).hex(), f"{mode} row {f} ({labels[f]}): sample digest"
        assert np.abs(s).max().view(np.uint32) == fx[f"mx_{mode}"][f].view(np.uint32), f"{mode} row {f} ({labels[f]}): max |s|"


def test_all_54_configurations_have_a_set_and_the_reference_refused_none(fx):
    assert len(T.MODES) == 54 and len({m for m, _ in T.MODES.values()}) == 9 and len({r for _, r in T.MODES.values()}) == 6
    assert list(fx["refused"]) == [], "a refused configuration is tested against the oracle only and listed in DESIGN.md"
    for mode in MODE_NAMES:
        assert f"coded_{mode}" in fx.files and f"dig_{mode}" in fx.files


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_inputs_hash_to_the_recorded_value(oracle, fx, mode):
    assert T.digest(T.input_set(oracle, mode)) == str(fx[f"sha_{mode}"]), f"{mode}: generator drifted"


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_oracle_geometry_equals_the_reference(oracle, fx, mode):
    assert np.array_equal(T.geometry(oracle, mode), fx[f"geom_{mode}"]), (mode, T.geometry(oracle, mode), fx[f"geom_{mode}"])
    g = T.geometry(oracle, mode)
    assert g[5] == -(-T.FRAME_BITS // g[4]) and g[6] == (2 + g[5]) * T.SYM and g[1] + g[2] == 59


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_oracle_encoder_and_modulator_equal_the_reference(oracle, fx, mode):
    S = T.input_set(oracle, mode)
    coded, samples = T.answers(oracle, oracle, mode)
    check_against_fixture(fx, mode, S, coded, samples)
    assert min(float(np.abs(s).max()) for s in samples) > 0, "the LTS symbols are never silent"


@pytest.mark.skipif(not po.Ref.available(), reason="oracle/_ref is not built here")
@pytest.mark.parametrize("mode", [m for m in MODE_NAMES if m.endswith(("R1_4", "R5_6"))])
def test_live_reference_equals_the_recorded_answers(oracle, fx, mode):
    """the compiled reference, where it is built, gives what the fixture holds.  Through the wrapper's entry points that
    every build of it has (ref_encode_fixed_frame, ref_modulate, ref_tx_frame, ref_tx_frame_nvis): every info row's coded
    bytes; for the eight modulations OFDMChirpWaveform takes, every row's samples and the geometry; for QAM256, whose
    modulator on arbitrary coded bytes is reached only through ref_modulate_nvis (the recipe's), the two valid frames
    through Ref.tx_frame(nvis=True)."""
    mod, rate = T.MODES[mode]
    S, R = T.input_set(oracle, mode), po.Ref()
    geom = fx[f"geom_{mode}"]
    labels = S["info_labels"] + S["coded_labels"]
    coded = np.stack([R.encode_fixed_frame(r, rate, True, int(geom[4])) for r in S["info"]])
    assert np.array_equal(coded, fx[f"coded_{mode}"]), f"{mode}: coded bytes of rows {np.nonzero((coded != fx[f'coded_{mode}']).any(1))[0]}"
    if not T.nvis(mode):
        check_against_fixture(fx, mode, S, coded, [R.modulate(mod, rate, c) for c in list(coded) + list(S["coded"])])
    for f in range(2):                                  # the valid frames, built by the reference's own frame builder
        row = S["info"][f]
        plen, seq = (int(row[13]) << 8) | int(row[14]), (int(row[4]) << 8) | int(row[5])
        s, info, cd, bps = R.tx_frame(mod, rate, row[17:17 + plen], seq, nvis=T.nvis(mode))
        assert np.array_equal(info[:len(row)], row) and np.array_equal(cd, fx[f"coded_{mode}"][f]), f"{mode} row {f} ({labels[f]})"
        assert bps == geom[4] and len(s) == geom[6] and geom[2] * T.BITS[mod] == bps and geom[1] + geom[2] == 59
        assert T.sample_digest(s) == bytes(fx[f"dig_{mode}"][f]).hex(), f"{mode} row {f} ({labels[f]}): sample digest"
        assert np.abs(s).max().view(np.uint32) == fx[f"mx_{mode}"][f].view(np.uint32)


@pytest.mark.parametrize("mod", [m for m, _ in T.MODS])
def test_the_full_frame_of_every_modulation_hashes_to_its_digest_and_the_oracle_gives_it(oracle, fx, mod):
    mode = f"{mod}_R3_4"
    row = int(fx[f"frame_row_{mod}"])
    s = T.frame_from_planes(fx[f"frame_{mod}"])
    assert T.sample_digest(s) == bytes(fx[f"dig_{mode}"][row]).hex()
    S = T.input_set(oracle, mode)
    mine = oracle.modulate(*T.MODES[mode], S["coded"][row - len(S["info"])])
    assert np.array_equal(mine.view(np.uint32), s.view(np.uint32)), f"{mode} row {row}"
    assert np.array_equal(T.frame_from_planes(T.frame_planes(s)).view(np.uint32), s.view(np.uint32))


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_coverage_conditions(oracle, mode):
    """conditions of the set, not measurements: every symbol value at least twice on at least two data carriers; in the
    differential modes every phase increment after every other; the families and walk positions present"""
    mod, rate = T.MODES[mode]
    S, c = T.input_set(oracle, mode), T.coverage(oracle, mode)
    g = T.geometry(oracle, mode)
    assert len(c["count"]) == 1 << T.BITS[mod]
    assert c["count"].min() >= 2 and c["carriers"].min() >= 2, (mode, c["count"].min(), c["carriers"].min())
    if mod in T.DIFFERENTIAL:
        assert c["trans"].min() >= 1, (mode, np.argwhere(c["trans"] == 0)[:4])
    # the straddling carrier exists exactly where a carrier's bits do not divide what the last symbol holds
    assert c["straddle"] == ((T.FRAME_BITS - (int(g[5]) - 1) * int(g[4])) % int(g[3]) != 0)
    assert c["straddle"] == (mod == po.QAM32), "2592 = 2^5 3^4: of 1, 2, 3, 4, 5, 6 and 8 bits only 5 do not divide it"
    assert c["unfilled"] >= 1, "every configuration leaves carriers of its last symbol without bits"
    il, cl = S["info_labels"], S["coded_labels"]
    assert S["info"].shape[1] == 4 * T.BPC[rate] and S["coded"].shape[1] == 324
    assert sum(l.startswith("valid") for l in il) == 2 and sum(l.startswith("constant") for l in il) == 4 and sum(l.startswith("random") for l in il) == 3
    assert sum(l.startswith("constant") for l in cl) == 2 and sum(l.startswith("random") for l in cl) == 2 and sum(l.startswith("tail") for l in cl) == 1
    assert np.array_equal(S["info"][1][4:6], [0xFF, 0xFF]), "one valid frame has seq 0xFFFF"
    bits = 8 * T.BPC[rate]
    walk = {(cw, j) for cw, j, _, _, _ in c["walk"]}
    assert {(cw, j) for cw in range(4) for j in (0, bits - 1)} <= walk
    assert ((0, T.K[rate] - 1) in walk) == (T.K[rate] - 1 < bits)
    assert sum(j >= T.K[rate] for _, j in walk) == max(0, bits - T.K[rate])
    pos = [p for _, _, p, _, _ in c["walk"]]
    assert len(set(pos)) == len({w[:2] for w in c["walk"]}) and min(pos) >= 0 and max(pos) < T.FRAME_BITS
    assert np.unpackbits(S["coded"][cl.index("tail: last 16 bits")]).nonzero()[0].tolist() == list(range(2576, 2592))


def test_which_rates_have_bits_beyond_k():
    """bytes_per_codeword * 8 > k at no rate; k - 1 lies inside the bytes at R2/3 only; at R1/4, R1/3, R1/2, R3/4 and R5/6 k
    exceeds the bytes and the encoder pads (the kernel's `j < bpc * 8` guard)"""
    assert T.BEYOND_K_RATES == () and T.K_MINUS_1_INSIDE == ("R2_3",) and set(T.PAD_RATES) == {"R1_4", "R1_3", "R1_2", "R3_4", "R5_6"}
    assert {n: T.K[r] - 8 * T.BPC[r] for n, r in T.RATES} == {"R1_4": 2, "R1_3": 108, "R1_2": 4, "R2_3": 0, "R3_4": 6, "R5_6": 4}


# ---------------------------------------------------------------------------------------------- make_frames restated
@pytest.mark.parametrize("rate_name,rate", T.RATES)
def test_make_frames_restatement_builds_what_the_oracle_builds(oracle, rate_name, rate):
    """same payload in, same frame out: the restatement's header, call-sign hashes and CRCs are make_frame's"""
    for seed, first_seq in ((0, 0), (1, 65530), (2 ** 32, 65535), (2 ** 64 - 1, 2 ** 31 - 17), (7, -3)):
        fr = T.make_frames(oracle, rate, seed, first_seq, 9)
        for f in range(9):
            seq = (first_seq + f) & 0xFFFF
            assert np.array_equal(oracle.make_frame(fr[f][17:-2], seq, rate), fr[f]), (rate_name, seed, first_seq, f)
    assert T.callsign_hash("TEST") == T.callsign_hash("test") and T.callsign_hash("TEST") != T.callsign_hash("RX")


def test_philox_restatement_known_answers():
    """Random123's known-answer vectors of philox4x32-10"""
    kat = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for ctr, key, want in kat:
        got = T.philox4x32(*[np.array([c], np.uint64) for c in ctr], *[np.array([k], np.uint64) for k in key])
        assert tuple(int(g[0]) for g in got) == want


def test_make_frames_restatement_properties(oracle):
    a = T.make_frames(oracle, po.R1_2, 5, 100, 8)
    for i in range(8):
        assert np.array_equal(T.make_frames(oracle, po.R1_2, 5, 100 + i, 1)[0], a[i])
    assert not np.array_equal(T.make_frames(oracle, po.R1_2, 5 + 2 ** 32, 100, 1)[0][17:], a[0][17:])
    b = T.make_frames(oracle, po.R1_2, 5, 100 + 65536, 1)[0]
    assert np.array_equal(b[:17], a[0][:17]) and not np.array_equal(b[17:], a[0][17:])
    assert np.array_equal(T.make_frames(oracle, po.R1_2, 5, -1, 1)[0], T.make_frames(oracle, po.R1_2, 5, 2 ** 32 - 1, 1)[0])


# ---------------------------------------------------------------------------------------------- the peak rule
@pytest.mark.parametrize("mod", [m for m, _ in T.MODS])
def test_peak_rule_is_the_reference_tools_formula_at_08(fx, mod):
    """tools/test_waveform_simple.cpp:365-371: max_val over the samples; if (max_val > 0) { scale = 0.8f / max_val; s *= scale; }"""
    s = T.frame_from_planes(fx[f"frame_{mod}"])
    max_val = np.float32(0)
    for v in (s.max(), -s.min()):
        max_val = max(max_val, np.float32(v))
    scale = np.float32(np.float32(0.8) / max_val)
    want = np.array([np.float32(v * scale) for v in s[:4096]], np.float32)
    got = T.peak_rule(s, 0.8)
    assert np.array_equal(got[:4096].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), (s * scale).view(np.uint32)) and np.abs(got).max() <= np.float32(0.8) * (1 + 2.0 ** -23)


def test_peak_rule_over_its_values(fx):
    s = T.frame_from_planes(fx["frame_QAM16"])
    for p in (0.0, -0.0, -1.0, float("nan")):
        assert np.array_equal(T.peak_rule(s, p).view(np.uint32), s.view(np.uint32)), p
    small, tiny, huge, inf = T.peak_rule(s, 1e-30), T.peak_rule(s, 1e-38), T.peak_rule(s, 3e38), T.peak_rule(s, float("inf"))
    den = (tiny != 0) & (np.abs(tiny) < np.finfo(np.float32).tiny)
    assert den.sum() > 0.9 * s.size and np.abs(tiny).max() == np.float32(1e-38), "1e-38 gives denormal samples"
    assert np.abs(small).max() == np.float32(1e-30) and np.abs(small[s != 0]).min() > 0, "1e-30 stays normal but for samples under 1.2e-8 of the peak"
    # 3e38 / max|s| overflows where max|s| < 3e38 / FLT_MAX = 0.88.  This recorded frame peaks above 1: its largest sample
    # lands on 3e38 (one rounding of the quotient, one of the product) and nothing is inf
    mx = np.abs(s).max()
    assert mx > 1 and np.isfinite(huge).all() and abs(float(np.abs(huge).max()) / 3e38 - 1) < 2.0 ** -22
    assert np.isinf(T.peak_rule(s / (2 * mx), 3e38)[s != 0]).all(), "a frame that peaks at 0.5 overflows in the quotient"
    assert np.isinf(inf[s != 0]).all()
    z = np.concatenate([s, np.zeros(1, np.float32)])
    assert np.isnan(T.peak_rule(z, float("inf"))[-1]), "0 * inf: NaN at a zero sample"


def test_rows_the_gpu_tries_the_peak_values_on(oracle):
    """test_peak_values (GPU) takes T.peak_rows of every modulation at R1/2, 27 rows.  Conditions on those rows: 3e38
    overflows in the quotient (max|s| < 0.88) on at least 9 of them and stays finite on at least 9, so both sides of the
    overflow are compared; none of the rows has an exactly zero sample, so the rule's NaN (0 * inf at peak +inf) does not
    occur in them and no NaN is compared."""
    finite = overflow = 0
    for mod, _ in T.MODS:
        mode = f"{mod}_R1_2"
        S = T.input_set(oracle, mode)
        _, samples = T.answers(oracle, oracle, mode)
        ri, rc = T.peak_rows(S)
        rows = [samples[r] for r in ri] + [samples[len(S["info"]) + rc]]
        over = [bool(np.isinf(T.peak_rule(x, 3e38)).any()) for x in rows]
        overflow += sum(over)
        finite += sum(not o for o in over)
        assert all(int((x == 0).sum()) == 0 for x in rows), mode
        assert all(not np.isnan(T.peak_rule(x, p)).any() for x in rows for p in T.PEAKS), mode
    assert overflow >= 9 and finite >= 9, (overflow, finite)


# ---------------------------------------------------------------------------------------------- the kernel's constant block
def test_tx_const_bounds_for_every_configuration():
    """tests/helpers/tx_const_check.cpp: build_tx_const for the 54 configurations against the sizes of TxConst and of the
    kernel's LDS areas; every data_bin / pilot_bin distinct and inside 0..1023"""
    src = os.path.join(ROOT, "tests", "helpers", "tx_const_check.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chk")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", exe, src])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "configurations 54 failures 0" in out.stdout, out.stdout
