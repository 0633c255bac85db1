"""CPU: the restatement of the MC-DPSK window (tests/mcdpsk_window_restatement.py) on the oracle equals, on every row of
tests/mcdpsk_window_inputs.py, what the same restatement gave on the compiled reference (tests/golden/mcdpsk_window.npz,
recorded by tools/record_mcdpsk_window_golden.py); where the reference library is built, the live comparison runs too.  The
table's own coverage, the float32 energy chain, and the host program for the shared rules (as built and under
AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone host program)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import pyoracle as po
import mcdpsk_window_inputs as WI
import mcdpsk_window_restatement as MW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_mcdpsk_window_golden as REC   # noqa: E402

SRC = os.path.join(ROOT, "tests", "helpers", "mcdpsk_window_rules_check.cpp")
NAMES = [r["name"] for r in WI.rows()]


def compare(got, want):
    assert set(got) == set(want.files if hasattr(want, "files") else want)
    for k in got:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.shape[0] == len(NAMES), k      # every row of the table is in the fixture
        for i, n in enumerate(NAMES):
            assert np.array_equal(a[i], b[i]), (k, n, a[i], b[i])


def test_the_table_reaches_every_statement(oracle):
    WI.assert_coverage(oracle)
    assert len(set(NAMES)) == len(NAMES) and all(r["purpose"] for r in WI.rows())
    assert set(WI.UNREACHED) == {"PROCESS_FAILED", "SALVAGE"} and all(WI.UNREACHED.values())


def test_restatement_on_the_oracle_equals_the_recorded_reference(oracle, golden):
    compare(REC.record(oracle), golden("mcdpsk_window"))


@pytest.mark.skipif(not po.Ref.available(), reason="the compiled reference is built only where its sources are")
def test_restatement_on_the_compiled_reference_equals_the_fixture(golden):
    ref = po.Ref()
    WI.assert_coverage(ref)
    compare(REC.record(ref), golden("mcdpsk_window"))


def test_fixture_is_numeric_and_small():
    path = os.path.join(ROOT, "tests", "golden", "mcdpsk_window.npz")
    g = np.load(path)
    assert all(g[k].dtype.kind in "iu" for k in g.files)
    assert os.path.getsize(path) < 64 * 1024


def test_energy_chain_is_the_ascending_float32_sum():
    rng = np.random.default_rng(5)
    v = (rng.standard_normal(5000) * 0.2).astype(np.float32)
    acc = np.float32(0.0)
    for s in v:
        acc = np.float32(acc + np.float32(s * s))
    want = np.float32(np.sqrt(np.float32(acc / np.float32(5000))))
    assert MW.chain_rms(v).view(np.uint32) == want.view(np.uint32)
    assert MW.chain_rms(np.zeros(0, np.float32)) == 0
    t, r, ping = MW.energy(np.concatenate([np.full(4608, 0.5, np.float32), np.zeros(5000, np.float32)]))
    assert (t, r, ping) == (np.float32(0.5), np.float32(0.0), True)
    assert MW.energy(np.zeros(9608, np.float32))[2] and not MW.energy(np.full(9608, 0.5, np.float32))[2]
    assert REC.search_tails() == {-1: WI.TAIL_UNDER, 0: WI.TAIL_AT, 1: WI.TAIL_OVER}      # the pinned tail constants


def test_parse_header_reads_twenty_bytes_only(oracle):
    """the peek hands parseHeader the whole decoded vector, decodeMCDPSKFrame 20 bytes of it: the same header"""
    from mcdpsk_acquire_restatement import ACK, control_frame, data_frame
    for f in (control_frame(ACK, 3), data_frame(0x30, 4, np.arange(25, dtype=np.uint8))[:20]):
        for tail in (b"", b"\x00", b"\xff\xff\xff"):
            d = np.concatenate([f, np.frombuffer(tail, np.uint8)])
            assert MW.parse_header(d) == MW.parse_header(f) and MW.parse_header(f)[0]
    assert MW.parse_header(control_frame(ACK, 3)[:19]) == (False, 0, 0)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_window_rules_host_program(flags):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chk")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-o", exe, SRC])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "failures 0" in out.stdout
