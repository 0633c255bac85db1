"""CPU: the restatement of the connected-mode window (tests/window_restatement.py) on the oracle equals, on every row of
tests/window_inputs.py, what the same restatement gave on the compiled reference (tests/golden/window_frames.npz, recorded by
tools/record_window_golden.py); where the reference library is built, the live comparison runs too.  The table's own coverage,
the float32 clamp, and the host program for the two shared rules (as built and under AddressSanitizer +
UndefinedBehaviorSanitizer: a stand-alone host program)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import pyoracle as po
import window_inputs as WI
import window_restatement as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_window_golden as REC   # noqa: E402

SRC = os.path.join(ROOT, "tests", "helpers", "window_rules_check.cpp")


@pytest.fixture(scope="module")
def recorded(oracle):
    return REC.record(oracle)


def compare(got, want, names):
    assert set(got) == set(want.files if hasattr(want, "files") else want)
    for k in got:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, k
        if a.ndim and a.shape[0] == len(names) and not k.startswith("llr_"):
            for i, n in enumerate(names):
                assert np.array_equal(a[i], b[i]), (k, n, a[i], b[i])
        else:
            assert np.array_equal(a, b), k


def test_the_table_reaches_every_statement(oracle):
    WI.assert_coverage(oracle)
    names = [r["name"] for r in WI.rows()]
    assert len(set(names)) == len(names) and all(r["purpose"] for r in WI.rows())


def test_restatement_on_the_oracle_equals_the_recorded_reference(recorded, golden):
    compare(recorded, golden("window_frames"), [r["name"] for r in WI.reference_rows()])


@pytest.mark.skipif(not po.Ref.available(), reason="the compiled reference is built only where its sources are")
def test_restatement_on_the_compiled_reference_equals_the_fixture(golden):
    compare(REC.record(po.Ref()), golden("window_frames"), [r["name"] for r in WI.reference_rows()])


def test_fixture_is_numeric_and_small():
    path = os.path.join(ROOT, "tests", "golden", "window_frames.npz")
    g = np.load(path)
    assert all(g[k].dtype.kind in "iu" for k in g.files)
    largest = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
                  if f != "window_frames.npz")
    assert os.path.getsize(path) < largest


def test_clamp_in_float32():
    f = np.float32
    assert WR.clamp_cfo(f(5), f(0)).view(np.uint32) == f(2).view(np.uint32)
    assert WR.clamp_cfo(f(-5), f(0)).view(np.uint32) == f(-2).view(np.uint32)
    assert WR.clamp_cfo(f(2), f(0)) == f(2) and WR.clamp_cfo(f(1.25), f(-0.5)) == f(1.25)
    assert WR.clamp_cfo(f(-39.250004), f(-37.25)) == f(-39.25) and np.isnan(WR.clamp_cfo(f(np.nan), f(1)))
    assert isinstance(WR.clamp_cfo(5.0, 0.1), np.float32) and WR.clamp_cfo(5.0, 0.1) == f(f(0.1) + f(2))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_clamp_and_consumed_rules_host_program(flags):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chk")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-o", exe, SRC])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "failures 0" in out.stdout
