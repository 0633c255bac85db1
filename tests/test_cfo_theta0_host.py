"""CPU: ria_amd/csrc/cfo_theta0.h (the initial CFO correction phase of the demodulator kernels) compiled for the host.
Inside the bound of include/ria_gpu.h (|cfo_hz * abs_position| <= 1.025e12) it equals the oracle's wrap bit for bit;
outside it, and for a non-finite product, where the reference's loop never ends, it returns 0 at once."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 2.0 ** 27            # on |ip| = |2 pi cfo pos / 48000| after rounding to float


@pytest.fixture(scope="module")
def helper(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("theta0") / "chk")
    src = os.path.join(ROOT, "tests", "helpers", "cfo_theta0_check.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, src, "-lm"])

    def run(pairs, timeout):
        text = "".join(f"{np.float32(c).view(np.uint32):08x} {int(p)}\n" for c, p in pairs)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=timeout, check=True)
        return np.array([int(v, 16) for v in out.stdout.split()], np.uint32)
    return run


def ip_of(cfo, pos):
    with np.errstate(over="ignore"):
        return np.float32(-2.0 * np.pi * float(np.float32(cfo)) * float(pos) / 48000.0)


def test_in_range_equals_the_oracle_wrap(oracle, helper):
    oracle.lib.ro_theta0.argtypes = [C.c_float, C.c_longlong]
    oracle.lib.ro_theta0.restype = C.c_float
    rng = np.random.default_rng(31415)
    pairs = [(c, p) for c in (0.0, -0.0, 0.011, -0.011, 2.0, -2.0, 60.0, -60.0, 1e-30, 1e-42)
             for p in (0, 1, 47999, 48000, 2 ** 24 - 1, 2 ** 24 + 1, 2 ** 31, 2 ** 32 + 5)]
    for _ in range(3000):                                    # |ip| log-uniform up to ~3e4 rad, both signs
        cfo = np.float32(rng.choice([-1, 1]) * 10.0 ** rng.uniform(-3, 2))
        pairs.append((cfo, int(10.0 ** rng.uniform(0, 6.5))))
    for k in range(400):                                     # phases next to +-pi and to multiples of 2 pi
        cfo = np.float32((1, -1)[k % 2] * (0.5, 1.0, 7.0, 60.0)[k % 4])
        pairs.append((cfo, max(0, int(round((k // 8 + 0.5 * (k % 3)) * 48000.0 / abs(float(cfo)))) + k % 5 - 2)))
    # the bound itself, from both sides, and the last binades below it (steps of 8 and of 6 instead of 2 pi)
    edge = int(BOUND * 48000.0 / (2.0 * np.pi * 60.0))
    big = [(s * 60.0, edge + d) for s in (1, -1) for d in (-3000, -1, 0)] + [(60.0, edge // 3), (-60.0, edge // 5), (2.0, 2 ** 36)]
    big = [(c, p) for c, p in big if abs(ip_of(c, p)) <= BOUND]
    assert len(big) >= 7 and max(abs(ip_of(c, p)) for c, p in big) >= BOUND - 16
    pairs += big
    # the oracle's loop, like the reference's, never ends outside the bound: nothing else may reach it
    assert all(0 <= p < 2 ** 63 and abs(ip_of(c, p)) <= BOUND for c, p in pairs)
    got = helper(pairs, 120)
    want = np.array([np.float32(oracle.lib.ro_theta0(float(np.float32(c)), int(p))) for c, p in pairs], np.float32).view(np.uint32)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{len(bad)} of {len(pairs)} differ, first {pairs[bad[0]]}: {got[bad[0]]:08x} oracle {want[bad[0]]:08x}"
    assert (np.abs(want.view(np.float32)) <= np.float32(np.pi) * (1 + 1e-6)).all()


def test_outside_the_bound_it_returns_zero_at_once(helper):
    """the reference's loop does not end on any of these; the helper must, well inside the time limit"""
    edge = int(BOUND * 48000.0 / (2.0 * np.pi * 60.0))
    pairs = [(np.inf, 1), (-np.inf, 1), (np.inf, 0), (np.nan, 0), (np.nan, 12345), (60.0, 2 ** 64 - 1), (-60.0, 2 ** 64 - 1),
             (60.0, edge + 3000), (-60.0, edge + 3000), (3.0e38, 2 ** 40), (-3.0e38, 2 ** 63)]
    assert all(not abs(ip_of(c, p)) <= BOUND for c, p in pairs)
    got = helper(pairs, 10)
    assert len(got) == len(pairs) and not got.any(), got
