"""CPU: ria_amd/csrc/ws_carve.hpp, the Carver every workspace of the library is laid out with.  The sizing pass on a null
base and the pass on the block agree; areas start on 256-byte boundaries, are disjoint and in call order; a zero-count area
consumes nothing; a list's arrays lie back to back and its rows add up to the per-row byte sum."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_carver_offsets_alignment_and_lists():
    src = os.path.join(ROOT, "tests", "helpers", "ws_carve_check.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chk")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, src])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "failures 0" in out.stdout
