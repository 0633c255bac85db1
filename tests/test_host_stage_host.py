"""CPU: ria_amd/csrc/host_stage.hpp, the StageCarver every host-buffer call lays its staging block out with.  For optional
inputs and optional outputs in each combination: the sizing pass on a null base and the pass on the block agree; every area
is 256-byte aligned, disjoint and where it is whatever is present; the upload covers the present inputs and no output; the
download starts at the first wanted output and ends with the block; fill and drain move the caller's buffers.  Built and
run a second time under AddressSanitizer and UBSan, as a stand-alone program."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_staging_layout_copies_and_optional_areas(flags):
    src = os.path.join(ROOT, "tests", "helpers", "host_stage_check.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chk")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, src])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "failures 0" in out.stdout
