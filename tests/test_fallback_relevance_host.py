"""CPU: ria_amd/csrc/fallback_relevance.hpp (which codewords' fallback re-decodes recovery_stage1_kernel queues) against a
plain restatement of reassemble + verify, over generated frames: header valid / wrong magic / wrong header CRC, every
control type, payload lengths around each codeword boundary and past the frame, the 0xD5 marker on CW1..3 in every
combination, 20 / 40 / 67 bytes per codeword (tests/helpers/fallback_relevance_check.cpp).  Once as built, once under
the address and undefined-behaviour sanitizers."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("extra", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_irrelevant_codewords_cannot_change_the_trial(extra):
    src = os.path.join(ROOT, "tests", "helpers", "fallback_relevance_check.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chk")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + extra + ["-o", exe, src])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        # 3 sizes x 3 header variants x 8 marker combinations x (8 control types + 8 payload lengths); both verdicts occur
        assert "frames 1152 " in out.stdout and "failures 0" in out.stdout, out.stdout
        words = out.stdout.split()
        assert int(words[words.index("relevant") + 1]) > 1152 and int(words[words.index("irrelevant") + 1]) > 1152
