"""ria_amd/csrc/search_rules.hpp on the host: tests/helpers/search_rules_check.cpp walks the rules over their domain (streaks
0..40, every modulation class, hint tiers on both sides of each boundary, gate clamps at both ends, catch-up at 1.5x and 2.5x
and one either side, backtrack at cursor 0 / backtrack - 1 / backtrack, anti-replay at distance 199 / 200, CFO sanity at
|diff| = 1.0 and known = +-0.01, NaN and +-inf for rms, floor, correlation and CFO) and prints every case; each line is
computed again here, in numpy float32 from streaming_decoder.cpp:386-941, and compared bit for bit.  Built and run plain and
with -fsanitize=address,undefined."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import search_restatement as SR

F = np.float32
SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "search_rules_check.cpp")
RING = 960000


def fl(h):
    return np.array([int(h, 16)], np.uint32).view(F)[0]


def same(got_hex, want):
    got = fl(got_hex)
    return (np.isnan(got) and np.isnan(want)) or got.view(np.uint32) == F(want).view(np.uint32)


def gate(light, floor, streak):
    if light:
        g = SR.std_clamp(floor * F(2.2), F(0.015), F(0.040))
        if streak >= 8:
            g = SR.std_max(F(0.012), g - SR.std_min(F(0.010), F(0.001) * F(streak - 7)))
    else:
        g = SR.std_clamp(floor * F(1.8), F(0.014), F(0.030))
        if streak >= 8:
            g = SR.std_max(F(0.010), g - SR.std_min(F(0.008), F(0.001) * F(streak - 7)))
    return g


def check(line):
    name, *rest = line.split()
    a, r = rest[:rest.index("->")], rest[rest.index("->") + 1:]
    if name == "min_search":
        return int(r[0]) == {0: 67304, 1: 31120, 2: 120000}[int(a[0])]
    if name == "feed":
        cursor, fed, streak, cap, step = map(int, a)
        count = min(step, cap - fed)
        if count > 0:
            if cursor > fed:
                cursor, streak = fed, 0
            fed += count
        return list(map(int, r)) == [max(count, 0), cursor, fed, streak]
    if name == "wait":
        cursor, fed, m = map(int, a)
        return int(r[0]) == int(fed < m or cursor > fed or fed - cursor < m)
    if name == "catch":
        cursor, fed, m = map(int, a)
        unsearched = fed - cursor
        scaled = unsearched * 10 // m
        kind = 0
        if scaled > 25:
            kind, cursor = 2, (fed + RING - m - 4800) % RING
        elif scaled > 15:
            kind, cursor = 1, (cursor + max(min((unsearched - m) // 2, 24000), 4800)) % RING
        return list(map(int, r)) == [kind, cursor]
    if name == "floor":
        prev, rms = fl(a[0]), fl(a[1])
        nf = SR.std_max(F(0.001), prev)
        fast = bool(rms < nf * F(3.0))
        want = F(0.98) * nf + F(0.02) * rms if fast else F(0.995) * nf + F(0.005) * rms
        return int(r[0]) == int(fast) and same(r[1], want)
    if name == "gate":
        return same(r[0], gate(int(a[0]), fl(a[1]), int(a[2])))
    if name == "start":
        cursor, zc = int(a[0]), int(a[1])
        back = 19200 if zc else 9600
        return list(map(int, r)) == [cursor - back if cursor >= back else 0, 1200 if zc else 4800]
    if name == "conf":
        cls, connected, streak = map(int, a[:3])
        conf, floor = SR.confidence(cls, bool(connected), streak, fl(a[3]), fl(a[4]))
        return same(r[0], conf) and same(r[1], floor) and same(r[2], conf if cls == SR.ZC_MODE else F(0.15))
    if name == "near":
        streak, c, floor = int(a[0]), fl(a[1]), fl(a[2])
        return int(r[0]) == (1 if c >= floor else (-1 if streak > 0 else 0))
    if name == "weak":
        cls, connected, streak = map(int, a[:3])
        c, conf, floor = fl(a[3]), fl(a[4]), fl(a[5])
        allow = cls in (SR.DIFFERENTIAL, SR.ZC_MODE) and bool(connected) and streak >= 3 and bool(c >= SR.std_max(floor, conf - F(0.08)))
        return list(map(int, r)) == [int(allow), max(1, streak // 2), 0]
    if name == "replay":
        sync, last = int(a[0]), int(a[1])
        rep = False
        if last != -2 ** 31:
            d1 = sync - last if sync >= last else RING - last + sync
            rep = min(d1, RING - d1) < 200
        return list(map(int, r)) == [int(rep), (sync + 9600 + 4800) % RING]
    if name == "cfo":
        connected, new, known = int(a[0]), fl(a[1]), fl(a[2])
        taken = bool(connected and abs(known) > F(0.01) and abs(new - known) > F(1.0))
        return int(r[0]) == int(taken) and same(r[1], known if taken else new)
    if name == "snr":
        snr = (fl(a[0]) - F(0.15)) / F(0.03)
        return same(r[0], SR.std_max(F(-5.0), SR.std_min(F(30.0), snr)))
    return False


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_search_rules_host_program(flags):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chk")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-o", exe, SRC])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = out.stdout.splitlines()
    names = {ln.split()[0] for ln in lines}
    assert names == {"min_search", "feed", "wait", "catch", "floor", "gate", "start", "conf", "near", "weak", "replay", "cfo", "snr"}
    assert len(lines) > 10000
    with np.errstate(all="ignore"):
        bad = [ln for ln in lines if not check(ln)]
    assert not bad, bad[:10]
    # the walk reaches what it is there for: both catch-ups, both tracker branches, replay on both sides of 200, CFO taken and kept
    assert {ln.split()[-2] for ln in lines if ln.startswith("catch")} == {"0", "1", "2"}
    assert {ln.split()[-2] for ln in lines if ln.startswith("floor")} == {"0", "1"}
    assert {ln.split()[-2] for ln in lines if ln.startswith("replay")} == {"0", "1"}
    assert {ln.split()[-2] for ln in lines if ln.startswith("cfo")} == {"0", "1"}
