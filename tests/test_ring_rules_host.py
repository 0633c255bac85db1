"""ria_amd/csrc/ring_rules.hpp on the host: tests/helpers/ring_rules_check.cpp walks the ring rules case by case - the closed
form of the ring's content and ringPosToAbsolute around index 0, the write position and the ring's end, for totals on both
sides of one, two and three laps; feedAudio with the cursor behind, at and ahead of the write position, the drift guard at
950 399 / 950 400 / 950 401, steps that reach 960 000 exactly and that overflow with need_to_drop == and < unsearched; both
waits with the cursor initialisation; the circular catch-up around 1.5x and 2.5x; the backtrack underflow; the span flag - and
prints every case.  Each line is computed again here from the statements of streaming_decoder.cpp:184-291 and :386-941 and
compared.  Built and run plain and with -fsanitize=address,undefined.  The record layouts are static_asserts of the program;
the null-handle return is checked on the library."""
import os
import subprocess
import tempfile

import pytest

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "ring_rules_check.cpp")
RING = 960000
GUARD, KEEP = 9600, 360000


def write_pos(t):
    return t % RING


def source(t, p):
    """the last sample k < t written to ring index p by buffer_[k % RING] = x[k]"""
    if t < RING:
        return p if p < t else -1
    k = t - 1
    while k % RING != p:           # at most one lap, walked 1 at a time only near the end: jump first
        k -= (k - p) % RING
    return k


def pos_to_absolute(t, ring_pos):   # :862-874
    if t < RING:
        return ring_pos
    oldest_abs, oldest_pos = t - RING, write_pos(t)
    offset = ring_pos - oldest_pos if ring_pos >= oldest_pos else RING - oldest_pos + ring_pos
    return oldest_abs + offset


def feed(cursor, t, streak, cap, step):   # :184-291
    ev, total, overflows, snaps, dropped = 0xFFFFFFFE, 5, 1, 2, 3
    count = min(step, cap - t)
    if count <= 0:
        return [0, cursor, t, streak, ev, total, overflows, snaps, dropped]
    wp = write_pos(t)

    def compute_unsearched(w, c):
        if t < RING:
            return w - c if w >= c else 0
        return w - c if w >= c else RING - c + w
    if t < RING and cursor > wp:
        cursor, streak = wp, 0
    unsearched = compute_unsearched(wp, cursor)
    if t >= RING and unsearched > RING - GUARD:
        cursor, unsearched = wp, 0
        snaps += 1
    if unsearched + count >= RING:
        incoming = unsearched + count
        target = min(KEEP, RING - 1)
        need = min(unsearched, incoming - target) if incoming > target else 0
        cursor = (cursor + need) % RING
        ev = (ev + 1) & 0xFFFFFFFF
        total += need
        overflows += 1
        dropped += need
    t += count
    if t < RING and cursor > write_pos(t):
        cursor = write_pos(t)
    return [count, cursor, t, streak, ev, total, overflows, snaps, dropped]


def wait(cursor, t, m):             # :449-481, the library's limit before the wrap
    if t < m:
        return [1, cursor, 0]
    wp, inits = write_pos(t), 0
    if cursor == 0 and t > 0 and t >= RING:
        cursor, inits = wp, 1
    if t < RING and cursor > wp:
        return [1, cursor, inits]
    unsearched = wp - cursor if wp >= cursor else RING - cursor + wp
    return [int(unsearched < m), cursor, inits]


def start(cursor, t, zc, m):        # :597-605 and the span flag
    back = 19200 if zc else 9600
    if cursor >= back:
        s = cursor - back
    elif t < RING:
        s = 0
    else:
        s = (RING + cursor - back) % RING
    wraps = t >= RING and 0 < (write_pos(t) - s) % RING < m
    return [s, int(wraps)]


def catch(cursor, wp, m):           # :488-522
    unsearched = wp - cursor if wp >= cursor else RING - cursor + wp
    scaled = unsearched * 10 // m
    if scaled > 25:
        return [2, (wp + RING - m - 4800) % RING]
    if scaled > 15:
        return [1, (cursor + max(min((unsearched - m) // 2, 24000), 4800)) % RING]
    return [0, cursor]


def check(line):
    name, *rest = line.split()
    a, r = list(map(int, rest[:rest.index("->")])), list(map(int, rest[rest.index("->") + 1:]))
    if name == "source":
        return r == [source(*a), pos_to_absolute(*a), write_pos(a[0])]
    if name == "feed":
        cursor, t, streak, cap, step = a
        return r == feed(cursor, t, streak, cap, step)
    if name == "wait":
        return r == wait(*a)
    if name == "start":
        return r == start(*a)
    if name == "catch":
        return r == catch(*a)
    if name == "drop":
        got = feed(a[0], a[1], 0, 3000000, a[2])
        return r == [got[1], got[2], got[6] - 1, got[8] - 3]
    if name == "arrive":
        full, abs_start, ahead, lag, nxt = a
        t, abs_cursor = abs_start + ahead + lag, abs_start + nxt
        unsearched, count = lag, max(0, abs_cursor - t)
        # the bound of the stream loop: backlog + arrivals < full <= 959 999, so feedAudio's overflow test (:242) cannot fire
        bound = unsearched + count < full <= RING - 1 if count > 0 else True
        return r == [unsearched, count, unsearched + count, max(t, abs_cursor), 0] and bound
    if name == "last":
        last, origin, wl = a
        none = -2 ** 31
        d = (last - origin) % RING
        rel = none if last == none else (d - RING if d >= RING // 2 else d)
        mc = none if wl == none else (wl + origin) % RING
        return r == [rel, mc, 7 if wl == 0 else last]
    if name == "sync":
        return r == [(a[0] + a[1]) % RING]
    return False


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_ring_rules_host_program(flags):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chk")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-o", exe, SRC])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = out.stdout.splitlines()
    assert {ln.split()[0] for ln in lines} == {"source", "feed", "wait", "start", "catch", "sync", "drop", "arrive", "last"}
    assert len(lines) > 10000
    bad = [ln for ln in lines if not check(ln)]
    assert not bad, bad[:10]
    # the walk reaches what it is there for
    feeds = [list(map(int, ln.replace("->", "").split()[1:])) for ln in lines if ln.startswith("feed")]
    assert any(f[12] == 3 for f in feeds) and any(f[12] == 2 for f in feeds)                       # the drift guard fired / did not
    over = [f for f in feeds if f[11] == 2]
    assert over and any(f[13] - 3 == 0 for f in over) and any(f[13] - 3 > 0 for f in over)         # overflow with nothing / something dropped
    assert any(f[9] == 0xFFFFFFFF for f in feeds) and any(f[1] < RING <= f[7] for f in feeds) and any(f[7] == RING for f in feeds)
    assert any(f[1] < RING and f[0] > f[1] % RING and f[8] == 0 and f[5] > 0 for f in feeds)         # the pre-wrap clamp clears the streak
    waits = [list(map(int, ln.replace("->", "").split()[1:])) for ln in lines if ln.startswith("wait")]
    assert {w[3] for w in waits} == {0, 1} and any(w[5] == 1 and w[4] != 0 for w in waits) and any(w[5] == 1 and w[4] == 0 for w in waits)
    starts = [list(map(int, ln.replace("->", "").split()[1:])) for ln in lines if ln.startswith("start")]
    assert any(s[5] == 1 for s in starts) and any(s[4] > s[0] for s in starts) and any(s[4] == 0 and s[0] > 0 for s in starts)
    assert {ln.split()[-2] for ln in lines if ln.startswith("catch")} == {"0", "1", "2"}
    assert any(int(ln.split()[-1]) < int(ln.split()[1]) for ln in lines if ln.startswith("sync"))
    # the two overflow branches on the program's own lines: everything dropped (need_to_drop == unsearched), part of it kept
    drops = [list(map(int, ln.replace("->", "").split()[1:])) for ln in lines if ln.startswith("drop")]
    assert drops == [[100000, 200000, 900000, 200000, 1100000, 1, 100000], [150000, RING + 100000, 100000, 150000 + 650000, RING + 200000, 1, 650000]]
    arrive = [list(map(int, ln.replace("->", "").split()[1:])) for ln in lines if ln.startswith("arrive")]
    assert any(x[6] > 0 and x[5] > 0 for x in arrive) and all(x[9] == 0 for x in arrive)            # arrivals on a backlog; no overflow ever


def test_null_handle():
    from ria_amd import capi
    L = capi.load()
    assert "ria_gpu_search_ring_batch" in capi.EXPORTS
    assert L.ria_gpu_search_ring_batch(None, 0, 0, None, None, 0, None, 1, None, 0, 1, None, None) == -1     # RIA_ERR_INVALID
    assert L.ria_gpu_rx_ring_batch(None, None, 0, 0, None, None, 0, None, 0, None, 0, 1, 1, None, None, 0, None, None) == -1
    assert L.ria_gpu_rx_ring_host(None, None, 0, 0, None, None, 0, None, 0, 1, 1, None, None, 0, None) == -1
