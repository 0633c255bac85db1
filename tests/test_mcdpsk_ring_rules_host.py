"""ria_amd/csrc/mcdpsk_ring_rules.hpp on the host: tests/helpers/mcdpsk_ring_rules_check.cpp walks the rules - the audio clock
on absolute positions on both sides of every lap with clocks that wrap 2^64; the pending fields' domain, every clause on both
sides of its bound; the re-entry fit at equality and a sample short; the re-entered window with the span below, at and above
`full` and at 959 999; the two total_fed assignments of a re-entry and their bound, backlog plus arrivals < 960 000 for every
span <= 959 999 - and every line is computed again from the Python twins in tests/mcdpsk_ring_restatement.py.  Built and run
plain and with -fsanitize=address,undefined, as a stand-alone program.  Then the binding's record layout and what the two
calls reject without a GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

import mcdpsk_ring_restatement as MR
import mcdpsk_stream_restatement as MS

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "mcdpsk_ring_rules_check.cpp")
RING = MR.RING


def check(line):
    name, *rest = line.split()
    a, r = list(map(int, rest[:rest.index("->")])), list(map(int, rest[rest.index("->") + 1:]))
    if name == "now":
        return r == [MR.now_ms(*a)]
    if name == "domain":
        return r == [int(MR.pending_domain_ok(*a))]
    if name == "fits":
        return r == [int(MS.reentry_fits(*a))]
    if name == "window":
        return r == [MS.reentry_window_len(*a)]
    if name == "fed":
        return r == [MR.reentry_fed(*a)]
    if name == "arrive":
        fed, start, sync, need, ahead, cap, nxt = a
        total, after = MR.reentry_arrival(fed, start, sync, need, ahead, cap, start + nxt if nxt >= 0 else -1)
        return r == [total, after, 1] and total < RING
    return False


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_mcdpsk_ring_rules_host_program(flags):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chk")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-o", exe, SRC])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = out.stdout.splitlines()
    assert {ln.split()[0] for ln in lines} == {"now", "domain", "fits", "window", "fed", "arrive"}
    assert len(lines) > 10000
    bad = [ln for ln in lines if not check(ln)]
    assert not bad, bad[:10]
    args = lambda name: [list(map(int, ln.replace("->", "").split()[1:])) for ln in lines if ln.startswith(name + " ")]
    # the grid reaches what it is there for.  The clock: one lap later is 20 000 ms later, never earlier; it wraps 2^64
    now = {(t0, pos): r for t0, pos, _, r in args("now")}
    assert [now[0, p] for p in (0, 47, 48, RING - 1, RING, RING + 48, 2 * RING)] == [0, 0, 1, 19999, 20000, 20001, 40000]
    assert now[2 ** 64 - 1, 48] == 0 and now[2 ** 64 - 1 - 20000, RING] == 2 ** 64 - 1 and now[2 ** 64 - 20000, RING] == 0
    top = 2 ** 31 - 1 - RING - 1                                   # the last index of the longest capture
    assert now[0, top] == top * 1000 // 48000 and now[2 ** 64 - 1, top] == top * 1000 // 48000 - 1
    # the domain: each clause of the ring decides some case on its own (everything else in the domain)
    dom = args("domain")
    ok = lambda d: MS.pending_domain_ok(d[0], d[1], d[2], d[3], d[4], d[5])
    span, held, fed_ok = (lambda d: d[3] - d[2] + d[1] <= 959999), (lambda d: d[6] - d[2] <= RING), (lambda d: d[2] + d[5] <= d[6])
    live = [d for d in dom if d[0] > 0 and ok(d)]
    assert any(d[7] == 1 for d in live) and any(d[2] > RING and d[7] == 1 for d in live)
    assert any(not span(d) and held(d) and fed_ok(d) and d[7] == 0 for d in live) and any(d[3] - d[2] + d[1] == 959999 and d[7] == 1 for d in live)
    assert any(span(d) and not held(d) and fed_ok(d) and d[7] == 0 for d in live) and any(d[6] - d[2] == RING and d[7] == 1 for d in live)
    assert any(span(d) and held(d) and not fed_ok(d) and d[7] == 0 for d in live) and any(d[2] + d[5] == d[6] and d[7] == 1 for d in live)
    assert all(d[7] == 1 for d in dom if d[0] == 0) and all(d[7] == 0 for d in dom if d[0] in (-1, 256))
    fits = args("fits")
    assert any(c == s + n and r == 1 for c, s, n, r in fits) and any(c == s + n - 1 and r == 0 for c, s, n, r in fits)
    win = args("window")
    assert any(w[5] == 959999 for w in win) and any(w[5] > w[0] for w in win) and any(w[5] == w[0] for w in win) and any(w[5] == w[1] - w[2] < w[0] for w in win)
    # the bound: no re-entry of a span <= 959 999 reaches feedAudio's overflow test; some come within `ahead` of it
    arrive = args("arrive")
    assert all(x[9] == 1 and x[7] < RING for x in arrive) and max(x[7] for x in arrive) == RING - 1
    assert any(x[3] + x[2] - x[1] == 959999 for x in arrive) and any(x[1] < RING < x[8] for x in arrive)       # a re-entry feeds across the wrap


def test_mcdpsk_ring_record_layout_and_symbols():
    from ria_amd import capi
    from ria_amd.engine import RxEngine
    assert C.sizeof(capi.McRingState) == 80 and capi.McRingState.pending_total_cw.offset == 48 and capi.McRingState.pend_known_cfo_hz.offset == 64
    dt = RxEngine.MCRING_STATE
    assert dt.itemsize == 80 and dt == MR.STATE
    flat = [(n, getattr(capi.RingState, n).offset) for n, _ in capi.RingState._fields_] + \
           [(n, getattr(capi.McRingState, n).offset) for n, _ in capi.McRingState._fields_[1:]]
    assert [(n, dt.fields[n][1]) for n in dt.names] == flat
    s = RxEngine.mcdpsk_ring_state(3, total_fed=[1, 2, 2 ** 31])
    assert list(s["total_fed"]) == [1, 2, 2 ** 31] and not any(s[f].any() for f in MR.PENDING)
    assert (s["last_decoded_sync_pos"] == capi.SEARCH_NO_LAST_SYNC).all() and s.tobytes()[:48] == RxEngine.ring_state(1, total_fed=1).tobytes()
    header = open(os.path.join(os.path.dirname(SRC), "..", "..", "include", "ria_gpu.h")).read()
    for name in ("ria_gpu_mcdpsk_ring_batch", "ria_gpu_mcdpsk_ring_host"):
        assert name in capi.EXPORTS and f"int {name}(" in header
    assert "typedef struct ria_mcdpsk_ring_state {" in header


def test_mcdpsk_ring_calls_reject_a_null_handle_without_a_gpu():
    from ria_amd import capi
    L = capi.load()
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    assert L.ria_gpu_mcdpsk_ring_batch(None, 1, 0, 0, 0, None, p, 1024, p, 1, p, 4800, 1, 1, None, None, None, p, p, 320, None, p, None) == -1
    assert L.ria_gpu_mcdpsk_ring_host(None, 1, 0, 0, 0, None, p, 16, p, 4800, 1, 1, None, 0, 0, p, p, 320, None, p) == -1
