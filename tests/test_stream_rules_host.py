"""ria_amd/csrc/stream_rules.hpp on the host: tests/helpers/stream_rules_check.cpp walks the rules of
ria_gpu_rx_stream_batch over their domain (the window length at capture_len - search_start = full - 1, full, full + 1 and 0;
last_decoded_sync = INT32_MIN and values on both sides of the clip; every window outcome of both families with next_pos -1
and >= 0; fed below and above the new cursor and above capture_len; a cursor at 959 998, 959 999 and 960 000; max_events
reached and not reached) and prints every case; each line is computed again from tests/stream_restatement.py, the statements
of ria_amd.acquire.rx_stream, and compared.  Built and run plain and with -fsanitize=address,undefined.  Then the record
layouts of the ctypes binding, and what the two calls reject before they touch a GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import stream_restatement as SR

F = np.float32
SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "stream_rules_check.cpp")


def fl(h):
    return np.array([int(h, 16)], np.uint32).view(F)[0]


def same(got_hex, want):
    got = fl(got_hex)
    return (np.isnan(got) and np.isnan(want)) or got.view(np.uint32) == F(want).view(np.uint32)


def check(line):
    name, *rest = line.split()
    a, r = rest[:rest.index("->")], rest[rest.index("->") + 1:]
    if name == "conf":
        return same(r[0], SR.min_confidence(fl(a[0]), fl(a[1])))
    a, got = list(map(int, a)), int(r[0])
    if name == "window":
        return got == SR.window_len(*a)
    if name == "rebase":
        return got == SR.rebase_last_sync(*a)
    if name == "moved":
        return got == int(SR.moved(*a))
    if name == "cursor":
        return got == SR.cursor(*a)
    if name == "close":
        return got == SR.close(*a)
    if name == "last":
        return got == SR.last_sync(a[0], bool(a[1]), *a[2:])
    if name == "fed":
        return got == SR.fed(*a)
    return False


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_stream_rules_host_program(flags):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chk")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-o", exe, SRC])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = out.stdout.splitlines()
    assert {ln.split()[0] for ln in lines} == {"window", "conf", "rebase", "moved", "cursor", "close", "last", "fed"}
    assert len(lines) > 1000
    with np.errstate(all="ignore"):
        bad = [ln for ln in lines if not check(ln)]
    assert not bad, bad[:10]
    # the walk reaches what it is there for: a cut window and a full one, "none" kept and both clips, every close reason
    last = lambda name: {ln.split()[-1] for ln in lines if ln.startswith(name + " ")}
    assert {"0", "70000", "69999"} <= last("window")
    assert {str(-2 ** 31), str(-2 ** 31 + 1), str(2 ** 31 - 1)} <= last("rebase")
    assert last("moved") == {"0", "1"}
    assert last("close") == {"0", "4", "5", "6"}
    assert str(-2 ** 31) in last("last")


def test_stream_record_layouts():
    """the sizes and offsets the static_assert of ria_gpu.hip names (include/ria_gpu.h: 64-byte records)"""
    from ria_amd import capi
    from ria_amd.engine import RxEngine
    assert C.sizeof(capi.StreamEvent) == 64 and C.sizeof(capi.StreamResult) == 64
    assert (capi.StreamEvent.next_pos.offset, capi.StreamEvent.delivered.offset, capi.StreamEvent.correlation.offset) == (16, 32, 40)
    assert capi.StreamResult.invocations.offset == 16
    for ct, dt in ((capi.StreamEvent, RxEngine.STREAM_EVENT), (capi.StreamResult, RxEngine.STREAM_RESULT)):
        assert dt.itemsize == C.sizeof(ct)
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(ct, n).offset) for n, _ in ct._fields_]
    header = open(os.path.join(os.path.dirname(SRC), "..", "..", "include", "ria_gpu.h")).read()
    for name, value in capi.STREAM_CLOSED.items():
        assert f"RIA_STREAM_{name} = {value}" in header


def test_stream_calls_reject_a_null_handle_without_a_gpu():
    """the one check of the two calls that comes before a handle exists (a handle needs a GPU): the rest of the argument
    checks are in tests/test_gpu_stream_call.py"""
    from ria_amd import capi
    L = capi.load()
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    assert L.ria_gpu_rx_stream_batch(None, None, 0, 0, None, p, 1024, p, 1, p, 0, 1, 1, p, p, 4096, p, None) == -1
    assert L.ria_gpu_rx_stream_host(None, None, 0, 0, None, p, 16, p, 0, 1, 1, p, p, 1024, p) == -1
