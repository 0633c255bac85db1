"""CPU tests of the MC-DPSK acquire-and-decode entry point (ria_gpu_mcdpsk_acquire_batch): its ABI, the ZC acceptance
tables of ria_amd.acquire, and the CPU restatement the GPU tests compare against (tests/mcdpsk_acquire_restatement.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pyoracle as po
from mcdpsk_acquire_restatement import ACK, CONNECT, acquire_window, control_frame, data_frame, encode_frame, frame_len, window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mcdpsk_acquire_symbol_struct_and_flags_match_the_header():
    from ria_amd import capi
    L = capi.load()
    assert "ria_gpu_mcdpsk_acquire_batch" in capi.EXPORTS and getattr(L, "ria_gpu_mcdpsk_acquire_batch") is not None
    assert C.sizeof(capi.McAcqParams) == 32 and C.sizeof(capi.McAcqResult) == 64
    header = open(os.path.join(ROOT, "include", "ria_gpu.h")).read()
    sizes = {"float": 4, "uint32_t": 4, "int32_t": 4, "uint64_t": 8, "int16_t": 2, "uint8_t": 1}
    for cname, ctype, total in (("ria_mcdpsk_acq_params", capi.McAcqParams, 32), ("ria_mcdpsk_acq_result", capi.McAcqResult, 64)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1)
        off = 0
        for t, name, count in re.findall(r"^\s*(\w+)\s+(\w+)(?:\[(\d+)\])?;", body, re.M):
            sz = sizes[t]
            off = (off + sz - 1) // sz * sz
            assert getattr(ctype, name).offset == off, (cname, name)
            off += sz * int(count or 1)
        assert off == total, cname
    from ria_amd.engine import RxEngine
    assert RxEngine.MCACQ_RESULT.itemsize == 64 and RxEngine.MCACQ_PARAMS.itemsize == 32
    for name in RxEngine.MCACQ_RESULT.names:
        assert RxEngine.MCACQ_RESULT.fields[name][1] == getattr(capi.McAcqResult, name).offset, name
    for flag in ("SYNC_CHIRP", "DISCONNECTED", "NO_RETRY", "CHANNEL_INTERLEAVE"):
        assert getattr(capi, "MACQ_" + flag) == int(re.search(r"#define RIA_MACQ_%s\s+(0x[0-9a-f]+)u" % flag, header).group(1), 16)
    assert "#define RIA_MACQ_FRAME_BYTES(frame_cw) (40 * (frame_cw))" in header and capi.macq_frame_bytes(3) == 120


def test_mcdpsk_acquire_rejects_a_null_handle_without_a_gpu():
    """A null handle is RIA_ERR_INVALID whatever the other arguments (the argument checks themselves are tested on a real
    handle in test_gpu_mcdpsk_acquire.py)."""
    from ria_amd import capi
    L = capi.load()
    buf = (C.c_uint8 * 256)()
    p = C.cast(buf, C.c_void_p)
    cfg = capi.McdpskConfig(10, 1, 1, 0)
    f = L.ria_gpu_mcdpsk_acquire_batch
    ok_args = dict(stride=200000, search_len=70000, window_len=170000, n=1, frame_cw=3, flags=capi.MACQ_SYNC_CHIRP | capi.MACQ_DISCONNECTED)
    bad = [dict(), dict(flags=capi.MACQ_DISCONNECTED), dict(frame_cw=0), dict(frame_cw=9), dict(search_len=180000), dict(n=-1)]
    for b in bad:
        a = dict(ok_args, **b)
        assert f(None, C.byref(cfg), p, a["stride"], a["search_len"], a["window_len"], a["n"], a["frame_cw"], p, a["flags"], p, p,
                 None, 0, None) == -1
    assert f(None, None, None, 0, 0, 0, 0, 0, None, 0, None, None, None, 0, None) == -1


# light_sync_min_confidence / weak_sync_floor of connected ZC mode (streaming_decoder.cpp:679-717)
@pytest.mark.parametrize("streak,conf,floor", [(0, 0.40, 0.30), (3, 0.40, 0.30), (4, 0.375, 0.275), (5, 0.35, 0.25),
                                               (6, 0.325, 0.225), (7, 0.30, 0.20), (8, 0.275, 0.20), (9, 0.25, 0.20),
                                               (10, 0.25, 0.20), (40, 0.25, 0.20)])
def test_zc_min_confidence_and_weak_floor_match_the_rule(streak, conf, floor):
    from ria_amd.acquire import zc_min_confidence, zc_weak_floor
    c, w = zc_min_confidence(streak), zc_weak_floor(streak)
    assert isinstance(c, np.float32) and isinstance(w, np.float32)
    assert abs(float(c) - conf) < 2e-7 and abs(float(w) - floor) < 2e-7, (streak, float(c), float(w))


def test_mcdpsk_window_recipe():
    from ria_amd.acquire import mcdpsk_frame_len, mcdpsk_window_recipe
    assert mcdpsk_frame_len(3) == 4608 + 3 * 65 * 512 == frame_len(3, 10, 1, 1)
    assert mcdpsk_frame_len(1, 10, 2, 4) == 4608 + 33 * 512 * 4
    sl, wl = mcdpsk_window_recipe(57600, 3)
    assert sl == 2000 + 57600 + 4096 and wl == 2000 + 57600 + mcdpsk_frame_len(3) + 2000


def _windows(checker):
    connect = encode_frame(data_frame(CONNECT, 7, np.arange(25, dtype=np.uint8)))
    ack = encode_frame(control_frame(ACK, 3))
    fl3, fl1 = frame_len(3, 10, 1, 1), frame_len(1, 10, 1, 1)
    chirp_sl, chirp_wl = 2000 + 57600 + 4096, 2000 + 57600 + fl3 + 2000
    zc_sl, zc_wl = 2000 + 2512 + 4096, 2000 + 2512 + fl1 + 2000
    return [
        (window(checker, connect, 10, po.DBPSK, 1, True, 2000, chirp_wl, 0, 10.0, 1), chirp_sl, 3, True),
        (window(checker, None, 10, po.DBPSK, 1, True, 2000, chirp_wl, 0, 10.0, 2), chirp_sl, 3, True),
        (window(checker, ack, 10, po.DBPSK, 1, False, 2000, zc_wl, 0, 10.0, 3), zc_sl, 1, False),
    ]


def test_cpu_restatement_decodes_connect_and_control_frames_and_rejects_noise(oracle):
    (x0, sl0, cw0, _), (x1, sl1, cw1, _), (x2, sl2, cw2, _) = _windows(oracle)
    r = acquire_window(oracle, x0, sl0, cw0)
    assert r["success"] == 1 and r["frame_type"] == CONNECT and r["header_total_cw"] == 3 and r["delta"] == 0
    assert np.array_equal(r["frame"], data_frame(CONNECT, 7, np.arange(25, dtype=np.uint8))) and r["candidates"] == 1
    r = acquire_window(oracle, x1, sl1, cw1)
    assert r["detected"] == 0 and r["accepted"] == 0 and r["candidates"] == 0 and r["frame_bytes"] == 0
    r = acquire_window(oracle, x2, sl2, cw2, chirp=False, min_confidence=0.25)
    assert r["detected"] == 1 and r["accepted"] == 1 and r["candidates"] == 1           # connected ZC: no fallbacks
    # a 1-CW control frame on the chirp path is a success with total_cw 1
    ack = encode_frame(control_frame(ACK, 4))
    x = window(oracle, ack, 10, po.DBPSK, 1, True, 2000, 2000 + 57600 + frame_len(1, 10, 1, 1) + 2000, 0, 10.0, 5)
    r = acquire_window(oracle, x, 2000 + 57600 + 4096, 1)
    assert r["success"] == 1 and r["frame_type"] == ACK and r["header_total_cw"] == 1
    assert np.array_equal(r["frame"], control_frame(ACK, 4))


def test_cpu_restatement_on_ref_equals_the_oracle(oracle):
    if not po.Ref.available():
        pytest.skip("the reference library (oracle/_ref) is not built")
    ref = po.Ref()
    for x, sl, cw, chirp in _windows(oracle):
        a = acquire_window(oracle, x, sl, cw, chirp=chirp, min_confidence=0.0 if chirp else 0.25)
        b = acquire_window(ref, x, sl, cw, chirp=chirp, min_confidence=0.0 if chirp else 0.25)
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
