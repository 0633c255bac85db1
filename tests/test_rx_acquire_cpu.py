"""CPU tests of the acquire-and-decode entry point (ria_gpu_rx_acquire_batch): its ABI, the host-side rules of
ria_amd.acquire, and the CPU restatement of StreamingDecoder's connected-mode OFDM data path the GPU tests compare
against (tests/acquire_restatement.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pyoracle as po
from acquire_restatement import acquire_window, window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_acquire_symbol_and_struct_layouts_match_the_header():
    from ria_amd import capi
    L = capi.load()
    assert "ria_gpu_rx_acquire_batch" in capi.EXPORTS and getattr(L, "ria_gpu_rx_acquire_batch") is not None
    assert C.sizeof(capi.AcqParams) == C.sizeof(capi.AcqResult) == 32
    header = open(os.path.join(ROOT, "include", "ria_gpu.h")).read()
    sizes = {"float": 4, "uint32_t": 4, "int32_t": 4, "uint64_t": 8, "int16_t": 2, "uint8_t": 1}
    for cname, ctype in (("ria_acq_params", capi.AcqParams), ("ria_acq_result", capi.AcqResult)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1)
        off = 0
        for t, name, count in re.findall(r"^\s*(\w+)\s+(\w+)(?:\[(\d+)\])?;", body, re.M):
            sz = sizes[t]
            off = (off + sz - 1) // sz * sz
            assert getattr(ctype, name).offset == off, (cname, name)
            off += sz * int(count or 1)
        assert off == 32, cname
    assert (capi.AcqResult.delta.offset, capi.AcqResult.candidates.offset, capi.AcqResult.burst_interleaved.offset) == (24, 26, 27)
    assert capi.ACQ_NO_TIMING_RETRY == int(re.search(r"#define RIA_ACQ_NO_TIMING_RETRY (0x[0-9a-f]+)u", header).group(1), 16)


def test_acquire_rejects_a_null_handle_and_bad_arguments_without_a_gpu():
    from ria_amd import capi
    L = capi.load()
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    assert L.ria_gpu_rx_acquire_batch(None, p, 40000, 21000, 39432, 1, p, 7, p, p, p, None, None) == -1
    assert L.ria_gpu_rx_acquire_batch(None, None, 0, 0, 0, 0, None, 0, None, None, None, None, None) == -1


# light_sync_min_confidence read off streaming_decoder.cpp:679-699 (connected, OFDM):
# (modulation, fading_hint, snr_hint, reject_streak) -> threshold
MIN_CONFIDENCE_POINTS = [
    ("QPSK", 0.0, 30.0, 0, 0.90), ("BPSK", 2.0, 3.0, 40, 0.90),           # coherent PSK: fixed, no relaxation
    ("QAM16", 0.0, 30.0, 0, 0.78), ("QAM256", 1.5, 5.0, 40, 0.78), ("QAM64", 0.6, 12.0, 9, 0.78),
    ("DQPSK", 0.0, 30.0, 0, 0.72), ("D8PSK", 0.49, 18.0, 7, 0.72),
    ("DQPSK", 0.5, 30.0, 0, 0.68), ("DBPSK", 0.0, 17.9, 0, 0.68),
    ("D8PSK", 0.7, 30.0, 0, 0.65), ("DQPSK", 0.0, 13.9, 0, 0.65), ("DQPSK", 0.69, 14.0, 0, 0.68),
    ("DQPSK", 1.0, 30.0, 0, 0.62), ("DBPSK", 0.0, 9.9, 0, 0.62), ("DQPSK", 0.99, 10.0, 0, 0.65),
    ("DQPSK", 0.0, 30.0, 8, 0.705), ("DQPSK", 0.0, 30.0, 12, 0.645), ("DQPSK", 0.0, 30.0, 15, 0.60),
    ("DQPSK", 0.0, 30.0, 40, 0.60), ("DQPSK", 1.2, 30.0, 10, 0.575), ("DQPSK", 1.2, 30.0, 11, 0.56),
    ("DQPSK", 1.2, 8.0, 60, 0.56), ("D8PSK", 0.8, 30.0, 9, 0.62),
]


@pytest.mark.parametrize("mod,fading,snr,streak,expect", MIN_CONFIDENCE_POINTS)
def test_lts_min_confidence_matches_the_reference_rule(mod, fading, snr, streak, expect):
    from ria_amd.acquire import lts_min_confidence
    got = lts_min_confidence(mod, fading, snr, streak)
    assert isinstance(got, np.float32)
    assert abs(float(got) - expect) < 2e-7, (mod, fading, snr, streak, float(got))


def test_window_recipe_does_not_depend_on_the_split():
    from ria_amd.acquire import window_recipe, SEARCH_LEN
    n = 10000
    offs, seeds = window_recipe(123456789, 3, np.arange(n))
    assert offs.min() >= 0 and offs.max() <= SEARCH_LEN - 4 * 1152 and len(np.unique(seeds)) > n - 5
    for chunk in (1, 37, 1000, 4096):
        parts = [window_recipe(123456789, 3, np.arange(s, min(n, s + chunk))) for s in range(0, n, chunk)]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), offs)
        assert np.array_equal(np.concatenate([p[1] for p in parts]), seeds)
    o2, s2 = window_recipe(123456789, 4, np.arange(n))
    assert not np.array_equal(s2, seeds)


def test_cpu_restatement_acquires_and_rejects(oracle):
    """The restatement on the oracle: a clean AWGN window is accepted at its primary candidate and decodes to the sent
    payload; a noise-only window is not detected; a window whose frame runs past the end is not accepted."""
    g = oracle.geom(po.QAM16, po.R1_2)
    search_len, wl = 21000, 21000 + g.frame_samples
    rng = np.random.default_rng(5)
    x, info = window(oracle, po.QAM16, po.R1_2, rng.integers(0, 256, 141, dtype=np.uint8), 3, 7000, wl, 0, 20.0, 77)
    r = acquire_window(oracle, po.QAM16, po.R1_2, x, search_len, 0.0, 0.15, 0.78, abs_base=1000)
    assert r["detected"] == 1 and r["accepted"] == 1 and r["delta"] == 0 and r["candidates"] == 1
    assert abs(r["sync_start"] - 7000) <= 64 and r["frame_start"] == r["sync_start"]
    assert r["cw_ok"].all() and np.array_equal(r["info"], info)
    x, _ = window(oracle, po.QAM16, po.R1_2, None, 0, None, wl, 0, 20.0, 78)
    r = acquire_window(oracle, po.QAM16, po.R1_2, x, search_len, 0.0, 0.15, 0.78)
    assert r["detected"] == 0 and r["accepted"] == 0 and r["sync_start"] == -1 and r["candidates"] == 0
    assert not r["info"].any()
    # the same frame with too little window behind it
    x, _ = window(oracle, po.QAM16, po.R1_2, rng.integers(0, 256, 141, dtype=np.uint8), 4, 7000, 7000 + g.frame_samples - 100, 0, 20.0, 79)
    r = acquire_window(oracle, po.QAM16, po.R1_2, x, search_len, 0.0, 0.15, 0.78)
    assert r["detected"] == 1 and r["accepted"] == 0 and r["frame_start"] == -1 and r["candidates"] == 0
