"""CPU tests of ria_gpu_rx_burst_batch's interface and of its restatement (tests/burst_restatement.py): the ctypes layout,
the energy gate's arithmetic, the recorded burst groups of tests/golden/burst_chain.npz, and the scenario set the GPU test
runs - every stop reason, both modes, the CFO clamp in both directions - shown here on the oracle alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import burst_restatement as br
import pyoracle as po
from test_oracle_golden import bits_equal, burst_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_burst_result_layout_matches_the_header():
    """ria_burst_result is 64 bytes with the header's field offsets; the Python mirrors (ctypes and numpy) agree with it,
    and the constants are the header's."""
    from ria_amd import capi
    from ria_amd.engine import RxEngine
    R = capi.BurstResult
    assert C.sizeof(R) == 64
    want = dict(detected=0, accepted=4, sync_start=8, frame_start=12, correlation=16, cfo_hz=20, delta=24, candidates=26,
                burst_interleaved=27, mode=28, frames=29, frames_decoded=30, stop=31, reserved=32)
    assert {n: getattr(R, n).offset for n in want} == want
    dt = RxEngine.BURST_RESULT
    assert dt.itemsize == 64 and {n: dt.fields[n][1] for n in want} == want
    hdr = open(os.path.join(ROOT, "include", "ria_gpu.h")).read()
    defs = dict(re.findall(r"#define (RIA_BURST_\w+)\s+(0x[0-9a-fA-F]+|\d+)", hdr))
    assert int(defs["RIA_BURST_MAX_FRAMES"], 0) == capi.BURST_MAX_FRAMES == br.SLOTS == 9
    assert int(defs["RIA_BURST_INTERLEAVE"], 0) == capi.BURST_INTERLEAVE and int(defs["RIA_BURST_NO_CONTINUE"], 0) == capi.BURST_NO_CONTINUE
    stops = dict(re.findall(r"RIA_BURST_STOP_(\w+) = (\d+)", hdr))
    assert {k: int(v) for k, v in stops.items()} == capi.BURST_STOP == br.STOP
    assert "ria_gpu_rx_burst_batch" in capi.EXPORTS and "int ria_gpu_rx_burst_batch(" in hdr
    # the 9-slot strides of the per-frame outputs
    assert C.sizeof(capi.DecodeStatus) * 9 == 180 and C.sizeof(capi.FrameStatus) * 9 == 288


def test_gate_sum_is_sequential_float32():
    """np.cumsum over float32 adds in order: equal to one float32 add per sample, and different from a pairwise sum"""
    rng = np.random.default_rng(5)
    differs = 0
    for k in range(4):
        x = (rng.standard_normal(18432) * 10.0 ** rng.uniform(-3, 1)).astype(np.float32)
        a, b = br.gate_rms(x), br.gate_rms_loop(x)
        assert a.dtype == np.float32 and a.view(np.uint32) == b.view(np.uint32)
        seg = x[1024:6024]
        differs += int(np.sqrt(np.float32(np.sum(seg * seg, dtype=np.float32) / np.float32(5000))) != a)
    assert differs >= 1, "a pairwise sum gives the same bits on all vectors: the check shows nothing"
    short = rng.standard_normal(3000).astype(np.float32)
    assert br.gate_rms(short).view(np.uint32) == br.gate_rms_loop(short).view(np.uint32)
    assert not (np.float32("nan") < np.float32(0.04))


def test_restatement_reproduces_the_recorded_groups(oracle, golden):
    """Every marked case of burst_chain.npz through burst_window (RIA_BURST_INTERLEAVE, group_size = n, the rebuilt buffer
    as the window): every frame passes the gate, and cfo_used, cfo_after, the decoded flags and bytes are the recorded
    ones.  A case that failed the gate would have to abort with STOP_ENERGY; at most one may."""
    left_out = 0
    for i, case, x, g in burst_cases(golden, oracle):
        mod, rate, n, lead, kind, snr, cfo0, abs_base, marker = case
        if not marker:
            continue
        n = int(n)
        r = br.burst_window(oracle, int(mod), int(rate), x, 21000, n, known_cfo=float(cfo0), detect_threshold=0.5, min_confidence=0.0,
                            abs_base=int(abs_base))
        assert r["mode"] == 2 and r["burst_interleaved"] == 1 and r["sync_start"] == int(g[f"sync_{i}"][1])
        fs = oracle.geom(int(mod), int(rate)).frame_samples
        rms = [br.gate_rms(x[r["sync_start"] + f * fs:r["sync_start"] + (f + 1) * fs]) for f in range(1, n)]
        if not all(v >= np.float32(0.04) for v in rms):
            assert r["stop"] == br.STOP["ENERGY"] and r["frames_decoded"] == 0 and not r["info"].any()
            left_out += 1
            continue
        assert r["stop"] == br.STOP["NONE"] and r["frames"] == n and r["frames_decoded"] == n
        assert np.array_equal(r["cfo_used"][:n].view(np.uint32), g[f"cfo_used_{i}"].view(np.uint32)), i
        assert np.array_equal(np.array([r["aux"][f]["cfo_hz"] for f in range(n)]).view(np.uint32), g[f"cfo_after_{i}"].view(np.uint32)), i
        assert np.array_equal(r["rms"][1:n].view(np.uint32), np.array(rms).view(np.uint32)) and r["rms"][0] == 0
        assert np.array_equal(r["cw_ok"][:n], g[f"dec_ok_{i}"]) and np.array_equal(r["info"][:n], g[f"dec_data_{i}"]), i
        assert not r["info"][n:].any() and not r["cw_ok"][n:].any()
    assert left_out <= 1


_scen = {}


def scenario_results(oracle):
    """name -> (window, restatement dict) of the scenario set, computed once per process"""
    if not _scen:
        for name, (x, stop, mode, known) in br.scenarios(oracle).items():
            r = br.burst_window(oracle, po.QAM16, po.R1_2, x, br.SEARCH_LEN, br.GROUP, known_cfo=known, abs_base=77000)
            _scen[name] = (x, r, stop, mode)
    return _scen


def test_scenarios_take_every_branch(oracle):
    """The scenario set on the oracle alone: each stop reason and each mode where it is meant to be, the clamp active
    upwards and downwards and inactive, plus the three per-call variants (no continuation, marker without the interleave
    flag, a silenced group leaves nothing)."""
    S = scenario_results(oracle)
    for name, (x, r, stop, mode) in S.items():
        assert r["mode"] == mode and r["stop"] == br.STOP[stop], (name, r["mode"], r["stop"])
        assert len(x) == br.WINDOW_LEN
    assert {r["stop"] for _, r, _, _ in S.values()} >= {br.STOP[k] for k in ("NONE", "ENERGY", "WINDOW", "DECODE", "NOT_DATA", "LIMIT", "RECOVERED")}
    r = S["energy"][1]; assert r["frames"] == 2 and r["frames_decoded"] == 2 and r["cw_ok"][:2].all() and 0 < r["rms"][2] < 0.04
    r = S["window"][1]; assert r["frames"] == 2 and r["sync_start"] + 3 * br.FS > br.WINDOW_LEN >= r["sync_start"] + 2 * br.FS
    r = S["decode"][1]; assert r["frames"] == 3 and r["frames_decoded"] == 3 and not r["cw_ok"][2].any() and r["rms"][2] >= 0.04
    r = S["not_data"][1]; assert r["frames"] == 1 and r["frame_valid"][0] and r["info"][0][2] == 0x20
    r = S["limit"][1]; assert r["frames"] == 9 and r["frames_decoded"] == 9 and r["cw_ok"].all() and r["frame_valid"].all()
    r = S["recovered"][1]; assert r["delta"] != 0 and r["frames"] == 1 and r["cw_ok"][0].all() and r["frame_valid"][0] and r["candidates"] > 1
    r = S["group_ok"][1]; assert r["frames_decoded"] == 4 and r["cw_ok"][:4].all(axis=1).sum() >= 3 and r["frame_valid"][:4].sum() >= 3 and r["candidates"] == 0
    r = S["group_energy"][1]; assert r["frames"] == 2 and r["frames_decoded"] == 0 and not r["info"].any() and not r["cw_ok"].any()
    r = S["group_window"][1]; assert r["frames"] == 2 and r["frames_decoded"] == 0 and not r["info"].any()
    up, down = S["clamp_up"][1], S["clamp_down"][1]
    assert up["cfo_used"][1] == np.float32(2.0) and down["cfo_used"][1] == np.float32(-2.0), (up["cfo_used"], down["cfo_used"])
    assert up["frames_decoded"] == 4 and down["frames_decoded"] == 4
    ok = S["group_ok"][1]
    assert all(abs(ok["aux"][f]["cfo_hz"] - ok["cfo_used"][f]) <= 2.0 and ok["cfo_used"][f + 1] == ok["aux"][f]["cfo_hz"] for f in range(3)), "clamp inactive"
    assert S["silence"][1]["accepted"] == 0
    # per-call variants
    x = S["limit"][0]
    r = br.burst_window(oracle, po.QAM16, po.R1_2, x, br.SEARCH_LEN, br.GROUP, continuation=False, abs_base=77000)
    assert r["mode"] == 1 and r["stop"] == br.STOP["NONE"] and r["frames"] == 1 and r["frames_decoded"] == 1 and not r["info"][1:].any()
    x = S["group_ok"][0]
    r = br.burst_window(oracle, po.QAM16, po.R1_2, x, br.SEARCH_LEN, br.GROUP, interleave=False, abs_base=77000)
    assert r["mode"] == 1 and r["burst_interleaved"] == 1 and r["frames_decoded"] >= 1
    # frame 0 carries interleaved bytes of four logical frames: no complete frame comes out of it, the burst ends there
    assert r["stop"] == br.STOP["DECODE"] and r["frames"] == 1 and r["frames_decoded"] == 1, (r["stop"], r["frames"], r["frames_decoded"])


def test_burst_tally_counts_modes_stops_and_frames():
    """acquire.burst_tally on a hand-made rx_burst result: windows per (mode, stop reason), frames demodulated, logical
    frames handed to the decoder, and those complete, CRC-valid and equal to the sent bytes (slots past frames_decoded and
    past the sent frames do not count)."""
    from ria_amd.acquire import BURST_COUNTERS, BURST_STOPS, burst_tally
    from ria_amd.engine import RxEngine
    from ria_amd import capi
    assert len(BURST_STOPS) == 8 and all(capi.BURST_STOP[s.upper()] == k for k, s in enumerate(BURST_STOPS))
    n, ib = 5, 12
    res = np.zeros(n, RxEngine.BURST_RESULT)
    res["detected"] = [1, 1, 1, 1, 0]
    res["accepted"] = [1, 1, 1, 0, 0]
    res["mode"] = [2, 1, 1, 0, 0]
    res["stop"] = [0, br.STOP["ENERGY"], br.STOP["DECODE"], 0, 0]
    res["frames"] = [4, 3, 1, 0, 0]
    res["frames_decoded"] = [4, 3, 1, 0, 0]
    sent = np.arange(n * 4 * ib, dtype=np.uint8).reshape(n, 4, ib)
    info = np.zeros((n, 9, ib), np.uint8)
    info[:, :4] = sent
    st = np.zeros((n, 9), RxEngine.DECODE_STATUS)
    st["cw_ok"] = 1
    st["frame_valid"] = 1
    info[0, 3, 5] ^= 1                 # a wrong byte
    st["cw_ok"][1, 1, 2] = 0           # an undecoded codeword
    st["frame_valid"][1, 2] = 0        # a frame whose CRC failed
    row = dict(zip(BURST_COUNTERS, burst_tally(dict(result=res, decode_status=st, info=info), sent)))
    assert row["windows"] == 5 and row["detected"] == 4 and row["accepted"] == 3
    assert row["mode2_none"] == 1 and row["mode1_energy"] == 1 and row["mode1_decode"] == 1
    assert sum(v for k, v in row.items() if k.startswith("mode")) == 3
    assert row["frames"] == 8 and row["frames_decoded"] == 8 and row["frames_ok"] == 3 + 1 + 1
