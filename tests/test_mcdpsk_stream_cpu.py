"""CPU: ria_gpu_mcdpsk_stream_batch without a GPU.

(1) ria_amd/csrc/mcdpsk_stream_rules.hpp on the host: tests/helpers/mcdpsk_stream_rules_check.cpp walks the rules - the audio
    clock at t0 = 0, 2^63 and 2^64 - 1 with a sync at sample 0, 47, 48 and 959 998; the re-entry fit at equality and one
    sample short; the re-entered window with need_samples below, at and above `full`; which of the seven RIA_MWIN_* outcomes
    keep the wait; the pending fields' domain - and every line is computed again from tests/mcdpsk_stream_restatement.py.
    Built and run plain and with -fsanitize=address,undefined.
(2) the record layout of the binding and what the two calls reject before they touch a GPU.
(3) the claims the GPU tests rely on, asserted on the restatement's loop (search, window and cache restated on the checker):
    (a) the HARQ recording: reception 1 fails with a valid header and stores, reception 2 alone fails, the sum recovers;
    (b) the same recording without a cache delivers no complete frame;
    (c) the interleaved recording decodes only with the flag;
    (d) on the cut capture the two calls' events, the NEED_SAMPLES event dropped, carry the outcome, next_pos, payload and
        flags of one call on the whole capture."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcdpsk_stream_restatement as MS
import mcdpsk_window_restatement as WR
from mcdpsk_harq_restatement import ChaseCache
from mcdpsk_acquire_restatement import frame_len

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "mcdpsk_stream_rules_check.cpp")


# ---- (1)
def check(line):
    name, *rest = line.split()
    a, got = list(map(int, rest[:rest.index("->")])), int(rest[-1])
    want = dict(now=MS.now_ms, fits=MS.reentry_fits, window=MS.reentry_window_len, fed=MS.reentry_fed, keeps=MS.keeps_pending,
                domain=MS.pending_domain_ok)[name](*a)
    return got == int(want)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_mcdpsk_stream_rules_host_program(flags):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chk")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-o", exe, SRC])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = out.stdout.splitlines()
    assert {ln.split()[0] for ln in lines} == {"now", "fits", "window", "fed", "keeps", "domain"}
    assert len(lines) > 1000
    bad = [ln for ln in lines if not check(ln)]
    assert not bad, bad[:10]
    args = lambda name: [tuple(map(int, ln.split()[1:ln.split().index("->")])) + (int(ln.split()[-1]),) for ln in lines if ln.startswith(name + " ")]
    # the grid reaches what it is there for
    now = {(t0, sync): r for t0, sync, _, r in args("now")}
    for t0 in (0, 2 ** 63, 2 ** 64 - 1):
        assert [now[t0, s] for s in (0, 47, 48, 959998)] == [t0, t0, (t0 + 1) % 2 ** 64, (t0 + 19999) % 2 ** 64]
    assert now[2 ** 64 - 1, 48] == 0 and now[2 ** 64 - 20000, 959998] == 2 ** 64 - 1
    fits = args("fits")
    assert any(cap == sync + need and r == 1 for cap, sync, need, r in fits) and any(cap == sync + need - 1 and r == 0 for cap, sync, need, r in fits)
    win = args("window")
    longer = [w for w in win if w[3] - w[2] + w[4] > w[0]]                    # the wait reaches past `full`
    assert any(w[5] > w[0] for w in longer) and any(w[5] == w[1] - w[2] for w in longer)
    assert any(w[3] - w[2] + w[4] == w[0] and w[5] == w[0] for w in win) and any(w[3] - w[2] + w[4] < w[0] and w[5] == w[0] for w in win)
    assert [r for _, r in args("keeps")] == [0, 0, 0, 0, 0, 0, 1, 0, 0]       # outcomes -1 .. 7: RIA_MWIN_NEED_SAMPLES (5) alone
    assert {r for *_, r in args("domain")} == {0, 1}


# ---- (2)
def test_mcdpsk_stream_record_layout_and_symbols():
    from ria_amd import capi
    from ria_amd.engine import RxEngine
    assert C.sizeof(capi.McStreamState) == 64 and capi.McStreamState.pending_total_cw.offset == 32 and capi.McStreamState.pend_known_cfo_hz.offset == 48
    dt = RxEngine.MCSTREAM_STATE
    assert dt.itemsize == 64 and dt == MS.STATE
    flat = [(n, getattr(capi.SearchState, n).offset) for n, _ in capi.SearchState._fields_] + \
           [(n, getattr(capi.McStreamState, n).offset) for n, _ in capi.McStreamState._fields_[1:]]
    assert [(n, dt.fields[n][1]) for n in dt.names] == flat
    s = RxEngine.mcdpsk_stream_state(3, fed=[1, 2, 3])
    assert list(s["fed"]) == [1, 2, 3] and not any(s[f].any() for f in MS.PENDING) and (s["last_decoded_sync_pos"] == capi.SEARCH_NO_LAST_SYNC).all()
    header = open(os.path.join(os.path.dirname(SRC), "..", "..", "include", "ria_gpu.h")).read()
    for name in ("ria_gpu_mcdpsk_stream_batch", "ria_gpu_mcdpsk_stream_host"):
        assert name in capi.EXPORTS and f"int {name}(" in header
    assert "#define RIA_GPU_ABI_VERSION 1" in header


def test_mcdpsk_stream_calls_reject_a_null_handle_without_a_gpu():
    from ria_amd import capi
    L = capi.load()
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    assert L.ria_gpu_mcdpsk_stream_batch(None, 1, 0, 0, 0, None, p, 1024, p, 1, p, 0, 1, 1, None, None, None, p, p, 320, None, p, None) == -1
    assert L.ria_gpu_mcdpsk_stream_host(None, 1, 0, 0, 0, None, p, 16, p, 0, 1, 1, None, 0, 0, p, p, 320, None, p) == -1


# ---- (3)
def delivered(events):
    return [e for e in events if e["frame"] is not None]


@pytest.fixture(scope="module")
def harq(oracle):
    x, frame, at = MS.harq_recording(oracle, **MS.HARQ_PIN)
    return x, frame, at


def test_a_harq_recording_recovers_through_the_sum(oracle, harq):
    x, frame, at = harq
    cache = ChaseCache()
    st, closed, ev = MS.link_stream(oracle, [x], "MCDPSK_ZC", feed_step=4800, caches=[cache], **MS.GEOM)
    ev = ev[0]
    assert [e["sync_position"] for e in ev] == [a + MS.ZC_LEN for a in at] and all(e["outcome"] == WR.DECODED for e in ev), MS.show(ev)
    first, second = ev
    assert (first["success"], first["codewords_ok"], first["codewords_failed"]) == (0, 2, 1) and first["harq"]["valid"] == 1
    assert first["harq"]["stored_mask"] == 0b10 and first["harq"]["sum_mask"] == 0 and first["harq"]["entry"] == 1
    assert second["success"] == 1 and second["harq"]["sum_mask"] == 0b10 and second["harq"]["recovered_mask"] == 0b10 and second["harq"]["entry"] == 2
    assert second["frame"] == frame
    assert cache.stats["stores"] == 2 and cache.stats["combines"] == 1 and cache.stats["recoveries"] == 1 and cache.size() == 0
    # the cache saw the audio clock: the two stores lie the two syncs' distance apart
    gap_ms = MS.now_ms(0, second["sync_position"]) - MS.now_ms(0, first["sync_position"])
    assert gap_ms == (second["sync_position"] * 1000 // 48000) - (first["sync_position"] * 1000 // 48000) > 0
    # reception 2 on its own fails: a fresh cache in front of it alone
    alone = ChaseCache()
    _, _, ev2 = MS.link_stream(oracle, [x[at[1] - 8000:]], "MCDPSK_ZC", feed_step=4800, caches=[alone], **MS.GEOM)
    assert len(ev2[0]) == 1 and ev2[0][0]["success"] == 0 and ev2[0][0]["codewords_failed"] == 1 and ev2[0][0]["harq"]["recovered_mask"] == 0, MS.show(ev2[0])
    # a TTL below the gap expires the stored codeword before the retransmission arrives
    short = ChaseCache(ttl_ms=gap_ms - 1)
    _, _, ev3 = MS.link_stream(oracle, [x], "MCDPSK_ZC", feed_step=4800, caches=[short], **MS.GEOM)
    assert short.stats["entries_expired"] == 1 and short.stats["recoveries"] == 0 and not any(e["success"] for e in ev3[0])
    edge = ChaseCache(ttl_ms=gap_ms)
    _, _, ev4 = MS.link_stream(oracle, [x], "MCDPSK_ZC", feed_step=4800, caches=[edge], t0_ms=2 ** 64 - 1 - MS.now_ms(0, first["sync_position"]), **MS.GEOM)
    assert edge.stats["entries_expired"] == 0 and edge.stats["recoveries"] == 1 and ev4[0][1]["success"] == 1      # the clock wraps between the two


def test_b_without_a_cache_no_complete_frame(oracle, harq):
    x, frame, at = harq
    _, closed, ev = MS.link_stream(oracle, [x], "MCDPSK_ZC", feed_step=4800, **MS.GEOM)
    assert len(ev[0]) == 2 and not any(e["success"] for e in ev[0]), MS.show(ev[0])
    assert all(e["codewords_ok"] == 2 and e["codewords_failed"] == 1 and e["delivered"] == 1 for e in ev[0])
    assert closed[0] == MS.SR.CLOSED["SEARCH_NEED_SAMPLES"]


@pytest.mark.parametrize("B", [216, 648])
def test_c_interleaved_recording_needs_the_flag(oracle, B):
    x, sent, at = MS.clean_recording(oracle, [5, 6], B=B)
    _, _, ev = MS.link_stream(oracle, [x], "MCDPSK_ZC", feed_step=4800, B=B, **MS.GEOM)
    assert [e["frame"] for e in delivered(ev[0])] == sent and all(e["success"] for e in ev[0]), MS.show(ev[0])
    _, _, ev = MS.link_stream(oracle, [x], "MCDPSK_ZC", feed_step=4800, **MS.GEOM)
    assert not any(e["success"] for e in ev[0]), MS.show(ev[0])


@pytest.mark.parametrize("case", list(MS.CUT_CASES))
def test_d_cut_capture_continues_as_one_call(oracle, case):
    K = MS.CUT_CASES[case]
    c, b, ncw = K["carriers"], K["bps"], K["frame_cw"]
    geom = dict(carriers=c, bps=b, spreading=1)
    x, sent, at = MS.clean_recording(oracle, [5, 6], carriers=c, bps=b, n_payload=K["n_payload"])
    cut = at[0] + MS.ZC_LEN + K["cut_behind_sync"]
    assert frame_len(1, c, b, 1) < K["cut_behind_sync"] < frame_len(ncw, c, b, 1)
    whole_state, whole_closed, whole = MS.link_stream(oracle, [x], "MCDPSK_ZC", feed_step=4800, **geom)
    assert [e["frame"] for e in whole[0]] == sent, MS.show(whole[0])
    st1, closed1, ev1 = MS.link_stream(oracle, [x[:cut]], "MCDPSK_ZC", feed_step=4800, **geom)
    assert closed1[0] == MS.SR.CLOSED["WINDOW_NEED_SAMPLES"] and len(ev1[0]) == 1 and ev1[0][0]["outcome"] == WR.NEED_SAMPLES, (closed1, MS.show(ev1[0]))
    assert st1["pending_total_cw"][0] == ncw and st1["need_samples"][0] == frame_len(ncw, c, b, 1) and st1["pend_sync_position"][0] == at[0] + MS.ZC_LEN
    assert st1["pend_search_start"][0] == ev1[0][0]["search_start"] and st1["pend_correlation"][0] == ev1[0][0]["correlation"]
    # one sample short of what the wait is for: closed again, no event, the state as it was
    short = at[0] + MS.ZC_LEN + frame_len(ncw, c, b, 1) - 1
    st_s, closed_s, ev_s = MS.link_stream(oracle, [x[:short]], "MCDPSK_ZC", state=st1, feed_step=4800, **geom)
    assert closed_s[0] == MS.SR.CLOSED["WINDOW_NEED_SAMPLES"] and ev_s[0] == [] and st_s.tobytes() == st1.tobytes()
    st2, closed2, ev2 = MS.link_stream(oracle, [x], "MCDPSK_ZC", state=st1, feed_step=4800, **geom)
    assert len(ev2[0]) == len(whole[0])
    for got, want in zip(ev2[0], whole[0]):
        for f in ("sync_position", "outcome", "next_pos", "frame", "delivered", "success", "codewords_ok", "codewords_failed", "frame_type", "frame_bytes",
                  "pending_total_cw"):
            assert got[f] == want[f], (f, got[f], want[f])
    assert closed2[0] == whole_closed[0] and not any(st2[f][0] for f in MS.PENDING)
    assert st2.tobytes() == whole_state.tobytes(), (st2, whole_state)
    # the caller gives up: the stream searches on from its cursor.  The search backtracks from it, so it meets the same sync
    # again - as a fresh one, with its peek - and, the samples being there now, delivers both frames
    gave_up = st1.copy()
    gave_up["pending_total_cw"] = 0
    _, closed3, ev3 = MS.link_stream(oracle, [x], "MCDPSK_ZC", state=gave_up, feed_step=4800, **geom)
    assert [e["frame"] for e in delivered(ev3[0])] == sent and closed3[0] == MS.SR.CLOSED["SEARCH_NEED_SAMPLES"], MS.show(ev3[0])
