"""GPU tests (-m gpu) of ria_gpu_rx_acquire_batch: LTS detection + acceptance + demod/decode at the detected start +
the reference's timing recovery, in one call over a batch of capture windows.  Bit-exact against the CPU restatement of
StreamingDecoder's connected-mode OFDM data path (tests/acquire_restatement.py) on the oracle and, where oracle/_ref is
built, on the compiled reference; consistent with sync_lts_batch + rx_batch called separately; independent of batching."""
import numpy as np
import pytest

import pyoracle as po
from acquire_restatement import acquire_window, window
from test_gpu_parity import bits, dev, engine

pytestmark = pytest.mark.gpu

SEARCH_LEN, WINDOW_LEN = 21000, 36000
DETECT_THRESHOLD, MIN_CONF = 0.15, 0.78
AUX_FIELDS = ("snr_db", "cfo_hz", "fading_index", "noise_variance", "lts_phase_slope", "snr_linear", "corr_phase")
ACQ_FIELDS = ("detected", "accepted", "sync_start", "frame_start", "delta", "candidates", "burst_interleaved")
# the parity set's categories as the restatement classifies them (pinned: a change of any of them is a change of the set)
PINNED = {"windows": 74, "noise_only": 3, "not_detected": 7, "rejected": 11, "not_fitting": 2, "primary_ok": 22,
          "recovered": 22, "all_failed": 10, "burst": 1, "recovery_deltas": 7}


def parity_set(oracle):
    """The fixed window set (CPU-built, oracle TX + oracle channel = the reference's channel stream) -> (windows [n, WINDOW_LEN],
    sent infos (None for noise), kinds).  64 Watterson-moderate windows at 12 dB (detections, rejections, primary
    successes, recoveries at several deltas, windows where every candidate fails), noise-only windows, AWGN primaries,
    one burst-marked frame and two frames too close to the window's end for the primary candidate."""
    rows, infos, kinds = [], [], []

    def add(kind, x, info):
        rows.append(x); infos.append(info); kinds.append(kind)
    for s in range(64):
        seed = 3000 + s
        rng = np.random.default_rng(seed)
        x, info = window(oracle, po.QAM16, po.R1_2, rng.integers(0, 256, 141, dtype=np.uint8), seed, 4000 + (s * 1237) % 7000,
                         WINDOW_LEN, 2, 12.0, seed)
        add("watterson", x, info)
    for s in range(3):
        x, _ = window(oracle, po.QAM16, po.R1_2, None, 0, None, WINDOW_LEN, 0, 20.0, 3100 + s)
        add("noise", x, None)
    for s, lead in enumerate((3000, 6000, 9000, 12000)):
        rng = np.random.default_rng(3200 + s)
        x, info = window(oracle, po.QAM16, po.R1_2, rng.integers(0, 256, 141, dtype=np.uint8), 3200 + s, lead, WINDOW_LEN, 0, 20.0, 3200 + s)
        add("awgn", x, info)
    rng = np.random.default_rng(3300)
    x, info = window(oracle, po.QAM16, po.R1_2, rng.integers(0, 256, 141, dtype=np.uint8), 3300, 8000, WINDOW_LEN, 0, 20.0, 3300,
                     negate_first_lts=True)
    add("burst", x, info)
    for s, lead in enumerate((17700, 18200)):
        rng = np.random.default_rng(3400 + s)
        x, info = window(oracle, po.QAM16, po.R1_2, rng.integers(0, 256, 141, dtype=np.uint8), 3400 + s, lead, WINDOW_LEN, 0, 20.0, 3400 + s)
        add("late", x, info)
    return np.stack(rows).astype(np.float32), infos, kinds


def classify(exp, kinds):
    c = dict(windows=len(exp), noise_only=kinds.count("noise"), not_detected=0, rejected=0, not_fitting=0, primary_ok=0,
             recovered=0, all_failed=0, burst=0)
    deltas = set()
    for r in exp:
        if not r["detected"]:
            c["not_detected"] += 1
        elif not r["accepted"]:
            fits = r["sync_start"] + 18432 <= WINDOW_LEN
            c["not_fitting" if not fits else "rejected"] += 1
        elif r["delta"] != 0:
            c["recovered"] += 1; deltas.add(r["delta"])
        elif r["cw_ok"].any():
            c["primary_ok"] += 1
        else:
            c["all_failed"] += 1
        c["burst"] += int(r["accepted"] and r["burst_interleaved"] == 1)
    c["recovery_deltas"] = len(deltas)
    return c


_checkers = {}


def _restate_one(job):
    """worker of restate(): one window on the oracle, in a fresh process of its own"""
    mod, rate, x, abs_base, conf = job
    if "oracle" not in _checkers:
        _checkers["oracle"] = po.Oracle()
    r = acquire_window(_checkers["oracle"], mod, rate, x, SEARCH_LEN, 0.0, DETECT_THRESHOLD, conf, abs_base)
    r["aux"] = None if r["aux"] is None else {f: np.float32(getattr(r["aux"], f)) for f in AUX_FIELDS}
    return r


def restate(X, abs_base, mod=po.QAM16, rate=po.R1_2, conf=MIN_CONF):
    """the restatement of every window on the oracle, spread over 8 spawned worker processes (the full decode cascade of
    failing candidates is slow on one core); the workers never touch the GPU"""
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(8, mp_context=mp.get_context("spawn")) as pool:
        return list(pool.map(_restate_one, [(mod, rate, X[i], int(abs_base[i]), float(conf)) for i in range(len(X))]))


def assert_window_equal(i, got_info, got_st, got_res, got_fst, r, full=True):
    """GPU outputs of window i vs the restatement's dict r: every ria_acq_result field, the bytes, the decode status the
    checker gives, the reported candidate's CFO (and the demod status when full)"""
    for f in ACQ_FIELDS:
        assert int(got_res[f][i]) == int(r[f]), (i, f, int(got_res[f][i]), r[f])
    assert bits(got_res["correlation"][i]) == bits(r["correlation"]), (i, "correlation")
    assert bits(got_res["cfo_hz"][i]) == bits(r["cfo_hz"]), (i, "cfo_hz")
    assert np.array_equal(got_info[i], r["info"]), (i, "bytes")
    assert np.array_equal(got_st["cw_ok"][i], r["cw_ok"]), (i, "cw_ok")
    if r["iterations"] is not None:
        assert np.array_equal(got_st["iterations"][i], r["iterations"]), (i, "iterations")
        assert np.array_equal(got_st["attempts"][i], r["attempts"]), (i, "attempts")
    if not r["accepted"]:
        assert not got_st[i].tobytes().strip(b"\0") and not got_fst[i].tobytes().strip(b"\0"), (i, "statuses of a window not accepted")
    elif full and r["aux"] is not None:
        a = r["aux"] if isinstance(r["aux"], dict) else {f: np.float32(getattr(r["aux"], f)) for f in AUX_FIELDS}
        for f in AUX_FIELDS[1:]:
            assert bits(got_fst[f][i]) == bits(a[f]), (i, f)
        assert np.isclose(got_fst["snr_db"][i], a["snr_db"], rtol=1e-5, atol=1e-5), i   # display value, log10f not bit-pinned


def run_gpu(e, X, abs_base, **kw):
    import torch
    info, st, res, fst = e.rx_acquire(dev(X), SEARCH_LEN, known_cfo=0.0, detect_threshold=DETECT_THRESHOLD, min_confidence=MIN_CONF,
                                      abs_base=abs_base, want_demod_status=True, **kw)
    torch.cuda.synchronize()
    return info.cpu().numpy(), e.decode_status(st), res, e.frame_status(fst)


_cache = {}


def _windows(oracle):
    """the parity set's windows without the restatement: (windows, sent infos, kinds, abs_base)"""
    if "windows" not in _cache:
        X, infos, kinds = parity_set(oracle)
        _cache["windows"] = (X, infos, kinds, 1_000_000 + 40_000 * np.arange(len(X), dtype=np.uint64))
    return _cache["windows"]


def _set(oracle):
    if "set" not in _cache:
        X, infos, kinds, abs_base = _windows(oracle)
        _cache["set"] = (X, infos, kinds, abs_base, restate(X, abs_base))
    return _cache["set"]


def test_acquire_parity_with_the_cpu_restatement(oracle):
    """Every output field bit-equal to the restatement on a pinned window set that holds every outcome: noise, rejected
    detections, primary successes, primaries that do not fit, a burst-marked frame, recoveries at several deltas, windows
    where all nine candidates fail."""
    X, infos, kinds, abs_base, exp = _set(oracle)
    c = classify(exp, kinds)
    assert c == PINNED, c
    assert sum(int(r["cw_ok"].all() and np.array_equal(r["info"], info)) for r, info in zip(exp, infos)) >= 8
    e = engine("QAM16", "R1_2")
    got = run_gpu(e, X, abs_base)
    for i, r in enumerate(exp):
        assert_window_equal(i, *got, r)
    assert got[2]["candidates"].sum() == sum(r["candidates"] for r in exp)


@pytest.mark.skipif(not po.Ref.available(), reason="oracle/_ref/libria_ref.so is not built (build() makes it where the reference sources are)")
def test_acquire_parity_with_the_compiled_reference(oracle):
    """The same pinned set through the restatement on the compiled reference (detectDataSync, process, decodeFixedFrame of
    the unmodified library), except the burst-marked window: the reference shim's process() has no marker input."""
    X, infos, kinds, abs_base, exp = _set(oracle)
    got = run_gpu(engine("QAM16", "R1_2"), X, abs_base)
    ref = po.Ref()
    for i, k in enumerate(kinds):
        if k == "burst":              # the reference shim's process() has no burst-marker input
            continue
        r = acquire_window(ref, po.QAM16, po.R1_2, X[i], SEARCH_LEN, 0.0, DETECT_THRESHOLD, MIN_CONF, int(abs_base[i]))
        assert_window_equal(i, *got, r, full=False)


def test_acquire_equals_the_separate_calls(oracle):
    """Windows decoded at their first candidate, and every window under RIA_ACQ_NO_TIMING_RETRY, equal sync_lts_batch
    followed by rx_batch at the reported offsets with the same metadata."""
    import torch
    X, infos, kinds, abs_base, exp = _set(oracle)
    e = engine("QAM16", "R1_2")
    full = run_gpu(e, X, abs_base)
    prim = run_gpu(e, X, abs_base, retry=False)
    Xd = dev(X)
    sync = e.sync_lts(Xd[:, :SEARCH_LEN].contiguous(), dev(np.zeros(len(X), np.float32)), DETECT_THRESHOLD)
    for name, (info, st, res, fst), sel in (("retry", full, full[2]["candidates"] == 1), ("no-retry", prim, prim[2]["accepted"] != 0)):
        assert np.array_equal(res["detected"], sync["detected"]) and np.array_equal(bits(res["correlation"]), bits(sync["correlation"]))
        assert np.array_equal(res["sync_start"], np.where(sync["detected"] != 0, sync["start_sample"], -1))
        idx = np.nonzero(sel)[0]
        assert len(idx) >= 20, (name, len(idx))
        start = res["frame_start"][idx].astype(np.uint64)
        offs = idx.astype(np.uint64) * np.uint64(WINDOW_LEN) + start
        i2, s2, _, f2 = e.rx(Xd, offsets=offs, cfo_hz=np.zeros(len(idx), np.float32), abs_pos=abs_base[idx] + start,
                             meta_flags=sync["burst_interleaved"][idx].astype(np.uint32), want_llr=True)
        torch.cuda.synchronize()
        assert np.array_equal(i2.cpu().numpy(), info[idx]), name
        assert e.decode_status(s2).tobytes() == st[idx].tobytes(), name
        assert e.frame_status(f2).tobytes() == fst[idx].tobytes(), name
        assert np.array_equal(bits(e.frame_status(f2)["cfo_hz"]), bits(res["cfo_hz"][idx])), name
    assert (prim[2]["candidates"] <= 1).all() and (prim[2]["delta"] == 0).all()
    assert np.array_equal(prim[2]["accepted"], full[2]["accepted"])


def _batch_windows(e, n, seed=4242):
    """n windows of the sweep recipe (ria_amd.acquire.make_windows) at a faded point where recovery happens"""
    from ria_amd.acquire import make_windows
    from ria_amd.sweep import SweepPoint
    win, sent, _ = make_windows(e, seed, SweepPoint(2, 12.0), 0, 0, n)
    return win, sent


def test_acquire_does_not_depend_on_batching():
    """6 000 windows in one call equal calls of 1, 37 and 4 096 windows (4 096 crosses rx_batch's split into internal
    parts), and a second identical call gives identical outputs: the handle carries nothing from one call to the next."""
    import torch
    e = engine("QAM16", "R1_2")
    n = 6000
    win, _ = _batch_windows(e, n)
    sl = win.shape[1] - e.geo.frame_samples
    abs_base = np.arange(n, dtype=np.uint64) * np.uint64(77777)

    def call(a, b):
        info, st, res, fst = e.rx_acquire(win[a:b].contiguous(), sl, abs_base=abs_base[a:b], want_demod_status=True)
        torch.cuda.synchronize()
        return info.cpu().numpy(), st.cpu().numpy(), res.tobytes(), fst.cpu().numpy()
    whole = call(0, n)
    res = np.frombuffer(whole[2], e.ACQ_RESULT)
    assert (res["delta"] != 0).sum() >= 20 and (res["accepted"] != 0).sum() >= 1000, np.unique(res["delta"], return_counts=True)
    again = call(0, n)
    assert all(np.array_equal(np.frombuffer(a, np.uint8) if isinstance(a, bytes) else a, np.frombuffer(b, np.uint8) if isinstance(b, bytes) else b)
               for a, b in zip(whole, again))
    for size in (4096, 37, 1):
        stops = list(range(0, n, size))[: (3 if size == 1 else None)]
        for a in stops:
            b = min(n, a + size)
            part = call(a, b)
            ib = e.geo.info_bytes_per_frame
            assert np.array_equal(part[0], whole[0][a:b]), (size, a)
            assert np.array_equal(part[1], whole[1][a:b]), (size, a)
            assert part[2] == whole[2][a * 32:b * 32], (size, a)
            assert np.array_equal(part[3], whole[3][a:b]), (size, a)
            del ib
    # size 1 over windows that were recovered, too
    for a in np.nonzero(res["delta"] != 0)[0][:5]:
        part = call(a, a + 1)
        assert part[2] == whole[2][a * 32:(a + 1) * 32] and np.array_equal(part[0], whole[0][a:a + 1])


@pytest.mark.parametrize("mod,rate", [("DQPSK", "R1_2"), ("QPSK", "R3_4")])
def test_acquire_other_modes_vs_the_restatement(oracle, mod, rate):
    """Other pilot layouts: a smaller faded set per mode, every field against the restatement on the oracle."""
    from ria_amd import capi
    from ria_amd.acquire import lts_min_confidence
    m, r = capi.MOD[mod], capi.RATE[rate]
    e = engine(mod, rate)
    conf = float(lts_min_confidence(mod, 0.0, 12.0, 0))
    wl = SEARCH_LEN + e.geo.frame_samples        # these modes' frames are longer than QAM16's
    rows = []
    for s in range(16):
        seed = 5000 + s
        rng = np.random.default_rng(seed)
        x, _ = window(oracle, m, r, rng.integers(0, 256, 141, dtype=np.uint8), seed, 4000 + (s * 977) % 6000, wl,
                      2 if s % 4 else 0, 16.0 if s % 4 else 24.0, seed)
        rows.append(x)
    X = np.stack(rows).astype(np.float32)
    abs_base = np.arange(len(X), dtype=np.uint64) * np.uint64(50000)
    exp = restate(X, abs_base, m, r, conf)
    import torch
    info, st, res, fst = e.rx_acquire(dev(X), SEARCH_LEN, known_cfo=0.0, min_confidence=conf, abs_base=abs_base, want_demod_status=True)
    torch.cuda.synchronize()
    got = (info.cpu().numpy(), e.decode_status(st), res, e.frame_status(fst))
    for i, rr in enumerate(exp):
        assert_window_equal(i, *got, rr)
    assert sum(rr["accepted"] for rr in exp) >= 8


def test_acquire_sweep_counters_do_not_depend_on_the_chunk():
    """run_acquire_point over 8 192 trials in chunks of 4 096 and of 1 000: identical counters, ordered."""
    from ria_amd.acquire import ACQ_COUNTERS, run_acquire_point
    from ria_amd.sweep import SweepPoint
    e = engine("QAM16", "R1_2")
    pt, n = SweepPoint(2, 12.0), 8192
    rows = {}
    for chunk in (4096, 1000):
        rows[chunk] = sum(run_acquire_point(e, pt, 99, 1, s, min(chunk, n - s)) for s in range(0, n, chunk))
    assert np.array_equal(rows[4096], rows[1000]), rows
    c = dict(zip(ACQ_COUNTERS, rows[4096]))
    assert c["windows"] == n and c["recovered"] <= c["accepted"] <= c["detected"] <= c["windows"]
    assert c["primary_ok"] + c["recovered"] <= c["accepted"] and c["decodes"] >= c["accepted"]
    assert c["recovered"] > 0 and c["frame_err"] <= n


def test_workspace_growth_leaves_results_alone(oracle):
    """A call on 2 windows, then one on the whole parity set, on a fresh handle: every array of the second equals the same
    call on another fresh handle that never ran the first, and the first equals that call's first two rows."""
    from ria_amd.engine import RxEngine
    X, _, _, abs_base = _windows(oracle)
    a, b = RxEngine("QAM16", "R1_2", max_batch=64), RxEngine("QAM16", "R1_2", max_batch=64)
    small = run_gpu(a, X[:2], abs_base[:2])
    big = run_gpu(a, X, abs_base)
    ref = run_gpu(b, X, abs_base)
    assert ref[2]["accepted"].sum() > 2 and (ref[2]["delta"] != 0).any()     # rounds ran, recoveries among them
    for k, (s, g, r) in enumerate(zip(small, big, ref)):
        assert g.tobytes() == r.tobytes(), k
        assert s.tobytes() == r[:2].tobytes(), k
    a.close()
    b.close()
