"""The four HIP acquisition detectors (ria_gpu_sync_zc_batch, ria_gpu_sync_chirp_batch, ria_gpu_sync_lts_batch,
ria_gpu_sync_cox_batch) against the compiled reference over their input domain (tests/sync_domain_inputs.py): every field
of every buffer, bit for bit, in every batch layout.  Answers come from the live reference where oracle/_ref is built and
from tests/golden/sync_domain.npz otherwise.

NaN rule (demod_domain_inputs.same_bits): where a float field is NaN the position must agree; the sign and payload of a
NaN are not compared.  Integer fields compare exactly."""
import ctypes as C

import numpy as np
import pytest

import pyoracle as po
import sync_domain_inputs as S

pytestmark = pytest.mark.gpu

_engines, _gpu, _ref = {}, {}, {}
KIND = {"chirp": 0, "lts": 1, "zc": 2, "cox": 3}          # ria_gpu_sync_host


def engine(det, mask=0):
    from ria_amd.engine import RxEngine
    key = ("DQPSK", "R1_4") if det == "cox" and mask == 1 else ("QAM16", "R1_2")
    if key not in _engines:
        _engines[key] = RxEngine(*key)
    return _engines[key]


def fields(det, r):
    """result structs -> float32 [n, k] in the order of sync_domain_inputs.expected_fields"""
    names = S.FIELDS[det] + (("cfo_hz",) if det == "lts" else ())
    return np.stack([r[k].astype(np.float32) for k in names], axis=1)


def call(det, X, thr, p, mask, gap=0):
    """one batch call on rows X [n, buf_len], laid out `gap` samples apart with NaN in the gaps; the gaps must come back
    untouched -> float32 [n, k]"""
    import torch
    from ria_amd.engine import _ptr, _stream_ptr
    e = engine(det, mask)
    n, buf_len = X.shape
    host = np.full((n, buf_len + gap), np.nan, np.float32)
    host[:, :buf_len] = X
    buf = torch.from_numpy(host).cuda()
    out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    pd = torch.from_numpy(np.ascontiguousarray(p, np.float32)).cuda()
    a = (e.h, _ptr(buf), buf_len + gap, buf_len, n)
    if det == "zc":
        rc = e.lib.ria_gpu_sync_zc_batch(*a, float(thr), int(mask), _ptr(pd), _ptr(out), _stream_ptr())
    elif det == "chirp":
        rc = e.lib.ria_gpu_sync_chirp_batch(*a, float(thr), _ptr(out), _stream_ptr())
    elif det == "lts":
        rc = e.lib.ria_gpu_sync_lts_batch(*a, _ptr(pd), float(thr), _ptr(out), _stream_ptr())
    else:
        rc = e.lib.ria_gpu_sync_cox_batch(*a, float(thr), _ptr(pd), _ptr(out), _stream_ptr())
    e._check(rc)
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == host.tobytes(), f"{det}: the call wrote into its input or the gaps"
    dt = {"zc": e.ZC_RESULT, "chirp": e.CHIRP_RESULT, "lts": e.LTS_RESULT, "cox": e.COX_RESULT}[det]
    return fields(det, e._status_array(out, dt))


def run(det, F, idx=None, gap=0):
    """the buffers idx (all) of a family, one call per (length, threshold, mask) -> float32 [len(idx), k]"""
    idx = list(range(len(F["x"]))) if idx is None else list(idx)
    out = [None] * len(idx)
    where = {i: k for k, i in enumerate(idx)}
    for g in S.groups(F):
        g = [i for i in g if i in where]
        if g:
            res = call(det, np.stack([F["x"][i] for i in g]), F["thr"][g[0]], F["p"][g], F["mask"][g[0]], gap)
            for k, i in enumerate(g):
                out[where[i]] = res[k]
    return np.stack(out)


def gpu_answers(golden, oracle, det, fam):
    """the batch call's answers on a whole family in the dense layout (computed once, never modified)"""
    if (det, fam) not in _gpu:
        F = S.family(oracle, det, fam)
        assert S.digest(F) == str(golden("sync_domain")[f"sha_{det}_{fam}"]), f"{det} {fam}: generator drifted"
        _gpu[(det, fam)] = run(det, F)
    return _gpu[(det, fam)]


def reference_answers(golden, oracle, det, fam):
    if (det, fam) not in _ref:
        F = S.family(oracle, det, fam)
        ans = S.answers(po.Ref(), det, F) if po.Ref.available() else golden("sync_domain")[f"ans_{det}_{fam}"]
        _ref[(det, fam)] = S.expected_fields(det, F, ans)
    return _ref[(det, fam)]


def differences(det, labels, got, exp, what):
    names = S.FIELDS[det] + (("cfo_hz",) if det == "lts" else ())
    return [f"{what} buffer {i} ({labels[i]}): {names[c]} gpu {got[i, c]!r} expected {exp[i, c]!r}"
            for i in range(len(exp)) for c in range(len(names)) if not S.same_bits(got[i, c:c + 1], exp[i, c:c + 1])]


def check(det, labels, got, exp, what):
    bad = differences(det, labels, got, exp, what)
    for b in bad:
        print(b)
    assert not bad, f"{what}: {len(bad)} fields differ, first: {bad[0]}"


@pytest.mark.parametrize("det,fam", S.CASES)
def test_detector_equals_the_reference(golden, oracle, det, fam):
    F = S.family(oracle, det, fam)
    check(det, F["labels"], gpu_answers(golden, oracle, det, fam), reference_answers(golden, oracle, det, fam), f"{det} {fam}")


@pytest.mark.parametrize("det", S.DETECTORS)
@pytest.mark.parametrize("gap", (1, 4099))
def test_rows_further_apart_than_their_length_give_the_same_answers(golden, oracle, det, gap):
    """stride > buf_len with NaN between the rows, every family: a read past buf_len changes an answer, a write there is caught
    by call()"""
    for fam in S.FAMILIES:
        if (det, fam) not in S.CASES:
            continue
        F = S.family(oracle, det, fam)
        idx = list(range(len(F["x"])))
        labels = [F["labels"][i] for i in idx]
        check(det, labels, run(det, F, idx, gap), gpu_answers(golden, oracle, det, fam)[idx], f"{det} {fam} stride buf_len + {gap}")


def _one_call_rows(oracle, det, fams):
    """rows of several families that can share one call (the commonest length, the default threshold and mask)"""
    X, P, src = [], [], []
    for fam in fams:
        F = S.family(oracle, det, fam)
        for i, x in enumerate(F["x"]):
            if len(x) == S.LEN[det] and F["thr"][i] == np.float32(S.THR[det]) and F["mask"][i] == (15 if det == "zc" else 0):
                X.append(x); P.append(F["p"][i]); src.append((fam, i))
    return np.stack(X), np.array(P, np.float32), src


@pytest.mark.parametrize("det", S.DETECTORS)
def test_rows_do_not_depend_on_their_neighbours(golden, oracle, det):
    """detecting, non-detecting and non-finite rows in one call, shuffled, and the first row alone: every row as in its
    family's own call.  Chirp: 1, 63, 64, 65 and 129 rows, across the 64-buffer workspace chunk."""
    X, P, src = _one_call_rows(oracle, det, ("nonfinite", "level", "weak", "silence"))
    exp = np.stack([gpu_answers(golden, oracle, det, fam)[i] for fam, i in src])
    labels = [f"{fam}: {S.family(oracle, det, fam)['labels'][i]}" for fam, i in src]
    assert (exp[:, 0] == 1).sum() >= 3 and (exp[:, 0] == 0).sum() >= 3 and np.isnan(X).any(axis=1).sum() >= 3
    rng = np.random.default_rng(5)
    thr, mask = S.THR[det], 15 if det == "zc" else 0
    sizes = (1, 63, 64, 65, 129) if det == "chirp" else (1, len(X))
    for n in sizes:
        order = rng.permutation(len(X))[:n] if n <= len(X) else np.concatenate([rng.permutation(len(X)) for _ in range(n // len(X) + 1)])[:n]
        if n == 1:
            order = np.array([0])
        got = call(det, X[order], thr, P[order], mask)
        check(det, [labels[i] for i in order], got, exp[order], f"{det} batch of {n}")


@pytest.mark.parametrize("det", S.DETECTORS)
def test_single_buffer_host_form_equals_the_batch_call(golden, oracle, det):
    for fam in S.FAMILIES:
        if (det, fam) not in S.CASES:
            continue
        F = S.family(oracle, det, fam)
        i = len(F["x"]) // 2
        e = engine(det, int(F["mask"][i]))
        dt = {"zc": e.ZC_RESULT, "chirp": e.CHIRP_RESULT, "lts": e.LTS_RESULT, "cox": e.COX_RESULT}[det]
        res = np.zeros(1, dt)
        x = F["x"][i]
        rc = e.lib.ria_gpu_sync_host(e.h, KIND[det], x.ctypes.data, len(x), C.c_float(float(F["thr"][i])), C.c_float(float(F["p"][i])),
                                     int(F["mask"][i]) if det == "zc" else 0, res.ctypes.data)
        assert rc == 0, (det, fam, rc)
        check(det, [F["labels"][i]], fields(det, res), gpu_answers(golden, oracle, det, fam)[i:i + 1], f"{det} {fam} host form")


def _with_mask(F, mask):
    G = dict(F)
    G["mask"] = np.full(len(F["x"]), mask, np.int32)
    return G


def _padded(x, pad):
    w = np.zeros(len(x) + pad, np.float32)
    w[:len(x)] = x
    return w


_checker = {}
LTS_PAD, MC_PAD = 20000, 40000          # room for the frame behind the latest detection
RX_AUX = ("snr_db", "cfo_hz", "fading_index", "noise_variance", "lts_phase_slope", "snr_linear", "corr_phase")
RX_INT = ("detected", "accepted", "sync_start", "frame_start", "delta", "candidates", "burst_interleaved")
MC_FIELDS = ("detected", "accepted", "sync_start", "frame_start", "cfo_hz", "fading_index", "delta", "modulation", "candidates", "success",
             "codewords_ok", "codewords_failed", "frame_type", "header_total_cw", "frame_bytes", "n_llr")


def _restate_lts(job):
    """worker: tests/acquire_restatement.py on one window with its own parameters, on the oracle (never touches the GPU)"""
    from acquire_restatement import acquire_window
    x, cfo, thr = job
    if "o" not in _checker:
        _checker["o"] = po.Oracle()
    with np.errstate(all="ignore"):
        r = acquire_window(_checker["o"], po.QAM16, po.R1_2, _padded(x, LTS_PAD), len(x), cfo, thr, 0.0, 0, retry=False)
    r["aux"] = None if r["aux"] is None else {f: np.float32(getattr(r["aux"], f)) for f in RX_AUX}
    return r


def _same(a, b):
    return S.same_bits(np.float32(a).reshape(1), np.float32(b).reshape(1))


def _lts_record_differences(e, F, idx, L, got):
    """ria_gpu_rx_acquire_batch's whole record of every window against the restatement: the ria_acq_result fields, the bytes,
    the decode status, and the demodulator's status of the reported candidate"""
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    info, st, res, fst = got
    info, st, fst = info.cpu().numpy(), e.decode_status(st), e.frame_status(fst)
    with ProcessPoolExecutor(8, mp_context=mp.get_context("spawn")) as pool:
        exp = list(pool.map(_restate_lts, [(F["x"][i], float(F["p"][i]), float(F["thr"][i])) for i in idx]))
    bad = []
    for k, r in enumerate(exp):
        msg = [f"{f} {int(res[f][k])} restated {int(r[f])}" for f in RX_INT if int(res[f][k]) != int(r[f])]
        msg += [f"{f} {res[f][k]!r} restated {r[f]!r}" for f in ("correlation", "cfo_hz") if not _same(res[f][k], r[f])]
        if not np.array_equal(info[k], r["info"]):
            msg.append("bytes")
        msg += [f"{f} {st[f][k]} restated {r[f]}" for f in ("cw_ok", "iterations", "attempts") if not np.array_equal(st[f][k], r[f])]
        if not r["accepted"]:
            if st[k].tobytes().strip(b"\0") or fst[k].tobytes().strip(b"\0"):
                msg.append("statuses of a window that is not accepted are not zero")
        else:
            msg += [f"demod {f} {fst[f][k]!r} restated {r['aux'][f]!r}" for f in RX_AUX[1:] if not _same(fst[f][k], r["aux"][f])]
            if not np.isclose(fst["snr_db"][k], r["aux"]["snr_db"], rtol=1e-5, atol=1e-5, equal_nan=True):   # display value
                msg.append(f"demod snr_db {fst['snr_db'][k]!r} restated {r['aux']['snr_db']!r}")
        if msg:
            bad.append(f"lts length {L} buffer {idx[k]} ({F['labels'][idx[k]]}): " + "; ".join(msg))
    return bad


def _mc_record_differences(det, F, idx, L, got):
    """ria_gpu_mcdpsk_acquire_batch's whole record against tests/mcdpsk_acquire_restatement.py: every ria_mcdpsk_acq_result
    field, the frame bytes and the reported soft bits"""
    from mcdpsk_acquire_restatement import acquire_window
    frames, res, llr = got
    frames, llr = frames.cpu().numpy(), llr.cpu().numpy()
    if "o" not in _checker:
        _checker["o"] = po.Oracle()
    bad = []
    for k, i in enumerate(idx):
        with np.errstate(all="ignore"):
            r = acquire_window(_checker["o"], _padded(F["x"][i], MC_PAD), L, 1, 10, 1, 1, det == "chirp", None,
                               float(F["p"][i]) if det == "zc" else 0.0, float(F["thr"][i]), 0.0, False)
        msg = []
        for f in MC_FIELDS + ("correlation",):
            same = _same(res[f][k], r[f]) if isinstance(r[f], np.float32) else int(res[f][k]) == int(r[f])
            if not same:
                msg.append(f"{f} {res[f][k]!r} restated {r[f]!r}")
        nb, nl = r["frame_bytes"], r["n_llr"]
        if not (np.array_equal(frames[k, :nb], r["frame"]) and not frames[k, nb:].any()):
            msg.append("frame bytes")
        if not (S.same_bits(llr[k, :nl], np.asarray(r["llr"], np.float32)) and not llr[k, nl:].any()):
            msg.append("soft bits")
        if msg:
            bad.append(f"{det} length {L} buffer {i} ({F['labels'][i]}): " + "; ".join(msg))
    return bad


@pytest.mark.parametrize("fam", ("level", "nonfinite", "threshold"))
@pytest.mark.parametrize("det", ("zc", "chirp", "lts"))
def test_acquire_batches_equal_the_separate_calls_and_the_restatements(golden, oracle, det, fam):
    """The composed paths run the same kernels with a threshold and a known CFO per buffer, read from their parameter
    records (threshold_dev / param_stride): LTS buffers through ria_gpu_rx_acquire_batch, ZC (the families rebuilt around
    root 5, since mc_dpsk_waveform.cpp searches the DATA and CONTROL roots only) and chirp buffers through ria_gpu_mcdpsk_acquire_batch, each buffer followed by silence so
    that a frame fits behind every detection, min_confidence 0 (a NaN correlation then meets `corr < min_confidence`), no
    timing retries.  The detection fields must be those of the separate call, and the whole record (accepted, frame_start,
    cfo_hz, delta, candidates, bytes, decode and demodulator status, soft bits) that of tests/acquire_restatement.py and
    tests/mcdpsk_acquire_restatement.py on the oracle.  Schmidl-Cox has no composed path."""
    import torch
    from ria_amd.engine import RxEngine
    F = _with_mask(S.zc_family_for_root(oracle, fam, 2), 12) if det == "zc" else S.family(oracle, det, fam)
    sep = run(det, F)
    key = ("QAM16", "R1_2") if det == "lts" else ("DBPSK", "R1_4")
    if key not in _engines:
        _engines[key] = RxEngine(*key)
    e = _engines[key]
    bad = []
    for L in sorted({len(x) for x in F["x"]}):
        idx = [i for i, x in enumerate(F["x"]) if len(x) == L]
        w = torch.from_numpy(np.stack([_padded(F["x"][i], LTS_PAD if det == "lts" else MC_PAD) for i in idx])).cuda()
        if det == "lts":
            got = e.rx_acquire(w, L, known_cfo=F["p"][idx], detect_threshold=F["thr"][idx], min_confidence=0.0, retry=False,
                               want_demod_status=True)
            acq = got[2]
        else:
            got = e.mcdpsk_acquire(w, L, 1, sync=det, known_cfo=F["p"][idx] if det == "zc" else None, detect_threshold=F["thr"][idx],
                                   min_confidence=0.0, retry=False, want_llr=True)
            acq = got[1]
        torch.cuda.synchronize()
        for k, i in enumerate(idx):
            s = sep[i]
            if det == "zc":
                exp = (s[0], s[2], s[3])
            elif det == "chirp":   # mc_dpsk_waveform.cpp: start behind the down chirp and its gap, confidence = std::max(up, down)
                exp = (s[0], s[2] + 28800 if s[0] else -1, s[5] if s[4] < s[5] else s[4])
            else:
                exp = (s[0], s[1] if s[0] else -1, s[2])
            g = (acq["detected"][k], acq["sync_start"][k], acq["correlation"][k])
            ok = g[0] == exp[0] and g[1] == exp[1] and _same(g[2], exp[2]) and (det != "lts" or acq["burst_interleaved"][k] == s[3])
            if not ok:
                bad.append(f"{det} {fam} buffer {i} ({F['labels'][i]}): acquire batch {g} separate call {exp}")
        bad += _lts_record_differences(e, F, idx, L, got) if det == "lts" else _mc_record_differences(det, F, idx, L, got)
    for b in bad:
        print(b)
    assert not bad, f"{len(bad)} buffers differ, first: {bad[0]}"
