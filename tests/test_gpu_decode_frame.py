"""GPU tests of ria_gpu_decode_frame_batch / ria_gpu_decode_frame_host / ria_host::decodeFrame: the OFDM branch of
StreamingDecoder::decodeFrame over the pinned rows of tests/decode_frame_inputs.py, every output against the CPU restatement
(tests/decode_frame_restatement.py) on the oracle, and on the compiled reference where it is built."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import pyoracle as po
import decode_frame_inputs as I
import decode_frame_restatement as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = [b[0] for b in I.batches()]
_engines = {}


def engine(mode, **kw):
    from ria_amd.engine import RxEngine
    key = (mode, tuple(sorted(kw.items())))
    if key not in _engines:
        mod, rate = mode.split("_", 1)
        _engines[key] = RxEngine(mod, rate, device=0, **kw)
    return _engines[key]


def batch(label):
    return next(b for b in I.batches() if b[0] == label)


def call_flags(ch, flags):
    from ria_amd import capi
    return flags | (0 if ch else capi.DECODE_NO_CHANNEL_DEINTERLEAVE)


def run(e, rows, n_llr, flags):
    """-> dict(result, frame, status, info) on the host"""
    frames, res, st, info = e.decode_frame(torch.from_numpy(np.ascontiguousarray(rows)).cuda(), n_llr, flags, want_info=True)
    torch.cuda.synchronize()
    return dict(result=res.copy(), frame=frames.cpu().numpy(), status=e.decode_status(st).copy(), info=info.cpu().numpy())


def check_rows(got, exp, bpc, who, ref=False):
    """every output of the rows in `got` against the restatement results `exp` (ref: the compiled reference's, which gives
    neither iterations nor attempts and zeroes the bytes of failed codewords)"""
    for i, r in enumerate(exp):
        g = got["result"][i]
        for k in R.RESULT_FIELDS:
            assert int(g[k]) == int(r[k]), (who, i, k, int(g[k]), r[k], R.PATH_NAMES[r["path"]])
        assert int(g["reserved0"]) == 0 and not g["reserved1"].any() and not g["reserved"].any(), (who, i)
        fr = got["frame"][i]
        assert np.array_equal(fr[:len(r["frame"])], r["frame"]) and not fr[len(r["frame"]):].any(), (who, i, "frame bytes")
        s, info = got["status"][i], got["info"][i]
        if not r["fixed_ran"]:
            assert not info.any() and all(not np.asarray(s[k]).any() for k in s.dtype.names), (who, i, "fixed outputs must be zero")
            continue
        assert np.array_equal(s["cw_ok"], r["fixed_ok"]), (who, i, "cw_ok")
        keep = np.repeat(r["fixed_ok"] != 0, bpc) if ref else np.ones(4 * bpc, bool)
        assert np.array_equal(info[keep], r["fixed_info"][keep]), (who, i, "info bytes")
        if not ref:
            assert np.array_equal(s["iterations"], r["fixed_iters"]) and np.array_equal(s["attempts"], r["fixed_attempts"]), (who, i)
            assert int(s["frame_valid"]) == r["fixed_valid"] and int(s["needs_recovery"]) == r["fixed_needs_recovery"], (who, i)
            assert not s["reserved"].any(), (who, i)


@pytest.mark.parametrize("label", LABELS)
def test_pinned_rows_in_one_call_equal_the_restatement(oracle, label):
    _, mode, ch, flags, recipes = batch(label)
    e = engine(mode)
    rows, n_llr, exp = I.expected("oracle", oracle, label)
    got = run(e, rows, n_llr, call_flags(ch, flags))
    check_rows(got, exp, e.geo.bytes_per_codeword, label)
    for rec, g in zip(recipes, got["result"]):
        assert R.PATH_NAMES[g["path"]] == rec[-1], (label, rec[0])
    if po.Ref.available() and flags == 7:
        check_rows(got, I.expected("ref", po.Ref(), label)[2], e.geo.bytes_per_codeword, label + "/ref", ref=True)
    assert e.lib.ria_gpu_debug_queue_fault(e.h) == 0


@pytest.fixture(scope="module")
def adaptor_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dframe") / "decode_frame_host_test")
    lib = os.path.join(ROOT, "ria_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "helpers", "decode_frame_host_test.cpp"),
                           "-L" + lib, "-lria_gpu", "-Wl,-rpath," + lib])
    return exe


@pytest.mark.parametrize("label", [b[0] for b in I.batches() if b[3] == 7])
def test_host_form_and_adaptor_row_by_row_equal_the_batch(oracle, adaptor_exe, tmp_path, label):
    from ria_amd import capi
    _, mode, ch, flags, _ = batch(label)
    e = engine(mode)
    bpc = e.geo.bytes_per_codeword
    rows, n_llr, _ = I.expected("oracle", oracle, label)
    got = run(e, rows, n_llr, call_flags(ch, flags))
    cap = got["frame"].shape[1]
    for i in range(len(rows)):
        n = min(int(n_llr[i]), I.STRIDE)
        soft = np.ascontiguousarray(rows[i, :n])
        need = max(4, n // 648) * bpc
        out = np.zeros(need, np.uint8)
        res, st = capi.DframeResult(), capi.DecodeStatus()
        rc = e.lib.ria_gpu_decode_frame_host(e.h, soft.ctypes.data_as(C.c_void_p), n, call_flags(ch, flags), out.ctypes.data_as(C.c_void_p),
                                             need, C.byref(res), C.byref(st))
        assert rc == 0, (label, i, e.lib.ria_gpu_last_error(e.h))
        assert bytes(res) == got["result"][i].tobytes(), (label, i)
        assert bytes(st) == got["status"][i].tobytes(), (label, i)
        assert np.array_equal(out, got["frame"][i, :need]) and not got["frame"][i, need:].any(), (label, i)
    fr, fn, fo = str(tmp_path / "rows.f32"), str(tmp_path / "n.i32"), str(tmp_path / "out.bin")
    rows.tofile(fr)
    n_llr.tofile(fn)
    mod, rate = I.MODES[mode]
    assert int(subprocess.check_output([adaptor_exe, str(mod), str(rate), str(int(ch)), fr, str(I.STRIDE), fn, fo]).decode()) == len(rows)
    rec = np.fromfile(fo, np.dtype([("detail", "u1", 32), ("head", "<i4", 5), ("frame", "u1", cap)]))
    for i, a in enumerate(rec):
        g = got["result"][i]
        assert a["detail"].tobytes() == g.tobytes(), (label, i)
        assert list(a["head"]) == [g["success"], g["codewords_ok"], g["codewords_failed"], g["frame_type"], g["frame_bytes"]], (label, i)
        assert np.array_equal(a["frame"], got["frame"][i]), (label, i)


def test_3000_tiled_rows_across_scan_chunks_and_workspace_growth(oracle):
    """3000 rows: more than two 1024-thread scan chunks and not a multiple, on an engine whose workspaces start at 64 frames:
    row for row the expectation of the distinct row, the same again on a second call, and - for the FIXED rows - the bytes and
    status ria_gpu_decode_batch gives for the same soft bits."""
    label = "QAM16_R1_2"
    rows, n_llr, exp = I.expected("oracle", oracle, label)
    e = engine(label, max_batch=64)
    idx = np.random.default_rng(2024).integers(0, len(rows), 3000)
    big, big_n = rows[idx], n_llr[idx]
    a = run(e, big, big_n, 7)
    check_rows(a, [exp[i] for i in idx], e.geo.bytes_per_codeword, "tiled")
    b = run(e, big, big_n, 7)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    fixed = np.flatnonzero(a["result"]["path"] == R.FIXED)
    assert len(fixed) > 100
    info, st = e.decode(torch.from_numpy(np.ascontiguousarray(big[fixed, :2592])).cuda(), flags=7)
    torch.cuda.synchronize()
    assert np.array_equal(info.cpu().numpy(), a["info"][fixed]) and e.decode_status(st).tobytes() == a["status"][fixed].tobytes()
    assert e.lib.ria_gpu_debug_queue_fault(e.h) == 0


def test_empty_batch_batches_without_a_stage_and_bad_arguments(oracle):
    from ria_amd import capi
    label = "QAM16_R1_2"
    rows, n_llr, exp = I.expected("oracle", oracle, label)
    names = [r[0] for r in batch(label)[4]]
    e = engine(label)
    bpc = e.geo.bytes_per_codeword
    frames, res, st = e.decode_frame(torch.zeros((0, I.STRIDE), dtype=torch.float32, device="cuda"))
    assert frames.shape == (0, 6 * bpc) and len(res) == 0
    for pick in (["ack14_648", "ack14_long", "ack14_over"], ["fixed_clean", "fixed_retry"], ["legacy2", "partial", "none_0"]):
        sel = np.array([names.index(p) for p in pick] * 3)
        check_rows(run(e, rows[sel], n_llr[sel], 7), [exp[i] for i in sel], bpc, str(pick))
    # n_llr NULL: every row holds llr_stride soft bits
    sel = np.array([names.index("ack14_long"), names.index("fixed_clean")])
    got = run(e, rows[sel, :2592], None, 7)
    assert [R.PATH_NAMES[p] for p in got["result"]["path"]] == ["CONTROL_R14", "FIXED"]
    x = torch.zeros((2, I.STRIDE), dtype=torch.float32, device="cuda")
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p, q, xp = C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + 2048), C.c_void_p(x.data_ptr())
    f = e.lib.ria_gpu_decode_frame_batch
    ok = dict(stride=I.STRIDE, n=2, flags=7, row=6 * bpc)
    for bad in (dict(stride=647), dict(stride=33 * 648), dict(row=6 * bpc - 1), dict(flags=capi.RX_DEMOD_ONLY), dict(flags=8), dict(n=-1)):
        a = dict(ok, **bad)
        assert f(e.h, xp, a["stride"], None, a["n"], a["flags"], p, a["row"], q, None, None, None) == -1, bad
    assert f(e.h, None, ok["stride"], None, 2, 7, p, ok["row"], q, None, None, None) == -1
    assert f(e.h, xp, 648, None, 2, 7, p, 4 * bpc, q, None, None, None) == 0       # the smallest row: 648 soft bits, 4 codewords of bytes
    torch.cuda.synchronize()
    assert e.lib.ria_gpu_debug_queue_fault(e.h) == 0
