"""GPU tests of ria_gpu_mcdpsk_acquire_batch: every ria_mcdpsk_acq_result field, the frame bytes and the reported soft bits
bit-equal to the CPU restatement of StreamingDecoder's MC-DPSK path (tests/mcdpsk_acquire_restatement.py) on pinned
windows built by the oracle."""
import numpy as np
import pytest
import torch

import pyoracle as po
from mcdpsk_acquire_restatement import (ACK, CONNECT, acquire_window, control_frame, data_frame, decode_mcdpsk_frame,
                                        encode_frame, frame_len, oracle, window)

pytestmark = pytest.mark.gpu

FIELDS = ("detected", "accepted", "sync_start", "frame_start", "cfo_hz", "fading_index", "delta", "modulation", "candidates",
          "success", "codewords_ok", "codewords_failed", "frame_type", "header_total_cw", "frame_bytes", "n_llr")


@pytest.fixture(scope="module")
def eng():
    from ria_amd.engine import RxEngine
    e = RxEngine("DQPSK", "R1_4", max_batch=64)
    yield e
    e.close()


def geometry(chirp, frame_cw, carriers=10, bps=1, spreading=1, lead=2000, tail=2000):
    pre = 57600 if chirp else 2512
    fl = frame_len(frame_cw, carriers, bps, spreading)
    return lead + pre + 8 * 512, lead + pre + fl + tail


def build(spec, chirp, frame_cw, carriers=10, bps=1, spreading=1, tail=2000):
    """spec: list of (coded bytes or None, tx modulation bps, channel kind, snr, seed[, shift of the frame behind the
    preamble]) -> (windows float32 [n, L], search_len)"""
    O = oracle()
    search_len, wl = geometry(chirp, frame_cw, carriers, bps, spreading, tail=tail)
    xs = [window(O, sp[0], carriers, po.DBPSK if sp[1] == 1 else po.DQPSK, spreading, chirp, 2000, wl, sp[2], sp[3], sp[4],
                 shift=sp[5] if len(sp) > 5 else 0) for sp in spec]
    return np.stack(xs), search_len


def run(eng, x, search_len, frame_cw, **kw):
    w = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(eng.device)
    frames, res, llr = eng.mcdpsk_acquire(w, search_len, frame_cw, want_llr=True, **kw)
    torch.cuda.synchronize()
    return frames.cpu().numpy(), res, llr.cpu().numpy()


def compare(eng, x, search_len, frame_cw, idx=None, carriers=10, bps=1, spreading=1, sync="chirp", disconnected=None,
            known_cfo=0.0, min_confidence=None, retry=True):
    chirp = sync == "chirp"
    if min_confidence is None:
        min_confidence = 0.0 if chirp else 0.25
    frames, res, llr = run(eng, x, search_len, frame_cw, carriers=carriers, modulation="DQPSK" if bps == 2 else "DBPSK",
                           spreading=spreading, sync=sync, disconnected=disconnected, known_cfo=known_cfo,
                           min_confidence=min_confidence, retry=retry)
    out = []
    for i in (range(len(x)) if idx is None else idx):
        r = acquire_window(oracle(), x[i], search_len, frame_cw, carriers, bps, spreading, chirp, disconnected, known_cfo,
                           None, min_confidence, retry)
        for f in FIELDS:
            got, want = res[f][i], r[f]
            if isinstance(want, np.float32):
                assert np.float32(got).view(np.uint32) == want.view(np.uint32), (i, f, got, want)
            else:
                assert int(got) == int(want), (i, f, got, want)
        assert np.float32(res["correlation"][i]).view(np.uint32) == r["correlation"].view(np.uint32), i
        nb, nl = r["frame_bytes"], r["n_llr"]
        assert np.array_equal(frames[i, :nb], r["frame"]) and not frames[i, nb:].any(), i
        assert np.array_equal(llr[i, :nl].view(np.uint32), np.asarray(r["llr"], np.float32).view(np.uint32)), i
        assert not llr[i, nl:].any(), i
        out.append(r)
    return res, out


def handshake_set():
    """disconnected chirp windows, primary DBPSK, frame_cw 3"""
    connect = encode_frame(data_frame(CONNECT, 7, np.arange(25, dtype=np.uint8)))
    salvage = encode_frame(data_frame(CONNECT, 8, np.arange(25, dtype=np.uint8), total_cw=4))
    bad = encode_frame(data_frame(CONNECT, 9, np.arange(25, dtype=np.uint8), total_cw=2))
    ack = encode_frame(control_frame(ACK, 10))
    spec = [(connect, 1, 0, 10.0, 1), (None, 1, 0, 10.0, 2), (salvage, 1, 0, 10.0, 3), (bad, 1, 0, 10.0, 4),
            (connect, 2, 0, 12.0, 5), (ack, 1, 2, 6.0, 6)]
    spec += [(connect, 1, 2, snr, 100 + s) for s, snr in enumerate((-4.0, -3.0, -2.0, -1.0, -4.0, -3.0, -2.0, -1.0))]
    return spec


def test_handshake_set_matches_the_restatement(eng):
    x, sl = build(handshake_set(), True, 3)
    res, rs = compare(eng, x, sl, 3)
    assert rs[0]["success"] == 1 and rs[0]["delta"] == 0 and rs[0]["frame_type"] == CONNECT and rs[0]["candidates"] == 1
    assert rs[1]["detected"] == 0 and rs[1]["candidates"] == 0
    assert rs[2]["header_total_cw"] == 4 and rs[2]["codewords_ok"] == 1 and rs[2]["frame_bytes"] == 20 and rs[2]["success"] == 0
    assert rs[3]["codewords_ok"] == 0 and rs[3]["candidates"] == 26 and rs[3]["success"] == 0 and rs[3]["delta"] == 0
    assert rs[4]["success"] == 1 and rs[4]["modulation"] == po.DQPSK and rs[4]["delta"] == 0 and rs[4]["candidates"] == 2
    assert rs[5]["success"] == 1 and rs[5]["header_total_cw"] == 1


def test_recovery_candidates_outside_the_window_are_skipped(eng):
    bad = encode_frame(data_frame(CONNECT, 9, np.arange(25, dtype=np.uint8), total_cw=2))
    x, sl = build([(bad, 1, 0, 10.0, 4)], True, 3, tail=20)
    _, rs = compare(eng, x, sl, 3)
    assert rs[0]["accepted"] == 1 and 2 < rs[0]["candidates"] < 26


def test_connected_zc_and_rejection(eng):
    ack = encode_frame(control_frame(ACK, 11))
    x, sl = build([(ack, 1, 0, 10.0, 21), (ack, 1, 2, 8.0, 22), (None, 1, 0, 10.0, 23)], False, 1)
    _, rs = compare(eng, x, sl, 1, sync="zc", known_cfo=0.0)
    assert rs[0]["accepted"] == 1 and rs[0]["candidates"] == 1 and rs[2]["accepted"] == 0   # connected: no fallbacks
    _, rs = compare(eng, x, sl, 1, sync="zc", min_confidence=0.999)
    assert rs[0]["detected"] == 1 and rs[0]["accepted"] == 0 and rs[0]["candidates"] == 0
    _, rs = compare(eng, x, sl, 1, sync="zc", known_cfo=5.0)          # the connected CFO rule
    assert rs[0]["accepted"] == 1 and rs[0]["cfo_hz"] == np.float32(5.0)


class _GpuRobust:
    """robust_decode of the restatement's decodeMCDPSKFrame served by ria_gpu_ldpc_decode_robust_batch"""

    def __init__(self, eng):
        self.eng = eng

    def robust_decode(self, rate, llr):
        row = torch.from_numpy(np.ascontiguousarray(llr, np.float32).reshape(1, 648)).to(self.eng.device)
        o, ok, it, tr = self.eng.ldpc_decode_robust(row)
        return bool(ok.cpu().numpy()[0]), o.cpu().numpy()[0], int(it.cpu().numpy()[0]), int(tr.cpu().numpy()[0])


def test_no_retry_equals_the_separate_calls(eng):
    """NO_RETRY: sync_chirp + mcdpsk_demod + ldpc_decode_robust, with decodeMCDPSKFrame's header, CONNECT guard and
    reassembly on the host"""
    x, sl = build(handshake_set()[:6] + [(handshake_set()[0][0], 1, 0, 0.0, 7, 256)], True, 3)
    frames, res, llr = run(eng, x, sl, 3, retry=False)
    w = torch.from_numpy(x).to(eng.device)
    ch = eng.sync_chirp(w[:, :sl].contiguous(), 0.15)
    fl = frame_len(3, 10, 1, 1)
    host = _GpuRobust(eng)
    for i in range(len(x)):
        assert bool(ch["success"][i]) == bool(res["detected"][i])
        if not res["accepted"][i]:
            assert res["candidates"][i] == 0 and not frames[i].any()
            continue
        assert res["candidates"][i] == 1 and res["delta"][i] == 0
        s = int(ch["down_chirp_start"][i]) + 28800
        assert res["sync_start"][i] == s and res["frame_start"][i] == s
        cfo = torch.tensor([float(ch["cfo_hz"][i])], dtype=torch.float32, device=eng.device)
        l, st = eng.mcdpsk_demod(w[i:i + 1, s:s + fl].contiguous(), 10, 1, 1, cfo_hz=cfo)
        n = int(st["n_llr"][0])
        assert res["n_llr"][i] == n and np.float32(res["fading_index"][i]) == np.float32(st["fading_index"][0])
        soft = l.cpu().numpy()[0, :n]
        assert np.array_equal(soft.view(np.uint32), llr[i, :n].view(np.uint32))
        d = decode_mcdpsk_frame(host, soft)
        for f in ("success", "codewords_ok", "codewords_failed", "frame_type", "header_total_cw"):
            assert int(res[f][i]) == int(d[f]), (i, f)
        assert res["frame_bytes"][i] == len(d["frame"]) and np.array_equal(frames[i, :len(d["frame"])], d["frame"])
        assert not frames[i, len(d["frame"]):].any()
    # the window whose frame sits 256 samples late fails at its primary and is not retried
    assert res["success"][-1] == 0 and res["candidates"][-1] == 1


def test_results_do_not_depend_on_batching_or_order(eng):
    x, sl = build(handshake_set(), True, 3)
    frames, res, llr = run(eng, x, sl, 3)
    perm = np.random.default_rng(3).permutation(len(x))
    f2, r2, l2 = run(eng, x[perm], sl, 3)
    assert np.array_equal(r2.view(np.uint8).reshape(len(x), -1), res[perm].view(np.uint8).reshape(len(x), -1))
    assert np.array_equal(f2, frames[perm]) and np.array_equal(l2.view(np.uint32), llr[perm].view(np.uint32))
    for a, b in ((0, 5), (5, 11), (11, len(x))):
        f3, r3, l3 = run(eng, x[a:b], sl, 3)
        assert np.array_equal(r3.view(np.uint8).reshape(b - a, -1), res[a:b].view(np.uint8).reshape(b - a, -1))
        assert np.array_equal(f3, frames[a:b]) and np.array_equal(l3.view(np.uint32), llr[a:b].view(np.uint32))


def test_dqpsk_primary_and_spreading(eng):
    connect = encode_frame(data_frame(CONNECT, 12, np.arange(25, dtype=np.uint8)))
    x, sl = build([(connect, 2, 0, 12.0, 31), (connect, 1, 0, 12.0, 32), (connect, 2, 2, -1.0, 33)], True, 3, bps=2)
    _, rs = compare(eng, x, sl, 3, bps=2)
    assert rs[0]["success"] == 1 and rs[0]["modulation"] == po.DQPSK
    ack = encode_frame(control_frame(ACK, 13))
    for sp in (2, 4):
        x, sl = build([(ack, 1, 0, 6.0, 40 + sp), (ack, 1, 2, 0.0, 50 + sp)], True, 1, spreading=sp)
        _, rs = compare(eng, x, sl, 1, spreading=sp)
        assert rs[0]["success"] == 1


def test_large_disconnected_batch_at_0db(eng):
    connect = encode_frame(data_frame(CONNECT, 14, np.arange(25, dtype=np.uint8)))
    x, sl = build([(connect, 1, 0, 0.0, 1000 + s) for s in range(16)], True, 3)
    big = np.tile(x, (256, 1))
    w = torch.from_numpy(big).to(eng.device)
    del big
    frames, res = eng.mcdpsk_acquire(w, sl, 3)
    torch.cuda.synchronize()
    assert len(res) == 4096
    frames = frames.cpu().numpy()
    sample = list(range(0, 4096, 257))
    for i in sample:
        r = acquire_window(oracle(), x[i % 16], sl, 3)
        for f in FIELDS:
            want = r[f]
            got = res[f][i]
            assert (np.float32(got).view(np.uint32) == want.view(np.uint32)) if isinstance(want, np.float32) else int(got) == int(want), (i, f)
        assert np.array_equal(frames[i, :r["frame_bytes"]], r["frame"])
    # windows with the same samples give the same results wherever they sit in the batch
    ref = res[:16].view(np.uint8).reshape(16, -1)
    assert np.array_equal(res.view(np.uint8).reshape(4096, -1), np.tile(ref, (256, 1)))


# (tx bits per symbol, frame shift behind the preamble) -> (winning delta, winner modulation), AWGN 0 dB, seed 7, primary DBPSK
RECOVERIES = [((1, 240), (8, po.DBPSK)), ((1, 256), (16, po.DBPSK)), ((1, -256), (-24, po.DBPSK)), ((1, 288), (48, po.DBPSK)),
              ((1, -288), (-48, po.DBPSK)), ((1, 300), (64, po.DBPSK)), ((1, -300), (-64, po.DBPSK)),
              ((2, 160), (24, po.DQPSK)), ((2, -160), (-24, po.DQPSK)), ((2, 192), (48, po.DQPSK)), ((2, -192), (-64, po.DQPSK))]


def test_timing_recoveries_match_the_restatement(eng):
    """frames placed off the detected start: the primary and the alternate fail, the first delta x modulation that decodes
    the whole frame wins; every field, the frame and the winner's soft bits equal the restatement"""
    connect = encode_frame(data_frame(CONNECT, 7, np.arange(25, dtype=np.uint8)))
    x, sl = build([(connect, tb, 0, 0.0, 7, shift) for (tb, shift), _ in RECOVERIES], True, 3)
    res, rs = compare(eng, x, sl, 3)
    order = [(0, False), (0, True)] + [(d, a) for d in (8, -8, 16, -16, 24, -24, 32, -32, 48, -48, 64, -64) for a in (False, True)]
    for r, (_, (delta, mod)) in zip(rs, RECOVERIES):
        assert r["success"] == 1 and r["delta"] == delta and r["modulation"] == mod, (r["delta"], r["modulation"])
        assert r["frame_start"] == r["sync_start"] + delta and r["frame_bytes"] == 44
        assert r["candidates"] == order.index((delta, mod == po.DQPSK)) + 1
    assert len({d for _, (d, _m) in RECOVERIES}) >= 6


def test_argument_rejections_on_a_real_handle(eng):
    import ctypes as C
    from ria_amd import capi
    L = capi.load()
    w = torch.zeros((2, 200000), dtype=torch.float32, device=eng.device)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=eng.device)
    cfg = capi.McdpskConfig(10, 1, 1, 0)
    p = C.c_void_p(buf.data_ptr())
    ok = dict(cfg=cfg, stride=200000, sl=70000, wl=170000, n=2, cw=3, flags=capi.MACQ_SYNC_CHIRP | capi.MACQ_DISCONNECTED)

    def call(h, **kw):
        a = dict(ok, **kw)
        rc = L.ria_gpu_mcdpsk_acquire_batch(h, C.byref(a["cfg"]), C.c_void_p(w.data_ptr()), a["stride"], a["sl"], a["wl"], a["n"],
                                            a["cw"], p, a["flags"], p, p, None, 0, None)
        torch.cuda.synchronize()
        return rc
    for kw in (dict(flags=capi.MACQ_DISCONNECTED), dict(cw=0), dict(cw=9), dict(sl=180000), dict(wl=210000), dict(n=-1),
               dict(flags=0x100), dict(cfg=capi.McdpskConfig(10, 3, 1, 0)), dict(cfg=capi.McdpskConfig(10, 1, 3, 0))):
        assert call(eng.h, **kw) == -1, kw
    assert call(eng.h, flags=capi.MACQ_SYNC_CHIRP | capi.MACQ_CHANNEL_INTERLEAVE) == -4
    assert call(eng.h, cw=8, cfg=capi.McdpskConfig(3, 1, 4, 0)) == -4          # frame too long for the demodulator
    assert call(eng.h, n=0) == 0
    from ria_amd.engine import RxEngine
    e2 = RxEngine("DQPSK", "R1_2", max_batch=8)
    try:
        assert call(e2.h, n=0) == -1                                         # MC-DPSK is R1/4 only
    finally:
        e2.close()


def test_workspace_growth_leaves_results_alone():
    """A call on 2 windows, then one on the handshake set, on a fresh R1/4 handle: every array of the second equals the same
    call on another fresh handle that never ran the first, and the first equals that call's first two rows."""
    from ria_amd.engine import RxEngine
    x, sl = build(handshake_set(), True, 3)
    a, b = RxEngine("DQPSK", "R1_4", max_batch=64), RxEngine("DQPSK", "R1_4", max_batch=64)
    small = run(a, x[:2], sl, 3)
    big = run(a, x, sl, 3)
    ref = run(b, x, sl, 3)
    assert ref[1]["success"].sum() >= 3 and ref[1]["candidates"].max() > 2   # decodes and fallback rounds ran
    for k, (s, g, r) in enumerate(zip(small, big, ref)):
        assert g.tobytes() == r.tobytes(), k
        assert s.tobytes() == r[:2].tobytes(), k
    a.close()
    b.close()
