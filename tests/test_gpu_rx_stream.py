"""ria_amd.acquire.rx_stream on two small recordings: capture in, frames out, by library calls only (RxEngine.search, then
rx_window / mcdpsk_window on the windows the search names).  Every sent frame is delivered once, in order, with the bytes
sent, at increasing positions; the events do not depend on whether the streams run as one batch or one by one.  The window
calls have their own parity tests: nothing here is compared against a CPU restatement of them."""
import numpy as np
import pytest
import torch

import pyoracle as po
import control_inputs as CI
import control_restatement as CR
from mcdpsk_acquire_restatement import ACK, control_frame, encode_frame, oracle

pytestmark = pytest.mark.gpu
F = np.float32


def _norm(s):
    return (s * F(0.8 / np.abs(s).max())).astype(F)


def ofdm_recording(O, seed):
    """three DQPSK R1/4 data frames and one ACK: the first gaps are silence, the later ones the channel's noise (AWGN, 20 dB)"""
    sent, parts = [], [np.zeros(16000, F)]
    for seq in (11, 12, 13):
        payload = ((np.arange(4 * 20 - 24) * 3 + seq + seed) % 251).astype(np.uint8)
        s, info, _ = O.tx_frame(po.DQPSK, po.R1_4, payload, seq)
        assert not info[len(payload) + 19:].any()
        sent.append(bytes(info[:len(payload) + 19]))       # the v2 data frame: 17 header bytes, the payload, CRC16; the rest of the four codewords is padding
        parts += [_norm(s), np.zeros(12000, F)]
    parts += [CI.clean_samples(O, "ack", 14), np.zeros(80000, F)]
    sent.append(bytes(CR.control_frame(CR.ACK, 14)))
    x = np.concatenate(parts).astype(F)
    quiet = 16000 + len(parts[1]) + 12000                  # up to the second frame the recording is the clean signal in silence
    y = O.channel(0, 20.0, seed, x)
    y[:quiet] = x[:quiet]
    return np.ascontiguousarray(y, F), sent


def zc_recording(O, seed):
    """three one-codeword MC-DPSK frames behind ZC preambles, 15 dB"""
    sent, parts = [], [np.zeros(14000, F)]
    for seq in (21, 22, 23):
        f = control_frame(ACK, seq + seed % 5)
        sent.append(bytes(f))
        parts += [_norm(O.mcdpsk_wf_tx(10, po.DQPSK, po.R1_4, 1, True, encode_frame(f))), np.zeros(9000, F)]
    parts.append(np.zeros(40000, F))
    return np.ascontiguousarray(O.channel(0, 15.0, seed, np.concatenate(parts).astype(F)), F), sent


def _stack(recs, device):
    n = max(len(r) for r in recs)
    x = np.zeros((len(recs), n), F)
    for i, r in enumerate(recs):
        x[i, :len(r)] = r
    return torch.from_numpy(x).to(device), np.array([len(r) for r in recs])


def _check(events, sent):
    got = [e for e in events if e["frame"] is not None]
    assert len(got) == len(sent), [(e["position"], e["outcome"], e["frame"] is not None) for e in events]
    for e, s in zip(got, sent):
        assert e["frame"] == s, (e["position"], e["outcome"], len(e["frame"]), len(s))
    pos = [e["position"] for e in events]
    assert pos == sorted(pos) and len(set(pos)) == len(pos), pos


def test_ofdm_recordings():
    from ria_amd.acquire import rx_stream
    from ria_amd.engine import RxEngine
    O = oracle()
    data, ctrl = RxEngine("DQPSK", "R1_4", max_batch=8), RxEngine("DQPSK", "R1_4", max_batch=8)
    recs = [ofdm_recording(O, 5), ofdm_recording(O, 6)]
    x, lens = _stack([r[0] for r in recs], data.device)
    both = rx_stream(data, x, lens, "OFDM_LTS", control_engine=ctrl)
    for ev, (_, sent) in zip(both, recs):
        _check(ev, sent)
    for i in range(2):
        one = rx_stream(data, x[i:i + 1].contiguous(), lens[i:i + 1], "OFDM_LTS", control_engine=ctrl)
        assert one[0] == both[i]
    data.close()
    ctrl.close()


def test_zc_recordings():
    from ria_amd.acquire import rx_stream
    from ria_amd.engine import RxEngine
    O = oracle()
    eng = RxEngine("DQPSK", "R1_4", max_batch=8)
    recs = [zc_recording(O, 7), zc_recording(O, 8)]
    x, lens = _stack([r[0] for r in recs], eng.device)
    kw = dict(feed_step=4800, carriers=10, modulation="DQPSK", spreading=1)     # fed as it arrives: no backlog, no catch-up
    both = rx_stream(eng, x, lens, "MCDPSK_ZC", **kw)
    for ev, (_, sent) in zip(both, recs):
        _check(ev, sent)
    for i in range(2):
        assert rx_stream(eng, x[i:i + 1].contiguous(), lens[i:i + 1], "MCDPSK_ZC", **kw)[0] == both[i]
    eng.close()
