"""RxEngine.rx_ring / rx_ring_host (ria_gpu_rx_ring_batch, ria_gpu_rx_ring_host) against the composition they replace,
ria_amd.acquire.rx_ring: the same events, the same final ria_ring_state bit for bit, the same close reasons and counters;
against ria_gpu_rx_stream_batch on recordings that never wrap; host form against batch form; max_events = 1 repeated against
one call; every output row written; SPAN_LOST; a window longer than the ring refused by the library.  Before anything is
compared with it, the composition is checked on its own:

ria_amd.acquire.rx_ring - the ring search (ria_gpu_search_ring_batch), windows cut from the capture by absolute index, the
existing window calls, the state rules modulo the ring - on recordings longer than the ring buffer, for OFDM, ZC and chirp.
Each recording holds noise-free frames placed by absolute index: one before the wrap, one whose samples straddle absolute
index 960 000, one behind it; a second recording holds a frame placed exactly one lap behind a delivered frame, at the same
ring index, which the reference's circular anti-replay rejects, and a third the same frame 300 samples later, which it does
not.  Every other placed frame must be delivered with its bytes.  On the short recordings of the stream tests rx_ring gives
rx_stream's events and (mapped) final state: before the wrap the two loops are the same loop."""
import numpy as np
import pytest
import torch

import pyoracle as po
import ring_inputs as RI
import ring_restatement as RR
import stream_restatement as SRS
from mcdpsk_acquire_restatement import ACK, control_frame, encode_frame, oracle
from test_gpu_rx_stream import _norm, _stack, ofdm_recording, zc_recording
from test_gpu_stream_call import MODES, handshake_recording

pytestmark = pytest.mark.gpu
F = np.float32
RING = RR.MAX_BUFFER_SAMPLES
CLOSED = {"NEED_SAMPLES": 2, "LIMIT": 3, "WINDOW_NEED_SAMPLES": 4, "EVENTS_FULL": 5}


@pytest.fixture(scope="module")
def rig():
    from ria_amd.engine import RxEngine
    data, ctrl = RxEngine("DQPSK", "R1_4", max_batch=8), RxEngine("DQPSK", "R1_4", max_batch=8)
    yield data, ctrl
    data.close()
    ctrl.close()


def frame_of(O, name, seq):
    """-> (samples at peak 0.8, the bytes a delivered event starts with)"""
    if name == "ofdm":
        payload = ((np.arange(4 * 20 - 24) * 3 + seq) % 251).astype(np.uint8)
        s, info, _ = O.tx_frame(po.DQPSK, po.R1_4, payload, seq)
        return _norm(s), bytes(info[:len(payload) + 19])
    f = control_frame(ACK, seq)
    zc = name == "zc"
    return _norm(O.mcdpsk_wf_tx(10, po.DQPSK if zc else po.DBPSK, po.R1_4, 1, zc, encode_frame(f))), bytes(f)


def recordings(O, name):
    """-> [(capture, [(absolute start, bytes or None = must not be delivered)])]: the three recordings of the module's docstring"""
    lead = {"ofdm": 10000, "zc": 3000, "chirp": 30000}[name]          # the straddling frame starts this far before absolute 960 000
    # from one frame's start to the next one's.  The disconnected chirp receiver decodes a handshake frame on a span of three
    # codewords (MIN_HANDSHAKE_CW), 104 448 samples behind the training that follows 57 600 samples of chirps: the next
    # frame has to start behind that
    gap = {"ofdm": 70000, "zc": 40000, "chirp": 180000}[name]
    tail = {"ofdm": 110000, "zc": 80000, "chirp": 175000}[name]       # behind the last frame's start: its window's samples
    third = RING + {"ofdm": 110000, "zc": 110000, "chirp": 150000}[name]
    frames = {seq: frame_of(O, name, seq) for seq in (31, 32, 33)}
    n = max(len(f[0]) for f in frames.values())
    assert lead < n and n + 2000 < gap and RING - lead + gap <= third

    def build(placed):
        x = np.zeros(placed[-1][0] + tail, F)
        for at, seq, _ in placed:
            s = frames[seq][0]
            x[at:at + len(s)] += s
        return x, [(at, frames[seq][1] if deliver else None) for at, seq, deliver in placed]
    a = build([(100000, 31, True), (RING - lead, 32, True), (third, 33, True)])
    b = build([(200000, 31, True), (RING + 200000, 32, False), (RING + 200000 + gap, 33, True)])
    c = build([(200000, 31, True), (RING + 200300, 32, True), (RING + 200300 + gap, 33, True)])
    return [a, b, c]


def show(events):
    return [(e["position"], e["search_start"], e["outcome"], None if e["frame"] is None else len(e["frame"])) for e in events]


@pytest.mark.parametrize("name", ["ofdm", "zc", "chirp"])
def test_frames_around_the_wrap(rig, name):
    from ria_amd.acquire import rx_ring
    data, ctrl = rig
    O = oracle()
    recs = recordings(O, name)
    x, lens = _stack([r[0] for r in recs], data.device)
    mode, kw = MODES[name]
    events, state, closed, counters = rx_ring(data, x, lens, mode, control_engine=ctrl if name == "ofdm" else None, feed_step=4800, **kw)
    near = 62000 if name == "chirp" else 3000      # chirp: the sync is the training, behind 57 600 samples of preamble
    for i, (_, placed) in enumerate(recs):
        got = [e for e in events[i] if e["frame"] is not None]
        want = [(at, sent) for at, sent in placed if sent is not None]
        assert len(got) == len(want), (name, i, show(events[i]))
        for e, (at, sent) in zip(got, want):
            assert e["frame"][:len(sent)] == sent and abs(e["position"] - at) < near, (name, i, show(events[i]))
            assert e["search_start"] <= e["position"] < e["search_start"] + 120000
        for at, sent in placed:
            if sent is None:                       # the lap-later frame: no event at all, it never left the search
                assert not [e for e in events[i] if abs(e["position"] - at) < near], (name, i, show(events[i]))
        assert closed[i] == "NEED_SAMPLES" and state["total_fed"][i] == lens[i]
    assert (state["total_fed"] > RING).all() and not counters[:, :3].any()
    # the straddling frame's window was cut across absolute 960 000
    straddle = [e for e in events[0] if e["frame"] is not None][1]
    assert straddle["search_start"] < RING < straddle["search_start"] + 120000


@pytest.mark.parametrize("name", ["ofdm", "zc", "chirp"])
def test_short_recordings_equal_rx_stream(rig, name):
    """captures that never wrap: rx_stream's events, its comparator's final state and close reasons"""
    from ria_amd.acquire import rx_ring, rx_stream
    data, ctrl = rig
    O = oracle()
    recs = {"ofdm": [ofdm_recording(O, 5), ofdm_recording(O, 6)], "zc": [zc_recording(O, 7), zc_recording(O, 8)], "chirp": [handshake_recording(O, 9)]}[name]
    x, lens = _stack([r[0] for r in recs], data.device)
    mode, kw = MODES[name]
    kw = dict(kw, control_engine=ctrl if name == "ofdm" else None)
    for fs in (0, 4800):
        want = rx_stream(data, x, lens, mode, feed_step=fs, **kw)
        _, want_state, want_closed = SRS.comparator(data, x, lens, mode, feed_step=fs, **kw)
        events, state, closed, counters = rx_ring(data, x, lens, mode, feed_step=fs, **kw)
        if (name, fs) != ("zc", 0):      # a ZC recording that "has all arrived" is a backlog: the catch-up jumps to its end (rx_stream's note)
            assert sum(len(e) for e in want) > 0
        assert [[{k: e[k] for k in ("position", "outcome", "frame")} for e in ev] for ev in events] == want, (name, fs)
        assert RR.to_search_state(state).tobytes() == np.ascontiguousarray(want_state).tobytes(), (name, fs)
        assert [CLOSED[c] for c in closed] == list(want_closed) and not counters.any()


def test_span_lost(rig):
    """a found sync whose span crossed the write position closes the stream: its window is no contiguous piece of the capture"""
    from ria_amd.acquire import rx_ring
    data, ctrl = rig
    O = oracle()
    row = next(r for r in RI.ROWS if r["name"] == "lts_span_wraps")
    cap, n, st, _, _ = RI.row_args(O, row)
    x = torch.from_numpy(cap[None, :]).to(data.device)
    events, state, closed, _ = rx_ring(data, x, [n], "OFDM_LTS", control_engine=ctrl, feed_step=0, state=np.array([st]))
    assert closed == ["SPAN_LOST"] and events == [[]]
    e_res, e_st = RI.expected(O, row)
    assert e_res["span_wraps"] == 1 and e_res["outcome"] == RR.SYNC_FOUND and state[0].tobytes() == e_st.tobytes()


def test_window_longer_than_the_ring_is_refused(rig):
    """full > 959 999: RIA_ERR_INVALID from the library (both forms), a ValueError from the composition"""
    from ria_amd import capi
    from ria_amd.acquire import rx_ring
    data, _ = rig
    x = torch.zeros((1, 1000), dtype=torch.float32, device=data.device)
    with pytest.raises(ValueError):
        rx_ring(data, x, [1000], "MCDPSK_ZC", carriers=1, modulation="DBPSK", spreading=4)
    with pytest.raises(capi.RiaError):
        data.rx_ring(x, [1000], "MCDPSK_ZC", carriers=1, modulation="DBPSK", spreading=4)
    with pytest.raises(capi.RiaError):
        data.rx_ring_host(np.zeros(1000, F), "MCDPSK_ZC", carriers=1, modulation="DBPSK", spreading=4)
    assert data.lib.ria_gpu_rx_ring_batch(None, None, 0, 0, None, None, 0, None, 0, None, 0, 1, 1, None, None, 0, None, None) == -1
    assert data.lib.ria_gpu_rx_ring_host(None, None, 0, 0, None, None, 0, None, 0, 1, 1, None, None, 0, None) == -1


# ---- the calls against the composition
RING_CLOSED = {"NEED_SAMPLES": 2, "LIMIT": 3, "WINDOW_NEED_SAMPLES": 4, "EVENTS_FULL": 5, "SPAN_LOST": 7}
COUNTERS = ("overflows", "overflow_dropped", "drift_snaps", "cursor_inits")


def call_events(data, mode, res, ev, frames):
    """the call's records in the composition's form"""
    from ria_amd import capi
    if isinstance(frames, torch.Tensor):
        frames = frames.cpu().numpy()
    ofdm = capi.SEARCH_MODE[mode] == capi.SEARCH_MODE["OFDM_LTS"]
    names = {v: k for k, v in (capi.WIN_OUTCOME if ofdm else capi.MWIN_OUTCOME).items()}
    return [[dict(position=int(e["sync_position"]), search_start=int(e["search_start"]), outcome=names[int(e["outcome"])],
                  frame=frames[s, k, :int(e["frame_bytes"])].tobytes() if e["delivered"] else None)
             for k, e in enumerate(ev[s, :int(res["n_events"][s])])] for s in range(len(res))]


def same_as_composition(data, mode, got, want, where):
    st, res, ev, frames = got
    events, state, closed, counters = want
    assert call_events(data, mode, res, ev, frames) == events, where
    assert st.tobytes() == np.ascontiguousarray(state).tobytes(), (where, st, state)
    assert list(res["closed"]) == [RING_CLOSED[c] for c in closed] and list(res["n_events"]) == [len(e) for e in events], where
    assert np.array_equal(np.stack([res[k].astype(np.int64) for k in COUNTERS], axis=1), counters), where


def unwritten(got):
    """every output row written: the result records, the event rows (cleared behind n_events) and the payload rows"""
    st, res, ev, frames = got
    frames = frames.cpu().numpy() if isinstance(frames, torch.Tensor) else frames
    assert (res["search_legs"] >= 1).all() and (res["reserved"] == 0).all() and (res["reserved1"] == 0).all()
    for s in range(len(res)):
        k = int(res["n_events"][s])
        assert not ev[s, k:].view(np.uint8).any() and not frames[s, k:].any()
        for j in range(k):
            nb = int(ev[s, j]["frame_bytes"]) if ev[s, j]["delivered"] else 0
            assert not frames[s, j, nb:].any()


@pytest.fixture(scope="module")
def long_recs():
    O = oracle()
    return {name: recordings(O, name) for name in ("ofdm", "zc", "chirp")}


@pytest.mark.parametrize("name", ["ofdm", "zc", "chirp"])
def test_call_equals_composition(rig, long_recs, name):
    """the recordings of test_frames_around_the_wrap, as one batch and one by one; then the host form on each"""
    from ria_amd.acquire import rx_ring
    data, ctrl = rig
    recs = long_recs[name]
    x, lens = _stack([r[0] for r in recs], data.device)
    mode, kw = MODES[name]
    kw = dict(kw, control_engine=ctrl if name == "ofdm" else None)
    want = rx_ring(data, x, lens, mode, feed_step=4800, **kw)
    assert sum(len([e for e in ev if e["frame"] is not None]) for ev in want[0]) == 8      # 3 + 2 + 3 delivered: not vacuous
    got = data.rx_ring(x, lens, mode, feed_step=4800, **kw)
    same_as_composition(data, mode, got, want, name)
    unwritten(got)
    for i in range(len(recs)):
        one = data.rx_ring(x[i:i + 1, :lens[i]].contiguous(), lens[i:i + 1], mode, feed_step=4800, **kw)
        same_as_composition(data, mode, one, ([want[0][i]], want[1][i:i + 1], [want[2][i]], want[3][i:i + 1]), (name, i))
        host = data.rx_ring_host(recs[i][0], mode, feed_step=4800, **kw)          # 1.2 - 1.5 M samples: five or six pieces of the pinned block
        assert host[0].tobytes() == one[0].tobytes() and host[1].tobytes() == one[1].tobytes() and host[2].tobytes() == one[2].tobytes()
        assert np.array_equal(host[3], one[3].cpu().numpy()), (name, i)


@pytest.mark.parametrize("name", ["ofdm", "zc", "chirp"])
def test_one_event_per_call_repeated(rig, long_recs, name):
    """max_events = 1 per call, the state handed on: the events and the final state of one call"""
    data, ctrl = rig
    rec = long_recs[name][0][0]
    x = torch.from_numpy(rec[None, :]).to(data.device)
    mode, kw = MODES[name]
    kw = dict(kw, control_engine=ctrl if name == "ofdm" else None)
    st_w, res_w, ev_w, fr_w = data.rx_ring(x, [len(rec)], mode, feed_step=4800, **kw)
    want = call_events(data, mode, res_w, ev_w, fr_w)[0]
    assert len(want) >= 3
    got, st = [], None
    for _ in range(len(want) + 2):
        st, res, ev, fr = data.rx_ring(x, [len(rec)], mode, state=st, feed_step=4800, max_events=1, **kw)
        got += call_events(data, mode, res, ev, fr)[0]
        if res["closed"][0] != RING_CLOSED["EVENTS_FULL"]:
            break
    assert got == want and st.tobytes() == st_w.tobytes() and res["closed"][0] == res_w["closed"][0]


@pytest.mark.parametrize("name", ["ofdm", "zc", "chirp"])
def test_short_recordings_equal_the_stream_call(rig, name):
    """recordings that never wrap: ria_gpu_rx_stream_batch's events and (mapped) final state"""
    from ria_amd.acquire import stream_events
    data, ctrl = rig
    O = oracle()
    recs = {"ofdm": [ofdm_recording(O, 5), ofdm_recording(O, 6)], "zc": [zc_recording(O, 7), zc_recording(O, 8)], "chirp": [handshake_recording(O, 9)]}[name]
    x, lens = _stack([r[0] for r in recs], data.device)
    mode, kw = MODES[name]
    kw = dict(kw, control_engine=ctrl if name == "ofdm" else None)
    for fs in (0, 4800):
        st_o, res_o, ev_o, fr_o = data.rx_stream(x, lens, mode, feed_step=fs, **kw)
        st, res, ev, fr = data.rx_ring(x, lens, mode, feed_step=fs, **kw)
        assert stream_events(res, ev, fr) == stream_events(res_o, ev_o, fr_o), (name, fs)
        assert ev.tobytes() == ev_o.tobytes() and np.array_equal(fr.cpu().numpy(), fr_o.cpu().numpy()), (name, fs)
        assert RR.to_search_state(st).tobytes() == st_o.tobytes(), (name, fs)
        for f in res_o.dtype.names:
            assert np.array_equal(res[f], res_o[f]), (name, fs, f)


def test_span_lost_equals_composition(rig):
    from ria_amd.acquire import rx_ring
    data, ctrl = rig
    O = oracle()
    row = next(r for r in RI.ROWS if r["name"] == "lts_span_wraps")
    cap, n, st, _, _ = RI.row_args(O, row)
    x = torch.from_numpy(cap[None, :]).to(data.device)
    want = rx_ring(data, x, [n], "OFDM_LTS", control_engine=ctrl, feed_step=0, state=np.array([st]))
    got = data.rx_ring(x, [n], "OFDM_LTS", control_engine=ctrl, feed_step=0, state=np.array([st]))
    assert want[2] == ["SPAN_LOST"] and got[1]["closed"][0] == 7 and got[1]["n_events"][0] == 0
    same_as_composition(data, "OFDM_LTS", got, want, "span_lost")
    unwritten(got)
