"""RxEngine.rx_stream (ria_gpu_rx_stream_batch) against the composition it replaces, ria_amd.acquire.rx_stream: the same
events - positions, outcome names, frame bytes, compared with == - and, through stream_restatement.comparator (the same loop
with its state returned, first checked against rx_stream itself), the same final ria_search_state bit for bit and the same
reason every stream closed for.  The recordings are those of tests/test_gpu_rx_stream.py (OFDM, ZC) and one dual-chirp
handshake recording (a PING, a 3-codeword CONNECT and a 1-codeword ACK behind silence and noise) whose three deliveries are
asserted on the comparator before anything is compared with it.  Nothing here is compared against a CPU restatement of the
search or of the window calls: they have their own parity tests."""
import ctypes as C

import numpy as np
import pytest
import torch

import pyoracle as po
import stream_restatement as SR
from mcdpsk_acquire_restatement import ACK, CONNECT, control_frame, data_frame, encode_frame, frame_len, oracle
from test_gpu_rx_stream import _norm, _stack, ofdm_recording, zc_recording

pytestmark = pytest.mark.gpu
F = np.float32
CONNECT3 = data_frame(CONNECT, 7, np.arange(25, dtype=np.uint8))
MODES = {"ofdm": ("OFDM_LTS", {}), "zc": ("MCDPSK_ZC", dict(carriers=10, modulation="DQPSK", spreading=1)),
         "chirp": ("MCDPSK_CHIRP", dict(carriers=10, modulation="DBPSK", spreading=1))}


def handshake_recording(O, seed):
    """a PING (dual chirp, training, reference symbol), a CONNECT of 3 codewords and an ACK of one, DBPSK on 10 carriers: the
    PING in silence, the rest in the channel's noise (AWGN, 15 dB)"""
    tx = lambda f: _norm(O.mcdpsk_wf_tx(10, po.DBPSK, po.R1_4, 1, False, encode_frame(f)))
    ack = control_frame(ACK, 40 + seed % 5)
    ping = _norm(O.mcdpsk_wf_tx(10, po.DBPSK, po.R1_4, 1, False, encode_frame(control_frame(ACK, 1)))[:57600 + 4608])
    parts = [np.zeros(20000, F), ping, np.zeros(30000, F), tx(CONNECT3), np.zeros(30000, F), tx(ack), np.zeros(130000, F)]
    x = np.concatenate(parts).astype(F)
    quiet = 20000 + len(ping) + 15000
    y = O.channel(0, 15.0, seed, x)
    y[:quiet] = x[:quiet]
    return np.ascontiguousarray(y, F), [b"", bytes(CONNECT3), bytes(ack)]


class Rig:
    def __init__(self):
        from ria_amd.engine import RxEngine
        self.data, self.ctrl = RxEngine("DQPSK", "R1_4", max_batch=8), RxEngine("DQPSK", "R1_4", max_batch=8)
        O = oracle()
        self.recs = {"ofdm": [ofdm_recording(O, 5), ofdm_recording(O, 6)], "zc": [zc_recording(O, 7), zc_recording(O, 8)],
                     "chirp": [handshake_recording(O, 9)]}
        self._ref = {}

    def kw(self, name):
        mode, kw = MODES[name]
        return mode, dict(kw, control_engine=self.ctrl if name == "ofdm" else None)

    def stack(self, name):
        return _stack([r[0] for r in self.recs[name]], self.data.device)

    def ref(self, name, feed_step):
        """the comparator on the mode's recordings as one batch, computed once: (events, state, closed)"""
        if (name, feed_step) not in self._ref:
            x, lens = self.stack(name)
            mode, kw = self.kw(name)
            self._ref[name, feed_step] = SR.comparator(self.data, x, lens, mode, feed_step=feed_step, **kw)
        return self._ref[name, feed_step]

    def new(self, x, lens, name, **more):
        from ria_amd.acquire import stream_events
        mode, kw = self.kw(name)
        st, res, ev, frames = self.data.rx_stream(x, lens, mode, **kw, **more)
        return stream_events(res, ev, frames), st, res, ev, frames


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.data.close()
    r.ctrl.close()


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def delivered(events):
    return [e for e in events if e["frame"] is not None]


def show(events):
    return [(e["position"], e["outcome"], None if e["frame"] is None else len(e["frame"])) for e in events]


def test_handshake_recording_is_delivered_by_the_comparator(rig):
    """the precondition of every chirp comparison below: the composition delivers the PING, the CONNECT and the ACK"""
    for fs in (0, 4800):
        events, _, _ = rig.ref("chirp", fs)
        got = delivered(events[0])
        assert [e["outcome"] for e in got] == ["PING", "DECODED", "DECODED"], show(events[0])
        for e, sent in zip(got, rig.recs["chirp"][0][1]):
            assert e["frame"][:len(sent)] == sent and len(e["frame"]) >= len(sent), show(events[0])


@pytest.mark.parametrize("feed_step", [0, 4800])
@pytest.mark.parametrize("name", ["ofdm", "zc", "chirp"])
def test_call_equals_composition(rig, name, feed_step):
    """as one batch, reversed and one by one: events == rx_stream's, state and close reason == the comparator's"""
    from ria_amd.acquire import rx_stream
    x, lens = rig.stack(name)
    mode, kw = rig.kw(name)
    want, want_state, want_closed = rig.ref(name, feed_step)
    assert want == rx_stream(rig.data, x, lens, mode, feed_step=feed_step, **kw)      # the local copy of the loop is the loop
    if (name, feed_step) != ("zc", 0):      # a ZC recording that "has all arrived" is a backlog: the catch-up jumps to its end (rx_stream's note)
        assert all(len(delivered(ev)) == len(rec[1]) for ev, rec in zip(want, rig.recs[name])), [show(ev) for ev in want]
    got, st, res, _, _ = rig.new(x, lens, name, feed_step=feed_step)
    assert got == want, ([show(e) for e in got], [show(e) for e in want])
    assert same_bytes(st, want_state), (st, want_state)
    assert np.array_equal(res["closed"], want_closed) and np.array_equal(res["n_events"], [len(e) for e in want])
    n = len(lens)
    rev = np.arange(n)[::-1].copy()
    got, st, res, _, _ = rig.new(x[torch.as_tensor(rev, device=x.device)].contiguous(), lens[rev], name, feed_step=feed_step)
    assert got == [want[i] for i in rev] and same_bytes(st, want_state[rev]) and np.array_equal(res["closed"], want_closed[rev])
    for i in range(n):
        got, st, res, _, _ = rig.new(x[i:i + 1].contiguous(), lens[i:i + 1], name, feed_step=feed_step)
        assert got == [want[i]] and same_bytes(st, want_state[i:i + 1]) and res["closed"][0] == want_closed[i]


@pytest.mark.parametrize("name", ["ofdm", "zc", "chirp"])
def test_host_form_equals_batch_form(rig, name):
    """ria_gpu_rx_stream_host on each recording: the records of the batch form on that recording alone, byte for byte"""
    mode, kw = rig.kw(name)
    fs = 4800 if name == "zc" else 0
    for rec, _ in rig.recs[name]:
        x = torch.from_numpy(rec[None, :]).to(rig.data.device)
        st, res, ev, frames = rig.data.rx_stream(x, [len(rec)], mode, feed_step=fs, max_events=8, **kw)
        hst, hres, hev, hframes = rig.data.rx_stream_host(rec, mode, feed_step=fs, max_events=8, **kw)
        assert res["n_events"][0] > 0
        assert same_bytes(st, hst) and same_bytes(res, hres) and same_bytes(ev, hev) and np.array_equal(frames.cpu().numpy(), hframes)


def test_ragged_batch(rig):
    """five ZC streams of odd lengths and odd offsets: a recording with 3 samples cut off its front and 12 345 off its end, one
    cut 601 samples before the end of its last frame, one whole, an empty one, and noise only; then the same streams in OFDM
    mode, where they hold no frame: whatever the composition makes of them, the call makes the same"""
    a, b = rig.recs["zc"][0][0], rig.recs["zc"][1][0]
    last = delivered(rig.ref("zc", 4800)[0][1])[-1]["position"]                # the training start of b's last frame
    noise = (np.random.default_rng(3).standard_normal(100001) * 0.012).astype(F)
    x, lens = _stack([a[3:][:(len(a) - 12348) | 1], b[:(last + frame_len(1, 10, 2, 1) - 601) | 1], a, np.zeros(0, F), noise], rig.data.device)
    assert (lens[[0, 1, 4]] % 2 == 1).all()
    for name, fs in (("zc", 4800), ("ofdm", 0)):
        mode, kw = rig.kw(name)
        want, want_state, want_closed = SR.comparator(rig.data, x, lens, mode, feed_step=fs, **kw)
        if name == "zc":
            assert len(delivered(want[0])) >= 1 and len(delivered(want[2])) == 3, [show(e) for e in want]
            assert not delivered(want[3]) and not delivered(want[4])
            assert want[3] == [] and want_closed[3] == SR.CLOSED["SEARCH_NEED_SAMPLES"]
        got, st, res, ev, _ = rig.new(x, lens, name, feed_step=fs)
        assert got == want, ([show(e) for e in got], [show(e) for e in want])
        assert same_bytes(st, want_state) and np.array_equal(res["closed"], want_closed)
        if name == "zc":
            # stream 0 is stream 2 moved by 3 samples: behind the first frame one of the two cursors is odd, and stays so
            assert (ev["search_start"][[0, 2], 1] % 2 == 1).any()
            # the cut stream's last window is shorter than the others of its round: two window calls in that round
            k = res["n_events"][1] - 1
            assert k >= 0 and res["n_events"][2] > k and 0 < ev["window_len"][1, k] < ev["window_len"][2, k]


@pytest.mark.parametrize("feed_step", [0, 4800])
def test_capture_cut_in_a_frame(rig, feed_step):
    """the handshake recording whole, and cut 20 000 samples before the end of its CONNECT: that stream's window is shorter
    than the other's in the same round - two window calls in one round - and ends in NEED_SAMPLES"""
    rec = rig.recs["chirp"][0][0]
    whole, _, _ = rig.ref("chirp", feed_step)
    connect = delivered(whole[0])[1]["position"]                               # the training start of the CONNECT
    cut = connect + frame_len(3, 10, 1, 1) - 20001
    x, lens = _stack([rec, rec[:cut]], rig.data.device)
    mode, kw = rig.kw("chirp")
    want, want_state, want_closed = SR.comparator(rig.data, x, lens, mode, feed_step=feed_step, **kw)
    assert want[0] == whole[0]
    assert want[1][-1]["outcome"] == "NEED_SAMPLES" and want_closed[1] == SR.CLOSED["WINDOW_NEED_SAMPLES"], show(want[1])
    got, st, res, ev, _ = rig.new(x, lens, "chirp", feed_step=feed_step)
    assert got == want, ([show(e) for e in got], [show(e) for e in want])
    assert same_bytes(st, want_state) and np.array_equal(res["closed"], want_closed)
    k = len(want[1]) - 1                                                       # an event's index is its round
    assert res["n_events"][0] > k and ev["window_len"][1, k] == cut - ev["search_start"][1, k] < ev["window_len"][0, k]
    assert ev["need_samples"][1, k] > 0 and ev["pending_total_cw"][1, k] > 0


def continue_until(rig, x, lens, name, again, **more):
    """calls on the streams whose close reason is in `again`, each with the state the call before left, until none is"""
    n = len(lens)
    state = rig.data.search_state(n, fed=0 if more.get("feed_step") else lens)
    events, closed, calls = [[] for _ in range(n)], np.zeros(n, np.int64), 0
    live = np.arange(n)
    while len(live):
        calls += 1
        assert calls < 200
        got, st, res, _, _ = rig.new(x[torch.as_tensor(live, device=x.device)].contiguous(), lens[live], name, state=state[live], **more)
        state[live] = st
        closed[live] = res["closed"]
        for i, s in enumerate(live):
            events[s] += got[i]
        live = live[np.isin(res["closed"], again)]
    return events, state, closed, calls


@pytest.mark.parametrize("name,feed_step", [("ofdm", 0), ("zc", 4800), ("chirp", 0)])
def test_one_event_per_call_equals_one_call(rig, name, feed_step):
    x, lens = rig.stack(name)
    want, want_state, want_closed = rig.ref(name, feed_step)
    assert max(len(e) for e in want) < 8
    got, st, res, _, _ = rig.new(x, lens, name, feed_step=feed_step, max_events=8)
    assert got == want and same_bytes(st, want_state)
    events, state, closed, calls = continue_until(rig, x, lens, name, [SR.CLOSED["EVENTS_FULL"]], feed_step=feed_step, max_events=1)
    assert events == want and same_bytes(state, want_state) and np.array_equal(closed, want_closed)
    assert calls == max(len(e) for e in want) + 1


def test_limit_and_continue(rig):
    """max_invocations = 3 per search leg: the first call equals the composition's and leaves LIMIT; going on with the
    returned state gives the walk of the unlimited call"""
    x, lens = rig.stack("ofdm")
    mode, kw = rig.kw("ofdm")
    want, want_state, want_closed = SR.comparator(rig.data, x, lens, mode, max_invocations=3, **kw)
    assert (want_closed == SR.CLOSED["SEARCH_LIMIT"]).all()
    got, st, res, _, _ = rig.new(x, lens, "ofdm", max_invocations=3)
    assert got == want and same_bytes(st, want_state) and np.array_equal(res["closed"], want_closed)
    assert (res["invocations"] == 3 * res["search_legs"]).all()
    full, full_state, full_closed = rig.ref("ofdm", 0)
    events, state, closed, calls = continue_until(rig, x, lens, "ofdm", [SR.CLOSED["SEARCH_LIMIT"]], max_invocations=3)
    assert events == full and same_bytes(state, full_state) and np.array_equal(closed, full_closed)
    assert calls > 3


@pytest.mark.parametrize("name,feed_step", [("ofdm", 0), ("zc", 4800), ("chirp", 0)])
def test_search_chunk_of_one(rig, name, feed_step):
    x, lens = rig.stack(name)
    want, want_state, want_closed = rig.ref(name, feed_step)
    rig.data.set_search_chunk(1)
    try:
        got, st, res, _, _ = rig.new(x, lens, name, feed_step=feed_step)
    finally:
        rig.data.set_search_chunk(0)
    assert got == want and same_bytes(st, want_state) and np.array_equal(res["closed"], want_closed)


def raw_call(rig, name, x, lens_in, state_in, n_events, fill=0xA5, **over):
    """ria_gpu_rx_stream_batch on outputs filled with `fill` -> (rc, state, results, events, frames) as uint8 arrays"""
    from ria_amd import capi
    from ria_amd.engine import _ptr
    e = rig.data
    mode, kw = MODES[name]
    n, stride = x.shape
    row = e.stream_frame_row(mode)
    dev = e.device
    lens_d = torch.from_numpy(np.asarray(lens_in, np.int32)).to(dev)
    st_d = torch.from_numpy(np.ascontiguousarray(state_in, e.SEARCH_STATE).view(np.uint8).reshape(n, 32).copy()).to(dev)
    res_d = torch.full((n, 64), fill, dtype=torch.uint8, device=dev)
    ev_d = torch.full((n, n_events, 64), fill, dtype=torch.uint8, device=dev)
    fr_d = torch.full((n, n_events, row), fill, dtype=torch.uint8, device=dev)
    cfg = C.byref(capi.McdpskConfig(kw["carriers"], {"DBPSK": 1, "DQPSK": 2}[kw["modulation"]], kw["spreading"], 0)) if kw else None
    a = dict(h=e.h, control=rig.ctrl.h if name == "ofdm" else None, mode=capi.SEARCH_MODE[mode], flags=0, cfg=cfg, samples=_ptr(x), stride=stride,
             lens=_ptr(lens_d), n=n, state=_ptr(st_d), feed_step=0, max_invocations=1 << 20, max_events=n_events, events=_ptr(ev_d),
             frames=_ptr(fr_d), frame_row=row, results=_ptr(res_d))
    a.update(over)
    rc = e.lib.ria_gpu_rx_stream_batch(*a.values(), None)
    torch.cuda.synchronize()
    return rc, st_d.cpu().numpy(), res_d.cpu().numpy(), ev_d.cpu().numpy(), fr_d.cpu().numpy()


@pytest.mark.parametrize("name", ["ofdm", "chirp"])
def test_every_output_row_is_written(rig, name):
    """outputs filled with 0xA5 first: every record comes back written, events past n_events and payload bytes past
    frame_bytes - whole rows where nothing is delivered - zero"""
    x, lens = rig.stack(name)
    e = rig.data
    rc, st, res, ev, fr = raw_call(rig, name, x, lens, e.search_state(len(lens), fed=lens), 8)
    assert rc == 0
    res, ev = res.view(e.STREAM_RESULT).reshape(-1), ev.view(e.STREAM_EVENT).reshape(len(lens), 8)
    want, _, _ = rig.ref(name, 0)
    assert np.array_equal(res["n_events"], [len(w) for w in want]) and not (res["reserved"] != 0).any()
    for s in range(len(lens)):
        for k in range(8):
            live = k < res["n_events"][s] and ev["delivered"][s, k]
            nbytes = int(ev["frame_bytes"][s, k]) if live else 0
            assert not fr[s, k, nbytes:].any(), (s, k)
            if k >= res["n_events"][s]:
                assert not ev[s, k:k + 1].view(np.uint8).any(), (s, k)
            else:
                assert want[s][k]["frame"] == (fr[s, k, :nbytes].tobytes() if live else None)


def test_argument_checks(rig):
    """each bad argument is RIA_ERR_INVALID with a message, and nothing is written; n_streams == 0 is RIA_OK"""
    e = rig.data
    x, lens = rig.stack("zc")
    fresh = e.search_state(len(lens), fed=lens)
    untouched = lambda out: all((o == 0xA5).all() for o in out[2:]) and same_bytes(out[1].reshape(-1), fresh)
    bad = [("ofdm", dict(mode=3)), ("ofdm", dict(flags=2)), ("zc", dict(cfg=None)), ("ofdm", dict(control=None)),
           ("zc", dict(control=rig.ctrl.h)), ("ofdm", dict(control=None, h=None)), ("zc", dict(max_events=0)), ("zc", dict(frame_row=319)),
           ("ofdm", dict(frame_row=e.stream_frame_row("OFDM_LTS") - 1)), ("zc", dict(n=-1)), ("zc", dict(feed_step=-1)),
           ("zc", dict(max_invocations=0)), ("zc", dict(stride=-1)), ("zc", dict(samples=None)), ("zc", dict(lens=None)),
           ("zc", dict(state=None)), ("zc", dict(events=None)), ("zc", dict(frames=None)), ("zc", dict(results=None))]
    for name, over in bad:
        out = raw_call(rig, name, x, lens, fresh, 4, **over)
        assert out[0] == -1 and untouched(out), (name, over, out[0])
        if over.get("h", 1) is not None:
            assert e.lib.ria_gpu_last_error(e.h).decode().startswith("ria_gpu_rx_stream_batch: "), (name, over)
    out = raw_call(rig, "zc", x, lens, fresh, 4, n=0)
    assert out[0] == 0 and untouched(out)
    # the search's domain: a capture longer than its stride, a state outside the call's domain - before anything is written
    out = raw_call(rig, "zc", x, lens + x.shape[1], fresh, 4)
    assert out[0] == -1 and untouched(out)
    broken = fresh.copy()
    broken["correlation_pos"][1] = 960000
    out = raw_call(rig, "zc", x, lens, broken, 4)
    assert out[0] == -1 and all((o == 0xA5).all() for o in out[2:]) and same_bytes(out[1].reshape(-1), broken)
    # the host form's own checks
    rec = rig.recs["zc"][0][0]
    with pytest.raises(Exception, match="ria_gpu_rx_stream_host"):
        e.rx_stream_host(rec, "MCDPSK_ZC", max_events=0, carriers=10, modulation="DQPSK")
    with pytest.raises(Exception, match="ria_gpu_rx_stream_host"):
        e.rx_stream_host(np.zeros(960000, F), "MCDPSK_ZC", carriers=10, modulation="DQPSK")
