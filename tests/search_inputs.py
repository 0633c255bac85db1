"""The seeded table of captures for ria_gpu_search_batch, shared by tests/test_search_cpu.py (the restatement's coverage) and
tests/test_gpu_search.py (the library against the restatement).  A row is a capture, an initial decoder state, a mode and
an invocation limit; every row runs with feed_step 0 (the recording is all there: fed = capture_len unless the row says
otherwise) and with feed_step 4800 (one min_search has arrived unless the row says otherwise; fed0: nothing has).  Captures are built from
the oracle's transmitters and its AWGN channel at the smallest lengths that reach the statements: one min_search plus a few
steps.  The table is an input, not a result: what the rows reach is asserted by test_search_cpu.py on the restatement.
Test infrastructure only (not collected: no test_ prefix)."""
import numpy as np

import pyoracle as po
import search_restatement as SR
from mcdpsk_acquire_restatement import ACK, control_frame, encode_frame

F = np.float32
LTS_MIN, ZC_MIN, CHIRP_MIN = SR.min_search_of(SR.LTS), SR.min_search_of(SR.ZC), SR.min_search_of(SR.CHIRP)
FEED_STEPS = (0, 4800)
_cache = {}


def _noise(O, n, seed, scale=1.0):
    """the oracle channel's AWGN on silence (rms 0.0128 at 20 dB), scaled"""
    return (O.channel(0, 20.0, seed, np.zeros(n, F)) * F(scale)).astype(F)


def _ofdm_frame(O, seq, peak=0.8):
    s, _, _ = O.tx_frame(po.DQPSK, po.R1_4, (np.arange(20) * 7 % 251).astype(np.uint8), seq)
    return (s * F(peak / np.abs(s).max())).astype(F)


def _mc_frame(O, seq, zc, peak=0.8):
    s = O.mcdpsk_wf_tx(10, po.DQPSK if zc else po.DBPSK, po.R1_4, 1, zc, encode_frame(control_frame(ACK, seq)))
    return (s * F(peak / np.abs(s).max())).astype(F)


def _place(x, at, s):
    n = min(len(s), len(x) - at)
    x[at:at + n] += s[:n]


def capture(O, key):
    if key not in _cache:
        _cache[key] = np.ascontiguousarray(_BUILD[key](O), F)
    return _cache[key]


def _lts_clean(O):          # two strong frames in silence, the second cut by the capture's end
    x = np.zeros(LTS_MIN + 14400 + 31104 + 4800, F)
    _place(x, 14400, _ofdm_frame(O, 1))
    _place(x, 14400 + 31104 + 4000, _ofdm_frame(O, 2))
    return x


def _lts_noisy(O):          # frames of falling amplitude in noise: LTS correlations from accepted down to rejected
    x = _noise(O, LTS_MIN + 9600 + 14 * 4800, 11)
    _place(x, 14400, _ofdm_frame(O, 3, peak=0.100))
    _place(x, 14400 + 31104 + 2400, _ofdm_frame(O, 4, peak=0.085))
    _place(x, 14400 + 2 * (31104 + 2400), _ofdm_frame(O, 5, peak=0.070))
    return x


def _lts_noise(O):          # noise alone, rms 0.038
    return _noise(O, LTS_MIN + 4 * 4800, 12, scale=3.0)


def _lts_silence(O):
    return np.zeros(LTS_MIN + 2 * 4800, F)


def _lts_nonfinite(O):      # a NaN in the first RMS span, an Inf in the second
    x = _noise(O, LTS_MIN + 4 * 4800, 13, scale=3.0)
    x[500] = np.nan
    x[4800 + 500] = np.inf
    return x


def _zc_clean(O):           # one frame behind 12000 samples of silence; short enough for no catch-up
    x = np.zeros(48000, F)
    _place(x, 12000, _mc_frame(O, 1, True))
    return _noise(O, len(x), 21) + x


def _zc_weak(O):            # a faint frame in noise: correlations around the weak floor and the confidence
    x = _noise(O, 48000, 22, scale=2.0)
    _place(x, 12000, _mc_frame(O, 2, True, peak=0.03))
    return x


def _zc_noise(O):
    return _noise(O, ZC_MIN + 6 * 1200, 23, scale=3.0)


def _zc_long(O):            # a long recording: noise, a frame near its end (severe catch-up lands before it)
    x = _noise(O, 3 * ZC_MIN, 24, scale=2.0)
    _place(x, 3 * ZC_MIN - ZC_MIN - 4800 + 9600, _mc_frame(O, 3, True))
    return x


def _zc_mid(O):             # 1.8 x min_search of noise: moderate catch-up
    return _noise(O, ZC_MIN * 18 // 10, 25, scale=2.0)


def _chirp_clean(O):
    x = np.zeros(CHIRP_MIN + 9600 + 3 * 4800, F)
    _place(x, 14400, _mc_frame(O, 4, False))
    return _noise(O, len(x), 31) + x


def _chirp_cfo(O):          # the same frame through a transmitter offset of 12 Hz: the detector measures it
    x = np.zeros(CHIRP_MIN + 9600 + 3 * 4800, F)
    seg, _ = O.apply_tx_cfo(_mc_frame(O, 5, False), 12.0)
    _place(x, 14400, np.asarray(seg, F))
    return _noise(O, len(x), 32) + x


def _chirp_noise(O):
    return _noise(O, CHIRP_MIN + 3 * 4800, 33, scale=3.0)


_BUILD = {"lts_clean": _lts_clean, "lts_noisy": _lts_noisy, "lts_noise": _lts_noise, "lts_silence": _lts_silence, "lts_nonfinite": _lts_nonfinite,
          "zc_clean": _zc_clean, "zc_weak": _zc_weak, "zc_noise": _zc_noise, "zc_long": _zc_long, "zc_mid": _zc_mid,
          "chirp_clean": _chirp_clean, "chirp_cfo": _chirp_cfo, "chirp_noise": _chirp_noise}


def R(name, mode, cap, purpose, modulation="DQPSK", connected=False, max_inv=64, fed=None, fed0=False, **state):
    """fed: `fed` of the initial state under either feed_step; fed0: under feed_step 4800 nothing has arrived yet"""
    return dict(name=name, mode=mode, cap=cap, purpose=purpose, modulation=modulation, connected=connected, max_inv=max_inv, fed=fed, fed0=fed0,
                state=state)


L, Z, C = SR.LTS, SR.ZC, SR.CHIRP
LTS_FIRST_SYNC = 14344          # where the LTS detector places the first frame of lts_clean (asserted by test_search_cpu.py)
HI = dict(snr_hint=20.0)        # hints that leave the differential tier at 0.72
ROWS = [
    # ---- OFDM light sync
    R("lts_clean", L, "lts_clean", "silence skipped, SYNC_FOUND at the first frame; fed from nothing", fed0=True, **HI),
    R("lts_clean_second", L, "lts_clean", "from behind the first frame: the second one", correlation_pos=14400 + 31104, **HI),
    R("lts_replay", L, "lts_clean", "anti-replay at distance 199, then the second frame", last_decoded_sync_pos=LTS_FIRST_SYNC + 199, **HI),
    R("lts_no_replay", L, "lts_clean", "distance 200: no replay", last_decoded_sync_pos=LTS_FIRST_SYNC + 200, **HI),
    R("lts_psk", L, "lts_clean", "coherent PSK tier 0.90", modulation="QPSK"),
    R("lts_qam", L, "lts_clean", "QAM tier 0.78", modulation="QAM16"),
    R("lts_noisy_diff", L, "lts_noisy", "differential 0.72: falling correlations, rejects raise the streak", max_inv=40, **HI),
    R("lts_noisy_weak", L, "lts_noisy", "streak 3: a correlation within 0.08 under the confidence is weak-accepted", reject_streak=3, max_inv=40, **HI),
    R("lts_noisy_qam", L, "lts_noisy", "QAM with streak 3: the weak accept is refused", modulation="QAM16", reject_streak=3, max_inv=40),
    R("lts_noisy_psk", L, "lts_noisy", "PSK with streak 3: refused", modulation="QPSK", reject_streak=3, max_inv=40),
    R("lts_tier_62", L, "lts_noise", "hint tier 0.62 (snr_hint below 10)", snr_hint=9.0, max_inv=3),
    R("lts_tier_65", L, "lts_noise", "hint tier 0.65 (fading 0.7)", snr_hint=20.0, fading_hint=0.7, max_inv=3),
    R("lts_tier_68", L, "lts_noise", "hint tier 0.68 (snr_hint below 18)", snr_hint=17.0, max_inv=3),
    R("lts_streak_relax", L, "lts_noise", "streak 12: gate and confidence relaxed", reject_streak=12, max_inv=3, **HI),
    R("lts_streak_floor", L, "lts_noise", "streak 40: the relaxation's floors", reject_streak=40, noise_floor=0.002, max_inv=3, **HI),
    R("lts_streak_056", L, "lts_noise", "streak 40 under the 0.62 tier: the confidence's floor of 0.56", reject_streak=40, snr_hint=5.0, max_inv=2),
    R("lts_gate_high", L, "lts_noise", "a floor of 0.03: the gate at its high clamp, skips", noise_floor=0.03, max_inv=3),
    R("lts_gate_mid", L, "lts_noise", "a floor of 0.01: the gate between its clamps", noise_floor=0.01, max_inv=3),
    R("lts_nan_floor", L, "lts_noise", "a NaN floor becomes 0.001 at the tracker", noise_floor=np.nan, max_inv=2),
    R("lts_silence", L, "lts_silence", "skips to NEED_SAMPLES"),
    R("lts_limit", L, "lts_silence", "LIMIT after two invocations", max_inv=2),
    R("lts_short", L, "lts_silence", "fewer samples than min_search: the first wait", fed=LTS_MIN - 1, max_inv=40),
    R("lts_cursor_ahead", L, "lts_noise", "a cursor ahead of fed: a feed clamps it and clears the streak; without a feed NEED_SAMPLES",
      correlation_pos=50000, fed=20000, reject_streak=5, max_inv=40),
    R("lts_nonfinite", L, "lts_nonfinite", "a NaN and an Inf inside RMS spans", max_inv=3),
    # ---- connected MC-DPSK (ZC)
    R("zc_clean", Z, "zc_clean", "ZC tier 0.40, search_start clipped, SYNC_FOUND; fed from nothing", fed0=True),
    R("zc_clean_cfo", Z, "zc_clean", "known CFO 0.5: the residual is within 1 Hz of it or not", last_cfo_hz=0.5),
    R("zc_clean_cfo_far", Z, "zc_clean", "known CFO 30: the sanity rule takes the known CFO", last_cfo_hz=30.0),
    R("zc_weak", Z, "zc_weak", "correlations between the weak floor and the threshold: near misses raise the streak, misses lower it", max_inv=60),
    R("zc_weak_streak", Z, "zc_weak", "streak 5: a near miss more and the breaker's threshold accepts the frame", reject_streak=5, max_inv=60),
    R("zc_noise", Z, "zc_noise", "noise: misses lower the streak", reject_streak=2, max_inv=8),
    R("zc_long", Z, "zc_long", "a long recording: severe catch-up"),
    R("zc_mid", Z, "zc_mid", "1.8 x min_search: moderate catch-up", max_inv=6),
    # ---- the dual-chirp path of the MC-DPSK waveform
    R("chirp_clean", C, "chirp_clean", "disconnected handshake: SYNC_FOUND, no CFO rule", last_cfo_hz=5.0),
    R("chirp_connected", C, "chirp_clean", "the connected weak profile: CFO sanity against a known 5 Hz", connected=True, last_cfo_hz=5.0),
    R("chirp_cfo_kept", C, "chirp_cfo", "a measured offset within 1 Hz of the known one is kept", connected=True, last_cfo_hz=12.3),
    R("chirp_noise", C, "chirp_noise", "noise: the chirp gate, nothing found", max_inv=3),
    R("chirp_gate_high", C, "chirp_noise", "the chirp gate at its high clamp", noise_floor=0.03, max_inv=2),
    R("chirp_streak", C, "chirp_noise", "the chirp gate relaxed by a streak of 20", reject_streak=20, noise_floor=0.01, max_inv=2),
]


def row_args(O, r, feed_step):
    """-> (capture, capture_len, STATE record, class, connected) of row r under feed_step"""
    x = capture(O, r["cap"])
    st = SR.fresh_state(1)[0]
    for k, v in r["state"].items():
        st[k] = v
    st["fed"] = r["fed"] if r["fed"] is not None else (len(x) if feed_step == 0 else (0 if r["fed0"] else min(len(x), SR.min_search_of(r["mode"]))))
    return x, len(x), st, SR.modulation_class(r["mode"], r["modulation"]), r["connected"]


_results = {}


def expected(O, r, feed_step, trace=None):
    """the restatement's (result, state) of row r, computed once"""
    key = (r["name"], feed_step)
    if key not in _results or trace is not None:
        x, n, st, cls, conn = row_args(O, r, feed_step)
        _results[key] = SR.search(O, x, n, st, r["mode"], cls, conn, feed_step, r["max_inv"], trace)
    return _results[key]
