"""Deterministic MC-DPSK demodulator and modulator inputs over their input domain (no test functions here).

Every frame is built from a seed through the oracle's modulator and channel restatements or plain numpy, float32
throughout, so the CPU tests, the GPU tests and oracle/gen_golden.py all rebuild the same bits.
tests/golden/mcdpsk_domain.npz holds the compiled reference's answers on these inputs and a sha256 per (configuration,
family): a generator that drifts fails the hash check instead of comparing different inputs.

A configuration is (carriers, bits per symbol, spreading, received data symbols, extra samples behind the last whole
symbol); its frames are (9 + received data symbols) * 512 + extra samples long.  A family is a dict: x float32
[n, frame_samples], cfo float32 [n], phase0 float32 [n], labels [n]; every frame of a family has one length, so a family
is one batch.  The base frames of a configuration are one AWGN 20 dB and one moderate-fading 20 dB frame at peak 0.8.

  level      base frames times 1e-30 .. 1e37 and the scales, worked out from the frame's own correlations (the
             demodulator is linear in the scale up to its gates), that put the quartiles of the reference symbol's
             amplitudes on 0.001, the median and the lower quartile of the per-symbol magnitudes on 0.0001, ref_mag on
             0.001, the median per-carrier mean on 1e-4 and on 0.001 and the mean over the carriers on 0.001; the scales,
             searched with the oracle, at which a reference amplitude is exactly 0.001 and a magnitude exactly 0.0001
  silence    +0.0, -0.0, denormals, a constant, zeroed training, zeroed reference symbol, one zeroed data symbol
  tail       the last 1, 2 and all-but-four data symbols at 0.15 / 0.19 / 0.21 / 0.5 of ref_mag (each symbol's total
             is set to exactly that multiple); the first four data symbols silent or tiny (ref_mag <= 0.001).  The
             configurations TAIL_SHORT have 3, 4 and 5 data symbols (nds >= 4, valid > 4)
  carrier    one carrier's bin of every symbol scaled to a mean ratio under 0.10 and to 1.5 % either side of 0.10, 0.20,
             0.35 and 1.25 (NEAR); one carrier scaled in the frequency
             domain over the whole frame to a mean ratio on both sides of 0.20, 0.35 and 1.25 (and to 0.08 and 0.12), one
             carrier removed, all but one removed and scaled so that only it exceeds 1e-4, one carrier amplitude-
             modulated over the symbols, the modulator's own output (no noise) plain and with one carrier x 4, of random
             bytes and of all-zero and all-one bytes (no phase error: the +-20 clamp)
  weak       AWGN at -10 .. 3 dB and pure Gaussian noise
  cfo        an analytic-signal rotation with the receiver told the same CFO, around the 0.1 Hz gate, with initial
             phases up to -1000 rad; frames told a CFO they do not carry
  nonfinite  frame 0 untouched, then one NaN / +inf / -inf / +-FLT_MAX sample in training symbol 0, training symbol 4, the reference symbol, the
             first, a middle and the last data symbol and the ignored tail (these frames are 100 samples longer than a
             whole number of symbols); a NaN data symbol; NaN and inf cfo_hz; NaN phase0.  What the reference does with
             them is recorded by tests/test_mcdpsk_domain_cpu.py: no LLR is ever NaN (the +-20 clamp, written with
             std::min / std::max, turns a NaN soft bit into +20), a NaN magnitude fails the 0.0001 gate and the chain
             continues from (1, 0), an infinite one makes the LLRs of its own and of the next symbol +20
  shape      (SHAPES, base AWGN frames only) carrier counts 1 .. 20, spreading with a received symbol count that is a
             multiple of it, no multiple of it and smaller than it, symbol counts around the row padding of
             mc_sym_row and, at 20 carriers, on both sides of every step of the staging chunk, frame lengths
             512 k + {0, 1, 511}

The compiled reference returned on every input tried: none is left out.

One carrier: MultiCarrierDPSKConfig::getCarrierFreqs (multi_carrier_dpsk.hpp:66-78) puts a single carrier on the
centre frequency, so MC-DPSK with one carrier is defined and the shape family has it.
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import pyoracle as po  # noqa: E402

SPS, PRE = 512, 9 * 512
MAIN = ((10, 1, 1, 65, 0), (10, 2, 1, 33, 0))         # the workload's DBPSK configuration and a DQPSK one
SHORT = (10, 1, 1, 1, 0)                              # the shortest frame the API takes (5120 samples)
TAIL_SHORT = tuple((10, b, 1, k, 0) for b in (1, 2) for k in (3, 4, 5))
FAMILIES = ("level", "silence", "tail", "carrier", "weak", "cfo", "nonfinite")
LEVELS = (1e-30, 1e-12, 1e-8, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 40.0, 32767.0, 1e6, 1e12, 1e19, 1e25, 1e37)
FLT_MAX = np.finfo(np.float32).max
GATE = np.float32(0.1)
CFOS = (0.0, 0.09, -0.09, float(GATE), -float(GATE), float(np.nextafter(GATE, np.float32(1))), -float(np.nextafter(GATE, np.float32(1))),
        0.11, -0.11, 2.0, -2.0, 50.0, -50.0, 200.0, -200.0)
PHASES = (0.0, float(np.float32(np.pi)), -float(np.float32(np.pi)), 3.2, -3.2, 100.0, -1000.0)
TAIL_EXTRA = 100                                      # samples behind the last whole symbol in the nonfinite family


def sym_row(n_sym):
    """floats per staged sample row as the kernel's comment states it: whole groups of four, never a multiple of 32"""
    r = (n_sym + 3) & ~3
    return r + 4 if r % 32 == 0 else r


def _rows(nc, n_sym, ch):
    return sym_row(n_sym) * ch * 4 + nc * (ch + 2) * 8


def _sums(nc, n_sym):
    return ((n_sym * nc * 8 + 15) & ~15) + 64


def corr_chunk(nc, n_sym):
    """the rule of the kernel's comment: the largest power of two, 128 down to 8, whose padded rows stay within 48 KB and,
    with the running sums, within the 160 KB of one workgroup"""
    ch = 128
    while ch > 8 and (_rows(nc, n_sym, ch) > 48 * 1024 or _sums(nc, n_sym) + _rows(nc, n_sym, ch) > 160 * 1024):
        ch >>= 1
    return ch


def lds_bytes(nc, n_sym):
    return _sums(nc, n_sym) + _rows(nc, n_sym, corr_chunk(nc, n_sym))


def chunk_steps(nc):
    """the received-symbol counts on either side of each step 128 -> 64 -> 32 -> 16 -> 8 of the staging chunk"""
    out, n = [], 4
    while corr_chunk(nc, n) > 8:
        if corr_chunk(nc, n + 1) != corr_chunk(nc, n):
            out += [n, n + 1]
        n += 1
    return out


def _shapes():
    s = [(nc, b, 1, 6, 0) for nc in (1, 2, 3, 7, 8, 13, 16, 20) for b in (1, 2)]
    # spreading: received symbols a multiple of it, no multiple of it, fewer than it
    s += [(10, 1, 2, 6, 0), (10, 1, 2, 7, 0), (10, 2, 2, 1, 0), (10, 2, 4, 8, 0), (10, 1, 4, 10, 0), (10, 1, 4, 3, 0), (8, 2, 4, 1, 0)]
    s += [(10, 1 + k % 2, 1, n_sym - 3, 0) for k, n_sym in enumerate((4, 5, 6, 7, 8, 9, 28, 29, 32, 33, 61, 65))]
    s += [(20, 1 + k % 2, 1, n_sym - 3, 0) for k, n_sym in enumerate(chunk_steps(20))]
    s += [(10, 1, 1, 6, 1), (10, 2, 1, 6, 511)]
    return tuple(dict.fromkeys(s))


SHAPES = _shapes()
CASES = tuple((c, f) for c in MAIN for f in FAMILIES) + tuple((c, "tail") for c in TAIL_SHORT) + ((SHORT, "cfo"),) + \
    tuple((c, "shape") for c in SHAPES)


def key(cfg, fam):
    return "c%d_b%d_s%d_n%d_x%d_%s" % (*cfg, fam)


def frame_samples(cfg):
    return PRE + cfg[3] * SPS + cfg[4]


def _seed(cfg, fam):
    return 880000 + 1000 * (FAMILIES + ("shape",)).index(fam) + 37 * cfg[0] + 11 * cfg[1] + 5 * cfg[2] + cfg[3] % 997 + cfg[4]


def rotate(x, hz):
    """the channel carries a frequency offset: analytic signal times exp(j 2 pi hz n / 48000), real part"""
    n = len(x)
    spec = np.fft.fft(x.astype(np.float64))
    h = np.zeros(n); h[0] = 1; h[1:n // 2] = 2; h[n // 2] = 1
    return np.real(np.fft.ifft(spec * h) * np.exp(2j * np.pi * float(hz) * np.arange(n) / 48000.0)).astype(np.float32)


def tx(O, cfg, rng, peak=0.8, byte=None):
    """the modulator's frame of random bytes (of one repeated byte value if given), cut to the configuration's length"""
    nc, bps, sp, num_rx, extra = cfg
    nds = -(-num_rx // sp)
    nb = -(-nds * nc * bps // 8)
    s = O.mcdpsk_modulate(nc, bps, sp, rng.integers(0, 256, nb, dtype=np.uint8) if byte is None else np.full(nb, byte, np.uint8))
    s = np.concatenate([s[:PRE + num_rx * SPS], np.zeros(extra, np.float32)])
    assert len(s) == frame_samples(cfg)
    return s if peak is None else s * np.float32(peak / np.abs(s).max())


_base = {}


def base_frames(O, cfg):
    """[AWGN 20 dB, moderate fading 20 dB] at peak 0.8 (copies; built once per process)"""
    if cfg not in _base:
        rng = np.random.default_rng(_seed(cfg, "shape") + 500000)
        _base[cfg] = [O.channel(kind, 20.0, 7700 + 3 * cfg[0] + cfg[3] + i, tx(O, cfg, rng)) for i, kind in enumerate((0, 2))]
    return [b.copy() for b in _base[cfg]]


def freqs(nc):
    return np.array([1500.0]) if nc == 1 else 500.0 + np.arange(nc) * (2000.0 / (nc - 1))


def magnitudes(cfg, x):
    """float64 picture of what the demodulator measures on a frame with spreading 1 ->
    (reference-symbol amplitude [nc], combined magnitude [nds, nc])"""
    nc, num_rx = cfg[0], cfg[3]
    assert cfg[2] == 1
    mix = np.exp(-2j * np.pi * np.outer(np.arange(SPS), freqs(nc)) / 48000.0)
    sym = x[8 * SPS:PRE + num_rx * SPS].astype(np.float64).reshape(1 + num_rx, SPS)
    y = np.abs(sym @ mix) / SPS
    return y[0], y[1:]


class _Fam:
    def __init__(self):
        self.x, self.cfo, self.ph, self.labels = [], [], [], []

    def add(self, x, label, cfo=0.0, phase0=0.0):
        with np.errstate(over="ignore", invalid="ignore"):
            self.x.append(np.asarray(x).astype(np.float32))
        self.cfo.append(cfo); self.ph.append(phase0); self.labels.append(label)

    def done(self):
        return {"x": np.ascontiguousarray(np.stack(self.x), np.float32), "cfo": np.array(self.cfo, np.float32),
                "phase0": np.array(self.ph, np.float32), "labels": list(self.labels)}


def edge_scales(O, cfg, x, name, target, estimate, want=2):
    """float32 scales at which the oracle finds a carrier's reference amplitude (REF_AMP_EDGE) or first data symbol's magnitude
    (SYM_MAG_EDGE) exactly on its threshold, where `>` and `>=` part: up to 64 float32 steps either side of target / estimate,
    tried on the frame's first ten symbols (both quantities are settled there)"""
    short, hits = x[:PRE + SPS], []
    for c in range(cfg[0]):
        s0 = np.array([target / estimate[c]], np.float32)
        for k in range(-64, 65):
            s = (s0.view(np.int32) + k).view(np.float32)[0]
            O.mcdpsk_demod_ex(cfg[0], cfg[1], 1, short * s)
            if O.mcdpsk_branch_counts()[2 * po.MBC.index(name)]:
                hits.append(s)
                break
        if len(hits) == want:
            break
    return hits


def level(O, cfg, rng):
    F = _Fam()
    for b, x in enumerate(base_frames(O, cfg)):
        for s in LEVELS:
            F.add(x * np.float32(s), f"base{b} x {s:g}")
        a, mag = magnitudes(cfg, x)
        for s in edge_scales(O, cfg, x, "REF_AMP_EDGE", 0.001, a):
            F.add(x * s, f"base{b} x {s!r}: a reference amplitude of exactly 0.001")
        for s in edge_scales(O, cfg, x, "SYM_MAG_EDGE", 0.0001, mag[0]):
            F.add(x * s, f"base{b} x {s!r}: a magnitude of data symbol 0 of exactly 0.0001")
        mean = mag.mean(0)
        ref_mag = mag[:4].sum(1).mean()
        for q in (0.75, 0.5, 0.25):
            F.add(x * np.float32(0.001 / np.quantile(a, q)), f"base{b}: quantile {q:g} of the reference amplitudes on 0.001")
        for q in (0.5, 0.25):
            F.add(x * np.float32(0.0001 / np.quantile(mag, q)), f"base{b}: quantile {q:g} of the symbol magnitudes on 0.0001")
        for side in (0.99, 1.01):
            F.add(x * np.float32(side * 0.001 / ref_mag), f"base{b}: ref_mag at {side:g} x 0.001")
            F.add(x * np.float32(side * 0.001 / mean.mean()), f"base{b}: mean over the carriers at {side:g} x 0.001")
        for thr in (1e-4, 0.001):
            F.add(x * np.float32(thr / np.median(mean)), f"base{b}: median carrier mean on {thr:g}")
    return F.done()


def silence(O, cfg, rng):
    F = _Fam()
    a, b = base_frames(O, cfg)
    n = len(a)
    F.add(np.zeros(n, np.float32), "+0.0")
    F.add(np.full(n, -0.0, np.float32), "-0.0")
    den = (rng.integers(1, 1 << 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)).view(np.float32)
    F.add(den, "denormals")
    F.add(np.full(n, 0.5, np.float32), "constant 0.5")
    for i, x in enumerate((a, b)):
        y = x.copy(); y[:8 * SPS] = 0
        F.add(y, f"base{i} training zeroed")
        y = x.copy(); y[8 * SPS:PRE] = 0
        F.add(y, f"base{i} reference symbol zeroed")
        y = x.copy(); y[PRE + (2 + i) * SPS:PRE + (3 + i) * SPS] = 0
        F.add(y, f"base{i} data symbol {2 + i} zeroed")
    return F.done()


def _tail_at(cfg, x, k, factor):
    """the last k data symbols scaled so that each one's total magnitude is factor x ref_mag (the first four symbols' level)"""
    _, mag = magnitudes(cfg, x)
    tot = mag.sum(1)
    ref = tot[:min(4, len(tot))].mean()
    y = x.astype(np.float64)
    for s in range(len(tot) - k, len(tot)):
        y[PRE + s * SPS:PRE + (s + 1) * SPS] *= factor * ref / tot[s]
    return y


def tail(O, cfg, rng):
    F = _Fam()
    nds = cfg[3]
    bases = base_frames(O, cfg)
    if nds <= 5:
        for i, x in enumerate(bases):
            F.add(x, f"base{i} with {nds} data symbols")
            for fac in (0.15, 0.21):
                F.add(_tail_at(cfg, x, 1, fac), f"base{i} with {nds} data symbols, the last at {fac:g} of ref_mag")
        return F.done()
    for i, x in enumerate(bases):
        for k in (1, 2, nds - 4):
            for fac in (0.15, 0.19, 0.21, 0.5):
                F.add(_tail_at(cfg, x, k, fac), f"base{i}: last {k} data symbols at {fac:g} of ref_mag")
        y = x.copy(); y[PRE:PRE + 4 * SPS] = 0
        F.add(y, f"base{i}: first four data symbols silent")
        y = x.copy(); y[PRE:PRE + 4 * SPS] *= np.float32(1e-3)
        F.add(y, f"base{i}: first four data symbols x 1e-3")
    return F.done()


def _band(cfg, n, c):
    """rfft bins nearer to carrier c than to its neighbours"""
    f = freqs(cfg[0])
    half = (f[1] - f[0]) / 2 if cfg[0] > 1 else 1000.0
    hz = np.fft.rfftfreq(n, 1 / 48000.0)
    return (hz >= f[c] - half) & (hz < f[c] + half)


def _gain(cfg, x, gains):
    """per-carrier gains applied to the whole frame in the frequency domain"""
    spec = np.fft.rfft(x.astype(np.float64))
    for c, g in gains.items():
        spec[_band(cfg, len(x), c)] *= g
    return np.fft.irfft(spec, len(x))


def _scale_bin(cfg, x, c, g):
    """carrier c's correlation of every data symbol, what it picks up from its neighbours included, times g: the symbol's
    own component at that frequency is subtracted in part (four passes settle the image term)"""
    y = x.astype(np.float64)
    w = np.exp(2j * np.pi * freqs(cfg[0])[c] * np.arange(SPS) / 48000.0)
    for s in range(cfg[3]):
        seg = y[PRE + s * SPS:PRE + (s + 1) * SPS]
        want = g * (seg @ np.conj(w)) / SPS
        for _ in range(4):
            seg += 2 * np.real((want - (seg @ np.conj(w)) / SPS) * w)
    return y


NEAR = (0.0985, 0.1015, 0.197, 0.203, 0.345, 0.355, 1.23, 1.27)    # mean ratios 1.5 % either side of 0.10, 0.20, 0.35, 1.25


def _at_ratio(cfg, x, c, r):
    """carrier c's bins scaled until its mean magnitude is r times the mean over the carriers (what the scaled bin sends into
    its neighbours moves that mean by a few per cent: the gain is solved again on the result, four times)"""
    g, y, nc = 1.0, x, cfg[0]
    for _ in range(4):
        m = magnitudes(cfg, y)[1].mean(0)
        g *= r * (m.sum() - m[c]) / (m[c] * (nc - r))
        y = _scale_bin(cfg, x, c, g)
    return y


def carrier(O, cfg, rng):
    F = _Fam()
    nc, nds = cfg[0], cfg[3]
    a, b = base_frames(O, cfg)
    mean = magnitudes(cfg, a)[1].mean(0)
    # what a removed carrier still picks up from its neighbours keeps its ratio near 0.2: the 0.10 floor of the magnitude
    # weight needs the carrier's own frequency bin of every symbol scaled
    for c, r in ((1, 0.05), (7, 0.08), (4, 0.09)):
        F.add(_scale_bin(cfg, a, c, r * (mean.sum() - mean[c]) / (mean[c] * (nc - r))), f"carrier {c}'s bin of every data symbol at {r:g} of the mean")
    for r in NEAR:
        F.add(_at_ratio(cfg, a, 3, r), f"carrier 3 at a mean ratio of {r:g}")
    for k, r in enumerate((0.08, 0.12, 0.18, 0.22, 0.33, 0.37, 1.2, 1.3)):
        for c in ((2 + k) % nc, nc - 1 - k % 3):
            g = r * (mean.sum() - mean[c]) / (mean[c] * (nc - r))        # mean[c] g / gmean = r
            F.add(_gain(cfg, a, {c: g}), f"carrier {c} at {r:g} of the mean over the carriers")
    for i, x in enumerate((a, b)):
        F.add(_gain(cfg, x, {3 + i: 0.0}), f"base{i}: carrier {3 + i} removed")
        y = _gain(cfg, x, {c: 0.0 for c in range(nc) if c != 4 + i})
        m = magnitudes(cfg, y)[1].mean(0)
        F.add(y * np.sqrt(1e-4 / m[4 + i] * 1e-4 / np.delete(m, 4 + i).max()), f"base{i}: only carrier {4 + i} above 1e-4")
        spec = np.fft.rfft(x.astype(np.float64))
        spec[~_band(cfg, len(x), 5)] = 0
        am = 0.8 * np.sin(2 * np.pi * np.arange(len(x)) / (SPS * min(nds, 12)))
        F.add(x + am * np.fft.irfft(spec, len(x)), f"base{i}: carrier 5 amplitude-modulated over the symbols")
    for t in range(2):
        s = tx(O, cfg, rng)
        F.add(s, f"tx {t} with no channel")
        F.add(_gain(cfg, s, {1 + t: 4.0}), f"tx {t} with no channel, carrier {1 + t} x 4")
    # a carrier that never changes phase (or turns by pi every symbol) sees the same interference in every symbol: no phase
    # error, scale 20, and the raised carrier's weight 1.25 takes cos(phase) = +-1 past the clamp
    for byte in (0x00, 0xFF):
        F.add(_gain(cfg, tx(O, cfg, rng, byte=byte), {6: 4.0}), f"tx of bytes {byte:#04x} with no channel, carrier 6 x 4")
    return F.done()


def weak(O, cfg, rng):
    F = _Fam()
    for i, snr in enumerate((-10.0, -5.0, 0.0, 3.0)):
        for t in range(2):
            F.add(O.channel(0, snr, _seed(cfg, "weak") + 10 * i + t, tx(O, cfg, rng)), f"AWGN {snr:g} dB #{t}")
    for sigma in (1e-3, 0.2, 10.0):
        F.add(rng.normal(0, sigma, frame_samples(cfg)), f"noise sigma {sigma:g}")
    return F.done()


def cfo(O, cfg, rng):
    F = _Fam()
    for k, hz in enumerate(CFOS):
        x = O.channel(0, 20.0, _seed(cfg, "cfo") + k, rotate(tx(O, cfg, rng), hz))
        F.add(x, f"carried and told {hz!r} Hz, phase0 {PHASES[k % len(PHASES)]:g}", cfo=hz, phase0=PHASES[k % len(PHASES)])
    x = base_frames(O, cfg)[0]
    for k, ph in enumerate(PHASES):
        F.add(x, f"carried 0 Hz, told {(5.0, -3.0)[k % 2]:g} Hz, phase0 {ph:g}", cfo=(5.0, -3.0)[k % 2], phase0=ph)
    F.add(O.channel(0, 20.0, _seed(cfg, "cfo") + 90, rotate(tx(O, cfg, rng), 3.0)), "carried 3 Hz, told -3 Hz", cfo=-3.0)
    F.add(O.channel(0, 20.0, _seed(cfg, "cfo") + 91, rotate(tx(O, cfg, rng), 4.0)), "carried 4 Hz, told 0 Hz", phase0=1.0)
    return F.done()


def nonfinite_places(cfg):
    """(name, sample index, first data symbol whose LLRs the value can reach or None)"""
    nds = cfg[3]
    return (("training symbol 0", 300, None), ("training symbol 4", 4 * SPS + 77, None), ("the reference symbol", 8 * SPS + 201, None),
            ("data symbol 0", PRE + 40, 0), (f"data symbol {nds // 2}", PRE + (nds // 2) * SPS + 511, nds // 2),
            (f"data symbol {nds - 1}", PRE + (nds - 1) * SPS + 5, nds - 1), ("the ignored tail", PRE + nds * SPS + 60, None))


def nonfinite(O, cfg, rng):
    F = _Fam()
    x = np.concatenate([base_frames(O, cfg)[0], rng.normal(0, 0.05, TAIL_EXTRA).astype(np.float32)])
    F.add(x, "untouched")
    for name, v in (("NaN", np.nan), ("+inf", np.inf), ("-inf", -np.inf), ("+FLT_MAX", FLT_MAX), ("-FLT_MAX", -FLT_MAX)):
        for where, i, _ in nonfinite_places(cfg):
            y = x.copy(); y[i] = v
            F.add(y, f"{name} in {where}")
    y = x.copy(); y[PRE + 3 * SPS:PRE + 4 * SPS] = np.nan
    F.add(y, "data symbol 3 all NaN")
    F.add(x, "cfo_hz NaN", cfo=np.nan)
    F.add(x, "cfo_hz +inf", cfo=np.inf)
    F.add(x, "phase0 NaN with cfo_hz 2", cfo=2.0, phase0=np.nan)
    return F.done()


def shape(O, cfg, rng):
    F = _Fam()
    for t in range(2):
        F.add(O.channel(0, 20.0, _seed(cfg, "shape") + t, tx(O, cfg, rng)), f"AWGN 20 dB #{t}")
    return F.done()


_BUILDERS = {"level": level, "silence": silence, "tail": tail, "carrier": carrier, "weak": weak, "cfo": cfo, "nonfinite": nonfinite,
             "shape": shape}
_cache = {}


def family(O, cfg, name):
    if (cfg, name) not in _cache:
        _cache[(cfg, name)] = _BUILDERS[name](O, cfg, np.random.default_rng(_seed(cfg, name)))
    return _cache[(cfg, name)]


def digest(F):
    """sha256 over the sample bits and the metadata of a family"""
    h = hashlib.sha256()
    for k in ("x", "cfo", "phase0"):
        h.update(np.ascontiguousarray(F[k]).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------- answers
AUX = ("cfo_hz", "fading_index", "freq_fading_index", "temporal_fading_index")


def oracle_answers(O, cfg, F):
    """-> (llr list, aux uint32 [n, 4] bit patterns in AUX order, training CFO residual float32 [n], valid symbols int32 [n],
    branch counts uint32 [n, 2 len(po.MBC)])"""
    llrs, aux, res, valid, bc = [], [], [], [], []
    for f in range(len(F["x"])):
        l, a, r, v = O.mcdpsk_demod_ex(cfg[0], cfg[1], cfg[2], F["x"][f], float(F["cfo"][f]), float(F["phase0"][f]))
        llrs.append(l); aux.append(a.view(np.uint32).copy()); res.append(r); valid.append(v); bc.append(O.mcdpsk_branch_counts())
    return llrs, np.stack(aux), np.array(res, np.float32), np.array(valid, np.int32), np.stack(bc)


def reference_answers(R, cfg, F):
    """the compiled reference on the same frames -> (llr list, aux uint32 [n, 4])"""
    llrs, aux = [], []
    for f in range(len(F["x"])):
        l, a = R.mcdpsk_demod(cfg[0], cfg[1], cfg[2], F["x"][f], float(F["cfo"][f]), float(F["phase0"][f]))
        llrs.append(l); aux.append(a.view(np.uint32).copy())
    return llrs, np.stack(aux)


def llr_digest(l):
    """sha256 of an LLR row's bit patterns, every NaN counted as one value (sign and payload of a NaN are not compared)"""
    u = np.ascontiguousarray(l, np.float32).view(np.uint32).copy()
    u[np.isnan(l)] = 0x7FC00000
    return hashlib.sha256(u.tobytes()).hexdigest()


def same_bits(a, b):
    """bit-for-bit equality of two float32 arrays under the NaN rule: NaN positions equal, every other bit equal"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# ---------------------------------------------------------------------------------------------- modulator cases
def _pad_bytes(bits, pad):
    """the smallest byte count >= 1 that leaves `pad` bits of padding in the last symbol, or None when 8 n never does"""
    for n in range(1, 4 * bits + 1):
        if (-8 * n) % bits == pad:
            return n
    return None


def _mod_cases():
    """(carriers, bits, spreading, n_bytes, pattern): every carriers x bits x spreading with byte counts and patterns in
    rotation, every byte count at the workload's configuration, 600-symbol chains and the largest byte count of the
    device modulator's 64 KB rule (8190 (symbol, carrier) pairs)"""
    cases, k = [], 0
    for nc in (2, 3, 8, 10, 13, 20):
        for bps in (1, 2):
            sizes = [0, 1, 20, 81] + [n for n in (_pad_bytes(nc * bps, 1), _pad_bytes(nc * bps, nc * bps - 1)) if n is not None]
            for sp in (1, 2, 4):
                for j in range(2):
                    cases.append((nc, bps, sp, sizes[(k + 3 * j) % len(sizes)], ("random", "zero", "one")[k % 3]))
                    k += 1
    cases += [(10, 1, 1, n, p) for n in (0, 1, 20, 81) for p in ("zero", "one", "random")]
    cases += [(13, 1, 1, _pad_bytes(13, 1), "one"), (13, 1, 2, _pad_bytes(13, 12), "random"), (3, 2, 1, _pad_bytes(6, 4), "one")]
    cases += [(10, 2, 1, 1500, "random"), (13, 1, 1, 975, "one"), (2, 1, 1, 150, "random")]      # 600 data symbols
    cases += [(20, 2, 1, (8190 // 20) * 5, "random")]
    return tuple(dict.fromkeys(cases))


MOD_CASES = _mod_cases()


def mod_data(case, index):
    nc, bps, sp, nb, pat = case
    if pat == "random":
        return np.random.default_rng(990000 + index).integers(0, 256, nb, dtype=np.uint8)
    return np.full(nb, 0 if pat == "zero" else 255, np.uint8)


def audio_digest(x):
    return hashlib.sha256(np.ascontiguousarray(x, np.float32).tobytes()).hexdigest()


if __name__ == "__main__":
    # the table of the pull request text: per (configuration, family) the frames on the true / false side of each condition
    O = po.Oracle()
    print("configuration family frames NaN-LLRs | " + " ".join(po.MBC) + " (frames true/false)")
    for cfg, fam in CASES:
        F = family(O, cfg, fam)
        llr, _, _, _, bc = oracle_answers(O, cfg, F)
        hit = (bc > 0).sum(0)
        print(key(cfg, fam), len(F["x"]), sum(int(np.isnan(l).sum()) for l in llr), "|",
              " ".join(f"{hit[2 * i]}/{hit[2 * i + 1]}" for i in range(len(po.MBC))))
