"""Deterministic OFDM demodulator inputs over the demodulator's input domain (no test functions here).

Every frame is built from a seed through the oracle's TX and channel restatements, so the CPU tests, the GPU tests and
oracle/gen_golden.py all rebuild the same float32 bits.  tests/golden/demod_domain.npz holds the compiled reference's
answers on these inputs and a sha256 per (mode, family): a generator that drifts fails the hash check instead of
comparing different inputs.

A family is a dict: x float32 [n, frame_samples], cfo float32 [n], pos uint64 [n], flags uint32 [n], labels [n].
The base frames of a mode are one AWGN 20 dB and one moderate-fading 20 dB frame at peak 0.8.

  level      base frames times 1e-30 .. 1e37, and the scales that put the quartiles of the oracle's |H| on 0.01
  clean      TX with no channel at peak 0.8 and at the modulator's own scale (noise variance 0)
  silence    +0.0, -0.0, denormals, zeroed LTS, zeroed data, one zeroed data symbol, a constant
  weak       AWGN at -10 .. 3 dB, pure Gaussian noise
  notch      y[n] = x[n] - a x[n-d] (spectral nulls on data carriers and pilots), a sine on a pilot's frequency
  clip       base frames clipped at 0.5, 0.1, 0.01 of their peak
  nonfinite  single NaN / +-inf samples in the LTS, a prefix, a data symbol and at the end; NaN symbols; +-FLT_MAX
  residual   an analytic-signal rotation the receiver is not told about, or only partly, around the 0.3 Hz and 5 Hz
             limits of the training re-run (channel_equalizer.cpp:327)
  meta       abs_position x cfo_hz with |2 pi cfo pos / 48000| <= 1e6 rad, flags bit 0 with and without a negated
             first LTS, flags bits 1..31 (ignored)

DBPSK and BPSK: OFDMChirpWaveform::configure accepts both (ofdm_chirp_waveform.cpp:83-91), so they are recorded like
the other modes.  QAM256 is recorded through the OFDM-COX object (configure maps it to DQPSK, :82-89).
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import pyoracle as po  # noqa: E402

# name -> (modulation, rate, recorded through the OFDM-COX object)
MODES = {"QAM16_R1_2": (po.QAM16, po.R1_2, False), "DQPSK_R1_4": (po.DQPSK, po.R1_4, False),
         "D8PSK_R1_2": (po.D8PSK, po.R1_2, False), "QPSK_R1_2": (po.QPSK, po.R1_2, False),
         "QAM64_R3_4": (po.QAM64, po.R3_4, False), "QAM256_R3_4": (po.QAM256, po.R3_4, True),
         "DBPSK_R1_4": (po.DBPSK, po.R1_4, False), "BPSK_R1_4": (po.BPSK, po.R1_4, False)}
ENGINE = {"QAM16_R1_2": ("QAM16", "R1_2"), "DQPSK_R1_4": ("DQPSK", "R1_4"), "D8PSK_R1_2": ("D8PSK", "R1_2"),
          "QPSK_R1_2": ("QPSK", "R1_2"), "QAM64_R3_4": ("QAM64", "R3_4"), "QAM256_R3_4": ("QAM256", "R3_4"),
          "DBPSK_R1_4": ("DBPSK", "R1_4"), "BPSK_R1_4": ("BPSK", "R1_4")}
FAMILIES = ("level", "clean", "silence", "weak", "notch", "clip", "nonfinite", "residual", "meta")
SOME = ("level", "silence", "notch", "nonfinite", "residual")          # the families of every mode but QAM16 R1/2
CASES = tuple((m, f) for m in MODES for f in (FAMILIES if m == "QAM16_R1_2" else SOME))

SYM = 1152
LEVELS = (1e-30, 1e-12, 1e-8, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 40.0, 32767.0, 1e6, 1e12, 1e19, 1e25, 1e37)
RESIDUALS = (0.0, 0.1, 0.2, 0.4, 0.6, 1.5, 4.0, 4.5, 5.6, 6.5, 20.0)     # Hz the receiver is not told about, both signs
META_POS = (0, 1, 47999, 48000, 2 ** 24 - 1, 2 ** 24 + 1, 2 ** 31, 2 ** 32 + 5, 2 ** 36)
META_CFO = (0.011, -0.011, 2.0, -2.0, 60.0, -60.0)
MAX_WRAP_RAD = 1e6                                                       # GPU tests pass only metadata inside this
FLT_MAX = np.finfo(np.float32).max
_BPC = {po.R1_4: 20, po.R1_3: 27, po.R1_2: 40, po.R2_3: 54, po.R3_4: 60, po.R5_6: 67}


def _seed(mode, fam):
    return 660000 + 100 * list(MODES).index(mode) + FAMILIES.index(fam)


def rotate(x, hz):
    """the channel carries a frequency offset: analytic signal times exp(j 2 pi hz n / 48000), real part"""
    n = len(x)
    spec = np.fft.fft(x.astype(np.float64))
    h = np.zeros(n); h[0] = 1; h[1:n // 2] = 2; h[n // 2] = 1
    return np.real(np.fft.ifft(spec * h) * np.exp(2j * np.pi * float(hz) * np.arange(n) / 48000.0)).astype(np.float32)


def tx(O, mode, seq, rng, peak=0.8):
    mod, rate, _ = MODES[mode]
    s, _, _ = O.tx_frame(mod, rate, rng.integers(0, 256, 4 * _BPC[rate] - 19, dtype=np.uint8), seq)
    return s if peak is None else s * np.float32(peak / np.abs(s).max())


_base = {}


def base_frames(O, mode):
    """[AWGN 20 dB, moderate fading 20 dB] at peak 0.8 (copies; built once per process)"""
    if mode not in _base:
        rng = np.random.default_rng(650000 + list(MODES).index(mode))
        _base[mode] = [O.channel(kind, 20.0, 6500 + 10 * list(MODES).index(mode) + i, tx(O, mode, i, rng))
                       for i, kind in enumerate((0, 2))]
    return [b.copy() for b in _base[mode]]


class _Fam:
    def __init__(self):
        self.x, self.cfo, self.pos, self.flags, self.labels = [], [], [], [], []

    def add(self, x, label, cfo=0.0, pos=0, flags=0):
        with np.errstate(over="ignore", invalid="ignore"):
            self.x.append(np.asarray(x).astype(np.float32))
        self.cfo.append(cfo); self.pos.append(pos); self.flags.append(flags); self.labels.append(label)

    def done(self):
        return {"x": np.ascontiguousarray(np.stack(self.x), np.float32), "cfo": np.array(self.cfo, np.float32),
                "pos": np.array(self.pos, np.uint64), "flags": np.array(self.flags, np.uint32), "labels": list(self.labels)}


def h_threshold_scales(O, mode, x):
    """the scales that put the lower quartile, the median and the upper quartile of the oracle's |H| on 0.01"""
    mod, rate, _ = MODES[mode]
    _, aux = O.rx_process(mod, rate, x)
    mag = np.hypot(*np.array(aux.h[:], np.float32).reshape(-1, 2).T.astype(np.float64))
    return [float(np.float32(0.01 / q)) for q in np.quantile(mag, (0.75, 0.5, 0.25))]


def level(O, mode, rng):
    F = _Fam()
    for b, x in enumerate(base_frames(O, mode)):
        for s in LEVELS:
            F.add(x * np.float32(s), f"base{b} x {s:g}")
        for s in h_threshold_scales(O, mode, x):
            F.add(x * np.float32(s), f"base{b} x {s:.6g} (|H| across 0.01)")
    return F.done()


def clean(O, mode, rng):
    F = _Fam()
    for t in range(2):
        F.add(tx(O, mode, 40 + t, rng), f"tx {t} peak 0.8")
        F.add(tx(O, mode, 50 + t, rng, peak=None), f"tx {t} native scale")
    return F.done()


def silence(O, mode, rng):
    F = _Fam()
    a, b = base_frames(O, mode)
    n = len(a)
    F.add(np.zeros(n, np.float32), "+0.0")
    F.add(np.full(n, -0.0, np.float32), "-0.0")
    den = (rng.integers(1, 1 << 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)).view(np.float32)
    F.add(den, "denormals")
    for i, x in enumerate((a, b)):
        y = x.copy(); y[:2 * SYM] = 0
        F.add(y, f"base{i} both LTS zeroed")
        y = x.copy(); y[2 * SYM:] = 0
        F.add(y, f"base{i} all data zeroed")
        y = x.copy(); y[(3 + i) * SYM:(4 + i) * SYM] = 0
        F.add(y, f"base{i} data symbol {1 + i} zeroed")
    F.add(np.full(n, 0.5, np.float32), "constant 0.5")
    return F.done()


def weak(O, mode, rng):
    F = _Fam()
    for i, snr in enumerate((-10.0, -5.0, 0.0, 3.0)):
        for t in range(2):
            F.add(O.channel(0, snr, _seed(mode, "weak") + 10 * i + t, tx(O, mode, 60 + 2 * i + t, rng)), f"AWGN {snr:g} dB #{t}")
    n = len(F.x[0])
    for sigma in (1e-3, 0.2, 10.0):
        F.add(rng.normal(0, sigma, n), f"noise sigma {sigma:g}")
    return F.done()


def notch(O, mode, rng):
    F = _Fam()
    mod, rate, _ = MODES[mode]
    g = O.geom(mod, rate)
    for i, x in enumerate(base_frames(O, mode)):
        for d in (1, 7, 37, 120, 200):
            for a in (1.0, 0.99, 0.5):
                y = x.astype(np.float64)
                y[d:] -= a * x[:-d].astype(np.float64)
                F.add(y, f"base{i} x[n] - {a:g} x[n-{d}]")
    # a sine on a pilot's frequency (modes without pilots: the lowest carrier), relative to the frame's rms
    x = base_frames(O, mode)[0]
    kbin = int(g.pilot_idx[g.n_pilot // 2]) if g.n_pilot else int(g.all_idx[0])
    hz = 1500.0 + (kbin - 1024 if kbin >= 512 else kbin) * 48000.0 / 1024.0
    rms = np.sqrt(np.mean(x.astype(np.float64) ** 2))
    for db in (0.0, 20.0):
        amp = rms * np.sqrt(2.0) * 10 ** (db / 20.0)
        F.add(x + amp * np.sin(2 * np.pi * hz * np.arange(len(x)) / 48000.0 + 0.3), f"sine at {hz:g} Hz, {db:+g} dB")
    return F.done()


def clip(O, mode, rng):
    F = _Fam()
    for i, x in enumerate(base_frames(O, mode)):
        for c in (0.5, 0.1, 0.01):
            lim = np.float32(c * np.abs(x).max())
            F.add(np.clip(x, -lim, lim), f"base{i} clipped at {c:g} of peak")
    return F.done()


def nonfinite(O, mode, rng):
    F = _Fam()
    x = base_frames(O, mode)[0]
    n = len(x)
    places = (("LTS 0", 128 + 300), ("LTS 1", SYM + 128 + 511), ("prefix of data symbol 2", 4 * SYM + 40),
              ("data symbol 0", 2 * SYM + 128 + 77), ("last sample", n - 1))
    for name, v in (("NaN", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
        for where, i in places:
            y = x.copy(); y[i] = v
            F.add(y, f"{name} at {where}")
    y = x.copy(); y[5 * SYM:6 * SYM] = np.nan
    F.add(y, "data symbol 3 all NaN")
    F.add(np.full(n, np.nan, np.float32), "all NaN")
    for name, v in (("+FLT_MAX", FLT_MAX), ("-FLT_MAX", -FLT_MAX)):
        y = x.copy(); y[[128 + 17, 3 * SYM + 500, n - 7]] = v
        F.add(y, f"{name} in LTS 0, data symbol 1 and near the end")
    y = x.copy(); y[2 * SYM + 300] = FLT_MAX; y[2 * SYM + 301] = -FLT_MAX
    F.add(y, "+FLT_MAX next to -FLT_MAX in data symbol 0")
    return F.done()


def residual(O, mode, rng):
    """told: what setFrequencyOffset gets; the channel carries told + r"""
    F = _Fam()
    k = 0
    for r in RESIDUALS:
        for sg in ((1,) if r == 0 else (1, -1)):
            told = (0.0, 3.0, -7.0)[k % 3]
            x = rotate(tx(O, mode, 100 + k, rng), told + sg * r)
            F.add(O.channel(0, 20.0, _seed(mode, "residual") + k, x), f"carried {told + sg * r:+g} Hz, told {told:+g} Hz",
                  cfo=told, pos=(0, 4800, 123457)[k % 3])
            k += 1
    return F.done()


def meta(O, mode, rng):
    F = _Fam()
    a, b = base_frames(O, mode)
    k = 0
    for pos in META_POS:
        for cfo in META_CFO:
            if abs(2.0 * np.pi * cfo * pos / 48000.0) > MAX_WRAP_RAD:
                continue
            F.add((a, b)[k % 2], f"cfo {cfo:g} Hz at {pos}", cfo=cfo, pos=pos)
            k += 1
    neg = a.copy(); neg[:SYM] = -neg[:SYM]
    F.add(neg, "first LTS negated, flag set", flags=1)
    F.add(a, "first LTS as sent, flag set", flags=1)
    F.add(neg, "first LTS negated, flag clear", flags=0)
    F.add(neg, "first LTS negated, flag set, cfo 2 Hz", cfo=2.0, pos=48001, flags=1)
    for fl in (0xFFFFFFFE, 0x80000000, 0x2, 0xFFFFFFFF, 0x7FFFFFFF):
        F.add(neg if fl & 1 else b, f"flags {fl:#x}", cfo=-2.0, pos=4801, flags=fl)
    return F.done()


_BUILDERS = {"level": level, "clean": clean, "silence": silence, "weak": weak, "notch": notch, "clip": clip,
             "nonfinite": nonfinite, "residual": residual, "meta": meta}
_cache = {}


def family(O, mode, name):
    key = (mode, name)
    if key not in _cache:
        _cache[key] = _BUILDERS[name](O, mode, np.random.default_rng(_seed(mode, name)))
    return _cache[key]


def digest(F):
    """sha256 over the sample bits and the metadata of a family"""
    h = hashlib.sha256()
    for k in ("x", "cfo", "pos", "flags"):
        h.update(np.ascontiguousarray(F[k]).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------- answers
AUX = ("cfo_hz", "fading_index", "noise_variance", "lts_phase_slope", "snr_linear", "corr_phase")


def oracle_answers(O, mode, F):
    """-> (llr list, aux uint32 [n, 6] bit patterns in AUX order, snr_db float32 [n], h float32 [n, 118])"""
    mod, rate, _ = MODES[mode]
    llrs, aux, snr, hs = [], [], [], []
    for f in range(len(F["x"])):
        l, a = O.rx_process(mod, rate, F["x"][f], float(F["cfo"][f]), int(F["pos"][f]), burst_marker=bool(F["flags"][f] & 1))
        llrs.append(l)
        aux.append(np.array([getattr(a, k) for k in AUX], np.float32).view(np.uint32))
        snr.append(a.snr_db)
        hs.append(np.array(a.h[:], np.float32))
    return llrs, np.stack(aux), np.array(snr, np.float32), np.stack(hs)


BRANCHES = ("H_SMALL", "MAG_SMALL", "CNT_SMALL", "RERUN", "SNR_LOW", "SNR_HIGH", "HM_SMALL", "SNV_SMALL", "DEN_SMALL", "CNV_LOW",
            "CNV_HIGH", "D8PSK_TWO_PASS", "SP_SMALL")          # RO_BC_* of oracle/ria_oracle.h


def branch_counts(O, mode, F):
    """how often the oracle took each data-dependent branch of the demodulator on every frame -> uint32 [n, len(BRANCHES)]"""
    import ctypes as C
    mod, rate, _ = MODES[mode]
    out = np.zeros((len(F["x"]), len(BRANCHES)), np.uint32)
    for f in range(len(F["x"])):
        O.rx_process(mod, rate, F["x"][f], float(F["cfo"][f]), int(F["pos"][f]), burst_marker=bool(F["flags"][f] & 1))
        O.lib.ro_branch_counts(out[f].ctypes.data_as(C.POINTER(C.c_uint)))
    return out


def reference_answers(R, mode, F):
    """the compiled reference on the same frames.  flags bit 0 (burst_interleaved_detected_): the reference negates the
    first LTS symbol on a copy before its demodulator sees it (ofdm_chirp_waveform.cpp:421-440); the recording does that
    to its input, which is the same arithmetic.  -> (llr list, aux uint32 [n, 6], snr_db float32 [n])"""
    mod, rate, nvis = MODES[mode]
    llrs, aux, snr = [], [], []
    for f in range(len(F["x"])):
        x = F["x"][f]
        if F["flags"][f] & 1:
            x = x.copy(); x[:SYM] = -x[:SYM]
        l, a, _, _ = R.rx_process(mod, rate, x, float(F["cfo"][f]), int(F["pos"][f]), nvis=nvis)
        llrs.append(l)
        aux.append(np.asarray(a[1:7], np.float32).view(np.uint32).copy())
        snr.append(a[0])
    return llrs, np.stack(aux), np.array(snr, np.float32)


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


if __name__ == "__main__":
    # the table of the pull request text: per (mode, family) the frames that took each branch at least once
    O = po.Oracle()
    print("mode family frames " + " ".join(BRANCHES) + " NaN-LLRs")
    for mode, fam in CASES:
        F = family(O, mode, fam)
        hit = (branch_counts(O, mode, F) > 0).sum(0)
        nan = sum(int(np.isnan(l).sum()) for l in oracle_answers(O, mode, F)[0])
        print(mode, fam, len(F["x"]), " ".join(str(int(h)) for h in hit), nan)
