"""Deterministic capture buffers over the input domain of the four acquisition detectors (no test functions here).

Every buffer is built from a seed through the oracle's generators (and, for Schmidl-Cox, the transmission kept in
tests/golden/cox_sync.npz), so the CPU tests, the GPU tests and oracle/gen_golden.py rebuild the same float32 bits.
tests/golden/sync_domain.npz holds the compiled reference's answers on these buffers and a sha256 per (detector, family).

A family is a dict: x list of float32 arrays (lengths differ), thr float32 [n] detection threshold, p float32 [n] (ZC and
LTS: known CFO in Hz; Cox: the noise-floor tracker before the call; chirp: unused), mask int32 [n] (ZC: root mask; Cox:
pilot layout 0 = QAM16 R1/2, 1 = DQPSK R1/4; else 0), labels [n].  An answer is float32 [n, 8]: the fields of FIELDS[det]
in order, integers converted to float32 (all are below 2^24), the rest zero.

  level      a clean and a 5 dB buffer times 1e-30 .. 1e37, and the scales that put the window energy on each side of the
             detector's denominator gate, of the overflow of energy * reference energy, and of the overflow of the energy
  silence    +0.0, -0.0, denormals, a constant, a +-c square wave, the preamble with its first part zeroed, the preamble
             followed by exact zeros
  nonfinite  one NaN / +inf / -inf before, inside, between the two parts of, after the preamble and as the last sample;
             all NaN; +-FLT_MAX singly and adjacent with opposite signs
  position   the preamble at offset 0 and 1, on and +-1 off every coarse grid, ending exactly at the buffer end, truncated by
             1 and by half; for ZC on both sides of the earlier-repetition rule (1016), for chirp late enough that the down
             window takes the time-domain path
  ties       two bit-identical preambles in a noiseless buffer, the preamble repeated periodically, one clean preamble
  threshold  ordinary buffers run again with the threshold on the correlation the oracle reports (the CPU tests pin it to
             the reference's), one float above and below, and 0, -1, 1, 2, +inf, NaN; for ZC a noise sweep that carries the
             correlation across 0.25, and a 24 kHz square wave whose correlation is below 0.01 (0.99 is out of reach of real samples:
             DESIGN.md); for Cox, whose result holds no
             metric, fixed thresholds around the plateau values 0.90 and 1.0
  meta       ZC: all 16 root masks, known CFO 0, +-23, +-100, +-1e4, NaN, +-inf; LTS: the same known CFOs; Cox: the noise
             floor at 0, a denormal, 1e-4, 5, 1e30, negative, NaN, +inf, on both pilot layouts.  The chirp detector takes
             no metadata: it has no meta family.
  weak       the preamble at -15 .. 0 dB, Gaussian noise at sigma 1e-3, 0.2, 10, a sine inside the band
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyoracle as po  # noqa: E402
from demod_domain_inputs import LEVELS, FLT_MAX, same_bits  # noqa: E402,F401

DETECTORS = ("zc", "chirp", "lts", "cox")
FAMILIES = ("level", "silence", "nonfinite", "position", "ties", "threshold", "meta", "weak")
CASES = tuple((d, f) for d in DETECTORS for f in FAMILIES if not (d == "chirp" and f == "meta"))
FIELDS = {"zc": ("detected", "frame_type", "start_sample", "correlation", "cfo_hz", "snr_estimate", "root_detected"),
          "chirp": ("success", "up_chirp_start", "down_chirp_start", "cfo_hz", "up_correlation", "down_correlation"),
          "lts": ("detected", "start_sample", "correlation", "burst_interleaved"),
          "cox": ("found", "start_sample", "cfo_hz", "noise_floor")}
THR = {"zc": 0.3, "chirp": 0.15, "lts": 0.5, "cox": 0.8}
LEN = {"zc": 4512, "chirp": 120000, "lts": 8000, "cox": 26000}            # the ordinary buffer of a detector
COX_MODES = ((po.QAM16, po.R1_2), (po.DQPSK, po.R1_4))
KNOWN_CFO = (0.0, 23.0, -23.0, 100.0, -100.0, 1e4, -1e4, np.nan, np.inf, -np.inf)
NOISE_FLOORS = (0.0, 1e-40, 1e-4, 5.0, 1e30, -1.0, np.nan, np.inf)
EDGE_THR = (0.0, -1.0, 1.0, 2.0, np.inf, np.nan)
SYM = 1152


def _seed(det, fam):
    return 770000 + 100 * DETECTORS.index(det) + FAMILIES.index(fam)


_pre = {}
_zc_default_root = 0


def preamble(O, det, which=None):
    """zc: root 1, 3, 5, 7 by `which` (default: root 1; zc_family_for_root builds a family around another root); chirp: the dual chirp; lts: two LTS symbols and the data symbols of one QAM16 R1/2
    frame at peak 0.5; cox: Schmidl-Cox preamble and frame of the reference (`which` 1: the DQPSK R1/4 preamble alone)"""
    which = (_zc_default_root if det == "zc" else 0) if which is None else which
    key = (det, which)
    if key not in _pre:
        if det == "zc":
            s = O.zc_generate((1, 3, 5, 7)[which])
        elif det == "chirp":
            s = O.chirp_generate()
        elif det == "lts":
            s, _, _ = O.tx_frame(po.QAM16, po.R1_2, np.random.default_rng(770900).integers(0, 256, 141, dtype=np.uint8), 7)
            s = s * np.float32(0.5 / np.abs(s).max())
        else:
            g = np.load(os.path.join(ROOT, "tests", "golden", "cox_sync.npz"))
            s = g["preamble_dqpsk_r14"] if which else g["tx"]
        _pre[key] = np.ascontiguousarray(s, np.float32)
    return _pre[key].copy()


# the part of the preamble a detector cannot do without (what `position` counts as "a whole preamble") and its two parts
CORE = {"zc": 2 * 1016, "chirp": 24000 + 4800 + 24000, "lts": 3 * SYM, "cox": 8 * SYM}
PARTS = {"zc": (1016, 1016), "chirp": (24000, 28800), "lts": (SYM, SYM), "cox": (4 * SYM, 4 * SYM)}   # (length of part 1, start of part 2)


def place(pre, n, off, rng=None, snr_db=None):
    """the preamble at `off` in exact zeros (cut at the buffer end), plus Gaussian noise `snr_db` below the preamble's rms"""
    x = np.zeros(n, np.float64)
    seg = pre[:max(0, min(len(pre), n - off))]
    x[off:off + len(seg)] = seg
    if snr_db is not None:
        rms = np.sqrt(np.mean(pre[pre != 0].astype(np.float64) ** 2))
        x += rng.normal(0, rms * 10 ** (-snr_db / 20.0), n)
    return x.astype(np.float32)


class _Fam:
    def __init__(self, det):
        self.det, self.x, self.thr, self.p, self.mask, self.labels = det, [], [], [], [], []

    def add(self, x, label, thr=None, p=0.0, mask=None):
        with np.errstate(over="ignore", invalid="ignore"):
            self.x.append(np.ascontiguousarray(np.asarray(x).astype(np.float32)))
        self.thr.append(THR[self.det] if thr is None else thr)
        self.p.append(p)
        self.mask.append((15 if self.det == "zc" else 0) if mask is None else mask)
        self.labels.append(label)

    def done(self):
        return {"x": self.x, "thr": np.array(self.thr, np.float32), "p": np.array(self.p, np.float32),
                "mask": np.array(self.mask, np.int32), "labels": list(self.labels)}


def _bases(O, det, rng):
    """[clean, 5 dB] ordinary buffers with the preamble inside"""
    pre, n = preamble(O, det), LEN[det]
    off = {"zc": 715, "chirp": 9000, "lts": 1500, "cox": 300}[det]
    return [place(pre, n, off), place(pre, n, off, rng, 5.0)], off


def gate_scales(det, x, off):
    """amplitude scales that put the energy of the detector's correlation window at the preamble on each side of: the
    denominator gate, the overflow of energy times reference energy, the overflow of the energy itself (estimated in double
    from the samples; a factor 2 in amplitude on either side covers the estimate's error)"""
    win, ref_e, gate = {"zc": (1016, 1016.0, 1e-20), "chirp": (24000, 12000.0, 1e-20), "lts": (SYM, None, 1e-10),
                        "cox": (512, None, 1e-10)}[det]
    at = off + (3 * SYM if det == "cox" else 0)                       # the Cox transmission opens with a silent guard
    e0 = float(np.sum(x[at:at + win].astype(np.float64) ** 2)) * (1.0 if ref_e else 2.0)   # analytic signal: twice
    flt_max = float(FLT_MAX)
    targets = ((("denominator gate", gate / ref_e), ("energy x reference overflow", flt_max / ref_e), ("energy overflow", flt_max))
               if ref_e else (("denominator gate", gate), ("energy product overflow", np.sqrt(flt_max)), ("energy overflow", flt_max)))
    return [(name, side, float(np.float32(np.sqrt(t / e0) * k))) for name, t in targets for side, k in (("below", 0.5), ("above", 2.0))]


def level(O, det, rng):
    F = _Fam(det)
    bases, off = _bases(O, det, rng)
    for b, x in enumerate(bases):
        few = det == "chirp" and b == 1
        for s in ((1e-30, 1e-8, 1e19, 1e37) if few else LEVELS):
            F.add(x * np.float32(s), f"base{b} x {s:g}")
        if not few:
            F.add(x, f"base{b} x 1")
            for name, side, s in gate_scales(det, x, off):
                F.add(x * np.float32(s), f"base{b} x {s:.6g} ({side} the {name})")
    return F.done()


def _zero_first(det, pre):
    y = pre.copy(); y[:PARTS[det][0]] = 0
    return y


def silence(O, det, rng):
    F = _Fam(det)
    pre, n = preamble(O, det), LEN[det]
    F.add(np.zeros(n, np.float32), "+0.0")
    F.add(np.full(n, -0.0, np.float32), "-0.0")
    den = (rng.integers(1, 1 << 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)).view(np.float32)
    F.add(den, "denormals")
    F.add(np.full(n, 0.25, np.float32), "constant 0.25")
    F.add(np.where(np.arange(n) % 32 < 16, 0.25, -0.25), "square wave +-0.25, period 32")
    off = {"zc": 715, "chirp": 9000, "lts": 1500, "cox": 300}[det]
    F.add(place(_zero_first(det, pre), n, off), "first part zeroed, noiseless")
    F.add(place(_zero_first(det, pre), n, off, rng, 20.0), "first part zeroed, 20 dB")
    F.add(place(pre[:CORE[det]], n, off), "preamble followed by exact zeros")
    y = place(pre, n, off, rng, 20.0); y[off + CORE[det]:] = 0
    F.add(y, "20 dB, exact zeros after the preamble")
    return F.done()


def nonfinite(O, det, rng):
    F = _Fam(det)
    pre, n = preamble(O, det), LEN[det]
    off = {"zc": 715, "chirp": 9000, "lts": 1500, "cox": 300}[det]
    x = place(pre, n, off, rng, 20.0)
    l1, s2 = PARTS[det]
    places = (("before", off // 2), ("in part 1", off + l1 // 3), ("between the parts", off + (l1 + s2) // 2 if s2 > l1 else off + l1),
              ("in part 2", off + s2 + l1 // 2), ("after", min(n - 2, off + CORE[det] + 100)), ("last sample", n - 1))
    for name, v in (("NaN", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
        for where, i in places:
            y = x.copy(); y[i] = v
            F.add(y, f"{name} {where}")
    F.add(np.full(n, np.nan, np.float32), "all NaN")
    for name, v in (("+FLT_MAX", FLT_MAX), ("-FLT_MAX", -FLT_MAX)):
        for where, i in (places[1], places[4]):
            y = x.copy(); y[i] = v
            F.add(y, f"{name} {where}")
    y = x.copy(); y[off + l1 // 3] = FLT_MAX; y[off + l1 // 3 + 1] = -FLT_MAX
    F.add(y, "+FLT_MAX next to -FLT_MAX in part 1")
    if det == "zc":
        # 16 samples off the coarse grid the peak stays below 0.25, so the two repetitions are combined: an infinity in the second
        # makes the combined metric NaN, and std::max(combined, peak) keeps it (zc_sync.hpp:289)
        weak = place(pre, n, 700, rng, 20.0)
        for name, v in (("+inf", np.inf), ("-inf", -np.inf)):
            for where, k in (("at the start of", 700 + 1016), ("in the middle of", 700 + 1016 + 508)):
                y = weak.copy(); y[k] = v
                F.add(y, f"preamble at 700 (off the grid), {name} {where} the second repetition")
    if det == "chirp":
        # The transform of the up search reads the first 131072 samples, so a non-finite sample behind them leaves the up chirp
        # found; with the up chirp at 85000 the down window (97000 .. 140000) takes the time-domain path, whose block arg-max
        # then meets NaN correlations: inside the down chirp (nothing left to find) and behind it (the down chirp is still found)
        late = place(pre, 140000, 85000, rng, 20.0)
        for name, v in (("NaN", np.nan), ("+inf", np.inf), ("+FLT_MAX", FLT_MAX)):
            for where, k in (("in the down chirp", 132000), ("behind the down chirp", 139000)):
                y = late.copy(); y[k] = v
                F.add(y, f"length 140000, chirp at 85000, {name} {where}")
    return F.done()


def position_offsets(det, n, plen):
    end = n - plen
    if det == "zc":      # coarse step 31; the earlier-repetition rule looks at peak >= 1016
        return [0, 1, 30, 31, 32, 61, 62, 63, 1015, 1016, 1017, end, end + 1, n - plen // 2]
    if det == "chirp":   # off > 60000: down window shorter than 48000 samples -> time-domain path with its grid of 48
        return [0, 1, 47, 48, 49, 30000, 60001, end, end + 1, end + 4800, end + 4801, n - plen // 2]
    if det == "lts":     # coarse step 8
        return [0, 1, 7, 8, 9, 15, 16, 17, 1000, end, end + 1, n - plen // 2]
    return [0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 5000, end, end + 1, n - plen // 2]   # cox: 64 and 8


def position(O, det, rng):
    """-> family with an extra key `whole` bool [n]: the buffer holds the whole CORE of the preamble"""
    F = _Fam(det)
    whole = []
    lens = {"zc": (4512, 1016, 2512, 16384, 16385), "chirp": (120000, 52800, 57600, 62400), "lts": (8000, 3456, 21000), "cox": (26000, 9216, 12000)}[det]
    for n in lens:
        pre = preamble(O, det)
        if det in ("lts", "cox") and n < 20000:
            pre = pre[:CORE[det]]
        if len(pre) > n:                       # ZC 1016: one repetition; chirp 52800: both chirps without the trailing gap
            pre = pre[:n]
        offs = position_offsets(det, n, len(pre)) if n == lens[0] else [o for o in (0, 1, (n - len(pre)) // 2, n - len(pre)) if o >= 0]
        for k, off in enumerate(sorted(set(offs))):
            if off < 0 or off >= n:
                continue
            F.add(place(pre, n, off, rng, (None, 15.0)[k % 2]), f"length {n}, preamble at {off}, " + ("noiseless", "15 dB")[k % 2])
            whole.append(off + min(CORE[det], len(pre)) <= n)
    if det == "zc":   # the workspace form
        F.add(place(preamble(O, det), 31120, 20011, rng, 15.0), "length 31120, preamble at 20011, 15 dB"); whole.append(True)
    if det == "chirp":   # above the FFT size: the reference clamps the transform input to 131072 samples
        F.add(place(preamble(O, det), 140000, 3000, rng, 15.0), "length 140000, preamble at 3000, 15 dB"); whole.append(True)
    if det == "cox":
        F.add(place(preamble(O, det), 240000, 150000, rng, 25.0), "length 240000, preamble at 150000, 25 dB"); whole.append(True)
    out = F.done()
    out["whole"] = np.array(whole, bool)
    return out


def ties(O, det, rng):
    F = _Fam(det)
    pre, n = preamble(O, det), {"zc": 8000, "chirp": 131000, "lts": 21000, "cox": 26000}[det]
    core = pre[:CORE[det]] if det in ("lts", "cox") else pre
    gap = {"zc": 3100, "chirp": 60000, "lts": 8 * SYM + 5, "cox": 10 * SYM + 3}[det]
    x = place(core, n, 200); x += place(core, n, 200 + gap)
    F.add(x, f"two identical preambles {gap} apart, noiseless")
    F.add(np.tile(core, n // len(core) + 1)[:n], "the preamble repeated periodically")
    F.add(place(core, n, 0), "one clean preamble at 0")
    F.add(place(core, n, 200), "one clean preamble at 200")
    if det == "zc":
        F.add(np.tile(pre[:1016], 8)[:8000], "one repetition repeated without a gap")
    if det == "lts":   # period 40 (5 coarse steps, no divisor of 1152): every fifth offset sees the same samples, below 0.95
        F.add(np.tile(rng.normal(0, 0.2, 40), n // 40 + 1)[:n], "a random pattern of period 40")
    if det == "chirp":
        F.add(np.where(np.arange(n) % 32 < 16, 0.25, -0.25), "square wave +-0.25, period 32")
        F.add(np.tile(rng.normal(0, 0.2, 64), n // 64 + 1)[:n], "a random pattern of period 64")
    return F.done()


def _call(C, det, x, thr, p, mask):
    """one detector call on the oracle or the reference -> float32 [8]"""
    out = np.zeros(8, np.float32)
    if det == "zc":
        out[:7] = C.zc_detect(x, float(thr), int(mask), float(p))
    elif det == "chirp":
        out[:6] = C.chirp_detect(x, float(thr))
    elif det == "lts":
        out[:4] = C.detect_data_sync(x, float(p), float(thr))
    else:
        o3, nf = C.cox_search(x, float(thr), float(p), *COX_MODES[int(mask)])
        out[:3] = o3; out[3] = nf
    return out


def zc_mixed_first_repetition(O, g):
    """root 1's preamble whose first repetition is g times itself plus (1 - g) times root 5's, noiseless, the second repetition
    on the coarse grid: the peak is the second repetition, the earlier one correlates less the smaller g is"""
    a, b = preamble(O, "zc", 0), preamble(O, "zc", 2)
    y = a.astype(np.float64)
    y[:1016] = g * a[:1016] + (1.0 - g) * b[:1016]
    return place(y.astype(np.float32), LEN["zc"], 1123)


def zc_earlier_ratio_gains(O):
    """searched with the oracle's own counter: the largest g found whose earlier repetition stays at or below 0.4 of the peak
    and the smallest found above it (bisection to neighbouring doubles or 40 steps), and one on either side further out"""
    def taken(g):
        O.zc_detect(zc_mixed_first_repetition(O, g), THR["zc"], 1, 0.0)
        c = sync_branch_counts_last(O)
        assert c[BRANCHES.index("ZC_EARLIER_T")] + c[BRANCHES.index("ZC_EARLIER_F")] == 1, "the peak is not the second repetition"
        return c[BRANCHES.index("ZC_EARLIER_T")] == 1
    lo, hi = 0.0, 1.0
    assert not taken(lo) and taken(hi)
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if taken(mid):
            hi = mid
        else:
            lo = mid
    return [(0.5 * lo, "below"), (lo, "below"), (hi, "above"), (0.5 * (hi + 1.0), "above")]


def threshold(O, det, rng):
    F = _Fam(det)
    pre, n = preamble(O, det), LEN[det]
    off = {"zc": 1117, "chirp": 20000, "lts": 1700, "cox": 900}[det]
    bufs = [(place(pre, n, off, rng, snr), f"{snr:g} dB") for snr in ((3.0, -6.0, 20.0) if det != "cox" else (25.0, 12.0))]
    if det == "chirp":   # the down window's time-domain path compares with >= and with 0.3 x threshold
        bufs.append((place(pre, n, 62000, rng, 6.0), "6 dB, late"))
    for x, name in bufs:
        if det == "cox":
            one = np.float32(1.0)
            ths = [0.5, 0.8, np.nextafter(np.float32(0.9), np.float32(0)), np.float32(0.9), np.nextafter(np.float32(0.9), one), 0.95, 0.99,
                   np.nextafter(one, np.float32(0)), one, np.nextafter(one, np.float32(2))]
        else:
            # LTS refines (and raises) the correlation only once the coarse maximum has passed the threshold: the compare is
            # on the coarse maximum, which a run that cannot detect (threshold 2) reports
            r = _call(O, det, x, 2.0 if det == "lts" else THR[det], 0.0, 15 if det == "zc" else 0)
            ths = []
            for c in {"zc": (r[3],), "chirp": (r[4], r[5]), "lts": (r[2],)}[det]:
                c = np.float32(c)
                ths += [np.nextafter(c, np.float32(-1)), c, np.nextafter(c, np.float32(2))]
            if det == "chirp":
                c = np.float32(r[5])   # best < threshold * 0.3f on the coarse grid of the time-domain path
                ths += [np.float32(c / np.float32(0.3)), np.float32(c / np.float32(0.3)) * np.float32(1.001)]
        for t in ths:
            F.add(x, f"{name}, threshold {float(t)!r}", thr=t)
        for t in EDGE_THR:
            F.add(x, f"{name}, threshold {t!r}", thr=t)
    if det == "zc":
        for snr in (-25.0, -21.0, -18.0, -15.0, -12.0, -9.0, -6.0, 10.0, 45.0):
            F.add(place(pre, n, off, rng, snr), f"{snr:g} dB, threshold 0.05", thr=0.05)
        F.add(place(pre, n, off), "noiseless, threshold 0.05", thr=0.05)
        for g, side in zc_earlier_ratio_gains(O):
            F.add(zc_mixed_first_repetition(O, g), f"first repetition {g!r} root 1 + rest root 5: earlier repetition {side} 0.4 of the peak", mask=1)
        F.add(np.full(n, 0.25, np.float32), "constant 0.25, threshold 0", thr=0.0)
        F.add(np.full(n, 0.25, np.float32), "constant 0.25, threshold -1", thr=-1.0)
        F.add(np.where(np.arange(n) % 2 == 0, 0.25, -0.25), "alternating +-0.25 (24 kHz), threshold 0", thr=0.0)
    return F.done()


def meta(O, det, rng):
    F = _Fam(det)
    n = LEN[det]
    if det == "zc":
        bufs = [place(preamble(O, det, r), n, (311, 715, 1116, 1522)[r], rng, 10.0) for r in range(4)]   # on the grid of 31: +1, +2, +0, +3
        for m in range(16):
            F.add(bufs[m % 4], f"root {2 * (m % 4) + 1}, mask {m}", mask=m)
        for k, cfo in enumerate(KNOWN_CFO):
            F.add(bufs[k % 4], f"root {2 * (k % 4) + 1}, known CFO {cfo!r}", p=cfo)
        two = place(preamble(O, det, 0), 8000, 94) + place(preamble(O, det, 2), 8000, 4000)
        for m in (15, 1, 4, 10):
            F.add(two, f"roots 1 and 5 in one buffer, mask {m}", mask=m)
    elif det == "lts":
        pre = preamble(O, det)
        neg = pre.copy(); neg[:SYM] = -neg[:SYM]
        for k, cfo in enumerate(KNOWN_CFO):
            F.add(place((pre, neg)[k % 2], n, 1200 + 3 * k, rng, 20.0), ("", "first LTS negated, ")[k % 2] + f"known CFO {cfo!r}", p=cfo)
    else:
        for layout in (0, 1):
            pre = preamble(O, det, layout)
            for k, nf in enumerate(NOISE_FLOORS):
                F.add(place(pre, n, 2000 + 11 * k, rng, 25.0), f"layout {layout}, noise floor {nf!r}", p=nf, mask=layout)
    return F.done()


def weak(O, det, rng):
    F = _Fam(det)
    pre, n = preamble(O, det), LEN[det]
    off = {"zc": 900, "chirp": 15000, "lts": 1300, "cox": 1000}[det]
    for snr in (-15.0, -10.0, -5.0, 0.0):
        F.add(place(pre, n, off, rng, snr), f"{snr:g} dB")
    for sigma in (1e-3, 0.2, 10.0):
        F.add(rng.normal(0, sigma, n), f"noise sigma {sigma:g}")
    F.add(0.3 * np.sin(2 * np.pi * 1400.0 * np.arange(n) / 48000.0 + 0.3), "sine at 1400 Hz")
    return F.done()


_BUILDERS = {"level": level, "silence": silence, "nonfinite": nonfinite, "position": position, "ties": ties,
             "threshold": threshold, "meta": meta, "weak": weak}
_cache = {}


def family(O, det, name):
    key = (det, name)
    if key not in _cache:
        _cache[key] = _BUILDERS[name](O, det, np.random.default_rng(_seed(det, name)))
    return _cache[key]


def zc_family_for_root(O, name, which):
    """a ZC family built the same way (same seed) around another root's preamble: the acquire batches search for the DATA
    and CONTROL roots only (5 and 7), so the composed-path tests use root 5.  Not recorded: those tests compare with the
    separate call and the restatements."""
    global _zc_default_root
    key = ("zc", name, which)
    if key not in _cache:
        _zc_default_root = which
        try:
            _cache[key] = _BUILDERS[name](O, "zc", np.random.default_rng(_seed("zc", name)))
        finally:
            _zc_default_root = 0
    return _cache[key]


def digest(F):
    """sha256 over the sample bits, lengths and the metadata of a family"""
    h = hashlib.sha256()
    for x in F["x"]:
        h.update(np.int64(len(x)).tobytes()); h.update(x.tobytes())
    for k in ("thr", "p", "mask"):
        h.update(np.ascontiguousarray(F[k]).tobytes())
    return h.hexdigest()


def answers(C, det, F):
    """the oracle's (pyoracle.Oracle) or the compiled reference's (pyoracle.Ref) answers -> float32 [n, 8]"""
    return np.stack([_call(C, det, F["x"][i], F["thr"][i], F["p"][i], F["mask"][i]) for i in range(len(F["x"]))])


def expected_fields(det, F, ans):
    """the answer of a buffer as the result struct holds it -> float32 [n, nf + 1]: FIELDS[det], then (LTS) cfo_hz = known"""
    nf = len(FIELDS[det])
    return np.concatenate([ans[:, :nf], F["p"][:, None]], axis=1) if det == "lts" else ans[:, :nf].copy()


def groups(F):
    """buffer indices grouped into batch calls: same length, threshold bits and mask"""
    g = {}
    for i, x in enumerate(F["x"]):
        g.setdefault((len(x), int(F["thr"][i:i + 1].view(np.uint32)[0]), int(F["mask"][i])), []).append(i)
    return list(g.values())


_PAIRS = ("ZC_DENOM", "ZC_PEAK", "ZC_EARLIER", "ZC_COMBINE", "ZC_CFO_OK", "ZC_DETECT", "ZC_SNR_LOW", "ZC_SNR_HIGH",
          "CH_FFT", "CH_DENOM", "CH_THR", "CH_TD_DENOM", "CH_TD_COARSE", "CH_TD_THR", "CH_CFO_REJ",
          "LTS_NOISE", "LTS_ENERGY", "LTS_EXIT", "LTS_DETECT", "LTS_MARKER",
          "COX_NF_INIT", "COX_ENERGY", "COX_NORM", "COX_THR", "COX_PLATEAU", "COX_RULE", "COX_LTS_NORM", "COX_EARLIER_LTS", "COX_CONFIRM")
BRANCHES = tuple(f"{n}_{tf}" for n in _PAIRS for tf in "TF") + ("ZC_TIE", "CH_TIE", "LTS_TIE", "COX_TIE")   # RO_SBC_* of oracle/ria_oracle.h
PREFIX = {"zc": "ZC_", "chirp": "CH_", "lts": "LTS_", "cox": "COX_"}


def sync_branch_counts_last(O):
    """the counters of the oracle's last detector call on this thread -> uint32 [len(BRANCHES)]"""
    import ctypes as C
    assert O.lib.ro_sync_branch_n() == len(BRANCHES)
    out = np.zeros(len(BRANCHES), np.uint32)
    O.lib.ro_sync_branch_counts(out.ctypes.data_as(C.POINTER(C.c_uint)))
    return out


def branch_counts(O, det, F):
    """how often the oracle found each data-dependent condition of the detector true / false on every buffer
    -> uint32 [n, len(BRANCHES)]"""
    out = np.zeros((len(F["x"]), len(BRANCHES)), np.uint32)
    for i in range(len(F["x"])):
        _call(O, det, F["x"][i], F["thr"][i], F["p"][i], F["mask"][i])
        out[i] = sync_branch_counts_last(O)
    return out


if __name__ == "__main__":
    # the table of DESIGN.md: per (detector, family) the buffers on which each condition was true / false at least once
    O = po.Oracle()
    for det in DETECTORS:
        cols = [i for i, b in enumerate(BRANCHES) if b.startswith(PREFIX[det])]
        names = sorted({BRANCHES[i].rsplit("_", 1)[0] for i in cols if not BRANCHES[i].endswith("_TIE")}, key=lambda n: BRANCHES.index(n + "_T"))
        print("| family | buffers | " + " | ".join(n[len(PREFIX[det]):] for n in names) + " | TIE |")
        print("|---" * (len(names) + 3) + "|")
        tot = np.zeros(len(BRANCHES), np.int64)
        for fam in FAMILIES:
            if (det, fam) not in CASES:
                continue
            F = family(O, det, fam)
            hit = (branch_counts(O, det, F) > 0).sum(0)
            tot += hit
            print(f"| {det} {fam} | {len(F['x'])} | " + " | ".join(f"{hit[BRANCHES.index(n + '_T')]} / {hit[BRANCHES.index(n + '_F')]}" for n in names) +
                  f" | {hit[BRANCHES.index(PREFIX[det] + 'TIE')]} |")
        print(f"| {det} all | | " + " | ".join(f"{tot[BRANCHES.index(n + '_T')]} / {tot[BRANCHES.index(n + '_F')]}" for n in names) +
              f" | {tot[BRANCHES.index(PREFIX[det] + 'TIE')]} |")
        print()

