"""Deterministic inputs of the reference-identical channel (ria_gpu_channel_exact_batch, _seeded_batch, _cfo_batch) and of
the transmitter frequency offset (ria_gpu_tx_cfo_batch) over their input domain (no test functions here).

Everything comes from fixed numpy seeds, so the CPU tests, the GPU tests and oracle/gen_golden.py rebuild the same rows;
tests/golden/channel_domain.npz holds a sha256 over all rows and the compiled reference's answers for a short subset.

A row is a dict.  Channel rows: family, label, kind (0 awgn, 1 good, 2 moderate, 3 poor, 4 flutter), snr, seed, x float32 [n],
call ("plain": WattersonChannel through ref_channel; "cfo": with Config::cfo_hz = cfo and random_cfo_max_hz = rmax), cls.
tx_cfo rows: family, label, x, cfo, phase (float32 accumulator before the call, None: the NULL accumulator), cls.
cls says what the expected output looks like (tests/test_channel_domain_cpu.py asserts it on the reference's answers):
  finite      no NaN in it
  nonfinite   no finite sample in it
  tail        (channel + CFO with an infinite or NaN offset) sample 0 is rotated by the phase 0 and is finite; the phase is
              infinite from sample 1 on and every later sample is NaN
  nan1        one NaN input sample at row["nan_at"]: NaNs exactly there and, with multipath, delay + 1 samples later
  nan_cfo     the same under applyCFO, whose running sums carry the NaN on: no NaN before nan_at
  nan_sample  tx_cfo on a buffer with a NaN or infinite sample: no finite sample (outside bit identity, see include/ria_gpu.h)
  any         nothing stated (compared bit for bit all the same)

channel families
  lengths   white non-zero samples at 0.3 rms, n around the 64-sample tile, the 128-entry history, the delay lines of
            delay + 1 = 25, 49, 97 samples (DELAYS, derived from the presets), the 48-tap sum and the 256-sample applyCFO gate;
            one impulse row (only sample 0 is non-zero) per preset at 800 dB, where the noise is denormal
  levels    the |x| > 1e-6 power gate at its threshold, silence (rms = 0.1), denormals, signed zeros, squares that overflow,
            infinite samples, one NaN sample
  snr       SNRS on one 300-sample frame
  seeds     SEEDS for the seeded call; the effective seeds of the plain call's wrap-around cases
  batch     130 frames of 70 samples per preset (taken as batches of 1, 63, 64, 65, 130) and 4097 frames of 8 samples
  stride    frames the layouts are tried on
  cfo       CFOS at n = 320 (every preset) and n = 255 (below the applyCFO gate); lengths 256 .. 600; a NaN sample under CFO
  random    random_cfo_max_hz values with a configured offset that the draw replaces
  bench     three 18 432-sample QAM16 R1/2 frames at peak 0.8, moderate, 20 dB
tx_cfo families
  lengths, offsets (CFOS), accumulators (PHASES), continue, chunks (distinct buffers the GPU test tiles), samples, nonfinite
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import pyoracle as po  # noqa: E402

F = np.float32
KINDS = (0, 1, 2, 3, 4)
KIND_NAMES = ("awgn", "good", "moderate", "poor", "flutter")
DELAY_MS = (0.0, 0.5, 1.0, 2.0, 0.5)                              # hf_channel.hpp:411-488
DELAY = tuple(int(F(ms) * 48000 / F(1000.0)) for ms in DELAY_MS)  # delay_samples_ (:74-76); the line holds delay + 1 samples
DELAYS = sorted({d for d in DELAY if d > 0})                      # 24, 48, 96
NAN, INF = float("nan"), float("inf")
FLT_MAX = float(np.finfo(np.float32).max)
GATE = F(1e-6)                                                    # process() :116
CFO_GATE = F(0.001)                                               # process() :172 (> gate applies) and applyTxCFO :299 (< gate copies)
PI_F = F(np.pi)
SENTINEL = np.array([0x7fc0dead], np.uint32).view(np.float32)[0]  # padding of the strided layouts: a NaN with a payload

LENGTHS = sorted({1, 2, 24, 25, 26, 47, 48, 49, 50, 63, 64, 65, 96, 97, 98, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 321, 575, 577}
                 | {d + k for d in DELAYS for k in (0, 1, 2)})
SNRS = (-300.0, -40.0, -0.0, 0.0, 3.01, 60.0, 200.0, 800.0, 1e30, INF, -INF, NAN)
SEEDS = (0, 1, 42, 5489, 0x7fffffff, 0x80000000, 0xffffffff)
WRAP = ((0xfffffffe, 0, 3), (1000, 2 ** 32 + 5, 3), (1000, 5, 3))  # (seed, first_frame, n_frames) of the plain call
BATCHES = (1, 63, 64, 65, 130)
GROW = 4097
STRIDE_EXTRA = (1, 7, 64)
CFOS = (0.0, -0.0, float(CFO_GATE), -float(CFO_GATE), float(np.nextafter(CFO_GATE, F(1))), float(np.nextafter(CFO_GATE, F(0))),
        0.5, -0.5, 12.5, -12.5, 50.0, -50.0, 2400.0, -2400.0, 24000.0, -24000.0, 48000.5, -48000.5, 1e6, -1e6, 1e38, INF, -INF, NAN)
CFO_LENGTHS = (256, 257, 303, 304, 320, 600)
RANDOM_MAX = (float(np.finfo(np.float32).smallest_subnormal), 1e-3, 0.5, 50.0, 1e30, FLT_MAX, INF)
TXCFO_LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097)
TXCFO_MAX = 131072
PHASES = (0.0, float(PI_F), -float(PI_F), float(np.nextafter(PI_F, F(4))), float(np.nextafter(PI_F, F(0))),
          float(np.nextafter(-PI_F, F(-4))), float(np.nextafter(-PI_F, F(0))), 3.2, -3.2, 100.0, -100.0, 1e9, NAN, INF)
CHUNK_BUFFERS = 32768                                             # buffers of one pass of ria_gpu_tx_cfo_batch (the grid's y extent)
CHUNK_BYTES = 256 << 20                                           # workspace of one pass


def txcfo_chunk(n, n_buffers):
    """buffers per pass of ria_gpu_tx_cfo_batch, from the rule its comment states: two complex arrays of N = 2^ceil(log2 n)
    and one float per sample for every buffer, a pass stays under 256 MiB and 32 768 buffers"""
    N = 1
    while N < n:
        N <<= 1
    per = 2 * N * 8 + n * 4
    return min(n_buffers, CHUNK_BUFFERS, max(1, CHUNK_BYTES // per))


def _name(v):
    return f"{float(v)!r}[{word(v):#010x}]"


def _white(rng, n, rms=0.3):
    x = (rng.standard_normal(n) * rms).astype(np.float32)
    x[np.abs(x) <= F(1e-3)] = F(rms)                              # non-zero and well above the power gate
    return x


def _ch(family, label, kind, x, snr=20.0, seed=1, call="plain", cfo=0.0, rmax=0.0, cls="finite", **kw):
    r = {"family": family, "label": f"{label} {KIND_NAMES[kind]}", "kind": kind, "snr": float(snr), "seed": int(seed) & 0xffffffff,
         "x": np.ascontiguousarray(x, np.float32), "call": call, "cfo": float(cfo), "rmax": float(rmax), "cls": cls}
    r.update(kw)
    return r


def _offset_cls(cfo, n):
    """what an offset does to a channel row of n samples"""
    if n < 256 or not abs(F(cfo)) > CFO_GATE:                     # NaN: the compare is false, applyCFO does not run
        return "finite"
    return "finite" if np.isfinite(cfo) else "tail"


# ---------------------------------------------------------------------------------------------- channel rows
def channel_rows(O):
    rows = []
    rng = np.random.default_rng(20261020)
    for kind in KINDS:
        # lengths
        for n in LENGTHS:
            rows.append(_ch("lengths", f"n {n}", kind, _white(rng, n), seed=3000 + n))
        imp = np.zeros(130, np.float32)
        imp[0] = 0.75
        rows.append(_ch("lengths", "impulse at 0", kind, imp, snr=800.0, seed=77, impulse=True))
        # levels, 300 samples each
        n = 300
        w = _white(rng, n)
        up, dn = np.nextafter(GATE, F(1)), np.nextafter(GATE, F(0))
        sgn = np.where(np.arange(n) % 3 == 0, F(-1), F(1)).astype(np.float32)
        lv = [("all zero", np.zeros(n, np.float32), "finite"),
              ("+-1e-6f exactly (not counted)", sgn * GATE, "finite"),
              ("nextafter(1e-6f, 1) (counted)", sgn * up, "finite"),
              ("nextafter(1e-6f, 0) (not counted)", sgn * dn, "finite"),
              ("denormals", sgn * F(1e-40), "finite"),
              ("signed zeros", sgn * F(0.0), "finite")]
        one = np.zeros(n, np.float32); one[100] = 0.5
        lv.append(("one counted sample among zeros", one, "finite"))
        sil = np.zeros(n, np.float32); sil[100:200] = w[100:200]
        lv.append(("leading and trailing silence", sil, "finite"))
        mix = w.copy(); mix[::7] = GATE; mix[1::7] = -up; mix[2::7] = dn
        lv.append(("white with threshold values", mix, "finite"))
        for v, c in ((1e19, "finite"), (3e19, "nonfinite"), (FLT_MAX, "nonfinite"), (INF, "nonfinite"), (-INF, "nonfinite")):
            b = w.copy(); b[7] = v
            lv.append((f"one sample {v!r}", b, c))
        for lab, x, c in lv:
            rows.append(_ch("levels", lab, kind, x, seed=4100 + kind, cls=c))
        nn = max(300, 10 * (DELAY[kind] + 2))                       # the NaN in the last tenth and its delayed copy inside the row
        b = _white(rng, nn); b[nn * 9 // 10] = NAN
        rows.append(_ch("levels", f"one NaN sample at {nn * 9 // 10} of {nn}", kind, b, seed=4100 + kind, cls="nan1", nan_at=nn * 9 // 10))
        # snr
        ws = _white(rng, 300)
        for snr in SNRS:
            c = "nonfinite" if (np.isnan(snr) or snr == -INF) else "finite"
            rows.append(_ch("snr", f"snr {_name(snr)}", kind, ws, snr=snr, seed=4200 + kind, cls=c))
        # seeds: 130 samples of a fading preset draw 650 normals, more than one twist of the generator gives
        wd = _white(rng, 130)
        eff = list(SEEDS) + [(s + ff + f) & 0xffffffff for s, ff, nf in WRAP for f in range(nf)]
        for s in sorted(set(eff)):
            rows.append(_ch("seeds", f"seed {s:#010x}", kind, wd, seed=s))
        # batch: distinct contents and seeds
        for f in range(max(BATCHES)):
            rows.append(_ch("batch", f"frame {f}", kind, _white(rng, 70), snr=15.0, seed=(0x9e3779b9 * (f + 1) + kind) & 0xffffffff))
        # stride
        for f in range(3):
            rows.append(_ch("stride", f"n 70 frame {f}", kind, _white(rng, 70), seed=5000 + f))
            rows.append(_ch("stride", f"n 300 frame {f} cfo", kind, _white(rng, 300), seed=5100 + f, call="cfo", cfo=(50.0, -12.5, 0.0005)[f]))
        # cfo
        wc = {n: _white(rng, n) for n in CFO_LENGTHS + (255,)}
        for cfo in CFOS:
            rows.append(_ch("cfo", f"n 320 cfo {_name(cfo)}", kind, wc[320], seed=6000 + kind, call="cfo", cfo=cfo, cls=_offset_cls(cfo, 320)))
            if kind in (0, 2):
                rows.append(_ch("cfo", f"n 255 cfo {_name(cfo)}", kind, wc[255], seed=6000 + kind, call="cfo", cfo=cfo, cls="finite"))
        for n in CFO_LENGTHS:
            if n == 320:
                continue
            for cfo in (50.0, -50.0, 48000.5, -1e6, float(CFO_GATE), float(np.nextafter(CFO_GATE, F(1)))):
                rows.append(_ch("cfo", f"n {n} cfo {_name(cfo)}", kind, wc[n], seed=6100 + n, call="cfo", cfo=cfo))
        b = wc[600].copy(); b[560] = NAN
        rows.append(_ch("cfo", "n 600 cfo 50 one NaN sample at 560", kind, b, seed=6200, call="cfo", cfo=50.0, cls="nan_cfo", nan_at=560))
        # random cfo: the draw replaces the configured 25 Hz
        if kind in (0, 2):
            for n in (255, 320):
                for rmax in RANDOM_MAX:
                    c = "finite" if (n < 256 or rmax <= 50.0) else "any"
                    rows.append(_ch("random", f"n {n} max {_name(rmax)}", kind, wc[n], seed=6300 + n, call="cfo", cfo=25.0, rmax=rmax, cls=c))
    # workspace growth: 4097 frames of 8 samples from 16 distinct contents, every frame its own seed
    base = [_white(rng, 8) for _ in range(16)]
    for f in range(GROW):
        rows.append(_ch("grow", f"frame {f}", 2, base[f % 16], snr=12.0, seed=(2654435761 * (f + 1)) & 0xffffffff))
    # bench shape
    for f in range(3):
        s, _, _ = O.tx_frame(po.QAM16, po.R1_2, rng.integers(0, 256, 141, dtype=np.uint8), f)
        x = (s * np.float32(0.8 / np.abs(s).max())).astype(np.float32)
        if f == 1:
            x[:700] = 0.0
        rows.append(_ch("bench", f"frame {f}" + (" with 700 leading zeros" if f == 1 else ""), 2, x, snr=20.0, seed=7000 + f))
    return rows


# ---------------------------------------------------------------------------------------------- tx_cfo rows
def _tx(family, label, x, cfo, phase=0.0, cls="finite", **kw):
    r = {"family": family, "label": label, "x": np.ascontiguousarray(x, np.float32), "cfo": float(cfo),
         "phase": None if phase is None else float(F(phase)), "cls": cls}
    r.update(kw)
    return r


def tx_active(cfo):
    """applyTxCFO :299 rotates unless |cfo| < 0.001f (a NaN offset rotates)"""
    return not abs(F(cfo)) < CFO_GATE


def txcfo_rows():
    rows = []
    rng = np.random.default_rng(20261021)
    for n in TXCFO_LENGTHS:
        x = _white(rng, n)
        rows.append(_tx("lengths", f"n {n} cfo 50", x, 50.0, 0.7))
        rows.append(_tx("lengths", f"n {n} cfo -13.25", x, -13.25, -2.0))
    for b in range(2):
        rows.append(_tx("lengths", f"n {TXCFO_MAX} buffer {b}", _white(rng, TXCFO_MAX), (50.0, -25.0)[b], (0.1, 3.1)[b]))
    x300 = _white(rng, 300)
    for cfo in CFOS:
        with np.errstate(all="ignore"):
            inc = F(2.0) * PI_F * F(cfo) / F(48000.0)             # :330, all float: 1e38 overflows in the first product
        c = "finite" if (np.isfinite(inc) or not tx_active(cfo)) else "any"
        rows.append(_tx("offsets", f"cfo {_name(cfo)}", x300, cfo, 0.25, cls=c))
    for cfo in (0.0, 0.0005, float(np.nextafter(CFO_GATE, F(0))), -float(np.nextafter(CFO_GATE, F(0)))):
        for ph in (NAN, 100.0):
            rows.append(_tx("offsets", f"below the gate: cfo {_name(cfo)} accumulator {_name(ph)}", x300, cfo, ph, cls="finite", copy=True))
    for ph in PHASES:
        for cfo in (50.0, -50.0):
            c = "finite" if np.isfinite(ph) else "any"
            rows.append(_tx("accumulators", f"accumulator {_name(ph)} cfo {cfo}", x300, cfo, ph, cls=c))
    for cfo in (50.0, -2400.0):
        rows.append(_tx("accumulators", f"accumulator NULL cfo {cfo}", x300, cfo, None))
    # continuation: 200 then 250 samples, both transformed at 256 points; the 450-sample row walks the same phases in one call
    a, b = _white(rng, 200), _white(rng, 250)
    for cfo in (50.0, -2400.0):
        rows.append(_tx("continue", f"first call cfo {cfo}", a, cfo, 3.0))
        rows.append(_tx("continue", f"second call cfo {cfo}", b, cfo, 3.0, after=f"first call cfo {cfo}"))
        rows.append(_tx("continue", f"one walk cfo {cfo}", np.concatenate([a, b]), cfo, 3.0))
    # chunks: distinct buffers, tiled by the GPU test
    for k in range(16):
        rows.append(_tx("chunks", f"small {k}", _white(rng, 2), (50.0, -50.0, 0.0005, 2400.0)[k % 4], 0.01 * k))
    for k in range(4):
        rows.append(_tx("chunks", f"large {k}", _white(rng, TXCFO_MAX), (50.0, -50.0, 12.5, 0.0005)[k], (0.0, 1.0, -3.0, 2.0)[k]))
    # samples: 300 (transformed at N = 512) unless the label says otherwise
    n, N = 300, 512
    e = lambda i: np.eye(1, n, i, dtype=np.float32)[0]
    tone = np.where(np.arange(256) % 2 == 0, F(1), F(-1)).astype(np.float32)
    for lab, x in (("silence", np.zeros(n, np.float32)), ("impulse at 0", e(0)), ("impulse at n-1", e(n - 1)), ("impulse at N/2", e(N // 2)),
                   ("dc", np.full(n, 0.5, np.float32)), ("tone on bin N/2 (n = N = 256)", tone),
                   ("denormals", np.where(np.arange(n) % 2 == 0, F(1e-40), F(-3e-41)).astype(np.float32)),
                   ("FLT_MAX/4 dc (n = 4: the bin reaches FLT_MAX)", np.full(4, FLT_MAX / 4, np.float32)),
                   ("FLT_MAX/4 alternating (n = 4)", np.array([1, -1, 1, -1], np.float32) * F(FLT_MAX / 4)),
                   ("FLT_MAX/4 (n = 2)", np.full(2, FLT_MAX / 4, np.float32))):
        for cfo in (50.0, -50.0):
            rows.append(_tx("samples", f"{lab} cfo {cfo}", x, cfo, 0.5))
    for v in (NAN, INF, -INF):
        b = x300.copy(); b[17] = v
        rows.append(_tx("nonfinite", f"one sample {v!r} at 17", b, 50.0, 0.5, cls="nan_sample"))
        rows.append(_tx("nonfinite", f"one sample {v!r} at 17, below the gate", b, 0.0005, 0.5, cls="any", copy=True))
    return rows


_rows = {}


def rows(O):
    """-> (channel rows, tx_cfo rows); built once, never modified"""
    if "c" not in _rows:
        _rows["c"], _rows["t"] = channel_rows(O), txcfo_rows()
        for part in _rows.values():
            keys = [(r["family"], r["label"]) for r in part]
            assert len(set(keys)) == len(keys), "labels are unique within a family"
            for r in part:
                r["x"].setflags(write=False)
    return _rows["c"], _rows["t"]


def select(part, family, **eq):
    return [r for r in part if r["family"] == family and all(r.get(k) == v for k, v in eq.items())]


def by_label(part, family):
    return {r["label"]: r for r in part if r["family"] == family}


def digest(O):
    ch, tx = rows(O)
    h = hashlib.sha256()
    for r in ch:
        h.update(f"{r['family']}|{r['label']}|{r['kind']}|{r['call']}|{r['seed']}|{r['cls']}".encode())
        h.update(np.array([r["snr"], r["cfo"], r["rmax"]], np.float32).tobytes())
        h.update(r["x"].tobytes())
    for r in tx:
        h.update(f"{r['family']}|{r['label']}|{r['phase'] is None}|{r['cls']}".encode())
        h.update(np.array([r["cfo"], 0.0 if r["phase"] is None else r["phase"]], np.float32).tobytes())
        h.update(r["x"].tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------- answers
def channel_answer(X, r):
    """X: the oracle or the compiled reference -> (samples float32 [n], getActualCFO() float32)"""
    if r["call"] == "plain":
        return X.channel(r["kind"], r["snr"], r["seed"], r["x"]), F(0.0)
    y, a = X.channel_cfo(r["kind"], r["snr"], r["seed"], r["x"], r["cfo"], r["rmax"])
    return y, F(a)


def txcfo_answer(X, r, phase=None):
    """-> (samples float32 [n], accumulator after float32); phase: the accumulator to start from instead of the row's"""
    p = r["phase"] if phase is None else phase
    y, p1 = X.apply_tx_cfo(r["x"], r["cfo"], 0.0 if p is None else float(p))
    return y, F(p1)


def answers(X, O, families=None):
    """X.channel / channel_cfo / apply_tx_cfo on every row -> ({(family, label): (y, actual)}, {(family, label): (y, phase)});
    a "continue" row with `after` starts from the accumulator its first call returned"""
    ch, tx = rows(O)
    A, B = {}, {}
    for r in ch:
        if families is None or r["family"] in families:
            A[(r["family"], r["label"])] = channel_answer(X, r)
    for r in tx:
        if families is None or r["family"] in families:
            start = B[(r["family"], r["after"])][1] if "after" in r else None
            B[(r["family"], r["label"])] = txcfo_answer(X, r, start)
    return A, B


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def word(v):
    """the bit pattern of one float32 as an int"""
    return int(np.array([v], np.float32).view(np.uint32)[0])


def differences(got, exp):
    """the comparison rule -> indices where got is wrong: the bits are equal wherever exp is not NaN; where exp is NaN got is
    NaN (sign and payload of a NaN are not compared)"""
    got, exp = np.ascontiguousarray(got, np.float32).reshape(-1), np.ascontiguousarray(exp, np.float32).reshape(-1)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    en = np.isnan(exp)
    return np.nonzero(np.where(en, ~np.isnan(got), bits(got) != bits(exp)))[0]


def explain(r, got, exp, what="samples"):
    """'' if got meets exp under the rule, else family, label, preset, count, first index and both values"""
    d = differences(got, exp)
    if len(d) == 0:
        return ""
    g, e = np.ravel(got)[d[0]], np.ravel(exp)[d[0]]
    kind = KIND_NAMES[r["kind"]] if "kind" in r else "tx_cfo"
    return (f"{r['family']} / {r['label']} / {kind}: {what}: {len(d)} of {np.size(exp)} differ, first at {int(d[0])}: "
            f"got {g!r} [{word(g):#010x}] expected {e!r} [{word(e):#010x}]")


RECORDED_TXCFO = ("lengths", "offsets", "accumulators", "continue", "samples", "nonfinite")


def recorded_rows(O):
    """the rows whose answers the fixture holds: per channel family and preset the first of its shortest rows (bench: frame
    0 only); per tx_cfo family the first three of its shortest rows"""
    ch, tx = rows(O)
    out_c, out_t = [], []
    for fam in dict.fromkeys(r["family"] for r in ch):
        for kind in KINDS:
            c = select(ch, fam, kind=kind)
            if c:
                out_c.append(min(c, key=lambda r: len(r["x"])))
    for fam in RECORDED_TXCFO:
        c = sorted(select(tx, fam), key=lambda r: len(r["x"]))
        out_t += [r for r in c if "after" not in r][:3]
    return out_c, out_t


if __name__ == "__main__":
    O = po.Oracle()
    ch, tx = rows(O)
    for name, part in (("channel", ch), ("tx_cfo", tx)):
        for fam in dict.fromkeys(r["family"] for r in part):
            print(name, fam, len(select(part, fam)))
    print("digest", digest(O))
