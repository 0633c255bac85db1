"""Deterministic LDPC decoder inputs over the decoder's whole input domain (no test functions here).

Every array is built from a seed and from real codewords encoded by the oracle's LDPCEncoder restatement, so the CPU
tests, the GPU tests and oracle/gen_golden.py all rebuild the same float32 bits.  tests/golden/ldpc_domain.npz holds the
reference's answers on these inputs and a sha256 per family: a generator that drifts fails the hash check instead of
comparing different inputs.

Families (codeword rows [n, 648] in decoder order, per code rate):
  waterfall  BPSK + Gaussian noise at sigmas around the rate's waterfall (many rows do not converge)
  erasures   a fraction p of positions zeroed (half +0.0, half -0.0), and zero tails (first L positions real)
  ties       magnitudes on a coarse grid with the signs of a noisy codeword; all-equal magnitudes with random signs
  clamp      magnitudes 49.99 / 50 / 50.01 / 1e3 / 1e29 / 1e30 mixed with small opposite-sign values
  tiny       f32 denormals and values near FLT_MIN, alone and mixed with normal LLRs
  ooc        out of contract: NaN, +-inf and finite |x| > 1e30 (see include/ria_gpu.h)
"""
import hashlib

import numpy as np

import pyoracle as po

RATES = {"R1_4": po.R1_4, "R1_3": po.R1_3, "R1_2": po.R1_2, "R2_3": po.R2_3, "R3_4": po.R3_4, "R5_6": po.R5_6}
FAMILIES = ("waterfall", "erasures", "ties", "clamp", "tiny")
OOC = "ooc"
# the five factors of the retry cascade, 1.0 (no scaling) and two factors whose products round
FACTORS = (0.9375, 0.875, 0.75, 0.625, 0.5, 1.0, 0.8, 0.3)
MAX_ITERS = (0, 1, 2, 50, 80, 200)
CONFIGS = tuple((f, mi) for f in FACTORS for mi in MAX_ITERS)
BOUNDARY_FACTORS = (0.9375, 0.8)     # iteration-boundary set: t*, t*+1, t*+2 at these factors
FLT_MIN = np.float32(np.finfo(np.float32).tiny)

# noise sigmas (BPSK amplitude 1) around each rate's waterfall at 200 iterations
WATERFALL_SIGMA = {po.R1_4: (0.95, 1.05, 1.15, 1.25, 1.35), po.R1_3: (0.7, 0.78, 0.86, 0.94, 1.02),
                   po.R1_2: (0.7, 0.78, 0.86, 0.94, 1.02), po.R2_3: (0.55, 0.62, 0.69, 0.76, 0.83),
                   po.R3_4: (0.5, 0.56, 0.62, 0.68, 0.74), po.R5_6: (0.42, 0.47, 0.52, 0.57, 0.62)}


def _seed(rate, family):
    return 770000 + 100 * int(rate) + (list(FAMILIES) + [OOC]).index(family)


def codewords(O, rate, n, rng):
    """n random information words encoded -> coded bits [n, 648] (0/1, float32)"""
    k = O.code(rate).k
    out = np.zeros((n, 648), np.float32)
    for t in range(n):
        info = rng.integers(0, 256, (k + 7) // 8, dtype=np.uint8)
        if k % 8:
            info[-1] &= (0xFF << (8 - k % 8)) & 0xFF
        out[t] = np.unpackbits(O.ldpc_encode(rate, info))[:648]
    return out


def noisy(bits, sigma, rng):
    """BPSK + AWGN LLRs, the recipe of oracle/check_against_ref.py section 6: (2(1-2c) + N(0, 2s)) * 2/(2s)^2"""
    x = 2.0 * (1.0 - 2.0 * bits) + rng.normal(0, 2.0 * sigma, bits.shape)
    return (x * (2.0 / (2.0 * sigma) ** 2)).astype(np.float32)


def waterfall(O, rate, rng):
    sig = WATERFALL_SIGMA[rate]
    bits = codewords(O, rate, 40, rng)
    return np.stack([noisy(bits[t], sig[t % len(sig)], rng) for t in range(len(bits))])


def erasures(O, rate, rng):
    rows = []
    for p in (0.05, 0.3, 0.7, 1.0):
        bits = codewords(O, rate, 5, rng)
        for t in range(5):
            x = noisy(bits[t], (0.35, 0.5, 0.6, 0.45, 0.55)[t], rng)
            pos = rng.permutation(648)[:int(round(p * 648))]
            x[pos[0::2]] = np.float32(0.0)
            x[pos[1::2]] = np.float32(-0.0)
            rows.append(x)
    for L in (2, 100, 324, 600):
        bits = codewords(O, rate, 2, rng)
        for t in range(2):
            x = noisy(bits[t], 0.4, rng)
            x[L:] = np.float32(0.0)
            rows.append(x)
    return np.stack(rows)


def ties(O, rate, rng):
    rows = []
    bits = codewords(O, rate, 24, rng)
    sig = WATERFALL_SIGMA[rate]
    for t in range(24):
        x = noisy(bits[t], sig[t % 3], rng)
        s = np.where(x < 0, np.float32(-1.0), np.float32(1.0))
        if t < 8:      # magnitudes on {1, 2, 3}
            m = np.clip(np.rint(np.abs(x)), 1, 3)
        elif t < 16:   # multiples of 0.5
            m = np.maximum(np.rint(np.abs(x) * 2.0) / 2.0, 0.5)
        elif t < 20:   # all equal, signs of the noisy codeword
            m = np.full(648, (1.0, 2.5, 0.75, 3.0)[t - 16])
        else:          # all equal, random signs
            m = np.full(648, (1.0, 2.0, 0.5, 4.0)[t - 20])
            s = np.where(rng.random(648) < 0.5, np.float32(-1.0), np.float32(1.0))
        rows.append((s * m).astype(np.float32))
    return np.stack(rows)


def clamp_edge(O, rate, rng):
    big = np.array([49.99, 50.0, 50.01, 1e3, 1e29, 1e30], np.float32)
    rows = []
    bits = codewords(O, rate, 24, rng)
    for t in range(24):
        s = (1.0 - 2.0 * bits[t]).astype(np.float32)
        x = s * rng.uniform(0.1, 1.5, 648).astype(np.float32)
        flip = rng.random(648) < (0.05 + 0.01 * (t % 8))
        x[flip] = -x[flip]                                   # small values of the wrong sign
        pos = rng.random(648) < (0.1, 0.3, 0.5)[t % 3]
        wrong = rng.random(648) < 0.03                       # some big magnitudes carry the wrong sign too
        mag = big[rng.integers(0, len(big), 648)] if t < 18 else np.full(648, big[t - 18])
        x[pos] = (np.where(wrong, -s, s) * mag)[pos]
        rows.append(x.astype(np.float32))
    return np.stack(rows)


def tiny(O, rate, rng):
    vals = np.array([1.4e-45, 1e-40, 1e-39, np.nextafter(FLT_MIN, np.float32(0)), FLT_MIN, np.float32(2) * FLT_MIN],
                    np.float32)
    rows = []
    bits = codewords(O, rate, 24, rng)
    for t in range(24):
        s = (1.0 - 2.0 * bits[t]).astype(np.float32)
        flip = rng.random(648) < 0.04
        s[flip] = -s[flip]
        if t < 8:        # tiny magnitudes only
            x = s * vals[rng.integers(0, len(vals), 648)]
        elif t < 16:     # noisy LLRs scaled into the denormal range
            x = noisy(bits[t], 0.6, rng) * np.float32((1e-39, 1e-42, 3e-38, 1e-44)[t % 4])
        else:            # normal LLRs with tiny ones mixed in
            x = noisy(bits[t], 0.7, rng)
            pos = rng.random(648) < 0.3
            x[pos] = (s * vals[rng.integers(0, len(vals), 648)])[pos]
        rows.append(x.astype(np.float32))
    return np.stack(rows)


def out_of_contract(O, rate, rng):
    specials = np.array([np.nan, np.inf, -np.inf, 1e31, -1e31, 3e38, -3e38, np.finfo(np.float32).max], np.float32)
    rows = []
    bits = codewords(O, rate, 16, rng)
    for t in range(16):
        x = noisy(bits[t], 0.5, rng)
        if t < 12:
            pos = rng.random(648) < (0.005, 0.05, 0.3)[t % 3]
            if t < 4:
                v = specials[rng.integers(0, len(specials), 648)]
            else:        # one kind per row
                v = np.full(648, specials[t % len(specials)], np.float32)
                if t % len(specials) in (1, 3, 5, 7):        # +big: keep it on the codeword's sign
                    v = np.where(x < 0, -np.abs(v), np.abs(v)).astype(np.float32) if t % len(specials) != 1 else v
            x[pos] = v[pos]
        else:
            x[:] = specials[t - 12]
        rows.append(x.astype(np.float32))
    return np.stack(rows)


_BUILDERS = {"waterfall": waterfall, "erasures": erasures, "ties": ties, "clamp": clamp_edge, "tiny": tiny, OOC: out_of_contract}
_cache = {}


def family(O, rate, name):
    """float32 [n, 648] rows of one family at one rate (built once per process)"""
    key = (int(rate), name)
    if key not in _cache:
        _cache[key] = np.ascontiguousarray(_BUILDERS[name](O, rate, np.random.default_rng(_seed(rate, name))), np.float32)
    return _cache[key]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def canon(x):
    """The decoder's input mapping as include/ria_gpu.h states it: NaN -> +1e30, clamp to [-1e30, +1e30],
    -0.0 -> +0.0 (every other value unchanged, denormals included)."""
    x = np.array(x, np.float32, copy=True)
    x[np.isnan(x)] = np.float32(1e30)
    x = np.clip(x, np.float32(-1e30), np.float32(1e30))
    x[x == 0] = np.float32(0.0)
    return x


# ---------------------------------------------------------------------------------------------- frames
# decodeFixedFrame inputs: real frames (header, payload, CRC) encoded per codeword, the codewords' LLRs built in decoder
# order in one of the shapes above and placed into the frame's soft-bit stream through the receiver's gather table.
FRAME_MODES = (("QAM16", po.R1_2), ("DQPSK", po.R1_4))
FRAME_SHAPES = ("erasures", "ties", "clamp", "tiny", "recovery")


def frame_codewords(O, rate, info):
    g = O.geom(po.QAM16, rate)
    bpc = g.bytes_per_cw
    return np.stack([np.unpackbits(O.ldpc_encode(rate, info[c * bpc:(c + 1) * bpc]))[:648].astype(np.float32) for c in range(4)])


def _cw_shape(shape, bits, rng, grade):
    """one codeword's LLRs in decoder order; grade 0..3 runs from 'decodes at once' to 'hopeless'"""
    s = (1.0 - 2.0 * bits).astype(np.float32)
    sigma = (0.55, 0.8, 0.95, 1.3)[grade]
    x = noisy(bits, sigma, rng)
    if shape == "erasures":
        pos = rng.permutation(648)[:int((0.05, 0.2, 0.35, 0.6)[grade] * 648)]
        x = noisy(bits, 0.5, rng)
        x[pos[0::2]] = np.float32(0.0)
        x[pos[1::2]] = np.float32(-0.0)
    elif shape == "ties":
        x = np.where(x < 0, np.float32(-1), np.float32(1)) * np.clip(np.rint(np.abs(x)), 1, 3)
    elif shape == "clamp":
        pos = rng.random(648) < 0.3
        x[pos] = (np.sign(x) * np.array([49.99, 50.0, 50.01, 1e3, 1e29, 1e30], np.float32)[rng.integers(0, 6, 648)])[pos]
    elif shape == "tiny":
        x = x * np.float32(1e-39)
    return x.astype(np.float32)


def _recovery_cw(O, rate, info, c, rng):
    """codeword c of a frame that converges to a WRONG valid codeword: the LLRs follow the codeword of info with two of
    its payload bits flipped, except that those two bits carry the TRUE sign at magnitude 1, and ~50 other information
    positions carry the wrong sign at magnitude 1.  All |LLR| lie on {1, 2, 3}: the suspects of the CRC recovery tie on
    |LLR| = 1, and which of them enter its 30-entry search is decided by the sort order of equal keys."""
    g = O.geom(po.QAM16, rate)
    bpc = g.bytes_per_cw
    true_bits = frame_codewords(O, rate, info)[c]
    lo = max(17 * 8 - c * bpc * 8, 0)            # payload bits only (after the 17-byte header)
    p = lo + rng.permutation(bpc * 8 - 16 - lo if c == 3 else bpc * 8 - lo)[:2]
    bad = info.copy()
    for b in p:
        bad[c * bpc + b // 8] ^= np.uint8(0x80 >> (b % 8))
    wrong_bits = frame_codewords(O, rate, bad)[c]
    s = (1.0 - 2.0 * wrong_bits).astype(np.float32)
    x = s * rng.choice(np.array([2.0, 3.0], np.float32), 648)
    x[p] = (1.0 - 2.0 * true_bits[p]) * np.float32(1.0)
    others = np.setdiff1d(np.arange(bpc * 8), p)
    q = rng.permutation(others)[:50]
    x[q] = -s[q]
    return x.astype(np.float32)


def frames(O, mod, rate, shape, n, seed, ch_deint=True):
    """-> (LLR stream [n, 2592] float32, info bytes [n, 4*bpc])"""
    rng = np.random.default_rng(seed)
    g = O.geom(getattr(po, mod), rate)
    bpc = g.bytes_per_cw
    table = O.gather_table(g.bits_per_symbol, ch_deint)
    out = np.zeros((n, 2592), np.float32)
    infos = np.zeros((n, 4 * bpc), np.uint8)
    for f in range(n):
        info = O.make_frame(rng.integers(0, 256, 4 * bpc - 19, dtype=np.uint8), 3000 + f, rate)
        infos[f] = info
        bits = frame_codewords(O, rate, info)
        for c in range(4):
            if shape == "recovery":
                x = _recovery_cw(O, rate, info, c, rng) if c == f % 4 else \
                    (np.where(bits[c] > 0, np.float32(-1), np.float32(1)) * rng.choice(np.array([2.0, 3.0], np.float32), 648))
            else:
                x = _cw_shape(shape, bits[c], rng, int(rng.integers(0, 4)) if f % 3 else 0)
            out[f, table[c * 648:(c + 1) * 648]] = x
    return out, infos


# ---------------------------------------------------------------------------------------------- answers
# FRAME_SETS: (mod, rate, shape, frames, seed); all use the channel de-interleaver (the GPU test also runs the
# NO_CHANNEL_DEINTERLEAVE layout of the same codewords against the oracle)
FRAME_SETS = tuple((mod, rate, shape, 24 if shape == "recovery" else 8, 880 + 10 * i + j)
                   for i, (mod, rate) in enumerate(FRAME_MODES) for j, shape in enumerate(FRAME_SHAPES))


def _pool_map(fn, items, threads=16):
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(fn, items))


def decode_answers(D, rate, X, threads=16):
    """LDPCDecoder answers of decoder D (pyoracle.Ref or pyoracle.Oracle) on rows X for every CONFIG:
    -> {"res": int32 [n, ncfg, 2] (ok, lastIterations), "bytes": uint8 [n, ncfg, nb]}"""
    def row(x):
        r = [D.ldpc_decode(rate, x, mi, f) for f, mi in CONFIGS]
        return np.array([[ok, it] for ok, _, it in r], np.int32), np.stack([b for _, b, _ in r])
    out = _pool_map(row, list(X), threads)
    return {"res": np.stack([a for a, _ in out]), "bytes": np.stack([b for _, b in out])}


def robust_answers(D, rate, X, threads=16):
    """robustDecodeSingleCW: -> {"rob": int32 [n, 3] (ok, tries, iterations), "rob_bytes": uint8 [n, nb]}"""
    out = _pool_map(lambda x: D.robust_decode(rate, x), list(X), threads)
    return {"rob": np.array([[ok, tr, it] for ok, _, it, tr in out], np.int32), "rob_bytes": np.stack([b for _, b, _, _ in out])}


def boundary_rows(rate, X, ans):
    """iteration-boundary set from the answers at 200 iterations: (row, factor, max_iter) for every converged
    (row, factor in BOUNDARY_FACTORS) at t*, t*+1, t*+2 where t* = its lastIterations() -> int32 [m, 2], float32 [m]"""
    rows, factors = [], []
    for f in BOUNDARY_FACTORS:
        c = CONFIGS.index((f, 200))
        for i in range(len(X)):
            ok, t = ans["res"][i, c]
            if ok:
                for mi in (t, t + 1, t + 2):
                    rows.append((i, mi)); factors.append(f)
    return np.array(rows, np.int32).reshape(-1, 2), np.array(factors, np.float32)


def boundary_answers(D, rate, X, rows, factors, threads=16):
    out = _pool_map(lambda a: D.ldpc_decode(rate, X[a[0][0]], int(a[0][1]), float(a[1])), list(zip(rows, factors)), threads)
    return {"bnd_res": np.array([[ok, it] for ok, _, it in out], np.int32).reshape(-1, 2),
            "bnd_bytes": np.stack([b for _, b, _ in out])}


def frame_answers(D, mod, rate, llr, threads=16):
    """decodeFixedFrame with the channel de-interleaver: -> {"ok": uint8 [n, 4], "data": uint8 [n, 4*bpc]}
    (data of the codewords that decoded, zero elsewhere)"""
    g = po.Oracle().geom(getattr(po, mod), rate)
    bpc, bps = g.bytes_per_cw, g.bits_per_symbol
    kw = {"flags": 7} if isinstance(D, po.Oracle) else {}        # the whole of decodeFixedFrame, CRC recovery included
    out = _pool_map(lambda x: D.decode_fixed_frame(x, rate, True, bps, **kw)[:2], list(llr), threads)
    ok = np.stack([o for _, o in out]).astype(np.uint8)
    data = np.stack([d[:4 * bpc] for d, _ in out]) * np.repeat(ok != 0, bpc, axis=1)
    return {"ok": ok, "data": data.astype(np.uint8)}
