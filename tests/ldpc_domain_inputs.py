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

Frame sets (decodeFixedFrame inputs [n, 2592], FRAME_SETS and NEW_FRAME_SETS):
  erasures, ties, clamp, tiny   the shapes above on the four codewords of real frames, at QAM16 R1/2 and DQPSK R1/4 with
             fixed noise grades, at DBPSK R1/3, D8PSK R2/3, QAM32 R5/6, QAM64 R3/4 and QAM256 R2/3 with grades taken
             from WATERFALL_SIGMA (all six code rates, all seven symbol sizes 53 .. 376 bits)
  recovery   (the first two modes) frames that converge to a wrong codeword whose CRC search EXHAUSTS WITHOUT A REPAIR
  hdr1 hdr2 single crc pair triple quad   (all seven modes) frames that this step of the CRC recovery repairs, 8 per set;
             STAGE_COUNTS says how many give the sent bytes back and in how many an earlier wrong match wins
  beyond     (the five new modes) five wrong bits, one more than the searches reach: no step repairs these
  fill       frames the fallback re-decode repairs, found by search: one codeword of a frame under Gaussian noise on the
             upper slope of its rate's waterfall.  20 000 candidates were searched per mode; hits (kept): QAM16 R1/2 0,
             DQPSK R1/4 8 (4), DBPSK R1/3 2 (2), D8PSK R2/3 2 (2), QAM32 R5/6 19 (4), QAM64 R3/4 13 (4), QAM256 R2/3 2 (2)
             - see FILL_SEARCH
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


# ---- all six code rates: the modes added to FRAME_MODES (every bits-per-symbol value 53 .. 376 occurs once)
NEW_FRAME_MODES = (("DBPSK", po.R1_3), ("D8PSK", po.R2_3), ("QAM32", po.R5_6), ("QAM64", po.R3_4), ("QAM256", po.R2_3))
ALL_FRAME_MODES = FRAME_MODES + NEW_FRAME_MODES
NOISE_SHAPES = ("erasures", "ties", "clamp", "tiny")
# CRC recovery steps in the order decodeFixedFrame tries them; a set of this name holds frames that step repairs
STAGES = ("hdr1", "hdr2", "single", "crc", "pair", "triple", "quad")
FILL = "fill"
BEYOND = "beyond"        # five wrong bits: one more than the searches reach


def _grade_sigma(rate, grade):
    """noise grades of the new modes, relative to the rate's waterfall: well inside it, on its lower and upper slope, far
    beyond it (the fixed sigmas of _cw_shape lie beyond the waterfall of the high rates altogether)"""
    w = WATERFALL_SIGMA[rate]
    return (0.7 * w[0], w[1], w[3], 1.5 * w[4])[grade]


def _cw_shape_rate(O, shape, bits, rng, grade, rate):
    """_cw_shape for the modes of NEW_FRAME_MODES: the same four shapes, their grades taken from WATERFALL_SIGMA[rate].
      erasures  a fraction of what the code can lose (its checks over the columns any check reads: R3/4 and R5/6 leave
                the info columns behind 324 and 216 out of every check), on noise well inside the waterfall
      clamp     the huge magnitudes go to soft bits of above-median magnitude (on any soft bit, as _cw_shape has it, a grade
                inside the waterfall of a high rate still puts 1e30 on a few wrong signs and never decodes at once)
      tiny      half the codewords scaled into the denormals whole (the noise the cascade adds drowns them, so only the factor
                retries of phase 0 can rescue one: every grade short of 'hopeless' lies one step nearer the waterfall), the
                other half with 30 % of their soft bits scaled so, which the cascade does rescue"""
    w = WATERFALL_SIGMA[rate]
    sigma = (0.7 * w[0], w[1], w[2], w[3])[grade] if shape == "tiny" else _grade_sigma(rate, 0 if shape == "erasures" else grade)
    x = noisy(bits, sigma, rng)
    if shape == "erasures":
        deg = _column_degree(O, rate)
        frac = (0.1, 0.6, 0.8, 1.3)[grade] * (648 - O.code(rate).k) / int((deg > 0).sum())
        pos = rng.permutation(648)[:int(frac * 648)]
        x[pos[0::2]] = np.float32(0.0)
        x[pos[1::2]] = np.float32(-0.0)
    elif shape == "ties":
        x = np.where(x < 0, np.float32(-1), np.float32(1)) * np.clip(np.rint(np.abs(x)), 1, 3)
    elif shape == "clamp":
        pos = (np.abs(x) > np.median(np.abs(x))) & (rng.random(648) < 0.6)
        x[pos] = (np.sign(x) * np.array([49.99, 50.0, 50.01, 1e3, 1e29, 1e30], np.float32)[rng.integers(0, 6, 648)])[pos]
    elif shape == "tiny":
        if rng.random() < 0.5:
            x = x * np.float32(1e-39)
        else:
            pos = rng.random(648) < 0.3
            x[pos] = x[pos] * np.float32(1e-39)
    return x.astype(np.float32)


def _clean_frame(O, rate, rng, seq, plen):
    """a data frame of plen payload bytes none of whose codewords 1..3 begins with the 0xD5 marker reassembly would strip"""
    bpc = O.geom(po.QAM16, rate).bytes_per_cw
    while True:
        info = O.make_frame(rng.integers(0, 256, plen, dtype=np.uint8), seq, rate)
        if not any(info[c * bpc] == 0xD5 for c in range(1, 4)):
            return info


def _confident(bits, rng):
    return ((1.0 - 2.0 * bits) * rng.choice(np.array([2.0, 3.0], np.float32), len(bits))).astype(np.float32)


def _mirror(i):
    """The suspect list compares the sign of soft bit i with bit i % 8 of the decoded byte counted from the LEAST significant
    end, while the codeword's bits are most significant first: bit i of a codeword is tested through soft bit mirror(i)."""
    return (i & ~7) | (7 - (i & 7))


_degree = {}


def _column_degree(O, rate):
    """checks per codeword bit"""
    if rate not in _degree:
        _degree[rate] = np.bincount(O.H_edges(rate)[1], minlength=648)
    return _degree[rate]


def _stage_frame(O, rate, stage, f, rng, bytes_only=False):
    """Frame f of a set the CRC recovery repairs in step `stage`: codeword c of the frame follows, at |LLR| 2..3, a WRONG
    valid codeword (the encoding of the frame's bytes with 1..4 bits flipped), the flipped bits themselves at |LLR| 1 (with
    the true sign there the high rates, whose later info columns no check reads, would simply decode the sent bytes).
    -> (four codewords' LLRs [4, 648] in decoder order, the sent bytes)

      hdr1, hdr2   1 / 2 bits of the 17-byte header in codeword 0: nothing reassembles, every bit (pair) of codeword 0 is tried
      single       1 payload bit: the CRC syndrome equals that bit's delta
      crc          1 bit of the frame's CRC field (every other frame ends early, one with its CRC across two codewords)
      pair, triple, quad   2 / 3 / 4 payload bits.  Each is a suspect only through its mirror soft bit (see _mirror), which
                   is set to disagree at |LLR| 1; decoys (soft bits that disagree with their mirror anyway, weakened to
                   |LLR| 1) tie with them, so the sort order of equal keys decides the search order.  The searched list
                   (30 entries, 15 for quad) is never filled beyond its end with |LLR| 1 entries.
      beyond       5 payload bits, built like quad: no step repairs it (the new modes' counterpart of the old "recovery" sets)
    The wrong codeword rotates over 0..3 for single and the searches.  bytes_only: -> (the wrong bytes, the sent bytes)."""
    bpc = O.geom(po.QAM16, rate).bytes_per_cw
    cap = 4 * bpc - 19
    k = {"hdr1": 1, "hdr2": 2, "single": 1, "crc": 1, "pair": 2, "triple": 3, "quad": 4, BEYOND: 5}[stage]
    c = f % 4
    plen = cap if f < 4 else cap - int(rng.integers(1, bpc - 3))
    if stage == "crc" and f % 4 == 3:
        plen = 3 * bpc - 18                                  # the CRC's two bytes end codeword 2 and begin codeword 3
    info = _clean_frame(O, rate, rng, 5000 + f, plen)
    end = 17 + plen                                          # first byte of the frame CRC
    if stage in ("hdr1", "hdr2"):
        c, lo, hi = 0, 0, 17
    elif stage == "crc":
        c, lo, hi = (end + (f >> 2 & 1)) // bpc, end, end + 2
    else:
        lo, hi = max(17, c * bpc), min(end, (c + 1) * bpc)
    sent = frame_codewords(O, rate, info)
    search = stage in ("pair", "triple", "quad", BEYOND)
    while True:                                              # k distinct bits of bytes lo..hi-1 inside codeword c, no two mirrored
        p = lo * 8 + rng.permutation((hi - lo) * 8)[:k]
        p = p[(p // 8) // bpc == c]
        i = p - c * bpc * 8
        # a mirror soft bit no check reads (R3/4 and R5/6 leave the info columns behind 324 and 216 out of every check) decides
        # its own bit alone: there it may only be weakened, not turned, so the sent bit and its mirror must be equal
        free = _column_degree(O, rate)[_mirror(i)] == 0
        if len(p) == k and len({int(_mirror(q)) for q in p} & {int(q) for q in p}) == 0 and \
                not (search and (free & (sent[c, i] != sent[c, _mirror(i)])).any()):
            break
    bad = info.copy()
    for q in p:
        bad[q // 8] ^= np.uint8(0x80 >> (q % 8))
    if bytes_only:
        return bad, info
    got = frame_codewords(O, rate, bad)
    x = np.stack([_confident(got[j], rng) for j in range(4)])
    x[c, i] = (1.0 - 2.0 * got[c, i]) * np.float32(1.0)      # the wrong bits: weak, and wrong
    if search:
        m = _mirror(i)
        x[c, m] = (1.0 - 2.0 * sent[c, i]) * np.float32(1.0)
        # suspects the |LLR| 1 soft bits of the flipped bits add themselves, then decoys up to the end of the searched list
        extra = int((got[c, i] != got[c, m]).sum())
        room = (15 if stage in ("quad", BEYOND) else 30) - k - extra
        want = min(int(rng.integers(0, 11 if stage in ("quad", BEYOND) else 27)), room)
        idx = np.arange(bpc * 8)
        cand = [(j, t) for j in range(4) for t in idx[got[j, idx] != got[j, _mirror(idx)]]
                if (j * bpc * 8 + t) // 8 < end and not (j == c and (t in i or t in m))]
        for q in rng.permutation(len(cand))[:want]:
            j, t = cand[q]
            x[j, t] = np.sign(x[j, t]) * np.float32(1.0)
    return x.astype(np.float32), info


# Frames the fallback step repairs (a re-decode at 0.75, 0.625, 0.5 or 0.875 gives the sent codeword) cannot be built by rule:
# they are found by searching candidates 0 .. 19 999 of _fill_candidate with the oracle (find_fill_frames below, seed 1700 +
# the mode's index in ALL_FRAME_MODES).  Per mode: (candidates searched, hits among them, the first hits, at most 4, kept as
# the set).  QAM16 R1/2 has no hit and no set; tests/test_ldpc_domain_cpu.py names it.  The hit totals and the later kept
# indices are RECORDED from that search, not tested: the tests check that every kept frame is such a frame, and repeat the
# search only over the first 414 candidates of one mode.
FILL_SEARCH = {"QAM16_R1_2": (20000, 0, ()), "DQPSK_R1_4": (20000, 8, (1014, 2021, 3664, 5210)), "DBPSK_R1_3": (20000, 2, (12444, 15266)),
               "D8PSK_R2_3": (20000, 2, (900, 15026)), "QAM32_R5_6": (20000, 19, (1236, 6789, 7060, 7665)),
               "QAM64_R3_4": (20000, 13, (411, 413, 4069, 5507)), "QAM256_R2_3": (20000, 2, (8330, 9927))}


def _fill_candidate(O, rate, idx, seed):
    """candidate idx of the fill search: a full-length frame, codeword idx % 4 BPSK + Gaussian noise on the upper
    slope of the rate's waterfall (on the soft bits some check reads: a noisy soft bit no check reads is a wrong byte no
    re-decode changes), the others confident -> ([4, 648], sent bytes)"""
    rng = np.random.default_rng([seed, idx])
    bpc = O.geom(po.QAM16, rate).bytes_per_cw
    info = _clean_frame(O, rate, rng, idx & 0xFFFF, 4 * bpc - 19)
    bits = frame_codewords(O, rate, info)
    x = np.stack([_confident(bits[j], rng) for j in range(4)])
    c = idx % 4
    read = _column_degree(O, rate) > 0
    x[c] = np.where(read, noisy(bits[c], WATERFALL_SIGMA[rate][2 + idx // 4 % 3], rng), x[c])
    return x, info


def fill_key(mod, rate):
    return f"{mod}_{[k for k, v in RATES.items() if v == rate][0]}"


def find_fill_frames(O, mod, rate, seed, budget=20000, threads=16):
    """the search behind FILL_SEARCH: -> (candidates searched, indices of all hits)"""
    g = O.geom(getattr(po, mod), rate)
    table = O.gather_table(g.bits_per_symbol, True)

    def hit(idx):
        x, info = _fill_candidate(O, rate, idx, seed)
        llr = np.zeros(2592, np.float32)
        llr[table] = x.reshape(-1)
        d, ok, _, _, stage, _ = O.decode_fixed_frame_stage(llr, rate, True, g.bits_per_symbol)
        return stage == FILL and bool(ok.all()) and np.array_equal(d, info)
    return budget, [i for i, h in enumerate(_pool_map(hit, range(budget), threads)) if h]


def frames(O, mod, rate, shape, n, seed, ch_deint=True):
    """-> (LLR stream [n, 2592] float32, info bytes [n, 4*bpc])"""
    rng = np.random.default_rng(seed)
    g = O.geom(getattr(po, mod), rate)
    bpc = g.bytes_per_cw
    table = O.gather_table(g.bits_per_symbol, ch_deint)
    out = np.zeros((n, 2592), np.float32)
    infos = np.zeros((n, 4 * bpc), np.uint8)
    new_mode = (mod, rate) in NEW_FRAME_MODES
    for f in range(n):
        if shape == FILL:
            x, infos[f] = _fill_candidate(O, rate, FILL_SEARCH[fill_key(mod, rate)][2][f], seed)
        elif shape in STAGES + (BEYOND,):
            x, infos[f] = _stage_frame(O, rate, shape, f, rng)
        else:
            infos[f] = info = O.make_frame(rng.integers(0, 256, 4 * bpc - 19, dtype=np.uint8), 3000 + f, rate)
            bits = frame_codewords(O, rate, info)
            x = np.zeros((4, 648), np.float32)
            for c in range(4):
                if shape == "recovery":
                    x[c] = _recovery_cw(O, rate, info, c, rng) if c == f % 4 else \
                        (np.where(bits[c] > 0, np.float32(-1), np.float32(1)) * rng.choice(np.array([2.0, 3.0], np.float32), 648))
                elif new_mode:
                    x[c] = _cw_shape_rate(O, shape, bits[c], rng, int(rng.integers(0, 4)) if f % 3 else 0, rate)
                else:
                    x[c] = _cw_shape(shape, bits[c], rng, int(rng.integers(0, 4)) if f % 3 else 0)
        out[f, table] = np.asarray(x, np.float32).reshape(-1)
    return out, infos


# ---------------------------------------------------------------------------------------------- answers
# FRAME_SETS: (mod, rate, shape, frames, seed); all use the channel de-interleaver (the GPU test also runs the
# NO_CHANNEL_DEINTERLEAVE layout of the same codewords against the oracle)
FRAME_SETS = tuple((mod, rate, shape, 24 if shape == "recovery" else 8, 880 + 10 * i + j)
                   for i, (mod, rate) in enumerate(FRAME_MODES) for j, shape in enumerate(FRAME_SHAPES))
# the sets added for all six rates: the four noise shapes at the new modes, one set per recovery step at every mode, and the
# fill frames of FILL_SEARCH.  The old "recovery" sets stay: their search exhausts without a repair.
# seeds moved until the oracle's answers hold frames of every kind (tests/test_ldpc_domain_cpu.py states the conditions)
NOISE_SEEDS = {("DBPSK", "ties"): 2201, ("D8PSK", "tiny"): 2213, ("QAM32", "clamp"): 4222, ("QAM256", "clamp"): 2242,
               ("QAM256", "tiny"): 3243}
NEW_NOISE_SETS = tuple((mod, rate, shape, 8, NOISE_SEEDS.get((mod, shape), 1200 + 10 * i + j))
                       for i, (mod, rate) in enumerate(NEW_FRAME_MODES) for j, shape in enumerate(NOISE_SHAPES))
STAGE_SETS = tuple((mod, rate, stage, 8, 1500 + 10 * i + j)
                   for i, (mod, rate) in enumerate(ALL_FRAME_MODES) for j, stage in enumerate(STAGES))
FILL_SETS = tuple((mod, rate, FILL, len(FILL_SEARCH[fill_key(mod, rate)][2]), 1700 + i)
                  for i, (mod, rate) in enumerate(ALL_FRAME_MODES) if FILL_SEARCH[fill_key(mod, rate)][2])
# per mode, in the order of STAGES: (frames of the set its step repairs to the sent bytes, frames where an earlier, wrong
# syndrome match validates other bytes - these pin the search ORDER).  Every frame of every set is one or the other.
STAGE_COUNTS = {"QAM16_R1_2": ((8, 0), (7, 1), (8, 0), (8, 0), (8, 0), (7, 1), (7, 1)),
                "DQPSK_R1_4": ((8, 0), (7, 1), (8, 0), (8, 0), (8, 0), (8, 0), (8, 0)),
                "DBPSK_R1_3": ((8, 0), (7, 1), (8, 0), (8, 0), (8, 0), (7, 1), (8, 0)),
                "D8PSK_R2_3": ((8, 0), (8, 0), (8, 0), (8, 0), (8, 0), (8, 0), (8, 0)),
                "QAM32_R5_6": ((8, 0), (7, 1), (8, 0), (8, 0), (8, 0), (8, 0), (8, 0)),
                "QAM64_R3_4": ((8, 0), (8, 0), (8, 0), (8, 0), (8, 0), (7, 1), (8, 0)),
                "QAM256_R2_3": ((8, 0), (8, 0), (8, 0), (8, 0), (8, 0), (7, 1), (8, 0))}
BEYOND_SETS = tuple((mod, rate, BEYOND, 8, 1500 + 10 * (i + len(FRAME_MODES)) + 7) for i, (mod, rate) in enumerate(NEW_FRAME_MODES))
NEW_FRAME_SETS = NEW_NOISE_SETS + STAGE_SETS + FILL_SETS + BEYOND_SETS
ALL_FRAME_SETS = FRAME_SETS + NEW_FRAME_SETS


def set_key(mod, rate, shape):
    return f"{fill_key(mod, rate)}_{shape}"


def recovery_mix(O, mod, rate):
    """every recovery frame of one mode - the sets of STAGES and FILL, the old "recovery" or the BEYOND set - and
    8 frames of confident soft bits that need no recovery -> (LLR stream [n, 2592], sent bytes [n, 4*bpc])"""
    sets = [s for s in ALL_FRAME_SETS if s[:2] == (mod, rate) and (s[2] in STAGES or s[2] in (FILL, BEYOND, "recovery"))]
    parts = [frames(O, *s) for s in sets]
    g = O.geom(getattr(po, mod), rate)
    rng = np.random.default_rng(1900 + g.bits_per_symbol)
    table = O.gather_table(g.bits_per_symbol, True)
    llr, infos = np.zeros((8, 2592), np.float32), np.zeros((8, 4 * g.bytes_per_cw), np.uint8)
    for f in range(8):
        cap = 4 * g.bytes_per_cw - 19
        infos[f] = _clean_frame(O, rate, rng, 7000 + f, cap - cap // 8 * f)       # frames that end in every codeword
        llr[f, table] = np.stack([_confident(b, rng) for b in frame_codewords(O, rate, infos[f])]).reshape(-1)
    return np.concatenate([p[0] for p in parts] + [llr]), np.concatenate([p[1] for p in parts] + [infos])


TX_STAGES = ("hdr1", "hdr2", "single", "crc", "pair")


def wrong_bytes(O, mod, rate):
    """Frames to TRANSMIT with wrong bytes, so that a clean receive chain decodes four good codewords whose frame check
    fails: 8 per step of TX_STAGES, with the wrong bits of _stage_frame, and 8 correct frames.  The header flips, the
    single-bit and the CRC-field step read no soft bit and repair theirs; the two wrong bits of "pair" are no suspects
    on a clean channel and go on to the fallback stage.  -> (bytes to send [48, 4*bpc], the bytes meant [48, 4*bpc])"""
    g = O.geom(getattr(po, mod), rate)
    rng = np.random.default_rng(2100 + g.bits_per_symbol)
    pairs = [_stage_frame(O, rate, stage, f, rng, bytes_only=True) for stage in TX_STAGES for f in range(8)]
    cap = 4 * g.bytes_per_cw - 19
    clean = [_clean_frame(O, rate, rng, 7100 + f, cap - cap // 8 * f) for f in range(8)]
    return np.stack([b for b, _ in pairs] + clean), np.stack([i for _, i in pairs] + clean)


# per mode, what the recovery does with the frames of wrong_bytes received over a clean channel: frames of each of the first
# four TX_STAGES that their step repairs to the bytes meant (in the others an earlier wrong header pair wins), and two-bit
# frames the recovery gives up on (in the others a wrong match among the clean channel's suspects wins)
TX_COUNTS = {"QAM16_R1_2": (8, 7, 8, 8, 8), "DQPSK_R1_4": (8, 6, 8, 8, 8), "DBPSK_R1_3": (8, 7, 8, 8, 8), "D8PSK_R2_3": (8, 8, 8, 8, 7),
             "QAM32_R5_6": (8, 8, 8, 8, 7), "QAM64_R3_4": (8, 7, 8, 8, 8), "QAM256_R2_3": (8, 5, 8, 8, 7)}


def tx_counts(stages, data, meant):
    """the counts of TX_COUNTS from the recovery step and the bytes decoded for each of the 48 frames of wrong_bytes"""
    assert list(stages[40:]) == ["none"] * 8 and np.array_equal(data[40:], meant[40:])
    good = [sum(stages[q] == stage and np.array_equal(data[q], meant[q]) for q in range(8 * k, 8 * k + 8))
            for k, stage in enumerate(TX_STAGES[:4])]
    return tuple(good) + (list(stages[32:40]).count("failed"),)


def recovery_classes(O, mod, rate, llr, infos, threads=16):
    """Per frame, from the oracle alone: (step that ended the CRC recovery, kind).  kind: "repaired" - the cascade alone
    gives four good codewords with wrong bytes and the recovery gives the sent bytes back; "wrong" - the recovery validates
    bytes that are NOT the sent ones (an earlier syndrome match won); "unrepaired" - the recovery gives up; "clean" - the
    cascade alone gives the sent bytes; "lost" - a codeword fails."""
    bps = O.geom(getattr(po, mod), rate).bits_per_symbol

    def one(a):
        x, info = a
        d3, ok3, _, _ = O.decode_fixed_frame(x, rate, True, bps, flags=3)
        d7, ok7, _, _, stage, _ = O.decode_fixed_frame_stage(x, rate, True, bps, flags=7)
        if not ok3.all():
            return stage, "lost"
        if stage == "none":
            return stage, "clean" if np.array_equal(d7, info) else "wrong"
        if not ok7.all():
            return stage, "unrepaired"
        return stage, "repaired" if np.array_equal(d7, info) and not np.array_equal(d3, info) else "wrong"
    return _pool_map(one, list(zip(llr, infos)), threads)


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
