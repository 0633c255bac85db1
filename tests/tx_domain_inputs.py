"""Deterministic inputs of the OFDM transmit chain over its input domain (no test functions here).

One set per configuration, for all 9 modulations x 6 code rates.  A set is a dict: info uint8 [n, 4 * bytes_per_codeword]
(what ria_gpu_tx_batch and ria_gpu_encode_frames_batch take), info_labels, coded uint8 [m, 324] (what ria_gpu_tx_coded_batch
takes), coded_labels.  Everything comes from fixed seeds and the geometry, so the CPU tests, the GPU tests and
oracle/gen_golden.py rebuild the same bytes; tests/golden/tx_domain.npz holds the compiled reference's answers and a sha256
per set, so that a generator that drifts fails the hash check instead of comparing different inputs.

info families
  valid     two frames of oracle.make_frame with random payload, one with seq 0xFFFF
  constant  every byte 0x00, 0xFF, 0x55, 0xAA
  walk      one 1-bit: the first and the last bit of each codeword's byte range; code bit k-1 where it lies inside the bytes
            (K_MINUS_1_INSIDE); the bits beyond k inside the bytes (BEYOND_K_RATES: no rate has any, bytes_per_codeword * 8 <= k
            everywhere.  The other way round is what happens: at R1/4, R1/3, R1/2, R3/4 and R5/6 (PAD_RATES) k exceeds the
            bytes, the encoder pads with zeros, and the walk bit at the start of the NEXT codeword is what a missing pad
            would read)
  random    three rows of uniform bytes that are not frames
coded families
  constant  0x00 and 0xFF (0xFF shows the zero padding of the carrier that straddles bit 2592 and the unfilled carriers)
  counter   symbol grids V[d, c] packed MSB first.  Coherent modes: V = (d * n_data + c + 97 r) mod 2^b for r = 0, 1, 2.
            Differential modes: V = (d * s + c) mod 2^b for every stride s, so that on a carrier value x is followed by x + s
  tail      zero but for the last 16 bits
  random    two rows of uniform bytes

The module also holds the plain restatements the tests compare the kernels with: make_frames (Philox4x32-10 in uint64
arithmetic, the v2 header, both CRCs) and the peak rule in float32.
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import pyoracle as po  # noqa: E402

MODS = (("DBPSK", po.DBPSK), ("BPSK", po.BPSK), ("DQPSK", po.DQPSK), ("QPSK", po.QPSK), ("D8PSK", po.D8PSK),
        ("QAM16", po.QAM16), ("QAM32", po.QAM32), ("QAM64", po.QAM64), ("QAM256", po.QAM256))
RATES = (("R1_4", po.R1_4), ("R1_3", po.R1_3), ("R1_2", po.R1_2), ("R2_3", po.R2_3), ("R3_4", po.R3_4), ("R5_6", po.R5_6))
MODES = {f"{m}_{r}": (mv, rv) for m, mv in MODS for r, rv in RATES}              # name -> (modulation, rate)
ENGINE = {f"{m}_{r}": (m, r) for m, _ in MODS for r, _ in RATES}
BITS = {po.DBPSK: 1, po.BPSK: 1, po.DQPSK: 2, po.QPSK: 2, po.D8PSK: 3, po.QAM16: 4, po.QAM32: 5, po.QAM64: 6, po.QAM256: 8}
DIFFERENTIAL = (po.DBPSK, po.DQPSK, po.D8PSK)
BPC = {po.R1_4: 20, po.R1_3: 27, po.R1_2: 40, po.R2_3: 54, po.R3_4: 60, po.R5_6: 67}       # bytes per codeword
K = {po.R1_4: 162, po.R1_3: 324, po.R1_2: 324, po.R2_3: 432, po.R3_4: 486, po.R5_6: 540}   # information bits of the code
BEYOND_K_RATES = tuple(n for n, r in RATES if BPC[r] * 8 > K[r])                  # bits of the bytes the code does not carry
K_MINUS_1_INSIDE = tuple(n for n, r in RATES if K[r] - 1 < BPC[r] * 8)
PAD_RATES = tuple(n for n, r in RATES if K[r] > BPC[r] * 8)                       # information bits the encoder pads with zeros
FRAME_BITS, SYM = 2592, 1152
# 1e-30 leaves only samples under 1.2e-8 of the peak denormal (none or few in a frame); 1e-38 makes every sample denormal.
# 3e38 / max|s| overflows to inf for a frame that peaks under 0.88 (most valid frames do) and stays finite above it
PEAKS = (0.0, 0.8, 1.0, 1e-30, 1e-38, 3e38, -0.0, -1.0, float("nan"), float("inf"))
LAYOUT_ROWS = 257


def nvis(mode):
    """recorded through the OFDM-COX object: OFDMChirpWaveform::configure turns QAM256 into DQPSK"""
    return MODES[mode][0] == po.QAM256


def geometry(O, mode):
    """-> int32 [7]: pilot_spacing, n_pilot, n_data, bits_per_carrier, bits_per_symbol, n_data_symbols, frame_samples"""
    g = O.geom(*MODES[mode])
    return np.array([g.pilot_spacing, g.n_pilot, g.n_data, g.bits_per_carrier, g.bits_per_symbol, g.n_data_symbols, g.frame_samples], np.int32)


def _seed(mode):
    return 770000 + list(MODES).index(mode)


def pack_grid(V, bits):
    """symbol values V [n_sym, n_data] -> 324 coded bytes: value (d, c) at stream bits d * bps + c * bits .., MSB first, cut at 2592"""
    n_sym, n_data = V.shape
    b = ((V[:, :, None] >> np.arange(bits - 1, -1, -1)) & 1).astype(np.uint8).reshape(-1)
    s = np.zeros(max(FRAME_BITS, b.size), np.uint8)
    s[:b.size] = b
    return np.packbits(s[:FRAME_BITS])


def _one_bit(n_bytes, bit):
    r = np.zeros(n_bytes, np.uint8)
    r[bit >> 3] = 0x80 >> (bit & 7)
    return r


def info_rows(O, mode):
    mod, rate = MODES[mode]
    bpc, k, total = BPC[rate], K[rate], 4 * BPC[rate]
    rng = np.random.default_rng(_seed(mode))
    rows, labels = [], []
    for seq in (0x0102, 0xFFFF):
        rows.append(O.make_frame(rng.integers(0, 256, total - 19, dtype=np.uint8), seq, rate)); labels.append(f"valid seq {seq:#06x}")
    for v in (0x00, 0xFF, 0x55, 0xAA):
        rows.append(np.full(total, v, np.uint8)); labels.append(f"constant {v:#04x}")
    for cw in range(4):
        rows.append(_one_bit(total, 8 * cw * bpc)); labels.append(f"walk first bit of codeword {cw}")
        rows.append(_one_bit(total, 8 * (cw + 1) * bpc - 1)); labels.append(f"walk last bit of codeword {cw}")
    if k - 1 < 8 * bpc:
        for cw in (0, 3):
            rows.append(_one_bit(total, 8 * cw * bpc + k - 1)); labels.append(f"walk code bit k-1 of codeword {cw}")
    for j in range(k, 8 * bpc):
        rows.append(_one_bit(total, j)); labels.append(f"walk bit {j} beyond k in codeword 0")
    for t in range(3):
        rows.append(rng.integers(0, 256, total, dtype=np.uint8)); labels.append(f"random {t}")
    return np.ascontiguousarray(np.stack(rows), np.uint8), labels


def coded_rows(O, mode):
    mod, rate = MODES[mode]
    g = geometry(O, mode)
    n_data, bits, n_sym = int(g[2]), int(g[3]), int(g[5])
    M = 1 << bits
    rng = np.random.default_rng(_seed(mode) + 5000)
    d, c = np.meshgrid(np.arange(n_sym), np.arange(n_data), indexing="ij")
    rows = [np.zeros(324, np.uint8), np.full(324, 0xFF, np.uint8)]
    labels = ["constant 0x00", "constant 0xff"]
    if mod in DIFFERENTIAL:
        for s in range(M):
            rows.append(pack_grid((d * s + c) % M, bits)); labels.append(f"counter stride {s}")
    else:
        for r in range(3):
            rows.append(pack_grid((d * n_data + c + 97 * r) % M, bits)); labels.append(f"counter offset {97 * r}")
    tail = np.zeros(324, np.uint8); tail[-2:] = 0xFF
    rows.append(tail); labels.append("tail: last 16 bits")
    for t in range(2):
        rows.append(rng.integers(0, 256, 324, dtype=np.uint8)); labels.append(f"random {t}")
    return np.ascontiguousarray(np.stack(rows), np.uint8), labels


_sets = {}


def input_set(O, mode):
    if mode not in _sets:
        info, il = info_rows(O, mode)
        coded, cl = coded_rows(O, mode)
        _sets[mode] = {"info": info, "info_labels": il, "coded": coded, "coded_labels": cl}
    return _sets[mode]


def digest(S):
    h = hashlib.sha256()
    for k in ("info", "coded"):
        h.update(np.ascontiguousarray(S[k]).tobytes())
    return h.hexdigest()


def symbol_values(coded, g):
    """coded uint8 [324] -> (V int [n_sym, n_data], sent bool [n_sym, n_data]): the value every data carrier maps, as the
    modulator reads the stream (zeros behind bit 2592); sent: the carrier starts inside the stream"""
    n_data, bits, bps, n_sym = int(g[2]), int(g[3]), int(g[4]), int(g[5])
    s = np.zeros(n_sym * bps + bits, np.int64)
    s[:FRAME_BITS] = np.unpackbits(np.ascontiguousarray(coded, np.uint8))[:FRAME_BITS]
    b = s[:n_sym * bps].reshape(n_sym, n_data, bits)
    V = (b << np.arange(bits - 1, -1, -1)).sum(2)
    b0 = np.arange(n_sym)[:, None] * bps + np.arange(n_data)[None, :] * bits
    return V, b0 < FRAME_BITS


def coverage(O, mode):
    """counts over the coded rows of the set, from the bit streams and the geometry alone:
    count [2^b] occurrences of every symbol value, carriers [2^b] distinct data carriers it occurs on, trans [2^b, 2^b] how
    often value y follows value x on a carrier in the next symbol (what a differential mode multiplies), straddle: a carrier
    starts before bit 2592 and ends behind it, unfilled: carriers of the last symbol that start behind it; walk: per info walk
    row the (codeword, code bit, stream bit, data symbol, carrier) its one bit lands on through the channel interleaver."""
    mod, rate = MODES[mode]
    g = geometry(O, mode)
    S = input_set(O, mode)
    bits, bps, n_sym = int(g[3]), int(g[4]), int(g[5])
    M = 1 << bits
    count, trans = np.zeros(M, np.int64), np.zeros((M, M), np.int64)
    on = np.zeros((M, int(g[2])), bool)
    for row in S["coded"]:
        V, sent = symbol_values(row, g)
        np.add.at(count, V[sent], 1)
        dd, cc = np.nonzero(sent)
        on[V[dd, cc], cc] = True
        both = sent[1:] & sent[:-1]
        np.add.at(trans, (V[:-1][both], V[1:][both]), 1)
    last = (n_sym - 1) * bps + np.arange(int(g[2])) * bits
    table = O.gather_table(bps, True)
    walk = []
    for row, lab in zip(S["info"], S["info_labels"]):
        if not lab.startswith("walk"):
            continue
        bit = int(np.nonzero(np.unpackbits(row))[0][0])
        cw, j = divmod(bit, 8 * BPC[rate])
        pos = int(table[cw * 648 + j]) if j < K[rate] else -1
        walk.append((cw, j, pos, pos // bps if pos >= 0 else -1, (pos % bps) // bits if pos >= 0 else -1))
    return {"count": count, "carriers": on.sum(1), "trans": trans, "straddle": bool(((last < FRAME_BITS) & (last + bits > FRAME_BITS)).any()),
            "unfilled": int((last >= FRAME_BITS).sum()), "walk": walk}


# ---------------------------------------------------------------------------------------------- answers
def sample_digest(s):
    return hashlib.sha256(np.ascontiguousarray(s, np.float32).tobytes()).hexdigest()


def frame_planes(s):
    """float32 [n] -> uint8 [4, n]: byte p of every little-endian sample in row p.  Lossless; the exponent bytes of a frame
    repeat and the fixture's deflate takes 40 % off such rows, nothing off the samples as they lie in memory"""
    return np.ascontiguousarray(np.ascontiguousarray(s, "<f4").view(np.uint8).reshape(-1, 4).T)


def frame_from_planes(p):
    return np.ascontiguousarray(np.asarray(p, np.uint8).T).view("<f4").reshape(-1)


def answers(X, O, mode):
    """X: the oracle or the compiled reference -> (coded uint8 [n_info, 324] of the info rows, samples: one float32 frame per
    info row, then per coded row, at the modulator's own scale)"""
    mod, rate = MODES[mode]
    S = input_set(O, mode)
    bps = int(geometry(O, mode)[4])
    coded = np.stack([X.encode_fixed_frame(r, rate, True, bps) for r in S["info"]])
    if isinstance(X, po.Ref):
        samples = [X.modulate(mod, rate, c, nvis=nvis(mode)) for c in list(coded) + list(S["coded"])]
    else:
        samples = [X.modulate(mod, rate, c) for c in list(coded) + list(S["coded"])]
    return coded, samples


def reference_geometry(R, mode):
    """the geometry as the reference's objects show it -> (int32 [7] as geometry(), refused): spacing and carrier count from
    the configured waveform, the symbol count from the length of a modulated frame"""
    mod, rate = MODES[mode]
    c = R.tx_config(mod, rate, nvis=nvis(mode))
    n_pilot = (int(c[3]) + int(c[1]) - 1) // int(c[1]) if c[2] else 0
    n_data = int(c[3]) - n_pilot
    n = len(R.modulate(mod, rate, np.zeros(324, np.uint8), nvis=nvis(mode)))
    assert n % SYM == 0
    return np.array([c[1], n_pilot, n_data, BITS[mod], n_data * BITS[mod], n // SYM - 2, n], np.int32), int(c[0]) != mod


# ---------------------------------------------------------------------------------------------- make_frames restated
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays that hold 32-bit words -> four uint64 arrays (constants and round order of
    make_frames_kernel's philox4x32)"""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, np.uint64) & _M32 for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def callsign_hash(s):
    h = 5381
    for ch in s.upper().encode():
        h = (((h << 5) + h) & 0xFFFFFFFF) ^ ch
    return h & 0xFFFFFF


def make_frames(O, rate, seed, first_seq, n):
    """ria_gpu_make_frames in exact integer arithmetic -> uint8 [n, 4 * bytes_per_codeword].  Frame f: sequence number
    (first_seq + f) mod 2^16; payload byte b (frame byte 17 + ..) = bits 11..18 of word b & 3 of Philox(counter = {(first_seq
    + f) mod 2^32, b >> 2, 0x5249, 0}, key = {seed low word, seed high word}); header, hashes and CRCs of a v2 data frame."""
    total = 4 * BPC[rate]
    plen = total - 19
    out = np.zeros((n, total), np.uint8)
    b = np.arange(total, dtype=np.uint64)
    hs, hd = callsign_hash("TEST"), callsign_hash("RX")
    for f in range(n):
        ctr = (int(first_seq) + f) & 0xFFFFFFFF
        r = np.stack(philox4x32(np.full(total, ctr, np.uint64), b >> np.uint64(2), 0x5249, 0, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
        byte = ((r[(b & np.uint64(3)).astype(np.int64), np.arange(total)] >> np.uint64(11)) & np.uint64(0xFF)).astype(np.uint8)
        fr = out[f]
        fr[17:17 + plen] = byte[17:17 + plen]
        seq = ctr & 0xFFFF
        fr[:15] = [0x55, 0x4C, 0x30, 0x01, seq >> 8, seq & 0xFF, hs >> 16, (hs >> 8) & 0xFF, hs & 0xFF, hd >> 16, (hd >> 8) & 0xFF, hd & 0xFF,
                   4, plen >> 8, plen & 0xFF]
        hc = O.lib.ro_crc16(po.up(fr), 15)
        fr[15], fr[16] = hc >> 8, hc & 0xFF
        fc = O.lib.ro_crc16(po.up(fr), total - 2)
        fr[total - 2], fr[total - 1] = fc >> 8, fc & 0xFF
    return out


# ---------------------------------------------------------------------------------------------- the peak rule
def peak_rule(s, peak):
    """peak_normalize of ria_gpu_tx_batch / ria_gpu_tx_coded_batch in float32: s * float32(float32(peak) / max|s|) where
    peak > 0 is true, s otherwise (0, -0.0, negative values and NaN leave the modulator's own scale)"""
    s = np.ascontiguousarray(s, np.float32)
    p = np.float32(peak)
    if not (p > 0):
        return s.copy()
    with np.errstate(all="ignore"):
        return (s * (p / np.abs(s).max())).astype(np.float32)


def same_bits(a, b):
    """bit-for-bit equality of two float32 arrays"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def peak_rows(S):
    """the three rows of a set that the peak values are tried on -> (two info rows: a valid frame and a random row, one coded
    row: the first counter row)"""
    return [0, len(S["info"]) - 1], [i for i, l in enumerate(S["coded_labels"]) if l.startswith("counter")][0]


if __name__ == "__main__":
    # the coverage table of DESIGN.md: per modulation (over its six rates) the least count of a symbol value, the least
    # number of carriers it occurs on and the least count of a transition
    O = po.Oracle()
    print("mode rows(info+coded) min-count min-carriers min-transition straddle unfilled")
    for mode in MODES:
        S, c = input_set(O, mode), coverage(O, mode)
        print(mode, f"{len(S['info'])}+{len(S['coded'])}", int(c["count"].min()), int(c["carriers"].min()), int(c["trans"].min()),
              int(c["straddle"]), c["unfilled"])
