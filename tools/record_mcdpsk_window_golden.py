"""Records tests/golden/mcdpsk_window.npz from the compiled reference (oracle/_ref/libria_ref.so; run after build() where the
reference sources exist): what test_mcdpsk_window_cpu.py requires the restatement of the MC-DPSK window on the oracle - and the
library, through it - to equal, for every row of tests/mcdpsk_window_inputs.py, in table order:

    fields      [rows, 12] mcdpsk_window_restatement.RESULT_FIELDS
    words       [rows, 2]  training_rms, rms as bit patterns
    acq         [rows, 16] mcdpsk_window_restatement.ACQ_FIELDS of the reported candidate
    acq_words   [rows, 3]  correlation, cfo_hz, fading_index as bit patterns
    harq        [rows, 9]  mcdpsk_window_restatement.HARQ_FIELDS
    frame_bytes [rows, 64] the first 64 bytes of the DecodeResult's frame_data, zero padded
    llr_crc     [rows]     CRC-32 of the reported candidate's soft bits (their bit patterns), 0 where there are none

Numeric arrays only.  --search finds, with the restatement's float32 chain, the last-sample values of the three synthetic-tail
rows (rms / training_rms one ulp under 0.6f, 0.6f, one ulp over): the only rows of the table that cannot be built by
construction."""
import argparse
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pyoracle as po                      # noqa: E402
import mcdpsk_window_inputs as WI          # noqa: E402
import mcdpsk_window_restatement as MW     # noqa: E402


def bits(*v):
    return np.array(v, np.float32).view(np.uint32)


def row_arrays(e):
    """one expected row -> the fixture's arrays for it"""
    a = e["acq"]
    fb = np.zeros(64, np.uint8)
    n = min(64, len(a["frame"]))
    fb[:n] = a["frame"][:n]
    llr = np.ascontiguousarray(a["llr"], np.float32)
    return dict(fields=[int(e[k]) for k in MW.RESULT_FIELDS], words=bits(*(e[k] for k in MW.RESULT_WORDS)),
                acq=[int(a[k]) for k in MW.ACQ_FIELDS], acq_words=bits(*(a[k] for k in MW.ACQ_WORDS)),
                harq=[int(e["harq"][k]) for k in MW.HARQ_FIELDS], frame_bytes=fb,
                llr_crc=zlib.crc32(llr.view(np.uint32).tobytes()) if len(llr) else 0)


def record(checker):
    """every array of the fixture from one checker (the compiled reference when recording, the oracle when testing)"""
    out = {k: [] for k in ("fields", "words", "acq", "acq_words", "harq", "frame_bytes", "llr_crc")}
    for _, _, _, exp in WI.expected_all(checker):
        for e in exp:
            for k, v in row_arrays(e).items():
                out[k].append(v)
    for k in ("fields", "acq", "harq"):
        out[k] = np.array(out[k], np.int64)
    for k in ("words", "acq_words"):
        out[k] = np.stack(out[k]).astype(np.uint32)
    out["frame_bytes"] = np.stack(out["frame_bytes"])
    out["llr_crc"] = np.array(out["llr_crc"], np.uint32)
    return out


def search_tails():
    """the last sample of the data region, the other 4999 at TAIL_BODY, for ratio - 0.6f = -1, 0, +1 ulp"""
    body = np.array([WI.TAIL_BODY], np.uint32).view(np.float32)[0]
    v = np.full(5000, body, np.float32)
    target = int(np.float32(0.6).view(np.uint32))
    found = {}
    for sb in range(0x3E800000, 0x3EC00000, 0x400):
        v[-1] = np.array([sb], np.uint32).view(np.float32)[0]
        d = int(np.float32(MW.chain_rms(v) / np.float32(0.5)).view(np.uint32)) - target
        if d in (-1, 0, 1) and d not in found:
            found[d] = sb
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mcdpsk_window.npz"))
    a = ap.parse_args()
    if a.search:
        f = search_tails()
        print("TAIL_UNDER, TAIL_AT, TAIL_OVER =", ", ".join("0x%08X" % f[d] for d in (-1, 0, 1)))
        return
    if not po.Ref.available():
        raise SystemExit("the compiled reference (oracle/_ref/libria_ref.so) is not built here")
    ref = po.Ref()
    WI.assert_coverage(ref)                  # the table reaches every statement on the reference itself
    arrays = record(ref)
    np.savez_compressed(a.out, **arrays)
    print(a.out, os.path.getsize(a.out), "bytes", len(arrays["fields"]), "rows")


if __name__ == "__main__":
    main()
