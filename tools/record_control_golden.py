"""Records tests/golden/control_frames.npz from the compiled reference (oracle/_ref/libria_ref.so; run after build() where
the reference sources exist): what test_control_cpu.py requires the oracle restatement - and the library, through it - to equal.

    tx_<mod>_<rate>_<bytes>     the reference modulator's samples (generateDataPreamble() ++ modulate) for a few byte counts, raw
    llr_<row>                   soft-bit bit patterns of process() on some pinned spans (tests/control_inputs.py SPANS)
    status                      [rows, 7] the seven float status words of every pinned span, as bit patterns
    n_soft                      [rows] soft bits process() hands on: the count produced if it is at least 648, else 0 (the waveform
                                object keeps the soft bits of a span whose process() is false to itself)
    outcome                     [rows, 12] the control hypothesis of every pinned span (control_restatement.RESULT_FIELDS)
    frames                      [rows, 20] the frame bytes it delivers

Numeric arrays only.  --search looks for the channel seeds of the rows that need 2..5 robust-decode tries."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pyoracle as po                # noqa: E402
import control_inputs as CI          # noqa: E402
import control_restatement as R      # noqa: E402

TX_CASES = (("dqpsk_r14", po.DQPSK, po.R1_4, 1), ("dqpsk_r14", po.DQPSK, po.R1_4, 81), ("d8psk_r12", po.D8PSK, po.R1_2, 80))
LLR_ROWS = ("ack_awgn20", "ack_mod10", "ack_cfo_marker", "ack_long_span", "ack_tries3", "noise", "silence", "ack_odd_span")


def tx_bytes(nb):
    return ((np.arange(nb) * 37 + 11 * nb) % 256).astype(np.uint8)


def record(checker):
    """every array of the fixture from one checker (the compiled reference when recording, the oracle when testing)"""
    out = {}
    for name, mod, rate, nb in TX_CASES:
        out[f"tx_{name}_{nb}"] = checker.modulate(mod, rate, tx_bytes(nb))
    status, n_soft, outcome, frames = [], [], [], []
    for row in CI.SPANS:
        x = CI.span(checker, row)
        llr, st, n_llr = R.process_span(checker, *CI.CTRL, x, row[7], row[8], row[9])
        if row[0] in LLR_ROWS:
            out["llr_" + row[0]] = llr.view(np.uint32).copy()
        r = R.control_hypothesis(checker, x, row[7], row[8], row[9])
        status.append(np.array([st[k] for k in R.STATUS_WORDS], np.float32).view(np.uint32))
        n_soft.append(n_llr)
        outcome.append([int(r[k]) for k in R.RESULT_FIELDS])
        frames.append(r["frame"])
    out.update(status=np.stack(status), n_soft=np.array(n_soft, np.int32), outcome=np.array(outcome, np.int32),
               frames=np.stack(frames).astype(np.uint8))
    return out


def search(checker, want_tries, seq, conditions=((2, 0.0), (2, -1.0), (0, -1.0)), seeds=range(100, 4000)):
    s = R.tx_var(checker, *CI.CTRL, R.encode_control(R.control_frame(R.ACK, seq)))
    for ch, snr in conditions:
        for seed in seeds:
            r = R.control_hypothesis(checker, checker.channel(ch, snr, seed, s))
            if (r["tries"] if r["cw_ok"] else 0) == want_tries and (want_tries == 0 or r["success"]):
                return ch, snr, seed
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "control_frames.npz"))
    a = ap.parse_args()
    if a.search:
        O = po.Oracle()
        for t, seq in ((2, 7), (3, 8), (4, 9), (5, 10), (0, 11)):
            print(t, search(O, t, seq), flush=True)
        return
    if not po.Ref.available():
        raise SystemExit("the compiled reference (oracle/_ref/libria_ref.so) is not built here")
    arrays = record(po.Ref())
    np.savez_compressed(a.out, **arrays)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
