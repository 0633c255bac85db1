"""Records tests/golden/window_frames.npz from the compiled reference (oracle/_ref/libria_ref.so; run after build() where
the reference sources exist): what test_window_cpu.py requires the restatement of the connected-mode window on the oracle -
and the library, through it - to equal, for every row of tests/window_inputs.py:

    fields      [rows, 11] window_restatement.WINDOW_FIELDS
    words       [rows, 3]  sync_cfo_hz, peek_cfo_hz, fading_index as bit patterns
    frame       [rows, 12] decode_frame_restatement.RESULT_FIELDS of the DecodeResult delivered
    frame_bytes [rows, 64] its first 64 bytes, zero padded
    acq         [rows, 7]  detected, accepted, sync_start, frame_start, delta, candidates, burst_interleaved
    acq_words   [rows, 2]  correlation and the reported span's CFO estimate as bit patterns
    control     [rows, 12] control_restatement.RESULT_FIELDS
    n_spans     [rows]     process() calls of the data profile
    pass2_cfo   [rows]     the CFO the second process() of the data profile ran at, as a bit pattern (0 where there is none): on
                           the rows with a transmitter CFO of 3 Hz this is known +- 2 exactly
    llr_<row>   soft-bit bit patterns of the last data-profile span of a few rows (a peek span, a pass-2 span at a fed-back
                CFO, a 3-codeword span, the R1/4 link whose control and data profiles coincide)

The reference's entries reset the waveform object before every process(); the rows of the DQPSK R1/4 link, where the receiver
runs process() twice on one object, are recorded that way too (window_restatement.py says why that is the same).
The QAM256 rows of the table are not in the fixture: OFDMChirpWaveform::configure (ofdm_chirp_waveform.cpp:81-89) turns QAM256
into DQPSK, so the compiled waveform has no such link; those rows are checked between the oracle and the library only.
Numeric arrays only.  --search looks, with the restatement on the oracle, for the seeds of the rows the table cannot build
by construction: the two small-frame branches and the recovery deltas."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pyoracle as po                # noqa: E402
import control_restatement as CR     # noqa: E402
import decode_frame_restatement as DF   # noqa: E402
import window_inputs as WI           # noqa: E402
import window_restatement as WR      # noqa: E402

LLR_ROWS = ("dqpsk_r12_var1", "qam16_r12_fixed_cfo1p5", "dqpsk_r12_var3", "dqpsk_r14_fixed")
ACQ_FIELDS = ("detected", "accepted", "sync_start", "frame_start", "delta", "candidates", "burst_interleaved")


def bits(*v):
    return np.array(v, np.float32).view(np.uint32)


def record(checker, rows=None):
    """every array of the fixture from one checker (the compiled reference when recording, the oracle when testing)"""
    rows = WI.reference_rows() if rows is None else rows
    out = {k: [] for k in ("fields", "words", "frame", "frame_bytes", "acq", "acq_words", "control", "n_spans", "pass2_cfo")}
    for r, e in zip(rows, WI.expected_all(checker, rows)):
        w, kw = WI.window(checker, r)
        out["fields"].append([int(e[k]) for k in WR.WINDOW_FIELDS])
        out["words"].append(bits(*(e[k] for k in WR.WINDOW_WORDS)))
        out["frame"].append([int(e["frame"][k]) for k in DF.RESULT_FIELDS])
        fb = np.zeros(64, np.uint8)
        n = min(64, len(e["frame"]["frame"]))
        fb[:n] = e["frame"]["frame"][:n]
        out["frame_bytes"].append(fb)
        out["acq"].append([int(e["acq"][k]) for k in ACQ_FIELDS])
        out["acq_words"].append(bits(e["acq"]["correlation"], e["acq"]["cfo_hz"]))
        out["control"].append([int(e["control"][k]) for k in CR.RESULT_FIELDS])
        out["n_spans"].append(len(e["spans"]))
        out["pass2_cfo"].append(bits(e["spans"][1][2] if len(e["spans"]) > 1 else 0.0)[0])
        if r["name"] in LLR_ROWS:
            s, n, cfo = e["spans"][-1]
            llr, _, _ = CR.process_span(checker, *WI.LINKS[r["link"]], w[s:s + n], float(cfo), kw["abs_base"] + s, False)
            out["llr_" + r["name"]] = llr.view(np.uint32).copy()
    for k in ("fields", "frame", "acq", "control", "n_spans"):
        out[k] = np.array(out[k], np.int32)
    for k in ("words", "acq_words"):
        out[k] = np.stack(out[k]).astype(np.uint32)
    out["pass2_cfo"] = np.array(out["pass2_cfo"], np.uint32)
    out["frame_bytes"] = np.stack(out["frame_bytes"])
    return out


def search(checker, what, link, kind, conditions, seeds):
    """first (channel kind, snr, seed) whose window reaches `what`: ("small", v) or ("delta", d)"""
    for ch, snr in conditions:
        for seed in seeds:
            r = WI.row(f"search_{link}_{kind}_{ch}_{snr}_{seed}", link, kind, 31, seed, "", chan=ch, snr=snr)
            w, kw = WI.window(checker, r)
            WI._cache.clear()
            if what[0] == "small":
                kw = dict(kw, retry=False)
            e = WR.rx_window(checker, *WI.LINKS[link], w, WI.SEARCH_LEN, **kw)
            hit = (e["small_frame"] & 0xF) == what[1] if what[0] == "small" else (e["outcome"] == WR.DECODED and e["acq"]["delta"] == what[1])
            if hit:
                return dict(link=link, kind=kind, chan=ch, snr=snr, seed=seed, small_frame=e["small_frame"], success=e["frame"]["success"],
                            delta=e["acq"]["delta"])
    return None


SMALL_SEARCH_SEEDS = range(5000, 5040)
# lead 300 puts the detected start 160 samples ahead of the frame, where QAM16 is at the edge of its timing tolerance and the
# primary candidate often fails whatever the span; lead 302 (start 148, 154 ahead) is the same search without that
SMALL_SEARCH_POINTS = tuple((kind, ch, snr, lead) for lead in (300, 302) for kind in ("var2", "var3") for ch in (WI.AWGN, WI.MODERATE)
                            for snr in (12.0, 10.0, 8.0, 6.0, 5.0, 4.0))


def small_search_point(point):
    """The issue's search for one (kind, channel, snr, lead): QAM16 frames of 2 / 3 codewords followed by noise, seeds
    SMALL_SEARCH_SEEDS, primary candidate only -> (point, windows that entered small-frame recovery, [(seed, small_frame,
    success)] of the windows that took one of its two branches)"""
    kind, ch, snr, lead = point
    O = po.Oracle()
    ran, hits = 0, []
    for seed in SMALL_SEARCH_SEEDS:
        r = WI.row(f"search_{kind}_{ch}_{snr}_{seed}", "qam16_r12", kind, 31, seed, "", chan=ch, snr=snr, retry=0, lead=lead)
        w, kw = WI.window(O, r)
        WI._cache.clear()
        e = WR.rx_window(O, *WI.LINKS["qam16_r12"], w, WI.SEARCH_LEN, **kw)
        ran += int(e["small_frame"] != 0)
        if (e["small_frame"] & 0xF) >= 2:
            hits.append((seed, int(e["small_frame"]), int(e["frame"]["success"])))
    return point, ran, hits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "window_frames.npz"))
    a = ap.parse_args()
    if a.search:
        from multiprocessing import Pool
        with Pool(a.jobs) as pool:
            for point, ran, hits in pool.imap(small_search_point, SMALL_SEARCH_POINTS):
                print("small-frame", point, "entered", ran, "branches", hits, flush=True)
        O = po.Oracle()
        low = tuple((WI.MODERATE, s) for s in (3.0, 2.0, 1.0, 0.0))
        print("small_frame 2, one codeword on the R1/4 link", search(O, ("small", 2), "dqpsk_r14", "var1", low, range(6000, 6300)), flush=True)
        print("small_frame 2, one codeword on DQPSK R1/2", search(O, ("small", 2), "dqpsk_r12", "var1", low, range(6000, 6300)), flush=True)
        print("delta -16, QAM16 R1/2", search(O, ("delta", -16), "qam16_r12", "fixed", ((WI.MODERATE, 12.0),), range(7000, 7200)), flush=True)
        return
    if not po.Ref.available():
        raise SystemExit("the compiled reference (oracle/_ref/libria_ref.so) is not built here")
    arrays = record(po.Ref())
    np.savez_compressed(a.out, **arrays)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
