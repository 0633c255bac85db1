"""GPU tests (-m gpu) of the pruned recovery fill: recovery_stage1_kernel queues a fallback re-decode of codeword c only if
a substitution of c alone can make the frame verify (ria_amd/csrc/fallback_relevance.hpp) - CW0 always, CW c >= 1 only if
the header in CW0 parses and the frame's bytes reach into c.  RIA_OPT_FALLBACK_QUEUE_ALL = 1 queues every missing
re-decode, as before the rule.  Results must not depend on the option and must equal the CPU oracle's decodeFixedFrame;
the number of queued decodes (ria_gpu_debug_recovery_counts) must be what the oracle alone predicts.

The first sample is the one of tests/test_gpu_lazy_factors.py (faded QAM16 R1/2 frames of the bench workload's stream);
the second is constructed: confident soft bits of re-encoded codewords that hold short data frames, a control frame and a
full-length frame with a wrong CRC, at R1/2 and at R1/4 (another code shape, 20 bytes per codeword)."""
import numpy as np
import pytest

import pyoracle as po
from test_gpu_lazy_factors import FRAMES, STATUS_FIELDS, _check, _expected, _threads, clf
from test_gpu_lazy_factors import sample  # noqa: F401  (module-scoped fixture: the sample, the oracle's LLRs and classification)
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

CONTROL_TYPES = (0x10, 0x11, 0x16, 0x17, 0x20, 0x21, 0x15, 0x40)


def _crc(O, d, n):
    return int(O.lib.ro_crc16(po.up(np.ascontiguousarray(d[:n], np.uint8)), n))


def _codewords_read(O, data, bpc):
    """(header parses, number of leading codewords reassembleCodewords reads): restated here from frame_v2.cpp, in Python"""
    cw = data.reshape(4, bpc)
    d = cw[0]
    if d[0] != 0x55 or d[1] != 0x4C:
        return False, 0
    if int(d[2]) in CONTROL_TYPES:
        if _crc(O, d, 18) != (int(d[18]) << 8 | int(d[19])):
            return False, 0
        expected = 20
    else:
        if _crc(O, d, 15) != (int(d[15]) << 8 | int(d[16])):
            return False, 0
        expected = 17 + (int(d[13]) << 8 | int(d[14])) + 2
    n = read = 0
    for i in range(4):
        if n >= expected:
            break
        read += 1
        n += bpc - (2 if i != 0 and cw[i][0] == 0xD5 else 0)
    return True, read


def _relevant(O, data, bpc, queue_all):
    hdr, read = _codewords_read(O, data, bpc)
    return [True] * 4 if queue_all else [c == 0 or (hdr and c < read) for c in range(4)]


# ---- the bench workload's sample ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fallback_frames(oracle, sample):  # noqa: F811
    """per frame of the sample that reaches the fallback stage: the bytes stage 1 leaves, whether the header parses, and the
    bounds on the re-decodes queued for it (lower: codewords phase 0 never lists, all four factors missing; upper: also the
    factors of listed codewords behind their first converging one, which phase 0 skips or not depending on timing)"""
    _, llr, cls = sample
    rows = {}
    for q, c in enumerate(cls):
        if c["stage"] not in (2, 3):
            continue
        d3 = oracle.decode_fixed_frame(llr[q], po.R1_2, True, 188, flags=3)[0]
        hdr, read = _codewords_read(oracle, d3, 40)
        bounds = {}
        for queue_all in (False, True):
            rel = _relevant(oracle, d3, 40, queue_all)
            per_cw = [(0, 0) if not rel[cw] else (4, 4) if not c["listed"][cw] else (0, 4 - min(c["tstar"][cw], 4)) for cw in range(4)]
            bounds[queue_all] = per_cw
        # classify() calls a frame "repaired by stage 2" when the fallback's substitution gives the final bytes; where those
        # differ from the decoded ones in at most 4 bits stage 1's own flips may reach the same bytes first, and the frame
        # then never asks for a re-decode.  With an unparsable header stage 1 tries EVERY single bit and pair of bits of CW0
        # (frame_v2.cpp:1596-1640), so a difference of at most 2 bits, all in CW0, is certainly its repair.
        diff = d3 ^ c["full"][0]
        stage1 = "no"
        if c["stage"] == 2 and c["s2_ambiguous"]:
            stage1 = "yes" if not hdr and int(np.unpackbits(diff).sum()) <= 2 and not diff[40:].any() else "maybe"
        if stage1 != "no":
            for queue_all in (False, True):
                bounds[queue_all] = [(0, 0 if stage1 == "yes" else hi) for _, hi in bounds[queue_all]]
        rows[q] = {"hdr": hdr, "read": read, "bounds": bounds, "stage": c["stage"], "s2_cw": c["s2_index"] & 3, "stage1": stage1}
    return rows


def test_sample_has_both_header_cases(sample, fallback_frames):  # noqa: F811
    """from the oracle alone: what the GPU test below relies on cannot drift"""
    fb = fallback_frames
    assert len(fb) == 30
    assert sum(not r["hdr"] for r in fb.values()) == 12 and sum(r["hdr"] for r in fb.values()) == 18
    repairs = sorted((FRAMES[q], r["s2_cw"], r["hdr"]) for q, r in fb.items() if r["stage"] == 2)
    assert repairs == [(25749, 0, False), (27604, 1, True), (39139, 1, True), (41970, 0, False)]
    # of these, 41970 (two bits of an unparsable CW0) is within stage 1's exhaustive pair search and 27604 / 39139 (4 and 2
    # bits) may be within its suspect search: the bounds below count no decode for the first and no certain one for the others
    assert sorted((FRAMES[q], r["stage1"]) for q, r in fb.items() if r["stage1"] != "no") == [(27604, "maybe"), (39139, "maybe"), (41970, "yes")]
    for q, r in fb.items():          # every repair goes through a codeword the rule keeps
        if r["stage"] == 2:
            assert r["s2_cw"] == 0 or (r["hdr"] and r["s2_cw"] < r["read"])
    # no frame with an invalid header contributes a decode of CW1..3
    bad = [r for r in fb.values() if not r["hdr"]]
    assert sum(hi for r in bad for _, hi in r["bounds"][False][1:]) == 0
    assert sum(hi for r in bad for _, hi in r["bounds"][False]) <= 4 * len(bad)
    assert sum(lo for r in bad for lo, _ in r["bounds"][True][1:]) > 0          # which queueing everything does decode


def test_rx_batch_pruned_and_unpruned(oracle, sample, fallback_frames):  # noqa: F811
    """ria_gpu_rx_batch, un-split, queueing everything and pruned, each twice on one handle: the same bytes and decode status
    as the oracle in both modes; the queued decodes within the oracle's bounds, fewer when pruned"""
    import torch
    from ria_amd.engine import RxEngine
    y, _, cls = sample
    exp_d, exp_st = _expected(oracle, cls)
    e = RxEngine("QAM16", "R1_2", max_batch=len(y))
    e.set_split_parts(1)
    x = dev(y)
    queued, results = {}, {}
    for queue_all in (True, False):
        e.set_fallback_queue_all(int(queue_all))
        lower = sum(lo for r in fallback_frames.values() for lo, _ in r["bounds"][queue_all])
        upper = sum(hi for r in fallback_frames.values() for _, hi in r["bounds"][queue_all])
        for rep in range(2):
            out, st = e.rx(x)
            torch.cuda.synchronize()
            out, s = out.cpu().numpy(), e.decode_status(st)
            _check(out, s, exp_d, exp_st, f"queue_all {queue_all} run {rep}")
            cnt = e.recovery_counts(0)
            print(f"queue_all {queue_all} run {rep}: {cnt}, bounds {lower} .. {upper}")
            n_fb = sum(r["stage1"] == "no" for r in fallback_frames.values())
            n_maybe = sum(r["stage1"] == "maybe" for r in fallback_frames.values())
            assert cnt["flagged"] == sum(c["flagged"] for c in cls) and n_fb <= cnt["fallback"] <= n_fb + n_maybe
            assert lower <= cnt["queued"] <= upper, (queue_all, rep, cnt, lower, upper)
            assert cnt["list2"] <= cnt["queued"] <= 4 * cnt["list2"]
            queued[(queue_all, rep)] = cnt["queued"]
            results[(queue_all, rep)] = (out, s)
    for rep in range(2):
        assert queued[(False, rep)] < queued[(True, rep)]
        assert np.array_equal(results[(False, rep)][0], results[(True, rep)][0])
        for k in STATUS_FIELDS:
            assert np.array_equal(results[(False, rep)][1][k], results[(True, rep)][1][k]), k
    assert e.lib.ria_gpu_debug_queue_fault(e.h) == 0
    e.close()


# ---- constructed frames ------------------------------------------------------------------------------------------------------
def _frame_bytes(O, bpc, kind, rng):
    """4 * bpc bytes of four codewords: a frame of the given kind with a wrong CRC, random bytes behind it"""
    data = rng.integers(0, 256, 4 * bpc, dtype=np.uint8)
    data[0], data[1] = 0x55, 0x4C
    if kind == "control":
        data[2] = 0x16
        c = _crc(O, data, 18)
        data[18], data[19] = c >> 8, c & 0xFF
        return data
    plen, marker = kind
    data[2] = 0x01
    data[13], data[14] = plen >> 8, plen & 0xFF
    h = _crc(O, data, 15)
    data[15], data[16] = h >> 8, h & 0xFF
    frame = data[:17 + plen + 2].copy()
    c = _crc(O, frame, 17 + plen)
    frame[17 + plen], frame[18 + plen] = c >> 8, c & 0xFF
    cw, n = data.reshape(4, bpc), 0
    for i in range(4):
        off = 0
        if i in marker:
            cw[i][0], off = 0xD5, 2
        take = min(len(frame) - n, bpc - off)
        cw[i][off:off + take] = frame[n:n + take]
        n += take
        if i != 0 and off == 0 and cw[i][0] == 0xD5:
            if take > 0:
                return None          # a frame byte that reads as a marker: the caller draws again
            cw[i][0] = 0x5D
    return data


def _constructed(O, mod, rate, e):
    """8 frames of confident LLRs, the oracle's answer for each, and the codewords the fallback reads of each"""
    bpc, bps, k = int(e.geo.bytes_per_codeword), int(e.geo.bits_per_symbol), int(e.geo.ldpc_k)
    nb = (k + 7) // 8
    table = O.gather_table(bps, True)
    # payload lengths that end inside CW0, CW1 (once behind a 0xD5 marker) and CW2, at the end of CW1, the largest, a control
    # frame, and a data frame whose header CRC is wrong as well
    kinds = [(1, ()), (bpc, ()), (bpc - 2, (1,)), (2 * bpc, ()), (2 * bpc - 19, ()), (4 * bpc - 19, ()), "control", (bpc + 3, ())]
    llr = np.zeros((len(kinds), max(2592, int(e.geo.llrs_per_frame))), np.float32)
    exp, reads = [], []
    for q, kind in enumerate(kinds):
        for attempt in range(32):        # a corruption stage 1 cannot repair: chosen with the oracle alone
            rng = np.random.default_rng([70707, bpc, q, attempt])
            data = _frame_bytes(O, bpc, kind, rng)
            if data is None:
                continue
            if kind == "control":
                data[18] ^= 0x21; data[19] ^= 0x84
            else:
                end = 17 + kind[0] + 2          # the stored frame CRC, found through the reassembly
                cw, n = data.reshape(4, bpc), 0
                for i in range(4):
                    off = 2 if i in kind[1] else 0
                    take = min(end - n, bpc - off)
                    for p in (end - 2, end - 1):
                        if n <= p < n + take:
                            cw[i][off + p - n] ^= 0x21 if p == end - 2 else 0x84
                    n += take
                if q == 7:
                    data[16] ^= 0x42
            for c in range(4):
                info = np.zeros(nb, np.uint8)
                info[:bpc] = data[c * bpc:(c + 1) * bpc]
                bits = np.unpackbits(O.ldpc_encode(rate, info)[:81])[:648].astype(np.float32)
                llr[q, table[c * 648:(c + 1) * 648]] = (1.0 - 2.0 * bits) * 8.0
            r = O.decode_fixed_frame(llr[q], rate, True, bps, flags=7)
            r3 = O.decode_fixed_frame(llr[q], rate, True, bps, flags=3)
            assert r3[1].all() and np.array_equal(r3[0], data)          # four first-try codewords holding these bytes
            if not r[1].any():
                break
        else:
            raise AssertionError(f"no unrepairable corruption found for frame {q}")
        exp.append(r)
        reads.append(_codewords_read(O, data, bpc))
    return kinds, llr, exp, reads


@pytest.mark.parametrize("mod,rate", [("QAM16", "R1_2"), ("DQPSK", "R1_4")])
def test_constructed_short_frames(oracle, mod, rate):
    """ria_gpu_decode_batch with the full flags: results equal the oracle, and exactly 4 re-decodes are queued per codeword
    the fallback reads of each unrepaired frame (no codeword is listed for phase 0: every first decode converges)"""
    from test_gpu_parity import engine
    e = engine(mod, rate)
    kinds, llr, exp, reads = _constructed(oracle, getattr(po, mod), getattr(po, rate), e)
    bpc = int(e.geo.bytes_per_codeword)
    assert [r for _, r in reads[:6]] == [1, 2, 2, 3, 2, 4] and [h for h, _ in reads] == [True] * 6 + [False] * 2
    want = {False: 4 * sum(max(r, 1) for _, r in reads), True: 16 * len(kinds)}
    x = dev(llr)
    try:
        for queue_all in (True, False, True, False):
            e.set_fallback_queue_all(int(queue_all))
            out, st = e.decode(x, flags=7)
            out, s = out.cpu().numpy(), e.decode_status(st)
            for q in range(len(kinds)):
                d, ok, iters, att = exp[q]
                assert np.array_equal(s["cw_ok"][q], ok) and np.array_equal(out[q], d), f"queue_all {queue_all} frame {kinds[q]}"
                assert np.array_equal(s["iterations"][q], iters.astype(np.uint16)) and np.array_equal(s["attempts"][q], att.astype(np.uint8))
                assert s["frame_valid"][q] == 0 and s["needs_recovery"][q] == 0
            cnt = e.recovery_counts(0)
            print(f"{rate} bpc {bpc} queue_all {queue_all}: {cnt}")
            assert cnt["flagged"] == len(kinds) and cnt["fallback"] == len(kinds)
            assert cnt["queued"] == want[queue_all], (queue_all, cnt, want)
    finally:
        e.set_fallback_queue_all(0)
    assert e.lib.ria_gpu_debug_queue_fault(e.h) == 0
