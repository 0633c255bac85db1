"""CPU: the restatement of the variable-length frame calls and of the control hypothesis (tests/control_restatement.py) on
the pinned inputs (tests/control_inputs.py) equals what the compiled reference recorded (tests/golden/control_frames.npz,
tools/record_control_golden.py): transmitted samples, soft bits and status words bit for bit, the robust decode's outcome
and every field of the hypothesis.  The oracle is compared always; the compiled reference where it is built."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import pyoracle as po                   # noqa: E402
import control_inputs as CI             # noqa: E402
import control_restatement as R         # noqa: E402
import record_control_golden as REC     # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "control_frames.npz")
CHECKERS = ["oracle", pytest.param("ref", marks=pytest.mark.skipif(not po.Ref.available(), reason="the compiled reference is not built here"))]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module", params=CHECKERS)
def recorded(request):
    return REC.record(po.Oracle() if request.param == "oracle" else po.Ref())


def test_fixture_is_small_and_numeric(golden):
    assert os.path.getsize(GOLDEN) < 150 * 1024
    assert all(v.dtype.kind in "iuf" for v in golden.values())
    assert golden["outcome"].shape == (len(CI.SPANS), len(R.RESULT_FIELDS))


def test_restatement_equals_the_recorded_reference(golden, recorded):
    assert set(recorded) == set(golden)
    for k, v in golden.items():
        if k.startswith("tx_"):
            assert np.array_equal(recorded[k].view(np.uint32), v.view(np.uint32)), k
        elif k == "status":
            # snr_db (word 0) is 10 log10f of snr_linear (word 5, compared bit for bit): a display value, its last bits are the libm's
            assert np.array_equal(recorded[k][:, 1:], v[:, 1:]), k
            a, b = recorded[k][:, 0].view(np.float32), v[:, 0].view(np.float32)
            assert np.allclose(a, b, rtol=1e-5, atol=1e-5, equal_nan=True), k
        else:
            assert np.array_equal(recorded[k], v), k


def test_pinned_rows_reach_what_they_are_meant_to(golden):
    o = {row[0]: dict(zip(R.RESULT_FIELDS, golden["outcome"][i])) for i, row in enumerate(CI.SPANS)}
    for name in ("ack_awgn20", "nack_awgn20", "ack_mod10", "nack_mod10", "ack_cfo_marker", "ack_long_span", "ack_odd_span"):
        assert o[name]["success"] == 1 and o[name]["tries"] == 1, name
    assert [o[f"ack_tries{t}"]["tries"] for t in TRIES_PINNED] == list(TRIES_PINNED)
    assert all(o[f"ack_tries{t}"]["success"] == 1 for t in TRIES_PINNED)
    assert o["ack_lost"]["cw_ok"] == 0 and o["ack_lost"]["tries"] == 5 and o["ack_lost"]["process_ok"] == 1
    assert o["fixed_head"]["success"] == 0
    assert (o["data1"]["header_valid"], o["data1"]["total_cw"], o["data1"]["frame_type"], o["data1"]["success"]) == (1, 1, R.DATA, 0)
    assert (o["badcrc"]["cw_ok"], o["badcrc"]["magic"], o["badcrc"]["header_valid"], o["badcrc"]["success"]) == (1, 1, 0, 0)
    assert o["noise"]["success"] == 0 and o["silence"]["success"] == 0
    i_short = [r[0] for r in CI.SPANS].index("ack_short")
    assert o["ack_short"]["process_ok"] == 0 and o["ack_short"]["tries"] == 0 and golden["n_soft"][i_short] == 0
    # six data symbols of 106 soft bits: the demodulator has produced 636, twelve short of a codeword
    assert len(R.process_span(po.Oracle(), *CI.CTRL, CI.span(po.Oracle(), CI.SPANS[i_short]))[0]) == 636
    sent = {row[0]: CI.frame_bytes(row[1], row[2]) for row in CI.SPANS if row[1] in ("ack", "nack")}
    for i, row in enumerate(CI.SPANS):
        if golden["outcome"][i][R.RESULT_FIELDS.index("success")]:
            assert np.array_equal(golden["frames"][i], sent[row[0]]), row[0]
        else:
            assert not golden["frames"][i].any(), row[0]


TRIES_PINNED = tuple(t for t in (2, 3, 4, 5) if any(r[0] == f"ack_tries{t}" for r in CI.SPANS))


def test_soft_bits_of_a_short_span_are_the_head_of_a_longer_one():
    """the statement the issue rests on: 9 symbols give the first 742 soft bits of 15 symbols, bit for bit; the status words differ"""
    O = po.Oracle()
    row = next(r for r in CI.SPANS if r[0] == "ack_mod10")
    x = np.zeros(15 * R.SYM, np.float32)
    s = CI.clean_samples(O, row[1], row[2])
    x[:len(s)] = s
    y = O.channel(row[3], row[4], row[5], x)
    a, sa, _ = R.process_span(O, *CI.CTRL, y[:9 * R.SYM])
    b, sb, _ = R.process_span(O, *CI.CTRL, y)
    assert len(a) == 742 and np.array_equal(a.view(np.uint32), b[:742].view(np.uint32))
    assert sa["fading_index"] != sb["fading_index"]


def test_geometry_restatement():
    assert R.var_frame_samples(po.DQPSK, po.R1_4, 81) == 10368 == R.control_frame_samples(po.QAM16, po.R1_2) == R.control_frame_samples(po.DQPSK, po.R1_4)
    assert R.control_frame_samples(po.DBPSK, po.R1_2) == R.var_frame_samples(po.DBPSK, po.R1_2, 81) > 10368
    O = po.Oracle()
    for mod, rate in ((po.DQPSK, po.R1_4), (po.QAM16, po.R1_2), (po.D8PSK, po.R1_2), (po.QAM32, po.R3_4)):
        for nb in (1, 80, 81, 82, 162, 323, 324):
            assert len(O.modulate(mod, rate, REC.tx_bytes(nb))) == R.var_frame_samples(mod, rate, nb), (mod, rate, nb)
