"""The HIP transmit chain against the oracle over its whole input domain (tests/tx_domain_inputs.py): ria_gpu_tx_batch,
ria_gpu_encode_frames_batch, ria_gpu_tx_coded_batch (tx_frames_kernel<0>, <1>, <2>) and ria_gpu_make_frames
(make_frames_kernel), for all 9 modulations x 6 code rates, bit for bit, in every batch layout.
The oracle is pinned to the compiled reference on the same inputs by tests/test_tx_domain_cpu.py; make_frames and
peak_normalize are compared with the exact restatements of tx_domain_inputs.

Every comparison is equality of bits.  No NaN is compared: the only NaN of the peak rule is 0 * inf at peak +inf, and none
of the rows the peak values are tried on has an exactly zero sample (tests/test_tx_domain_cpu.py asserts that)."""
import ctypes as C
import re

import numpy as np
import pytest

import tx_domain_inputs as T

pytestmark = pytest.mark.gpu

MODE_NAMES = list(T.MODES)
REFUSED = ()                      # configurations ria_gpu_create answers RIA_ERR_UNSUPPORTED (shape_fits); none today
RIA_ERR_INVALID, RIA_ERR_UNSUPPORTED = -1, -4
_engines, _gpu, _orc = {}, {}, {}


def create(mode):
    """-> (engine or None, status of ria_gpu_create); engines are built once with a small workspace and kept"""
    from ria_amd import capi
    from ria_amd.engine import RxEngine
    if mode not in _engines:
        try:
            _engines[mode] = (RxEngine(*T.ENGINE[mode], max_batch=8), 0)
        except capi.RiaError as e:
            _engines[mode] = (None, int(re.search(r"status (-?\d+)", str(e)).group(1)))
    return _engines[mode]


def engine(mode):
    e, rc = create(mode)
    assert e is not None, f"{mode}: ria_gpu_create answered {rc}"
    return e


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(a, b):
    """device tensors, equal in every bit"""
    import torch
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and bool(torch.equal(a, b))


def gpu_answers(golden, oracle, mode):
    """the one-call run on the whole set (kept on the device, never modified): coded of the info rows, samples of the info
    rows through tx, samples of the coded rows through tx_coded, all at peak 0"""
    if mode not in _gpu:
        S = T.input_set(oracle, mode)
        assert T.digest(S) == str(golden("tx_domain")[f"sha_{mode}"]), f"{mode}: generator drifted"
        e = engine(mode)
        info, coded = dev(S["info"]), dev(S["coded"])
        _gpu[mode] = {"info": info, "coded": coded, "enc": e.encode_frames(info), "tx": e.tx(info, peak=0.0), "txc": e.tx_coded(coded, peak=0.0)}
    return _gpu[mode]


def oracle_answers(oracle, mode):
    if mode not in _orc:
        _orc.clear()                                     # one configuration's frames at a time (up to 8 MB)
        _orc[mode] = T.answers(oracle, oracle, mode)
    return _orc[mode]


# ---------------------------------------------------------------------------------------------- configurations
def test_accepted_configurations():
    """every configuration ria_gpu_create's argument checks take is created; one that the compiled decoder shape refuses
    answers RIA_ERR_UNSUPPORTED and is listed in REFUSED, not skipped"""
    status = {mode: create(mode)[1] for mode in MODE_NAMES}
    assert {m for m, rc in status.items() if rc != 0} == set(REFUSED), status
    assert all(status[m] == RIA_ERR_UNSUPPORTED for m in REFUSED)
    for mode in MODE_NAMES:
        if mode not in REFUSED:
            g = engine(mode).geo
            assert g.info_bytes_per_frame == 4 * T.BPC[T.MODES[mode][1]] and g.n_data_symbols <= 64 and g.n_data_carriers <= 59


ACCEPTED = [m for m in MODE_NAMES if m not in REFUSED]


# ---------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("mode", ACCEPTED)
def test_encoder_and_modulator_equal_the_oracle(golden, oracle, mode):
    S, G = T.input_set(oracle, mode), gpu_answers(golden, oracle, mode)
    coded_o, samples_o = oracle_answers(oracle, mode)
    n_info = len(S["info"])
    enc, tx, txc = G["enc"].cpu().numpy(), G["tx"].cpu().numpy(), G["txc"].cpu().numpy()
    bad = []
    for f in range(n_info):
        if not np.array_equal(enc[f], coded_o[f]):
            d = np.nonzero(np.unpackbits(enc[f] ^ coded_o[f]))[0]
            bad.append(f"encode_frames row {f} ({S['info_labels'][f]}): {len(d)} coded bits differ, first {d[0]}")
        if not np.array_equal(tx[f].view(np.uint32), samples_o[f].view(np.uint32)):
            d = np.nonzero(tx[f].view(np.uint32) != samples_o[f].view(np.uint32))[0]
            bad.append(f"tx row {f} ({S['info_labels'][f]}): {len(d)} samples differ, first {d[0]}: gpu {tx[f][d[0]]!r} oracle {samples_o[f][d[0]]!r}")
    for f in range(len(S["coded"])):
        o = samples_o[n_info + f]
        if not np.array_equal(txc[f].view(np.uint32), o.view(np.uint32)):
            d = np.nonzero(txc[f].view(np.uint32) != o.view(np.uint32))[0]
            bad.append(f"tx_coded row {f} ({S['coded_labels'][f]}): {len(d)} samples differ, first {d[0]} (symbol {d[0] // T.SYM}): gpu {txc[f][d[0]]!r} oracle {o[d[0]]!r}")
    for b in bad:
        print(b)
    assert not bad, f"{mode}: {len(bad)} rows differ from the oracle, first: {bad[0]}"
    assert float(np.abs(tx).max(1).min()) > 0 and float(np.abs(txc).max(1).min()) > 0, "max |s| > 0 on every row: the LTS symbols are never silent"


@pytest.mark.parametrize("mode", ACCEPTED)
def test_two_step_call_equals_the_one_step_call(golden, oracle, mode):
    e, G = engine(mode), gpu_answers(golden, oracle, mode)
    for p in (0.0, 0.8):
        assert same(e.tx_coded(e.encode_frames(G["info"]), peak=p), e.tx(G["info"], peak=p)), f"{mode} peak {p}"
    assert same(e.tx(G["info"], peak=0.0), G["tx"])


@pytest.mark.parametrize("mode", ACCEPTED)
def test_batch_layouts(golden, oracle, mode):
    """one row per call, 5 rows, the set repeated to 257 rows and the rows reversed give every row the bits of the one-call run"""
    import torch
    e, G = engine(mode), gpu_answers(golden, oracle, mode)
    calls = (("tx", "info", lambda x: e.tx(x, peak=0.0)), ("enc", "info", e.encode_frames), ("txc", "coded", lambda x: e.tx_coded(x, peak=0.0)))
    for what, src, fn in calls:
        n = len(G[src])
        layouts = [np.array([f]) for f in range(n)] + [np.arange(5), np.arange(n - 5, n), np.resize(np.arange(n), T.LAYOUT_ROWS), np.arange(n)[::-1].copy()]
        for idx in layouts:
            i = dev(idx.astype(np.int64))
            out = fn(G[src][i].contiguous())
            if not same(out, G[what][i]):
                rows = [int(idx[k]) for k in range(len(idx)) if not same(out[k], G[what][i[k]])]
                raise AssertionError(f"{mode} {what}: batch of {len(idx)} starting with row {idx[0]}: rows {rows[:8]} differ from the one-call run")
    torch.cuda.synchronize()


def test_instance_switching_and_streams(golden, oracle):
    """tx, encode_frames and tx_coded interleaved on two engines of different modes, on a side stream and on the default
    stream: the per-instance kernel attributes and the per-handle tables do not leak into each other"""
    import torch
    a, b = "QAM32_R5_6", "D8PSK_R1_4"
    ea, eb, Ga, Gb = engine(a), engine(b), gpu_answers(golden, oracle, a), gpu_answers(golden, oracle, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = []
    for rnd in range(3):
        with torch.cuda.stream(side):
            got.append(("side: b tx_coded", eb.tx_coded(Gb["coded"], peak=0.0), Gb["txc"]))
            got.append(("side: a encode_frames", ea.encode_frames(Ga["info"]), Ga["enc"]))
        got.append(("default: b tx", eb.tx(Gb["info"], peak=0.0), Gb["tx"]))
        got.append(("default: a tx_coded", ea.tx_coded(Ga["coded"], peak=0.0), Ga["txc"]))
        with torch.cuda.stream(side):
            got.append(("side: a tx", ea.tx(Ga["info"], peak=0.0), Ga["tx"]))
        got.append(("default: b encode_frames", eb.encode_frames(Gb["info"]), Gb["enc"]))
    side.synchronize()
    torch.cuda.synchronize()
    for what, out, want in got:
        assert same(out, want), what


# ---------------------------------------------------------------------------------------------- peak values
@pytest.mark.parametrize("mod", [m for m, _ in T.MODS])
def test_peak_values(golden, oracle, mod):
    """peak_normalize over 0, 0.8, 1, 1e-30, 1e-38 (denormal samples), 3e38 (the quotient overflows to inf on the rows that
    peak under 0.88, 14 of the 27, and stays finite on the others), -0.0, -1, NaN and +inf on three rows: the float32 rule of
    tx_domain_inputs.peak_rule applied to the oracle's unscaled frame"""
    mode = f"{mod}_R1_2"
    e, S, G = engine(mode), T.input_set(oracle, mode), gpu_answers(golden, oracle, mode)
    _, samples_o = oracle_answers(oracle, mode)
    n_info = len(S["info"])
    rows_i, row_c = T.peak_rows(S)                                              # a valid frame, a random row; a counter row
    for p in T.PEAKS:
        out = e.tx(G["info"][dev(np.array(rows_i))].contiguous(), peak=p).cpu().numpy()
        outc = e.tx_coded(G["coded"][row_c:row_c + 1].contiguous(), peak=p).cpu().numpy()
        for got, o, name in ((out[0], samples_o[rows_i[0]], "tx valid"), (out[1], samples_o[rows_i[1]], "tx random"), (outc[0], samples_o[n_info + row_c], "tx_coded counter")):
            assert np.abs(o).max() > 0
            want = T.peak_rule(o, p)
            if not T.same_bits(got, want):
                d = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
                raise AssertionError(f"{mode} {name} peak {p!r}: {len(d)} samples differ, first {d[0]}: gpu {got[d[0]]!r} rule {want[d[0]]!r} unscaled {o[d[0]]!r}")


# ---------------------------------------------------------------------------------------------- make_frames
SEEDS = (0, 1, 2 ** 32, 2 ** 64 - 1)
FIRST_SEQS = (0, 65530, 65535, 65536, 2 ** 31 - 17)


@pytest.mark.parametrize("rate_name,rate", T.RATES)
def test_make_frames_equals_the_restatement(oracle, rate_name, rate):
    e = engine(f"QAM16_{rate_name}")
    n = 9
    for seed in SEEDS:
        for first in FIRST_SEQS:
            got = e.make_frames(seed, first, n).cpu().numpy()
            want = T.make_frames(oracle, rate, seed, first, n)
            assert np.array_equal(got, want), f"{rate_name} seed {seed} first_seq {first}: frames {np.nonzero((got != want).any(1))[0]} differ"
            for i in (0, 4, 8):
                assert np.array_equal(e.make_frames(seed, first + i, 1).cpu().numpy()[0], got[i]), "a frame does not depend on how the batch is split"
    a = e.make_frames(5, 100, 4).cpu().numpy()
    hi = e.make_frames(5 + 2 ** 32, 100, 4).cpu().numpy()
    assert np.array_equal(a[:, :17], hi[:, :17]) and all(not np.array_equal(a[f, 17:-2], hi[f, 17:-2]) for f in range(4)), "the seed's high word is used"
    w = e.make_frames(5, 100 + 65536, 4).cpu().numpy()
    assert np.array_equal(a[:, :17], w[:, :17]) and all(not np.array_equal(a[f, 17:-2], w[f, 17:-2]) for f in range(4)), "same seq, other payload"
    # a negative first_seq counts as first_seq + 2^32 (include/ria_gpu.h): frames 2^32 - 3 .. 2^32 - 1, then 0 .. 5
    neg = e.make_frames(7, -3, n).cpu().numpy()
    assert np.array_equal(neg, T.make_frames(oracle, rate, 7, -3, n))
    assert np.array_equal(neg[3:], e.make_frames(7, 0, n - 3).cpu().numpy()) and [int(f[4]) << 8 | int(f[5]) for f in neg[:4]] == [65533, 65534, 65535, 0]
    # every frame is a frame of the oracle's builder with that payload
    for f in range(n):
        assert np.array_equal(oracle.make_frame(neg[f][17:-2], (f - 3) & 0xFFFF, rate), neg[f])


# ---------------------------------------------------------------------------------------------- arguments
def test_argument_validation(golden, oracle):
    import torch
    mode = "QAM16_R1_2"
    e, G = engine(mode), gpu_answers(golden, oracle, mode)
    L, h = e.lib, e.h
    info, coded = G["info"], G["coded"]
    fs, n = e.geo.frame_samples, 3
    canary_s = torch.full((n, fs), 7.25, dtype=torch.float32, device="cuda")
    canary_b = torch.full((n, 324), 0xA5, dtype=torch.uint8, device="cuda")
    canary_i = torch.full((n, info.shape[1]), 0xA5, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    calls = {
        "tx": lambda i, nf, o: L.ria_gpu_tx_batch(h, i, nf, 0.0, o, None),
        "tx_coded": lambda i, nf, o: L.ria_gpu_tx_coded_batch(h, i, nf, 0.0, o, None),
        "encode": lambda i, nf, o: L.ria_gpu_encode_frames_batch(h, i, nf, o, None),
    }
    ins = {"tx": info, "tx_coded": coded, "encode": info}
    outs = {"tx": canary_s, "tx_coded": canary_s, "encode": canary_b}
    for name, call in calls.items():
        for args in ((None, n, p(outs[name])), (p(ins[name]), n, None), (p(ins[name]), -1, p(outs[name]))):
            assert call(*args) == RIA_ERR_INVALID, name
            assert len(L.ria_gpu_last_error(h)) > 0 and name.split("_")[0].encode() in L.ria_gpu_last_error(h)
        assert call(p(ins[name]), 0, p(outs[name])) == 0, name
    assert L.ria_gpu_make_frames(h, 1, 0, n, None, None) == RIA_ERR_INVALID and b"make_frames" in L.ria_gpu_last_error(h)
    assert L.ria_gpu_tx_batch(h, None, n, 0.0, p(canary_s), None) == RIA_ERR_INVALID and b"make_frames" not in L.ria_gpu_last_error(h)
    assert L.ria_gpu_make_frames(h, 1, 0, -1, p(canary_i), None) == RIA_ERR_INVALID and b"make_frames" in L.ria_gpu_last_error(h)
    assert L.ria_gpu_make_frames(h, 1, 0, 0, p(canary_i), None) == 0
    assert L.ria_gpu_tx_batch(None, p(info), n, 0.0, p(canary_s), None) == RIA_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((canary_s == 7.25).all()) and bool((canary_b == 0xA5).all()) and bool((canary_i == 0xA5).all()), "n_frames 0 and refused calls write nothing"


# ---------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("mode", ACCEPTED)
def test_round_trip_through_the_receive_oracle(golden, oracle, mode):
    """one GPU-made valid frame per configuration through oracle.rx_process and oracle.decode_fixed_frame returns the info
    bytes: ties the suite to the receive oracle and not only to the transmit oracle"""
    mod, rate = T.MODES[mode]
    S, G = T.input_set(oracle, mode), gpu_answers(golden, oracle, mode)
    x = G["tx"][0].cpu().numpy()
    llr, _ = oracle.rx_process(mod, rate, x * np.float32(0.8 / np.abs(x).max()))
    data, ok, _, _ = oracle.decode_fixed_frame(llr, rate, True, engine(mode).geo.bits_per_symbol, flags=7)
    assert ok.all() and np.array_equal(data, S["info"][0]), f"{mode}: cw_ok {ok}"
