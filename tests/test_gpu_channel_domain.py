"""The reference-identical channel (ria_gpu_channel_exact_batch, _seeded_batch, _cfo_batch: channel_power_kernel,
channel_exact_kernel) and the transmitter frequency offset (ria_gpu_tx_cfo_batch: txcfo_phase_kernel, txcfo_fft_pass<1..6>,
txcfo_rotate_kernel) over their input domain (tests/channel_domain_inputs.py), through the C ABI.

The expectation is the compiled reference where oracle/_ref travelled with the tree, else the oracle, which
tests/test_channel_domain_cpu.py pins to the reference on the same rows.  The rule of every comparison: the float32 bits are
equal wherever the expected value is not NaN; where it is NaN the device's value is NaN (sign and payload not compared).  No
tolerance anywhere.  A tx_cfo buffer with a NaN or infinite sample is outside bit identity (include/ria_gpu.h): every sample
of its output is non-finite and the other buffers of the batch are exact."""
import ctypes as C

import numpy as np
import pytest

import channel_domain_inputs as D
import pyoracle as po

pytestmark = pytest.mark.gpu

RIA_ERR_INVALID, RIA_ERR_UNSUPPORTED = -1, -4
SENT = D.word(D.SENTINEL)
_state = {}


def new_engine():
    from ria_amd.engine import RxEngine
    return RxEngine("QAM16", "R1_2", max_batch=8)


def engine():
    if "e" not in _state:
        _state["e"] = new_engine()
    return _state["e"]


def expected(oracle):
    if "E" not in _state:
        _state["E"] = D.answers(po.Ref() if po.Ref.available() else oracle, oracle)
    return _state["E"]


def up(a, dtype):
    """host array -> device tensor of 32-bit words (int32, so that no NaN payload is touched)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype).view(np.int32)).cuda()


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def padded(X, n, stride):
    host = np.full((len(X), stride), SENT, np.uint32)
    host[:, :n] = np.stack([D.bits(x) for x in X]).reshape(len(X), n)
    return host


def unpad(t, n, what):
    """device words [rows, stride] -> float32 [rows, n]; the padding still holds the sentinel"""
    out = t.cpu().numpy().view(np.uint32)
    assert (out[:, n:] == SENT).all(), f"{what}: padding behind the {n} samples of a row was written"
    return np.ascontiguousarray(out[:, :n]).view(np.float32)


def chan(e, call, kind, snr, X, seeds=None, seed=0, first_frame=0, cfo=None, rmax=0.0, actual=True, extra=0):
    """one channel call on the frames X (equal lengths) at stride n + extra -> (float32 [nf, n], getActualCFO float32 [nf] or None)"""
    import torch
    n, nf = len(X[0]), len(X)
    buf = up(padded(X, n, n + extra), np.uint32)
    sd = up(np.asarray(seeds, np.uint32), np.uint32) if seeds is not None else None
    act = None
    if call == "plain":
        rc = e.lib.ria_gpu_channel_exact_batch(e.h, kind, snr, seed, first_frame, p(buf), n + extra, n, nf, None)
    elif call == "seeded":
        rc = e.lib.ria_gpu_channel_exact_seeded_batch(e.h, kind, snr, p(sd), p(buf), n + extra, n, nf, None)
    else:
        cf = up(np.asarray(cfo, np.float32), np.float32) if cfo is not None else None
        act = up(np.full(nf + 2, D.SENTINEL, np.float32), np.float32) if actual else None
        rc = e.lib.ria_gpu_channel_exact_cfo_batch(e.h, kind, snr, p(sd), p(cf), rmax, p(act), p(buf), n + extra, n, nf, None)
    assert rc == 0, (call, rc, e.lib.ria_gpu_last_error(e.h))
    torch.cuda.synchronize()
    if act is not None:
        a = act.cpu().numpy().view(np.uint32)
        assert (a[nf:] == SENT).all(), "actual_cfo_out written behind n_frames"
        act = a[:nf].view(np.float32)
    return unpad(buf, n, f"{call} kind {kind} n {n} stride {n + extra}"), act


def tx_cfo(e, X, cfo, phase, extra_in=0, extra_out=0):
    """-> (float32 [nb, n], accumulators after float32 [nb] or None); the input tensor is unchanged"""
    import torch
    n, nb = len(X[0]), len(X)
    src_host = padded(X, n, n + extra_in)
    src, out = up(src_host, np.uint32), up(np.full((nb, n + extra_out), SENT, np.uint32), np.uint32)
    cf = up(np.asarray(cfo, np.float32), np.float32)
    ph = up(np.concatenate([np.asarray(phase, np.float32), np.full(2, D.SENTINEL, np.float32)]), np.float32) if phase is not None else None
    rc = e.lib.ria_gpu_tx_cfo_batch(e.h, p(src), n + extra_in, n, nb, p(cf), p(ph), p(out), n + extra_out, None)
    assert rc == 0, (rc, e.lib.ria_gpu_last_error(e.h))
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy().view(np.uint32), src_host), "tx_cfo wrote to its input"
    if ph is not None:
        a = ph.cpu().numpy().view(np.uint32)
        assert (a[nb:] == SENT).all(), "phase accumulators written behind n_buffers"
        ph = a[:nb].view(np.float32)
    return unpad(out, n, f"tx_cfo n {n} out_stride {n + extra_out}"), ph


def answer(E, r):
    """E: (channel answers, tx_cfo answers) of channel_domain_inputs.answers -> (samples, actual CFO or accumulator) of a row"""
    return E[0 if "kind" in r else 1][(r["family"], r["label"])]


def check(rows, got, E, what=""):
    """rows with their device answers [(samples, scalar or None)] against the expectation; every failing row is reported"""
    bad = []
    for r, (y, a) in zip(rows, got):
        ey, ea = answer(E, r)
        m = D.explain(r, y, ey)
        if not m and a is not None:
            m = D.explain(r, [a], [ea], "actual CFO" if "kind" in r else "accumulator")
        if m:
            bad.append(what + m)
    assert not bad, f"{len(bad)} of {len(rows)} rows differ:\n" + "\n".join(bad[:12])


def groups(rows, key):
    g = {}
    for r in rows:
        g.setdefault(key(r), []).append(r)
    return g.values()


def run_channel(e, rows, E, actual=True, what=""):
    """rows with the same call, preset, length, SNR and random_cfo_max_hz go into one call; plain rows through the seeded call"""
    n_calls = 0
    for g in groups(rows, lambda r: (r["call"], r["kind"], len(r["x"]), D.word(r["snr"]), D.word(r["rmax"]))):
        r0 = g[0]
        seeds = [r["seed"] for r in g]
        if r0["call"] == "plain":
            Y, A = chan(e, "seeded", r0["kind"], r0["snr"], [r["x"] for r in g], seeds)
        else:
            Y, A = chan(e, "cfo", r0["kind"], r0["snr"], [r["x"] for r in g], seeds, cfo=[r["cfo"] for r in g], rmax=r0["rmax"], actual=actual)
        check(g, [(Y[i], A[i] if A is not None else None) for i in range(len(g))], E, what)
        n_calls += 1
    return n_calls


def run_tx(e, rows, E, what=""):
    for g in groups(rows, lambda r: (len(r["x"]), r["phase"] is None)):
        null = g[0]["phase"] is None
        Y, P = tx_cfo(e, [r["x"] for r in g], [r["cfo"] for r in g], None if null else [r["phase"] for r in g])
        exact = [i for i, r in enumerate(g) if r["cls"] != "nan_sample"]
        check([g[i] for i in exact], [(Y[i], None if null else P[i]) for i in exact], E, what)
        for i, r in enumerate(g):
            if r["cls"] == "nan_sample":
                assert not np.isfinite(Y[i]).any(), f"{r['family']} / {r['label']}: {int(np.isfinite(Y[i]).sum())} finite samples, first at {int(np.nonzero(np.isfinite(Y[i]))[0][0])}"
                assert D.explain(r, [P[i]], [answer(E, r)[1]], "accumulator") == ""


# ---------------------------------------------------------------------------------------------- channel
@pytest.mark.parametrize("family", ["lengths", "levels", "snr", "bench"])
def test_channel_family(oracle, golden, family):
    if family == "lengths":
        assert D.digest(oracle) == str(golden("channel_domain")["sha"]), "generator drifted"
    rows = D.select(D.rows(oracle)[0], family)
    assert len({r["kind"] for r in rows}) == (1 if family == "bench" else 5)
    run_channel(engine(), rows, expected(oracle))


def test_channel_seeds(oracle):
    """the seeded call at SEEDS; the plain call where seed + first_frame + f wraps 2^32 inside the batch and where
    first_frame exceeds 2^32; the plain, the seeded and the cfo call (NULL offsets, no draw) give the same bits"""
    e, E = engine(), expected(oracle)
    ch = D.rows(oracle)[0]
    rows = D.select(ch, "seeds")
    run_channel(e, rows, E)
    for kind in D.KINDS:
        R = {r["seed"]: r for r in rows if r["kind"] == kind}
        assert set(D.SEEDS) <= set(R)
        for seed, first, nf in D.WRAP:
            g = [R[(seed + first + f) & 0xffffffff] for f in range(nf)]
            x = [r["x"] for r in g]
            Y, _ = chan(e, "plain", kind, g[0]["snr"], x, seed=seed, first_frame=first)
            check(g, [(y, None) for y in Y], E, f"plain call seed {seed:#x} first_frame {first:#x}: ")
            Ys, _ = chan(e, "seeded", kind, g[0]["snr"], x, [r["seed"] for r in g])
            Yc, A = chan(e, "cfo", kind, g[0]["snr"], x, [r["seed"] for r in g], cfo=None, rmax=0.0)
            assert np.array_equal(D.bits(Y), D.bits(Ys)) and np.array_equal(D.bits(Y), D.bits(Yc)), (kind, seed, first)
            assert (D.bits(A) == 0).all(), "getActualCFO() of NULL offsets is +0.0"


@pytest.mark.parametrize("kind", D.KINDS)
def test_channel_batches(oracle, kind):
    """1, 63, 64, 65 and 130 frames: one block of the power kernel, one short of it, one more; a frame's result does not
    depend on the batch it sat in"""
    e, E = engine(), expected(oracle)
    rows = D.select(D.rows(oracle)[0], "batch", kind=kind)
    assert len(rows) == max(D.BATCHES)
    for nf in D.BATCHES:
        g = rows[-nf:] if nf == 65 else rows[:nf]          # 65: other frames in the lanes
        Y, _ = chan(e, "seeded", kind, g[0]["snr"], [r["x"] for r in g], [r["seed"] for r in g])
        check(g, [(y, None) for y in Y], E, f"batch of {nf}: ")


def test_channel_workspace_growth(oracle):
    """4097 frames as the first channel call of a fresh handle (the per-frame sigma workspace starts at 4096), then 3 frames"""
    E = expected(oracle)
    rows = D.select(D.rows(oracle)[0], "grow")
    assert len(rows) == D.GROW == 4097
    e = new_engine()
    try:
        for g in (rows, rows[:3], rows[4000:]):
            Y, _ = chan(e, "seeded", 2, g[0]["snr"], [r["x"] for r in g], [r["seed"] for r in g])
            check(g, [(y, None) for y in Y], E, f"batch of {len(g)}: ")
    finally:
        e.close()


def test_channel_strides(oracle):
    """stride = n + 1, 7, 64 with a sentinel in the padding, for the three calls: rows equal the dense expectation and the
    padding is untouched (chan() asserts it)"""
    e, E = engine(), expected(oracle)
    ch = D.rows(oracle)[0]
    for kind in D.KINDS:
        a = [r for r in D.select(ch, "stride", kind=kind) if r["call"] == "plain"]
        b = [r for r in D.select(ch, "stride", kind=kind) if r["call"] == "cfo"]
        assert len(a) == 3 and len(b) == 3 and [r["seed"] for r in a] == [5000, 5001, 5002]
        for extra in D.STRIDE_EXTRA:
            xa, sa = [r["x"] for r in a], [r["seed"] for r in a]
            for call, kw in (("plain", dict(seed=4990, first_frame=10)), ("seeded", dict(seeds=sa)), ("cfo", dict(seeds=sa, cfo=None))):
                Y, _ = chan(e, call, kind, a[0]["snr"], xa, extra=extra, **kw)
                check(a, [(y, None) for y in Y], E, f"{call} call, stride n + {extra}: ")
            Y, A = chan(e, "cfo", kind, b[0]["snr"], [r["x"] for r in b], [r["seed"] for r in b], cfo=[r["cfo"] for r in b], extra=extra)
            check(b, list(zip(Y, A)), E, f"cfo call, stride n + {extra}: ")


def test_channel_cfo(oracle):
    """every offset of CFOS, both sides of the 0.001 Hz gate and of the 256-sample gate, gated and ungated frames in one
    call; actual_cfo_out NULL gives the same samples"""
    e, E = engine(), expected(oracle)
    rows = D.select(D.rows(oracle)[0], "cfo")
    n_calls = run_channel(e, rows, E)
    assert n_calls < len(rows) / 4, "offsets are mixed within calls"
    run_channel(e, [r for r in rows if len(r["x"]) in (255, 320)], E, actual=False, what="actual_cfo_out NULL: ")


def test_channel_random_cfo(oracle):
    """random_cfo_max_hz from the smallest denormal to +inf: the draw replaces the configured 25 Hz; getActualCFO() is
    compared bit for bit, as "is NaN" where the reference's is (0 * inf at +inf)"""
    e, E = engine(), expected(oracle)
    rows = D.select(D.rows(oracle)[0], "random")
    assert len(rows) == 2 * 2 * len(D.RANDOM_MAX) and all(r["cfo"] == 25.0 for r in rows)
    run_channel(e, rows, E)
    assert all(D.word(answer(E, r)[1]) != D.word(25.0) for r in rows)


# ---------------------------------------------------------------------------------------------- tx_cfo
@pytest.mark.parametrize("family", ["lengths", "offsets", "accumulators", "samples"])
def test_tx_cfo_family(oracle, family):
    run_tx(engine(), D.select(D.rows(oracle)[1], family), expected(oracle))


def test_tx_cfo_continuation(oracle):
    """the second call starts from the accumulators the device returned for the first; after it the accumulator equals the
    one of a single walk over both lengths"""
    e, E = engine(), expected(oracle)
    T = D.by_label(D.rows(oracle)[1], "continue")
    cfos = (50.0, -2400.0)
    first, second, walk = ([T[f"{s} cfo {c}"] for c in cfos] for s in ("first call", "second call", "one walk"))
    Y1, P1 = tx_cfo(e, [r["x"] for r in first], cfos, [r["phase"] for r in first])
    check(first, list(zip(Y1, P1)), E)
    Y2, P2 = tx_cfo(e, [r["x"] for r in second], cfos, P1)
    check(second, list(zip(Y2, P2)), E, "continued: ")
    Yw, Pw = tx_cfo(e, [r["x"] for r in walk], cfos, [r["phase"] for r in walk])
    check(walk, list(zip(Yw, Pw)), E)
    assert np.array_equal(D.bits(P2), D.bits(Pw))


def test_tx_cfo_nonfinite_samples(oracle):
    """a NaN or infinite sample in an active buffer: every sample of that buffer's output is non-finite; the other buffers
    of the same call (finite ones, and copies below the gate that carry the sample through) are exact"""
    tx = D.rows(oracle)[1]
    rows = D.select(tx, "nonfinite") + [r for r in D.select(tx, "offsets") if r["cls"] == "finite"]
    assert sum(r["cls"] == "nan_sample" for r in rows) == 3 and len({len(r["x"]) for r in rows}) == 1
    run_tx(engine(), rows[::2] + rows[1::2], expected(oracle))


def test_tx_cfo_strides(oracle):
    e, E = engine(), expected(oracle)
    rows = [r for r in D.select(D.rows(oracle)[1], "offsets") if r["label"].startswith(("cfo 50.0[", "cfo -12.5[", "cfo 0.0["))]
    assert len(rows) == 3
    for ei, eo in ((1, 64), (7, 1), (64, 7), (0, 7), (7, 0)):
        Y, P = tx_cfo(e, [r["x"] for r in rows], [r["cfo"] for r in rows], [r["phase"] for r in rows], extra_in=ei, extra_out=eo)
        check(rows, list(zip(Y, P)), E, f"stride n + {ei}, out_stride n + {eo}: ")


def tiled_tx(e, rows, n_buffers, E):
    """n_buffers buffers tiled from the distinct rows, compared on the device with the tiled expectation (no NaN in it)"""
    import torch
    k, n = len(rows), len(rows[0]["x"])
    idx = torch.arange(n_buffers, device="cuda") % k
    src = up(np.stack([r["x"] for r in rows]), np.float32)[idx].contiguous()
    cf = up(np.array([r["cfo"] for r in rows], np.float32), np.float32)[idx].contiguous()
    ph = up(np.array([r["phase"] for r in rows], np.float32), np.float32)[idx].contiguous()
    exp = up(np.stack([answer(E, r)[0] for r in rows]), np.float32)
    exp_ph = up(np.array([answer(E, r)[1] for r in rows], np.float32), np.float32)
    assert not bool(np.isnan(exp.cpu().numpy().view(np.float32)).any())
    out = torch.full((n_buffers, n), SENT, dtype=torch.int32, device="cuda")
    rc = e.lib.ria_gpu_tx_cfo_batch(e.h, p(src), n, n, n_buffers, p(cf), p(ph), p(out), n, None)
    assert rc == 0, (rc, e.lib.ria_gpu_last_error(e.h))
    torch.cuda.synchronize()
    wrong = (out != exp[idx]).any(1) | (ph != exp_ph[idx])
    if bool(wrong.any()):
        b = int(torch.nonzero(wrong)[0])
        y = out[b].cpu().numpy().view(np.float32)
        pytest.fail(f"{int(wrong.sum())} of {n_buffers} buffers differ, first {b}: " + D.explain(rows[b % k], y, answer(E, rows[b % k])[0]))


def test_tx_cfo_chunks(oracle):
    """32 769 buffers of 2 samples cross the 32 768-buffer pass; one buffer more than fit 256 MiB of workspace at 131072
    samples (the count comes from the rule stated at the call, channel_domain_inputs.txcfo_chunk) crosses the other limit"""
    e, E = engine(), expected(oracle)
    tx = D.rows(oracle)[1]
    small = [r for r in D.select(tx, "chunks") if r["label"].startswith("small")]
    large = [r for r in D.select(tx, "chunks") if r["label"].startswith("large")]
    assert len(small) == 16 and len(large) == 4 and D.txcfo_chunk(2, 32769) == 32768
    tiled_tx(e, small, 32769, E)
    per_pass = D.txcfo_chunk(D.TXCFO_MAX, 10 ** 6)
    assert 64 <= per_pass <= 128
    tiled_tx(e, large, per_pass + 1, E)


# ---------------------------------------------------------------------------------------------- arguments
def test_argument_checks(oracle):
    """refused calls answer the documented status, leave a message and launch nothing; empty calls are RIA_OK and write
    nothing (every buffer holds a sentinel before and after)"""
    import torch
    e = engine()
    L, h = e.lib, e.h
    n, nf = 300, 3
    buf = torch.full((nf, n + 4), 7.25, dtype=torch.float32, device="cuda")
    out = torch.full((nf, n + 4), 7.25, dtype=torch.float32, device="cuda")
    sd = torch.full((nf,), 9, dtype=torch.int32, device="cuda")
    cf = torch.full((nf,), 50.0, dtype=torch.float32, device="cuda")
    ph = torch.full((nf,), 7.25, dtype=torch.float32, device="cuda")
    act = torch.full((nf,), 7.25, dtype=torch.float32, device="cuda")
    S = n + 4
    plain = lambda kind=0, s=p(buf), st=S, ns=n, f=nf: L.ria_gpu_channel_exact_batch(h, kind, 20.0, 1, 0, s, st, ns, f, None)
    seeded = lambda kind=0, s=p(buf), st=S, ns=n, f=nf, sp=p(sd): L.ria_gpu_channel_exact_seeded_batch(h, kind, 20.0, sp, s, st, ns, f, None)
    cfo = lambda kind=0, s=p(buf), st=S, ns=n, f=nf, sp=p(sd), rmax=0.0: L.ria_gpu_channel_exact_cfo_batch(h, kind, 20.0, sp, p(cf), rmax, p(act), s, st, ns, f, None)
    txc = lambda i=p(buf), st=S, ns=n, nb=nf, c=p(cf), o=p(out), ost=S: L.ria_gpu_tx_cfo_batch(h, i, st, ns, nb, c, p(ph), o, ost, None)

    def refused(rc, name, status=RIA_ERR_INVALID):
        assert rc == status, (name, rc)
        msg = L.ria_gpu_last_error(h)
        assert len(msg) > 0 and name.encode() in msg, (name, msg)

    for name, call in (("ria_gpu_channel_exact_batch", plain), ("ria_gpu_channel_exact_seeded_batch", seeded), ("ria_gpu_channel_exact_cfo_batch", cfo)):
        for kw in (dict(kind=-1), dict(kind=5), dict(f=-1), dict(ns=-1), dict(st=n - 1), dict(s=None)):
            refused(call(**kw), name)
        assert call(f=0) == 0 and call(ns=0) == 0 and call(f=0, s=None) == 0, name
    refused(seeded(sp=None), "ria_gpu_channel_exact_seeded_batch")
    refused(cfo(sp=None), "ria_gpu_channel_exact_cfo_batch")
    for rmax in (-1.0, -1e-45, float("nan"), float("-inf")):
        refused(cfo(rmax=rmax), "ria_gpu_channel_exact_cfo_batch")
    for kw in (dict(o=p(buf)), dict(c=None), dict(ost=n - 1), dict(st=n - 1), dict(i=None), dict(o=None), dict(nb=-1), dict(ns=-1)):
        refused(txc(**kw), "ria_gpu_tx_cfo_batch")
    refused(txc(ns=131073, st=131073, ost=131073), "ria_gpu_tx_cfo_batch", RIA_ERR_UNSUPPORTED)
    assert txc(ns=0) == 0 and txc(nb=0) == 0
    torch.cuda.synchronize()
    for t in (buf, out, ph, act):
        assert bool((t == 7.25).all()), "a refused or an empty call wrote something"
    assert bool((sd == 9).all()) and bool((cf == 50.0).all())
