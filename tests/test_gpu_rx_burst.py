"""GPU tests (-m gpu) of ria_gpu_rx_burst_batch: burst-interleaved groups and burst continuation in one call.  Bit-exact
against the recorded reference groups (tests/golden/burst_chain.npz), against the CPU restatement
(tests/burst_restatement.py) on a scenario set that holds every stop reason and both modes, against the existing separate
calls, and independent of batching and of what the handle did before."""
import ctypes as C

import numpy as np
import pytest

import burst_restatement as br
import pyoracle as po
from test_gpu_parity import bits, dev, engine
from test_oracle_golden import burst_cases
from test_rx_burst_cpu import scenario_results

pytestmark = pytest.mark.gpu

RES_FIELDS = ("detected", "accepted", "sync_start", "frame_start", "delta", "candidates", "burst_interleaved", "mode", "frames",
              "frames_decoded", "stop")


def assert_equal_to_restatement(tag, out, i, r):
    """window i of an rx_burst() result against the restatement's dict r, every field"""
    res = out["result"]
    for f in RES_FIELDS:
        assert int(res[f][i]) == int(r[f]), (tag, f, int(res[f][i]), int(r[f]))
    assert bits(res["correlation"][i]) == bits(r["correlation"]) and bits(res["cfo_hz"][i]) == bits(r["cfo_hz"]), (tag, "correlation / cfo")
    assert not res["reserved"][i].any()
    assert np.array_equal(bits(out["cfo_used"][i]), bits(r["cfo_used"])), (tag, out["cfo_used"][i], r["cfo_used"])
    assert np.array_equal(bits(out["rms"][i]), bits(r["rms"])), (tag, out["rms"][i], r["rms"])
    st = out["decode_status"][i]
    assert np.array_equal(out["info"][i], r["info"]), (tag, "bytes")
    assert np.array_equal(st["cw_ok"], r["cw_ok"]) and np.array_equal(st["iterations"], r["iterations"]), (tag, "decode status")
    assert np.array_equal(st["attempts"], r["attempts"]) and np.array_equal(st["frame_valid"], r["frame_valid"]), (tag, "attempts / frame_valid")
    fst = out["frame_status"][i]
    for f in range(br.SLOTS):
        a = r["aux"][f]
        if a is None:
            assert not fst[f].tobytes().strip(b"\0"), (tag, f, "demod status of a frame that did not run")
            continue
        for name in br.AUX_FIELDS[1:]:
            assert bits(fst[name][f]) == bits(a[name]), (tag, f, name)
        assert np.isclose(fst["snr_db"][f], a["snr_db"], rtol=1e-5, atol=1e-5)   # display value, log10f not bit-pinned
        assert fst["n_llr"][f] > 0


def test_recorded_groups_in_padded_batches(oracle, golden):
    """The seven recorded captures, one padded batch per (modulation, rate, group size): marked cases against the golden
    record (cfo_used, cfo_after, codeword flags, bytes) and every case against the restatement on every field."""
    from ria_amd import capi
    names = {v: k for k, v in capi.MOD.items()}, {v: k for k, v in capi.RATE.items()}
    batches = {}
    for i, case, x, g in burst_cases(golden, oracle):
        batches.setdefault((int(case[0]), int(case[1]), int(case[2])), []).append((i, case, x, g))
    assert len(batches) == 5
    left_out = 0
    for (mod, rate, n), items in batches.items():
        e = engine(names[0][mod], names[1][rate])
        wl = max(len(x) for _, _, x, _ in items)
        X = np.zeros((len(items), wl), np.float32)
        for k, (_, _, x, _) in enumerate(items):
            X[k, :len(x)] = x
        known = np.array([c[6] for _, c, _, _ in items], np.float32)
        base = np.array([int(c[7]) for _, c, _, _ in items], np.uint64)
        out = e.rx_burst(dev(X), 21000, group_size=n, known_cfo=known, detect_threshold=0.5, min_confidence=0.0, abs_base=base)
        for k, (i, case, x, g) in enumerate(items):
            r = br.burst_window(oracle, mod, rate, X[k], 21000, n, known_cfo=float(case[6]), detect_threshold=0.5, min_confidence=0.0,
                                abs_base=int(case[7]))
            assert_equal_to_restatement(f"case {i}", out, k, r)
            if not case[8]:
                assert out["result"]["mode"][k] == 1
                continue
            if r["stop"] == br.STOP["ENERGY"]:      # a faded frame under the gate: the reference would discard the group
                left_out += 1                       # (tests/test_rx_burst_cpu.py allows one such case)
                assert out["result"]["stop"][k] == br.STOP["ENERGY"] and out["result"]["frames_decoded"][k] == 0 and not out["info"][k].any()
                continue
            assert out["result"]["mode"][k] == 2 and out["result"]["frames_decoded"][k] == n and out["result"]["stop"][k] == 0
            assert np.array_equal(bits(out["cfo_used"][k][:n]), bits(g[f"cfo_used_{i}"]))
            assert np.array_equal(bits(out["frame_status"]["cfo_hz"][k][:n]), bits(g[f"cfo_after_{i}"]))
            assert np.array_equal(out["decode_status"]["cw_ok"][k][:n], g[f"dec_ok_{i}"])
            assert np.array_equal(out["info"][k][:n], g[f"dec_data_{i}"])
    assert left_out <= 1


@pytest.mark.skipif(not po.Ref.available(), reason="oracle/_ref/libria_ref.so is not built (build() makes it where the reference sources are)")
def test_recorded_groups_against_the_compiled_reference(oracle, golden):
    """One reference waveform object driven in StreamingDecoder's order (Ref.burst_rx) on the marked captures.  At most one
    capture may fail the energy gate (as in tests/test_rx_burst_cpu.py); its frames before the gate are still compared."""
    from ria_amd import capi
    import gen_golden
    names = {v: k for k, v in capi.MOD.items()}, {v: k for k, v in capi.RATE.items()}
    ref = po.Ref()
    left_out = 0
    for i, case, x, g in burst_cases(golden, oracle):
        mod, rate, n, lead, kind, snr, cfo0, abs_base, marker = case
        if not marker:
            continue
        n = int(n)
        rr = ref.burst_rx(int(mod), int(rate), x, n, known_cfo=float(cfo0), abs_base=int(abs_base), bpc=gen_golden.BURST_BPC[rate])
        e = engine(names[0][int(mod)], names[1][int(rate)])
        out = e.rx_burst(dev(x[None, :]), 21000, group_size=n, known_cfo=float(cfo0), detect_threshold=0.5, min_confidence=0.0,
                         abs_base=int(abs_base))
        if out["result"]["stop"][0] == br.STOP["ENERGY"]:
            # the shim's burst_rx has no energy gate; a faded frame under it makes StreamingDecoder discard the group
            f = int(out["result"]["frames"][0])
            s0 = int(out["result"]["sync_start"][0]) + f * e.geo.frame_samples
            assert br.gate_rms(x[s0:s0 + e.geo.frame_samples]) < np.float32(0.04) and out["result"]["frames_decoded"][0] == 0
            assert np.array_equal(bits(out["cfo_used"][0][:f]), bits(rr["cfo_used"][:f]))
            left_out += 1
            continue
        assert out["result"]["frames_decoded"][0] == n
        assert np.array_equal(bits(out["cfo_used"][0][:n]), bits(rr["cfo_used"])) and np.array_equal(bits(out["frame_status"]["cfo_hz"][0][:n]), bits(rr["cfo_after"]))
        assert np.array_equal(out["decode_status"]["cw_ok"][0][:n], rr["dec_ok"]) and np.array_equal(out["info"][0][:n], rr["dec_data"])
    assert left_out <= 1


def test_scenario_set_mixed_modes_one_call(oracle):
    """The CPU scenario set as one shuffled batch with NaN-filled gaps between the windows (stride > window_len): equal to
    the restatement on every field, and to the same windows run one per call."""
    S = scenario_results(oracle)
    names = sorted(S)
    order = np.random.default_rng(11).permutation(len(names))
    stride = br.WINDOW_LEN + 777
    X = np.full((len(names), stride), np.nan, np.float32)
    for k, j in enumerate(order):
        X[k, :br.WINDOW_LEN] = S[names[j]][0]
    e = engine("QAM16", "R1_2")
    Xd = dev(X)
    kw = dict(group_size=br.GROUP, known_cfo=0.0, abs_base=77000, window_len=br.WINDOW_LEN)
    out = e.rx_burst(Xd, br.SEARCH_LEN, **kw)
    assert set(out["result"]["mode"]) == {0, 1, 2} and set(out["result"]["stop"]) == set(range(8)) - {br.STOP["PROCESS"]}
    for k, j in enumerate(order):
        assert_equal_to_restatement(names[j], out, k, S[names[j]][1])
    for k in range(len(names)):
        one = e.rx_burst(Xd[k:k + 1], br.SEARCH_LEN, **kw)
        for key in out:
            assert out[key][k].tobytes() == one[key][0].tobytes(), (names[order[k]], key)


def test_variants_equal_the_separate_calls(oracle):
    """RIA_BURST_NO_CONTINUE on unmarked windows equals ria_gpu_rx_acquire_batch on every shared field; a marked window
    without RIA_BURST_INTERLEAVE too; complete groups equal sync_lts -> demod per frame -> burst_deinterleave -> decode."""
    import torch
    from test_oracle_golden import burst_cfo_feedback
    S = scenario_results(oracle)
    e = engine("QAM16", "R1_2")
    names = ["limit", "energy", "decode", "not_data", "window", "group_ok", "silence"]
    X = dev(np.stack([S[k][0] for k in names]))
    for kw in (dict(continuation=False, interleave=False), dict(interleave=False, continuation=False, retry=False)):
        out = e.rx_burst(X, br.SEARCH_LEN, group_size=br.GROUP, abs_base=5, **kw)
        info, st, res, fst = e.rx_acquire(X, br.SEARCH_LEN, abs_base=5, want_demod_status=True, retry=kw.get("retry", True))
        torch.cuda.synchronize()
        for f in ("detected", "accepted", "sync_start", "frame_start", "correlation", "delta", "candidates", "burst_interleaved"):
            assert out["result"][f].tobytes() == res[f].tobytes(), f
        assert np.array_equal(out["info"][:, 0], info.cpu().numpy()) and not out["info"][:, 1:].any()
        assert out["decode_status"][:, 0].tobytes() == e.decode_status(st).tobytes()
        assert out["frame_status"][:, 0].tobytes() == e.frame_status(fst).tobytes()
        assert (out["result"]["stop"] == 0).all() and (out["result"]["mode"] == (res["accepted"] != 0)).all()
        assert (out["result"]["frames_decoded"] == (res["accepted"] != 0)).all() and not out["rms"].any()
    # groups against the composition of the separate calls
    gn = ["group_ok", "clamp_up", "clamp_down"]
    G = dev(np.stack([S[k][0] for k in gn]))
    out = e.rx_burst(G, br.SEARCH_LEN, group_size=br.GROUP, abs_base=9000)
    sync = e.sync_lts(G[:, :br.SEARCH_LEN].contiguous(), dev(np.zeros(len(gn), np.float32)), 0.15)
    assert (sync["burst_interleaved"] == 1).all() and (out["result"]["frames_decoded"] == br.GROUP).all()
    start = sync["start_sample"].astype(np.uint64)
    cfo = np.zeros(len(gn), np.float32)
    llrs = []
    for f in range(br.GROUP):
        assert np.array_equal(bits(out["cfo_used"][:, f]), bits(cfo))
        offs = np.arange(len(gn), dtype=np.uint64) * np.uint64(br.WINDOW_LEN) + start + np.uint64(f * br.FS)
        llr, st = e.demod(G, cfo_hz=cfo, abs_pos=np.uint64(9000) + start, flags=np.full(len(gn), 1 if f == 0 else 0, np.uint32), offsets=offs)
        fs = e.frame_status(st)
        assert fs.tobytes() == out["frame_status"][:, f].tobytes(), f
        cfo = np.array([burst_cfo_feedback(c, v) for c, v in zip(cfo, fs["cfo_hz"])], np.float32)
        llrs.append(llr)
    phys = torch.stack(llrs, dim=1).reshape(len(gn) * br.GROUP, -1).contiguous()
    info, st = e.decode(e.burst_deinterleave(phys, br.GROUP))
    torch.cuda.synchronize()
    assert np.array_equal(info.cpu().numpy().reshape(len(gn), br.GROUP, -1), out["info"][:, :br.GROUP])
    assert e.decode_status(st).tobytes() == np.ascontiguousarray(out["decode_status"][:, :br.GROUP]).tobytes()
    assert np.array_equal(bits(out["result"]["cfo_hz"]), bits(cfo))


def test_marked_window_without_the_interleave_flag_continues_like_any_other(oracle):
    """A marked, burst-interleaved window with RIA_BURST_INTERLEAVE clear and continuation on: continuation mode, frame 0
    with its first LTS un-negated, and STOP_DECODE there (frame 0 holds interleaved bytes) - every field as the restatement."""
    x = scenario_results(oracle)["group_ok"][0]
    e = engine("QAM16", "R1_2")
    out = e.rx_burst(dev(x[None, :]), br.SEARCH_LEN, group_size=br.GROUP, interleave=False, abs_base=77000)
    r = br.burst_window(oracle, po.QAM16, po.R1_2, x, br.SEARCH_LEN, br.GROUP, interleave=False, abs_base=77000)
    assert r["mode"] == 1 and r["burst_interleaved"] == 1 and r["stop"] == br.STOP["DECODE"] and r["frames"] == 1
    assert_equal_to_restatement("group_ok without interleave", out, 0, r)


def test_argument_checks():
    """group_size 1 and 9, unknown flag bits, window_len < search_len and null outputs are RIA_ERR_INVALID; n_windows = 0 is
    RIA_OK and touches nothing."""
    import torch
    from ria_amd import capi
    e = engine("QAM16", "R1_2")
    n, wl = 2, 40000
    x = torch.zeros((n, wl), dtype=torch.float32, device=e.device)
    params = torch.zeros((n, 32), dtype=torch.uint8, device=e.device)
    info = torch.full((n, 9, e.geo.info_bytes_per_frame), 0xAB, dtype=torch.uint8, device=e.device)
    st = torch.full((n, 9, 20), 0xAB, dtype=torch.uint8, device=e.device)
    res = torch.full((n, 64), 0xAB, dtype=torch.uint8, device=e.device)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(group=4, flags=capi.DECODE_FULL | capi.BURST_INTERLEAVE, search=21000, window=wl, nw=n, i=info, s=st, r=res):
        return e.lib.ria_gpu_rx_burst_batch(e.h, p(x), wl, search, window, nw, group, p(params), flags, p(i) if i is not None else None,
                                            p(s) if s is not None else None, p(r) if r is not None else None, None, None, None, None)
    assert call(group=1) == -1 and call(group=9) == -1 and call(flags=0x2000) == -1 and call(flags=capi.RX_DEMOD_ONLY) == -1
    assert call(search=30000, window=25000) == -1
    assert call(i=None) == -1 and call(s=None) == -1 and call(r=None) == -1
    assert call(nw=0) == 0
    torch.cuda.synchronize()
    assert (info == 0xAB).all() and (st == 0xAB).all() and (res == 0xAB).all()
    assert call() == 0          # silence: nothing detected, every output zero
    torch.cuda.synchronize()
    assert not info.any() and not st.any() and not res[:, 4:8].any()


def test_workspace_growth_leaves_results_alone(oracle):
    """A call on 2 windows, then one on all of them, on a fresh handle: the second equals the same call on another handle
    that never ran the first."""
    from ria_amd.engine import RxEngine
    S = scenario_results(oracle)
    names = sorted(S)
    X = dev(np.stack([S[k][0] for k in names]))
    kw = dict(group_size=br.GROUP, abs_base=123)
    a = RxEngine("QAM16", "R1_2", max_batch=64)
    small = a.rx_burst(X[:2].contiguous(), br.SEARCH_LEN, **kw)
    big = a.rx_burst(X, br.SEARCH_LEN, **kw)
    ref = engine("QAM16", "R1_2").rx_burst(X, br.SEARCH_LEN, **kw)
    for key in big:
        assert big[key].tobytes() == ref[key].tobytes(), key
        assert small[key].tobytes() == ref[key][:2].tobytes(), key
    a.close()
