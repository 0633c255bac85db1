"""CPU tests of the decodeFrame entry points (ria_gpu_decode_frame_batch / _host): their ABI, the pinned rows the GPU tests
run (tests/decode_frame_inputs.py) and the CPU restatement they are compared against (tests/decode_frame_restatement.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pyoracle as po
import decode_frame_inputs as I
import decode_frame_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"


def test_decode_frame_symbols_struct_flags_and_enum_match_the_header():
    from ria_amd import capi
    from ria_amd.engine import RxEngine
    L = capi.load()
    for sym in ("ria_gpu_decode_frame_batch", "ria_gpu_decode_frame_host"):
        assert sym in capi.EXPORTS and getattr(L, sym) is not None
    assert C.sizeof(capi.DframeResult) == 32
    header = open(os.path.join(ROOT, "include", "ria_gpu.h")).read()
    sizes = {"int32_t": 4, "uint16_t": 2, "uint8_t": 1}
    body = re.search(r"typedef struct ria_dframe_result \{(.*?)\} ria_dframe_result;", header, re.S).group(1)
    off = 0
    for t, name, count in re.findall(r"^\s*(\w+)\s+(\w+)(?:\[(\d+)\])?;", body, re.M):
        sz = sizes[t]
        off = (off + sz - 1) // sz * sz
        assert getattr(capi.DframeResult, name).offset == off, name
        assert RxEngine.DFRAME_RESULT.fields[name][1] == off, name
        off += sz * int(count or 1)
    assert off == 32 and RxEngine.DFRAME_RESULT.itemsize == 32
    enum = dict((k, int(v)) for k, v in re.findall(r"RIA_DFRAME_(\w+) = (\d+)", header))
    assert enum == capi.DFRAME_PATH and len(enum) == 10
    assert [capi.DFRAME_PATH[n] for n in R.PATH_NAMES] == list(range(10))
    from ria_amd.acquire import DFRAME_PATHS
    assert DFRAME_PATHS == R.PATH_NAMES
    assert capi.DECODE_FULL == int(re.search(r"#define RIA_DECODE_FULL\s+(0x[0-9a-f]+)u", header).group(1), 16)
    assert capi.DECODE_NO_CHANNEL_DEINTERLEAVE == int(re.search(r"#define RIA_DECODE_NO_CHANNEL_DEINTERLEAVE (0x[0-9a-f]+)u", header).group(1), 16)


def test_decode_frame_rejects_a_null_handle_without_a_gpu():
    """A null handle is RIA_ERR_INVALID whatever the other arguments (the argument checks themselves are tested on a real
    handle in test_gpu_decode_frame.py)."""
    from ria_amd import capi
    L = capi.load()
    buf = (C.c_uint8 * 256)()
    p = C.cast(buf, C.c_void_p)
    for stride, n, flags, row in ((2592, 1, 7, 160), (647, 1, 7, 160), (2592, -1, 7, 160), (2592, 1, 0x200, 160), (2592, 1, 7, 1)):
        assert L.ria_gpu_decode_frame_batch(None, p, stride, None, n, flags, p, row, p, None, None, None) == -1
    assert L.ria_gpu_decode_frame_batch(None, None, 0, None, 0, 0, None, 0, None, None, None, None) == -1
    assert L.ria_gpu_decode_frame_host(None, p, 648, 7, p, 160, p, None) == -1


def test_dframe_tally_counts_rows_per_path_and_stage():
    from ria_amd.acquire import DFRAME_COUNTERS, dframe_tally
    from ria_amd.engine import RxEngine
    res = np.zeros(5, RxEngine.DFRAME_RESULT)
    res["path"] = [1, 3, 3, 7, 0]
    res["success"] = [1, 1, 0, 1, 0]
    res["stages"] = [1, 7, 7, 0x23, 0]
    res["iters_r14"] = [3, 50, 50, 50, 0]
    res["iters_cw0"] = [0, 80, 80, 2, 0]
    row = dict(zip(DFRAME_COUNTERS, dframe_tally(res)))
    assert row["rows"] == 5 and row["success"] == 3 and row["path_CONTROL_R14"] == 1 and row["path_FIXED"] == 2
    assert row["path_LEGACY"] == 1 and row["path_NONE"] == 1 and row["stage_r14"] == 4 and row["stage_rate"] == 3
    assert row["stage_fixed"] == 2 and row["stage_legacy"] == 1 and row["stage_salvage_r14"] == 0 and row["probe_iterations"] == 315


def test_channel_permutation_of_the_gather_tables_is_the_channel_interleavers():
    for mode, (mod, rate) in I.MODES.items():
        bps = R.oracle().geom(mod, rate).bits_per_symbol
        P = R.channel_perm(bps)
        assert P[0] == 0 and len(set(P)) == 648
        if po.Ref.available():
            assert np.array_equal(P, po.Ref().channel_interleaver_inv(bps)), mode


def test_pinned_rows_reach_every_path_and_stage_and_land_where_their_recipe_says(oracle):
    """The condition on the inputs: a row that drifts off its path fails here, not silently on the GPU."""
    paths, stages = set(), 0
    for label, mode, ch, flags, recipes in I.batches():
        rows, n_llr, res = I.expected("oracle", oracle, label)
        assert rows.shape == (len(recipes), I.STRIDE) and rows.dtype == np.float32
        for rec, r in zip(recipes, res):
            assert R.PATH_NAMES[r["path"]] == rec[-1], (label, rec[0], R.PATH_NAMES[r["path"]])
            paths.add(r["path"])
            stages |= r["stages"]
    assert paths == set(range(10)) and stages == 0x3F
    by = {rec[0]: r for rec, r in zip(I.ROWS["QAM16_R1_2"], I.expected("oracle", oracle, "QAM16_R1_2")[2])}
    assert by["fixed_retry"]["success"] == 1 and by["fixed_retry"]["fixed_attempts"].max() > 1
    assert by["salv14"]["tries_r14"] >= 1 and by["salv14"]["iters_r14"] == 50 and by["salv14"]["frame_bytes"] == 20
    assert by["salv_rate"]["tries_r14"] == 5 and by["salv_rate"]["tries_rate"] >= 1 and by["salv_rate"]["frame_bytes"] == 40
    assert by["legacy4"]["success"] == 1 and by["legacy4"]["codewords_ok"] == 4 and by["legacy4"]["codewords_failed"] > 0   # the carried count
    assert by["legacy3_cut"]["success"] == 0 and (by["legacy3_cut"]["codewords_ok"], by["legacy3_cut"]["codewords_failed"]) == (2, 1)
    assert by["ack14_over"]["frame_bytes"] == 20 and by["fixed_clean"]["iters_r14"] == 50 and by["fixed_clean"]["iters_cw0"] == 80
    nr = I.expected("oracle", oracle, "QAM16_R1_2_norecover")[2][0]
    assert nr["path"] == R.FIXED and nr["success"] == 0 and (nr["codewords_ok"], nr["codewords_failed"], nr["frame_bytes"]) == (4, 0, 0)


def test_restatement_on_ref_equals_the_oracle(oracle):
    if not po.Ref.available():
        pytest.skip("the reference library (oracle/_ref) is not built")
    ref = po.Ref()
    for label, mode, ch, flags, recipes in I.batches():
        if flags != 7:
            continue                                   # the compiled reference has no decodeFixedFrame without its recovery
        a, b = I.expected("oracle", oracle, label)[2], I.expected("ref", ref, label)[2]
        bpc = R.bytes_per_cw(I.MODES[mode][1])
        for rec, x, y in zip(recipes, a, b):
            for k in R.RESULT_FIELDS + ("frame", "fixed_ran"):
                assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), (label, rec[0], k)
            if x["fixed_ran"]:
                keep = np.repeat(x["fixed_ok"] != 0, bpc)
                assert np.array_equal(x["fixed_ok"], y["fixed_ok"]) and np.array_equal(x["fixed_info"][keep], y["fixed_info"][keep]), (label, rec[0])


def decode_frame_block():
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```cpp\n(.*?)```", md, re.S) if "gpuDecodeFrame" in b]
    assert len(blocks) == 1 and not re.match(r"// src/\S+\s+\(new file in the reference\)", blocks[0])
    return blocks[0]


def test_integration_md_binds_the_whole_of_decode_frame():
    b = decode_frame_block()
    assert "ria_host::decodeFrame" in b and "DecodeResult" in b


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="reference sources not present on this box")
def test_integration_decode_frame_block_compiles_against_the_reference_headers(tmp_path):
    tu = tmp_path / "decode_frame_binding.cpp"
    tu.write_text(decode_frame_block() + """
static ultra::gui::DecodeResult dec(ria_host::GpuHandle& h, const std::vector<float>& s) { return ultra::gui::gpuDecodeFrame(h, s, true, 1.0f, 2.0f); }
int main() { (void)&dec; return 0; }
""")
    cmd = ["g++", "-std=c++20", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-I" + os.path.join(REF, "include"), "-I" + os.path.join(REF, "src"), "-I" + os.path.join(REF, "src", "waveform"),
           "-I" + os.path.join(REF, "src", "gui"), "-I" + os.path.join(REF, "src", "gui", "modem"),
           "-I" + os.path.join(REF, "thirdparty"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ria_amd", "host"), str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
