"""Child process of tests/test_gpu_var_frames.py::test_variable_spans_are_unsupported_by_the_one_wave_per_frame_kernel: the
library reads RIA_DEMOD_FUSED once per process, so demod_frames_kernel can only be selected in a fresh process.  Calls the
three entry points that demodulate spans and prints the status each returns; the fixed-frame call of the same handle works."""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main():
    assert os.environ.get("RIA_DEMOD_FUSED") == "1"
    import torch
    from ria_amd import capi
    from ria_amd.engine import RxEngine, _ptr, _stream_ptr
    assert capi.load().ria_gpu_demod_variant() == 1, "the library did not select demod_frames_kernel"
    e = RxEngine("DQPSK", "R1_4")
    x = torch.zeros((2, 9 * 1152), dtype=torch.float32, device="cuda")
    llr = torch.zeros((2, 742), dtype=torch.float32, device="cuda")
    st = torch.zeros((2, 32), dtype=torch.uint8, device="cuda")
    fr = torch.zeros((2, 20), dtype=torch.uint8, device="cuda")
    acq = torch.zeros((2, 32), dtype=torch.uint8, device="cuda")
    params = e.acq_params(2, min_confidence=0.5)
    L = e.lib
    rc = [L.ria_gpu_demod_var_batch(e.h, _ptr(x), None, None, 2, 9 * 1152, _ptr(llr), 742, _ptr(st), _stream_ptr()),
          L.ria_gpu_rx_control_batch(e.h, _ptr(x), None, None, 2, 9 * 1152, _ptr(fr), _ptr(st), None, _stream_ptr()),
          L.ria_gpu_control_acquire_batch(e.h, _ptr(x), 9 * 1152, 2000, 9 * 1152, 2, 4 * 1152, _ptr(params), 0, _ptr(fr), _ptr(st), _ptr(acq),
                                          None, _stream_ptr())]
    full = torch.zeros((1, e.geo.frame_samples), dtype=torch.float32, device="cuda")
    e.demod(full)
    torch.cuda.synchronize()
    print("status", *rc)


if __name__ == "__main__":
    main()
