"""Child process of tests/test_gpu_window.py::test_unsupported_by_the_one_wave_per_frame_kernel: the library reads
RIA_DEMOD_FUSED once per process, so demod_frames_kernel can only be selected in a fresh process.  Calls
ria_gpu_rx_window_batch and prints the status it returns."""
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
    ce, de = RxEngine("DQPSK", "R1_4"), RxEngine("QAM16", "R1_2")
    n, wlen = 2, 20000
    x = torch.zeros((n, wlen), dtype=torch.float32, device="cuda")
    row = de.window_frame_row()
    frames = torch.zeros((n, row), dtype=torch.uint8, device="cuda")
    res = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    acq = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    params = de.acq_params(n, min_confidence=0.5)
    rc = de.lib.ria_gpu_rx_window_batch(ce.h, de.h, _ptr(x), wlen, 5000, wlen, n, _ptr(params), capi.DECODE_FULL, _ptr(frames), row, _ptr(res),
                                        _ptr(acq), None, None, _stream_ptr())
    torch.cuda.synchronize()
    print("status", rc)


if __name__ == "__main__":
    main()
