"""GPU test (-m gpu): a handle gives back all the device memory it took.  Every device and pinned block of a handle is owned
by a member of the handle (ria_amd/csrc/device_buffers.hpp), so ria_gpu_destroy has no list of buffers to keep complete; this
test is the check that none is left behind."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# Free device memory after the close of cycle 3 may lie below the figure after cycle 2 by at most ALLOWANCE bytes: the
# difference the same test body shows on the parent commit, whose ria_gpu_destroy freed every buffer by a hand-kept list,
# plus one allocation granule of the device.  Measured on an MI355X in one run with this build:
#   parent commit: free after cycle 2 = free after cycle 3 = 308344258560 bytes, PARENT_DROP = 0 (this build: the same, 0)
#   granule: hipMemGetAllocationGranularity (minimum and recommended, device memory on device 0) = 4096 bytes.
# hipMemGetInfo itself was seen to move in steps of 4 MiB there (a hipMalloc of up to 1 MiB moved it by 0, one of 2 MiB + 1
# by 4194304): the runtime's own figure is the smaller of the two, so a single such step already fails the test.
PARENT_DROP = 0
GRANULE = 4096
ALLOWANCE = PARENT_DROP + GRANULE


def _cycle(inputs):
    """Builds a QAM16 R1/2 and an R1/4 engine, makes one small call of each family so that every lazily built buffer
    exists, closes both.  Every engine call raises unless the library returned RIA_OK."""
    import torch
    from ria_amd import capi
    from ria_amd.engine import RxEngine
    e = RxEngine("QAM16", "R1_2", max_batch=64)
    frames, windows, rows, zc, chirp, cox, mc_frames, mc_windows = inputs
    e.rx(frames, flags=0)
    e.rx(frames, flags=capi.DECODE_FULL)
    e.rx_acquire(windows, 21000)
    e.rx_burst(windows, 21000, group_size=4)
    e.decode_frame(rows)
    e.sync_zc(zc)                      # longer than the LDS form holds: the global baseband workspace
    e.sync_chirp(chirp)
    e.sync_lts(windows[:1, :21000].contiguous())
    e.sync_cox(cox)
    host = frames.cpu().numpy()
    info = np.zeros((len(host), e.geo.info_bytes_per_frame), np.uint8)
    st = np.zeros((len(host), 20), np.uint8)

    def vp(a):
        return a.ctypes.data_as(C.c_void_p)
    assert e.lib.ria_gpu_rx_frames_host(e.h, vp(host), None, len(host), capi.DECODE_FULL, vp(info), vp(st), None, None) == capi.RIA_OK
    m = RxEngine("DQPSK", "R1_4", max_batch=64)
    m.mcdpsk_demod(mc_frames, cfo_hz=torch.zeros(len(mc_frames), device=mc_frames.device))
    m.mcdpsk_acquire(mc_windows, 70000, 3)
    torch.cuda.synchronize()
    for eng in (e, m):
        eng.close()
        assert eng.h is None
        eng.close()                    # a second close is a no-op
        assert eng.h is None


def free_after_cycles():
    """-> free device bytes after the close of cycles 2 and 3 (cycle 1 absorbs code-object loading and torch's cache)"""
    import torch
    from ria_amd.engine import RxEngine
    g = torch.Generator(device="cuda").manual_seed(7)
    noise = lambda *shape: 0.05 * torch.randn(shape, generator=g, device="cuda", dtype=torch.float32)
    fs = RxEngine("QAM16", "R1_2", max_batch=64)
    frame_samples = fs.geo.frame_samples
    fs.close()
    inputs = (noise(8, frame_samples), noise(2, 36000), 4.0 * noise(4, 8 * 648), noise(1, 20000), noise(1, 60000), noise(1, 21000),
              noise(2, (9 + 65) * 512), noise(2, 80000))
    free = []
    for cycle in range(3):
        _cycle(inputs)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    return free[1], free[2]


def test_create_use_destroy_returns_the_memory():
    """Three cycles of create / one call of every family / destroy on two engines.  Figures of the run that set the
    allowance (MI355X): parent commit free(2) - free(3) = 0 bytes, granule = 4096 bytes, ALLOWANCE = 4096 bytes; this build
    showed 0 bytes in the same run."""
    after2, after3 = free_after_cycles()
    print(f"free after cycle 2: {after2}  after cycle 3: {after3}  drop: {after2 - after3}  allowance: {ALLOWANCE}")
    assert after3 >= after2 - ALLOWANCE, (after2, after3, after2 - after3)
