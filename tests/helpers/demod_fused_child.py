"""Child process of tests/test_gpu_demod_domain.py::test_one_wave_per_frame_kernel_equals_the_default_path: the library
reads RIA_DEMOD_FUSED once per process, so the one-wave-per-frame demod_frames_kernel can only be selected in a fresh
process.  Demodulates every family of the given modes and writes LLRs and status words to argv[1] (.npz)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    assert os.environ.get("RIA_DEMOD_FUSED") == "1"
    import torch
    import pyoracle as po
    import demod_domain_inputs as D
    from ria_amd.engine import RxEngine
    from ria_amd import capi
    assert capi.load().ria_gpu_demod_variant() == 1, "the library did not select demod_frames_kernel"
    O = po.Oracle()
    out = {}
    for mode in sys.argv[2:]:
        e = RxEngine(*D.ENGINE[mode])
        for m, fam in D.CASES:
            if m != mode:
                continue
            F = D.family(O, mode, fam)
            llr, st = e.demod(torch.from_numpy(F["x"]).cuda(), cfo_hz=F["cfo"], abs_pos=F["pos"], flags=F["flags"])
            torch.cuda.synchronize()
            out[f"llr_{mode}_{fam}"] = llr.cpu().numpy().view(np.uint32)
            out[f"st_{mode}_{fam}"] = st.cpu().numpy()
        e.close()
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
