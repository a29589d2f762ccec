"""Record the real-size ControlNet oracle output ONCE, in the build container (CPU), as the fixture of
tests/test_gpu_controlnet.py::test_real_sd15_controlnet_forward_vs_oracle_fixture.

    python tests/golden/make_controlnet_golden.py

Inputs and tolerance live in tests/realsize_controlnet.py; only this repo's restatements (tests/controlnet_ref.py on
``oracle/``, fp32 torch on CPU) run.  The fixture holds the fp32 eps [2, 4, 64, 64].
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import realsize_controlnet as RC  # noqa: E402

import numpy as np  # noqa: E402


def main():
    t0 = time.time()
    out = RC.oracle()
    np.savez(RC.FIXTURE, **out)
    print(RC.FIXTURE, {k: (v.shape, str(v.dtype)) for k, v in out.items()}, f"{time.time() - t0:.1f} s", flush=True)


if __name__ == "__main__":
    main()
