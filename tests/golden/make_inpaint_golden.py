"""Record the real-size inpaint-UNet oracle output ONCE, in the build container (CPU), as the fixture of
tests/test_gpu_inpaint.py::test_real_sd15_inpaint_forward_vs_oracle_fixture.

    python tests/golden/make_inpaint_golden.py

Inputs and tolerance live in tests/realsize_inpaint.py; only this repo's ``oracle/`` restatement (fp32 torch on CPU) runs.
The fixture holds the fp32 eps [2, 4, 64, 64].
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import realsize_inpaint as RI  # noqa: E402

import numpy as np  # noqa: E402


def main():
    t0 = time.time()
    out = RI.oracle()
    np.savez(RI.FIXTURE, **out)
    print(RI.FIXTURE, {k: (v.shape, str(v.dtype)) for k, v in out.items()}, f"{time.time() - t0:.1f} s", flush=True)


if __name__ == "__main__":
    main()
