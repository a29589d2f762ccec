"""Record the real-size IP-Adapter oracle output ONCE, in the build container (CPU), as the fixture of
tests/test_gpu_ip_adapter.py::test_real_sd15_ip_adapter_forward_vs_oracle_fixture.

    python tests/golden/make_ip_adapter_golden.py

Inputs and tolerance live in tests/realsize_ip.py; only this repo's restatements (tests/ip_adapter_ref.py on ``oracle/``, fp32
torch on CPU) run.  The recorder asserts that the eps with and without the adapter differ by more than 10 x the tolerance.  The
fixture holds the fp32 eps [2, 4, 64, 64].
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import realsize_ip as RI  # noqa: E402

import numpy as np  # noqa: E402


def main():
    t0 = time.time()
    out = RI.oracle()
    np.savez(RI.FIXTURE, **out)
    print(RI.FIXTURE, {k: (v.shape, str(v.dtype)) for k, v in out.items()}, f"{time.time() - t0:.1f} s", flush=True)


if __name__ == "__main__":
    main()
