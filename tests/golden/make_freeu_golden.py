"""Record the real-size FreeU oracle output ONCE (CPU), as the fixture of
tests/test_gpu_freeu_net.py::test_real_sd15_freeu_forward_vs_oracle_fixture.

    python tests/golden/make_freeu_golden.py

Inputs and tolerance live in tests/realsize_freeu.py; only this repo's restatements (tests/freeu_ref.py on ``oracle/``, fp32 torch
on CPU) run.  The recorder asserts that the eps with and without FreeU differ by more than 10 x the tolerance, starting from
s1 = 0.9, s2 = 0.2, b1 = 1.5, b2 = 1.6 and doubling the values' distance from 1 until they do; the fixture holds the fp32 eps
[2, 4, 64, 64], that distance and the (s1, s2, b1, b2) used.
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import realsize_freeu as RF  # noqa: E402

import numpy as np  # noqa: E402


def main():
    t0 = time.time()
    out = RF.oracle()
    np.savez(RF.FIXTURE, **out)
    print(RF.FIXTURE, {k: (v.shape, str(v.dtype)) for k, v in out.items()}, "moved", float(out["moved"]), "freeu", out["freeu"].tolist(),
          f"{time.time() - t0:.1f} s", flush=True)


if __name__ == "__main__":
    main()
