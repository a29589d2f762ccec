import os
import sys

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")      # as cfgpp_amd/__init__.py (must precede the first HIP call)
os.environ.setdefault("CFGPP_TUNE_CACHE", "0")           # hermetic tests: no tile pins from / to ~/.cache (test_gpu_unet.py tests the cache itself)

import pytest  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden():
    import json

    import numpy as np
    g = np.load(os.path.join(ROOT, "tests", "golden", "sampler_golden.npz"))
    with open(os.path.join(ROOT, "tests", "golden", "sampler_golden.json")) as f:
        meta = json.load(f)
    return g, meta


@pytest.fixture(scope="session")
def golden_h16():
    """inversion / edit trajectories recorded from the reference with an fp16 VAE (fp16 latents end to end)"""
    import json

    import numpy as np
    g = np.load(os.path.join(ROOT, "tests", "golden", "sampler_golden_h16.npz"))
    with open(os.path.join(ROOT, "tests", "golden", "sampler_golden_h16.json")) as f:
        meta = json.load(f)
    return g, meta


@pytest.fixture(scope="session")
def golden_r3():
    """round-3 additions recorded from the reference: SDXL euler / *_lightning trajectories, the 'npi' initialisation"""
    import json

    import numpy as np
    g = np.load(os.path.join(ROOT, "tests", "golden", "sampler_golden_r3.npz"))
    with open(os.path.join(ROOT, "tests", "golden", "sampler_golden_r3.json")) as f:
        meta = json.load(f)
    return g, meta


@pytest.fixture
def recorded_sqrt(monkeypatch):
    """``Tensor.sqrt`` of the scheduler's alpha table as the golden vectors' recording host evaluated it.  torch's fp32 CPU
    sqrt goes through MKL, whose result depends on the CPU: the vectors were recorded on MKL's Intel AVX-512 branch, and on
    an AMD CPU MKL takes another branch (1 ulp apart on ~18 % of the table; MKL_CBWR does not change that).  The
    sampler's own sigma / sqrt(alpha) arithmetic runs live, as the reference's does, so a bit-exact comparison with the
    recordings needs the recording host's roots: cfgpp_amd/data/ddim_sqrt_tables.npz pins sqrt(a) and sqrt(1 - a) over
    ``cat([1.0], abar)`` as recorded.  Inside a test that takes this fixture, every element of an fp32 CPU tensor that is
    such an a or 1 - a gets that root; any other element gets torch's own.  A no-op on the recording host's branch."""
    import numpy as np
    import torch
    from cfgpp_amd.schedule import alphas_cumprod, ddim_sqrt_tables
    a = torch.cat([torch.ones(1), alphas_cumprod()])
    roots = torch.cat(ddim_sqrt_tables()).numpy()
    bits = torch.cat([a, 1 - a]).view(torch.int32).numpy()
    keys, first, inv = np.unique(bits, return_index=True, return_inverse=True)
    assert np.array_equal(roots, roots[first][inv]), "one input, two recorded roots"
    roots = torch.from_numpy(roots[first].copy())
    sqrt = torch.Tensor.sqrt

    def recorded(x):
        out = sqrt(x)
        if x.dtype != torch.float32 or x.device.type != "cpu" or x.numel() == 0:
            return out
        xb = x.detach().contiguous().view(torch.int32).numpy().reshape(-1)
        i = np.minimum(np.searchsorted(keys, xb), len(keys) - 1)
        hit = torch.from_numpy(keys[i] == xb)
        out.view(-1)[hit] = roots[torch.from_numpy(i)[hit]]
        return out
    monkeypatch.setattr(torch.Tensor, "sqrt", recorded)


# ---- order of the -m gpu suite: cheap -> expensive -------------------------------------------------------------------
# The driver runs `pytest tests/ -x -q -m gpu`: with -x a failure (or a native abort) hides every test behind it, so the
# single-kernel parity tests go first and the real-size nets (minutes each, tens of GB of host memory) go last.
_GPU_FILE_ORDER = ["test_gpu_kernels.py", "test_gpu_step.py", "test_gpu_torch_semantics.py", "test_gpu_graph.py",
                   "test_gpu_unet.py", "test_gpu_vae.py", "test_gpu_text.py", "test_gpu_weights.py", "test_gpu_examples.py",
                   "test_gpu_configs.py", "test_gpu_realsize.py"]


def pytest_collection_modifyitems(config, items):
    if os.environ.get("CFGPP_TEST_ORDER") == "alpha":       # diagnostics: pytest's own order
        return

    def key(it_idx):
        idx, it = it_idx
        fname = os.path.basename(str(it.fspath))
        if it.get_closest_marker("gpu") is None or fname not in _GPU_FILE_ORDER:
            return (0, 0, idx)                                 # CPU tests and unknown files keep their place, first
        return (1, _GPU_FILE_ORDER.index(fname), idx)
    items[:] = [it for _, it in sorted(enumerate(items), key=key)]
