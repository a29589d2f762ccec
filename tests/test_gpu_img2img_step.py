"""-m gpu: cfgpp_img2img_start (include/cfgpp_img2img.h) on the MI355X - every case of tests/img2img_cases.py into NaN-filled
destinations between guard rows against the fp64 model inside the derived per-element bound (tests/img2img_ref.py: bound), mode 0
against the torch expression bit for bit, the in-kernel draw against the tensor form fed by cfgpp_philox_normal(stream 4, draw 0) bit
for bit, batched chains against single ones, seeds."""
import numpy as np
import pytest
import torch

import img2img_cases as T
import img2img_ref as M

pytestmark = pytest.mark.gpu


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def run_case(c, inp, noise="case", seeds="case", B=None, rows=slice(None)):
    """launch one case -> (x [B, C, h, w] on the GPU, the whole guarded buffer).  The destination is the middle of a NaN-filled
    buffer with one guard row on either side; a one-row source is the first row of its B-row parent, so that a broadcast that read
    row b would stay in bounds - and be wrong."""
    from cfgpp_amd import engine as E
    B = c["B"] if B is None else B
    h, w = c["hw"]
    dt = torch.float16 if c["x_half"] else torch.float32
    buf = torch.full((B + 2, T.C, h, w), float("nan"), dtype=dt, device="cuda")
    x = buf[1:B + 1]
    src = None
    if inp["src_parent"] is not None:
        parent = torch.from_numpy(inp["src_parent"][rows]).to(torch.float16 if c["src_half"] else torch.float32).cuda().contiguous()
        src = parent[: min(c["src_rows"], B)]
    nz = inp["noise"] if isinstance(noise, str) else noise
    if isinstance(nz, np.ndarray):
        nz = torch.from_numpy(nz[rows]).cuda().contiguous()
    sd = seeds
    if isinstance(seeds, str):
        sd = None if inp["seeds"] is None else list(inp["seeds"])[rows]
    E.img2img_start(x, src, c["a"], c["s"], c["mode"], noise=nz, seeds=sd)
    torch.cuda.synchronize()
    return x, buf


@pytest.fixture(scope="module")
def table():
    out = {}
    for c in T.CASES:
        inp = T.make_inputs(c)
        ref, mag = T.model(c, inp)
        out[c["name"]] = (c, inp, ref, M.bound(ref, mag, c["x_half"]))
    return out


@pytest.mark.parametrize("name", [c["name"] for c in T.CASES])
def test_case_inside_the_bound(table, name):
    need_gpu()
    c, inp, ref, bnd = table[name]
    x, buf = run_case(c, inp)
    assert torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all(), "a guard row was written"
    got = x.double().cpu().numpy()
    assert np.isfinite(got).all(), "an element of the destination was not written"
    ratio = np.abs(got - ref) / bnd
    print(f"{name}: worst error / bound {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0, (name, float(ratio.max()), np.unravel_index(int(ratio.argmax()), ratio.shape))


def test_identity_fp32_is_the_torch_expression(table):
    """mode 0 with an fp32 x: c2 * z_src.float() + c1 * noise of inpaint._prepare_job, evaluated by torch on the CPU and on the GPU"""
    need_gpu()
    seen = 0
    for name, (c, inp, ref, bnd) in table.items():
        if c["mode"] != "identity" or c["x_half"] or c["a"] == 0.0 or c["noise"] != "tensor":
            continue
        x, _ = run_case(c, inp)
        z = torch.from_numpy(inp["src_parent"][: c["src_rows"]]).to(torch.float16 if c["src_half"] else torch.float32)
        n = torch.from_numpy(inp["noise"])
        a, s = float(np.float32(c["a"])), float(np.float32(c["s"]))
        assert torch.equal(x.cpu(), a * z.float() + s * n), name
        assert torch.equal(x, a * z.cuda().float() + s * n.cuda()), name
        seen += 1
    assert seen == 2


def test_in_kernel_draw_is_philox_stream_4_draw_0(table):
    """noise = NULL equals the tensor form fed by cfgpp_philox_normal(.., draw 0, stream 4, ..), bit for bit; the same seeds give the same
    bits; another seed moves the chain it keys and no other"""
    need_gpu()
    from cfgpp_amd import engine as E
    seen = 0
    for name, (c, inp, ref, bnd) in table.items():
        if c["noise"] != "philox":
            continue
        B, (h, w) = c["B"], c["hw"]
        x, _ = run_case(c, inp)
        n = E.philox_normal(torch.empty((B, T.C, h, w), dtype=torch.float32, device="cuda"), inp["seeds"], 0, 4)
        y, _ = run_case(c, inp, noise=n, seeds=None)
        assert torch.equal(x, y), name
        assert torch.equal(run_case(c, inp)[0], x), name
        other = list(inp["seeds"])
        other[B - 1] += 1
        z, _ = run_case(c, inp, seeds=other)
        assert torch.equal(z[: B - 1], x[: B - 1]) and not torch.equal(z[B - 1], x[B - 1]), name
        assert float((z[B - 1].float() - x[B - 1].float()).abs().mean()) > 0.1 * abs(c["s"]), name
        other = [v + 1 for v in inp["seeds"]]
        z, _ = run_case(c, inp, seeds=other)
        assert all(not torch.equal(z[b], x[b]) for b in range(B)), name
        seen += 1
    assert seen == 5


@pytest.mark.parametrize("name", ["b33-bilinear", "b33-bicubic-philox"])
def test_chain_b_of_the_batch_is_chain_b_alone(table, name):
    """B = 33 takes two launches (32 chains carry their keys in one): chains 0, 31 and 32 equal their single runs"""
    need_gpu()
    c, inp, ref, bnd = table[name]
    x, _ = run_case(c, inp)
    for b in (0, 31, 32):
        one, buf = run_case(c, inp, B=1, rows=slice(b, b + 1))
        assert torch.equal(one[0], x[b]), (name, b)
        assert torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all()
