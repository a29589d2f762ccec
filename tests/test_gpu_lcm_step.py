"""-m gpu: the LCM kernels (include/cfgpp_lcm.h; csrc/lcm_kernels.hip) - the raw Philox words against the Python Philox, the normals
against the float64 model, the fp16 fill, chain independence, and the fused step bit for bit against torch evaluating the header's
expression sequence (tests/lcm_ref.py: step_lcm) on torch-CPU and on torch-ROCm.

Bound of the normals.  The issue's convention is 4 x A_case, A_case = the max abs error of the numpy-float32 restatement
(lcm_ref.normals(dtype=float32)) against float64 on the same case.  On the shortest rows (4 .. 12 values) A_case is the error of a
handful of draws and can be almost nothing, so the bound is also derived from the accuracy of the device functions the header names,
per element of value v = rho * c:  logf within 1 ulp gives rho (a correctly rounded sqrt of an exactly doubled value) a relative
error of 2^-24 + 2^-24; sincospif within 2 ulp gives c a relative error of 2^-22; the product rounds once more, 2^-24 - together
7 * 2^-24 |v|, taken at 8 * 2^-24 |v| + 2^-40 for the second-order terms.  An element has to be within the LARGER of the two.
Measured on the MI355X (profiles/lcm/README.md): max |error| 3.351e-7 over all cases (A_case 2.9e-7 on the 4-value rows, 7.2e-7 on the
others), 0.117 of the bound at worst.

Like tests/test_gpu_vpred.py every buffer carries guard elements that must stay untouched, inputs are NaN there, and torch-ROCm is
asked on tensors padded to whole 4096-element blocks (see that file's docstring)."""
import math

import numpy as np
import pytest
import torch

import lcm_ref as R

pytestmark = pytest.mark.gpu

H, F = torch.float16, torch.float32
GUARD = 64
SENTINEL = 1234.0


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from cfgpp_amd import engine
    return engine


def _rand(shape, seed, scale=1.0, dtype=F):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ the integer part
def test_raw_words_equal_the_python_philox(E):
    for ctr, key, want in R.KNOWN_ANSWERS:
        got = _u32(E.philox_raw(ctr, key, 1))
        assert tuple(int(v) for v in got[0]) == want
    # a range that wraps c0, more than one block of threads
    ctr, key = (0xFFFFFF00, 5, 77, 1), (0x89ABCDEF, 0x01234567)
    got = _u32(E.philox_raw(ctr, key, 1000))
    want = R.philox_words(1000, (key[1] << 32) | key[0], ctr[2], ctr[3], c0_start=ctr[0], c1=ctr[1])
    assert np.array_equal(got, want)
    assert tuple(int(v) for v in got[256]) == R.philox4x32_10((0, 5, 77, 1), key)           # 0xFFFFFF00 + 256 wraps to 0


# ------------------------------------------------------------------------------------------------ the normals
SEEDS = [0x0123456789ABCDEF, 7, (1 << 63) + 12345]


def _fill(E, B, row, seeds, draw, stream_id, dtype):
    """cfgpp_philox_normal into a NaN-filled [B][row] buffer between NaN guard rows -> (values on the host, guards intact?)"""
    buf = torch.full((GUARD + B * row + GUARD,), float("nan"), dtype=dtype).cuda()
    out = buf[GUARD:GUARD + B * row].view(B, row)
    E.philox_normal(out, seeds, draw, stream_id)
    torch.cuda.synchronize()
    h = buf.cpu()
    ok = bool(torch.isnan(h[:GUARD]).all()) and bool(torch.isnan(h[GUARD + B * row:]).all())
    return h[GUARD:GUARD + B * row].view(B, row).clone(), ok


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("row", [4, 1020, 1024, 4100])
def test_philox_normal_fp32_within_the_bound_of_the_float64_model(E, B, row):
    seeds = SEEDS[:B]
    got, guards = _fill(E, B, row, seeds, 3, 0, F)
    assert guards and bool(torch.isfinite(got).all())
    model = R.normal_rows(B, row, seeds, 3, 0)
    a_case = float(np.abs(R.normal_rows(B, row, seeds, 3, 0, np.float32).astype(np.float64) - model).max())
    bound = np.maximum(4.0 * a_case, 8.0 * 2.0 ** -24 * np.abs(model) + 2.0 ** -40)
    err = np.abs(got.numpy().astype(np.float64) - model)
    print(f"philox_normal B={B} row={row}: max |err| {err.max():.3e}, A_case {a_case:.3e}, worst err / bound {(err / bound).max():.3f}")
    assert bool((err <= bound).all()), (float(err.max()), a_case)
    assert float(np.abs(got.numpy()).max()) <= 5.78


def test_fp16_fill_is_the_rne_of_the_fp32_fill(E):
    for B, row in ((1, 4), (3, 1020), (2, 4100)):
        a, ok_a = _fill(E, B, row, SEEDS[:B], 5, 1, F)
        b, ok_b = _fill(E, B, row, SEEDS[:B], 5, 1, H)
        assert ok_a and ok_b and torch.equal(a.to(H), b)


def test_chain_independence_and_draw_and_stream(E):
    row = 1020
    batch, _ = _fill(E, 3, row, SEEDS, 2, 0, F)
    for b in range(3):
        alone, _ = _fill(E, 1, row, SEEDS[b:b + 1], 2, 0, F)
        assert torch.equal(alone[0], batch[b])                      # row b of a batch of 3 = the same seed alone
    assert not torch.equal(batch[0], batch[1])
    other_draw, _ = _fill(E, 3, row, SEEDS, 3, 0, F)
    other_stream, _ = _fill(E, 3, row, SEEDS, 2, 1, F)
    assert not torch.equal(other_draw, batch) and not torch.equal(other_stream, batch) and not torch.equal(other_draw, other_stream)
    again, _ = _fill(E, 3, row, SEEDS, 2, 0, F)
    assert torch.equal(again, batch)
    # more chains than one launch carries keys for (32): the second launch's rows are keyed by their own seeds
    seeds = list(range(100, 135))
    big, ok = _fill(E, 35, 8, seeds, 0, 0, F)
    one, _ = _fill(E, 1, 8, seeds[33:34], 0, 0, F)
    assert ok and torch.equal(big[33], one[0])


# ------------------------------------------------------------------------------------------------ the step
def _coef_cases():
    """(coef6, pred_v): epsilon form with both divisor signs (IEEE division / multiplication by the reciprocal), v form; coefficients
    of the 4-step schedule's first and third step, under both scalar semantics"""
    from cfgpp_amd.lcm import step_coeffs
    from cfgpp_amd.schedule import SchedulerTables
    tb = SchedulerTables(4)
    out = []
    for t, tp in ((999, 759), (499, 259)):
        for sem in ("cpu", "cuda"):
            out.append((step_coeffs(tb, t, tp, False, sem), False))
            out.append((step_coeffs(tb, t, tp, True, sem), True))
    assert {c[0][1] > 0 for c in out if not c[1]} == {True, False}          # both divisor signs
    return out


def _guarded(x, fill):
    n = x.numel()
    buf = torch.full((n + GUARD,), fill, dtype=x.dtype)
    buf[:n] = x.flatten()
    buf = buf.cuda()
    return buf, buf[:n].view(x.shape)


def _tail_ok(buf, n, fill):
    t = buf[n:].float().cpu()
    return bool(torch.isnan(t).all()) if math.isnan(fill) else bool((t == fill).all())


def _on_rocm(fn, *tensors):
    n = tensors[0].numel()
    L = (n // 4096 + 2) * 4096
    dev = [torch.cat([t.flatten(), torch.zeros(L - n, dtype=t.dtype)]).cuda() for t in tensors]
    return tuple(o[:n].cpu() for o in fn(*dev))


STEP_SHAPES = [(1, 4), (3, 1020), (2, 4 * 12 * 12), (2, 4100)]


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("last", [False, True])
def test_step_lcm_equals_torch_bit_for_bit(E, last, single):
    bad = []
    for k, (coef, pred_v) in enumerate(_coef_cases()):
        for B, row in STEP_SHAPES:
            for lam in ((1.0,) if single else (1.5, 7.5)):
                seed = 100 * k + row % 97
                z = _rand((B, row), seed, 1.3)
                m_uc, noise = _rand((B, row), seed + 1, dtype=H), _rand((B, row), seed + 3)
                m_c = m_uc if single else _rand((B, row), seed + 2, dtype=H)
                w = R.step_lcm(z, m_uc, m_c, lam, coef, pred_v, last, noise)                                   # torch-CPU
                g = _on_rocm(lambda a, b, c, d: R.step_lcm(a, b, c, lam, coef, pred_v, last, d), z, m_uc, m_c, noise)     # torch-ROCm
                n = B * row
                zb, zv = _guarded(z, SENTINEL)
                ob, ov = _guarded(torch.zeros_like(z), SENTINEL)
                ub, uv = _guarded(m_uc, float("nan"))
                cb, cv = (ub, uv) if single else _guarded(m_c, float("nan"))
                nb, nv = _guarded(noise, float("nan"))
                E.step_lcm(zv, ov, uv, cv, lam, coef, pred_v, last, noise=nv)
                torch.cuda.synchronize()
                k0, k1 = ov.cpu(), zv.cpu()
                assert bool(torch.isfinite(k0).all()) and bool(torch.isfinite(k1).all())
                for name, (r0, r1) in (("cpu", w), ("rocm", g)):
                    d = (int((k0.flatten() != r0.flatten()).sum()), int((k1.flatten() != r1.flatten()).sum()))
                    if sum(d):
                        bad.append((name, k, B, row, lam, d))
                if last:
                    assert torch.equal(k0, k1)                      # on the last step z == den_out
                else:
                    assert not torch.equal(k0, k1)
                assert _tail_ok(zb, n, SENTINEL) and _tail_ok(ob, n, SENTINEL) and _tail_ok(ub, n, float("nan"))
                assert _tail_ok(cb, n, float("nan")) and _tail_ok(nb, n, float("nan"))
    assert not bad, bad[:8]


@pytest.mark.parametrize("pred_v", [False, True])
def test_in_register_noise_equals_the_fill(E, pred_v):
    """cfgpp_step_lcm with noise = NULL == the same call fed cfgpp_philox_normal's output (stream 0, the same draw), bit for bit"""
    coef = [c for c, v in _coef_cases() if v == pred_v][1]
    for B, row in STEP_SHAPES:
        seeds = SEEDS[:B]
        z = _rand((B, row), 5 + row, 1.3)
        m_uc, m_c = _rand((B, row), 6, dtype=H), _rand((B, row), 7, dtype=H)
        noise, ok = _fill(E, B, row, seeds, 2, 0, F)
        assert ok
        outs = []
        for kw in (dict(noise=noise.cuda()), dict(seeds=seeds, draw=2)):
            zb, zv = _guarded(z, SENTINEL)
            ob, ov = _guarded(torch.zeros_like(z), SENTINEL)
            E.step_lcm(zv, ov, m_uc.cuda(), m_c.cuda(), 1.5, coef, pred_v, False, **kw)
            torch.cuda.synchronize()
            assert _tail_ok(zb, B * row, SENTINEL) and _tail_ok(ob, B * row, SENTINEL)
            outs.append((ov.cpu(), zv.cpu()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        # another draw index gives another z, the same den
        zb, zv = _guarded(z, SENTINEL)
        ob, ov = _guarded(torch.zeros_like(z), SENTINEL)
        E.step_lcm(zv, ov, m_uc.cuda(), m_c.cuda(), 1.5, coef, pred_v, False, seeds=seeds, draw=3)
        assert torch.equal(ov.cpu(), outs[0][0]) and not torch.equal(zv.cpu(), outs[0][1])


def test_step_refusals(E):
    from cfgpp_amd._lib import CfgppError
    z = torch.zeros(2, 8, device="cuda")
    m = torch.zeros(2, 8, dtype=H, device="cuda")
    coef = (0.5, 0.5, 1.0, 0.0, 1.0, 0.0)
    with pytest.raises(CfgppError, match="needs seeds or noise"):
        E.step_lcm(z, z.clone(), m, m, 1.0, coef, False, False)
    with pytest.raises(CfgppError, match="3 seeds for 2 chains"):
        E.step_lcm(z, z.clone(), m, m, 1.0, coef, False, False, seeds=[1, 2, 3])
    z6 = torch.zeros(2, 6, device="cuda")
    with pytest.raises(CfgppError, match="row_elems=6"):
        E.philox_normal(z6, [1, 2], 0, 0)
    E.step_lcm(z, z.clone(), m, m, 1.0, coef, False, True)           # the last step needs neither
