"""-m gpu: the v-prediction kernels (include/cfgpp_vpred.h) bit for bit against torch, the guidance-rescale factor against float64,
the SD2.x-shaped tiny UNet against the oracle and v-prediction sampling chains against the CPU mock.

The step kernels follow the pattern of test_gpu_torch_semantics.py: the update written as a torch user writes it (0-dim fp32 CPU
scalars first; tests/vpred_ref.py) is evaluated by torch-ROCm on device tensors and must equal the kernel driven by the "cuda"
coefficients in every element; the same update with every rounding spelled out, evaluated by torch-CPU, must equal the kernel
driven by the "cpu" coefficients.  Every buffer carries guard elements behind ``n`` that must stay untouched, and the inputs are
NaN there.

How torch-ROCm is asked (``_on_rocm``): its elementwise kernels handle the last, partial block of a tensor (fewer than 2048 fp16
elements) on another code path than full blocks, and on that path a ``scalar * fp16`` product is not always the fp32 product rounded
to fp16 - measured on the MI355X: of the same 2047 values, elements 1028 and 1140 of ``s * x`` change when the tensor grows to 2048
elements; a 1152-element update differed from the kernel in 1 element, the same values inside a longer tensor in none.  Full blocks
are what every real latent is made of and what test_gpu_torch_semantics.py pins (its tensors are multiples of 2048), so the
reference tensors are zero-padded to whole 4096-element blocks plus one and the first ``n`` results are compared.  The kernel under
test always runs at the exact ``n``."""
import math
import os
import types

import pytest
import torch

import vpred_ref as R

pytestmark = pytest.mark.gpu

H, F, D = torch.float16, torch.float32, torch.float64
GUARD = 64
SENTINEL = 1234.0           # exact in fp16 too
EPS_REL = 2.5e-3            # the tiny-net forward tolerance of test_gpu_unet.py


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from cfgpp_amd import engine
    return engine


def _rand(shape, seed, scale=1.0, dtype=F):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _guarded(x, fill):
    """x (1-D) followed by GUARD elements of ``fill`` on the device -> (whole buffer, the view of x)"""
    n = x.numel()
    buf = torch.full((n + GUARD,), fill, dtype=x.dtype)
    buf[:n] = x.flatten()
    buf = buf.cuda()
    return buf, buf[:n]


def _on_rocm(fn, *tensors):
    """``fn`` evaluated by torch-ROCm on zero-padded device copies of the flattened tensors (see the module docstring) -> the
    first n elements of each result, on the host"""
    n = tensors[0].numel()
    L = (n // 4096 + 2) * 4096
    dev = [torch.cat([t.flatten(), torch.zeros(L - n, dtype=t.dtype)]).cuda() for t in tensors]
    return tuple(o[:n].cpu() for o in fn(*dev))


def _tail_ok(buf, n, fill):
    t = buf[n:].float().cpu()
    return bool(torch.isnan(t).all()) if math.isnan(fill) else bool((t == fill).all())


def _sqrt4_cases():
    from cfgpp_amd.schedule import SchedulerTables
    tb = SchedulerTables(50)
    zt = SchedulerTables(4, zero_terminal_snr=True, timestep_spacing="trailing")
    s0 = zt.ddim_sqrt_coeffs(999)
    assert s0[:2] == (1.0, 0.0)                                        # the step a = 0, s = 1
    return [tb.ddim_sqrt_coeffs(981), tb.ddim_sqrt_coeffs(21, inversion=True), s0]


# n = 4 (one thread), 1020 (no multiple of the block), 2*4*12*12, and one where the grid-stride loop iterates (n / 4 > 2048 * 256)
SMALL_N = (4, 1020, 2 * 4 * 12 * 12)
LARGE_N = 4 * (2048 * 256 + 300)
FLAGS = [(False, False), (False, True), (True, False), (True, True)]


def _check_step(E, n, z_half, tw, rn, lam, s4, seed):
    from cfgpp_amd.coeffs import ddim_v_coeffs_pinned
    z = _rand((n,), seed, 1.3, H if z_half else F)
    v_uc, v_c = _rand((n,), seed + 1, dtype=H), _rand((n,), seed + 2, dtype=H)
    bad = []
    # "cpu": torch-CPU on the spelled-out roundings
    w0, w1 = R.ddim_v_step(z, v_uc, v_c, lam, s4, tw, rn, "cpu")
    # "cuda": torch-ROCm on the natural expression (CPU 0-dim scalars, device tensors)
    g0, g1 = _on_rocm(lambda a, b, c: R.ddim_v_natural(a, b, c, lam, s4, tw, rn), z, v_uc, v_c)
    assert g0.dtype == z.dtype and g1.dtype == z.dtype
    for sem, (r0, r1) in (("cpu", (w0, w1)), ("cuda", (g0, g1))):
        zb, zv = _guarded(z, SENTINEL)
        ob, ov = _guarded(torch.zeros_like(z), SENTINEL)
        ub, uv = _guarded(v_uc, float("nan"))
        cb, cv = _guarded(v_c, float("nan"))
        E.step_ddim_v(zv, ov, uv, cv, lam, ddim_v_coeffs_pinned(s4, sem, z_half), tw, rn)
        torch.cuda.synchronize()
        k0, k1 = ov.cpu(), zv.cpu()
        assert bool(torch.isfinite(k0.float()).all()) and bool(torch.isfinite(k1.float()).all())
        nb = (int((k0 != r0).sum()), int((k1 != r1).sum()))
        if sum(nb):
            bad.append((sem, n, lam, nb))
        assert _tail_ok(zb, n, SENTINEL) and _tail_ok(ob, n, SENTINEL) and _tail_ok(ub, n, float("nan")) and _tail_ok(cb, n, float("nan"))
    return bad


@pytest.mark.parametrize("z_half", [False, True])
@pytest.mark.parametrize("tw,rn", FLAGS)
def test_step_ddim_v_equals_torch_bit_for_bit(E, tw, rn, z_half):
    bad = []
    for k, s4 in enumerate(_sqrt4_cases()):
        for n in SMALL_N:
            for lam in (0.0, 0.6, 1.0, 7.5):
                bad += _check_step(E, n, z_half, tw, rn, lam, s4, 100 * k + n % 97)
    bad += _check_step(E, LARGE_N, z_half, tw, rn, 0.6, _sqrt4_cases()[0], 7)
    bad += _check_step(E, LARGE_N, z_half, tw, rn, 7.5, _sqrt4_cases()[2], 8)
    assert not bad, f"elements differing from torch (semantics, n, lam, (z0t, zt)): {bad}"


def test_step_ddim_v_refuses_bad_sizes(E):
    from cfgpp_amd._lib import CfgppError
    z = torch.zeros(6, device="cuda")
    v = torch.zeros(6, device="cuda", dtype=H)
    with pytest.raises(CfgppError, match="multiple of 4"):
        E.step_ddim_v(z, z.clone(), v, v, 0.6, (1, 0, 1, 0, 1, 0), False, True)
    z = torch.zeros((2, 6), device="cuda")
    v = torch.zeros((2, 6), device="cuda", dtype=H)
    with pytest.raises(CfgppError, match="row_elems"):
        E.step_ddim_v(z, z.clone(), v, v, 0.6, (1, 0, 1, 0, 1, 0), False, True, torch.ones(2, device="cuda"))


@pytest.mark.parametrize("in_place", [False, True])
def test_v_to_eps_equals_torch_bit_for_bit(E, in_place):
    from cfgpp_amd.coeffs import v_to_eps_coeffs
    bad = []
    for n in SMALL_N + (LARGE_N,):
        for k, sigma in enumerate((14.6146, 1.7, 0.03) if n != LARGE_N else (1.7,)):
            x = _rand((n,), 3 * k + n % 89, 1.1, H)
            v_uc, v_c = _rand((n,), 50 + k, dtype=H), _rand((n,), 60 + k, dtype=H)
            a, s = R.v_to_eps_scalars(sigma)
            cpu = [R.v_to_eps_step(v, x, a, s, "cpu") for v in (v_uc, v_c)]
            rocm = [_on_rocm(lambda vv, xx: (R.v_to_eps_natural(vv, xx, a, s),), v, x)[0] for v in (v_uc, v_c)]
            for sem, want in (("cpu", cpu), ("cuda", rocm)):
                xb, xv = _guarded(x, float("nan"))
                ub, uv = _guarded(v_uc, SENTINEL)
                cb, cv = _guarded(v_c, SENTINEL)
                if in_place:
                    ob0, o0, ob1, o1 = ub, uv, cb, cv
                else:
                    ob0, o0 = _guarded(torch.zeros_like(x), SENTINEL)
                    ob1, o1 = _guarded(torch.zeros_like(x), SENTINEL)
                E.v_to_eps(o0, o1, uv, cv, xv, *v_to_eps_coeffs(sigma, sem))
                torch.cuda.synchronize()
                nb = (int((o0.cpu() != want[0]).sum()), int((o1.cpu() != want[1]).sum()))
                if sum(nb):
                    bad.append((sem, n, sigma, nb))
                assert all(_tail_ok(b, n, SENTINEL) for b in (ub, cb, ob0, ob1)) and _tail_ok(xb, n, float("nan"))
    assert not bad, f"elements differing from torch (semantics, n, sigma, (eps_uc, eps_c)): {bad}"


# ------------------------------------------------------------------------------------------------ guidance rescale
RESCALE_SHAPES = [(1, 4), (3, 144), (2, 1024), (8, 16384), (2, 65536)]


def _rescale(E, v_uc, v_c, lam, phi):
    B, n = v_uc.shape
    ub, uv = _guarded(v_uc, float("nan"))
    cb, cv = _guarded(v_c, float("nan"))
    out = torch.full((B + GUARD,), SENTINEL, device="cuda")
    f = E.cfg_rescale(uv.view(B, n), cv.view(B, n), lam, phi, out[:B])
    torch.cuda.synchronize()
    assert bool((out[B:] == SENTINEL).all())
    return f.cpu()


@pytest.mark.parametrize("B,n", RESCALE_SHAPES)
def test_cfg_rescale_against_float64(E, B, n):
    """f_b within (log2(row_elems) + 8) * 2^-23 relative of float64, on ordinary data and on the cancellation case; the degenerate
    row gives exactly 1; two runs give the same bits"""
    bound = R.rescale_bound(n)
    cases = [(_rand((B, n), n, dtype=H), _rand((B, n), n + 1, 1.3, H)), R.cancellation_case(B, n, seed=n)]
    for i, (v_uc, v_c) in enumerate(cases):
        for lam, phi in ((7.5, 0.7), (0.6, 1.0), (1.0, 0.25)):
            want = R.rescale_f64(v_uc, v_c, lam, phi)
            got = _rescale(E, v_uc, v_c, lam, phi)
            rel = float(((got.double() - want).abs() / want).max())
            print(f"cfg_rescale B={B} n={n} case={i} lam={lam} phi={phi}: rel {rel:.3e} (bound {bound:.3e})")
            assert got.dtype == F and rel <= bound, (B, n, i, lam, phi, rel, bound)
            assert torch.equal(got, _rescale(E, v_uc, v_c, lam, phi))
    const = torch.full((B, n), 0.3, dtype=H)
    mixed_uc, mixed_c = cases[0][0].clone(), cases[0][1].clone()
    mixed_uc[0], mixed_c[0] = 0.3, 0.3
    assert _rescale(E, const, const, 7.5, 0.7).tolist() == [1.0] * B
    assert float(_rescale(E, mixed_uc, mixed_c, 7.5, 0.7)[0]) == 1.0


@pytest.mark.parametrize("z_half", [False, True])
def test_step_ddim_v_with_the_gpus_own_row_scale(E, z_half):
    from cfgpp_amd.coeffs import ddim_v_coeffs_pinned
    bad = []
    for (B, n), s4 in zip([(3, 144), (2, 1024), (2, 4 * 12 * 12)], _sqrt4_cases()):
        z = _rand((B, n), n, 1.3, H if z_half else F)
        v_uc, v_c = _rand((B, n), n + 1, dtype=H), _rand((B, n), n + 2, 1.2, H)
        for tw, rn in FLAGS:
            f = E.cfg_rescale(v_uc.cuda(), v_c.cuda(), 7.5, 0.7)
            w0, w1 = R.ddim_v_step(z, v_uc, v_c, 7.5, s4, tw, rn, "cpu", f.cpu())
            f_el = f.cpu().repeat_interleave(n)              # the factor of every element: the reference runs on flat, padded tensors
            g0, g1 = _on_rocm(lambda a, b, c, fe: R.ddim_v_natural(a, b, c, 7.5, s4, tw, rn, fe), z, v_uc, v_c, f_el)
            g0, g1 = g0.view(B, n), g1.view(B, n)
            for sem, (r0, r1) in (("cpu", (w0, w1)), ("cuda", (g0, g1))):
                zk, z0 = z.clone().cuda(), torch.empty_like(z).cuda()
                E.step_ddim_v(zk, z0, v_uc.cuda(), v_c.cuda(), 7.5, ddim_v_coeffs_pinned(s4, sem, z_half), tw, rn, f)
                nb = (int((z0.cpu() != r0).sum()), int((zk.cpu() != r1).sum()))
                if sum(nb):
                    bad.append((sem, B, n, tw, rn, nb))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ nets
@pytest.mark.parametrize("rows,hw", [(2, 12), (4, 12), (2, 16), (4, 16)])
def test_tiny_sd2_forward_vs_oracle(E, rows, hw):
    """the SD2.x shape in small: 64-wide heads, linear proj_in / proj_out, a context width that is not SD1.5's; 12 x 12 latents give
    the ragged token counts 144 / 36 / 9"""
    import gpu_diag
    r = gpu_diag.unet_case("tiny_sd2", rows, hw)
    for k in ("t981", "t1"):
        print(f"tiny_sd2 rows={rows} hw={hw} {k}: {r[k]}")
        assert r[k]["finite"] and r[k]["rel_l2"] < EPS_REL, f"tiny_sd2 {k}: {r[k]}"


def _rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _sd_pair(name, nfe, B, hw, **kw):
    from cfgpp_amd.latent_diffusion import get_solver
    from cfgpp_amd.unet_config import TINY_SD2 as cfg
    from cfgpp_amd.weights import synth_state_dict
    from oracle.unet_ref import UNetRef
    from vpred_mock import VPredMockEngine
    sc = types.SimpleNamespace(num_sampling=nfe)
    hip = get_solver(name, solver_config=sc, device="cuda", unet_config=cfg, max_batch=B, latent_hw=(hw, hw), scalar_semantics="cuda", **kw)
    net = UNetRef(cfg, synth_state_dict(cfg, 0))
    eng = VPredMockEngine(lambda z, t, ehs, te, ti: net(z.float(), t, ehs.float())["sample"].half(), (hw, hw))
    ref = get_solver(name, solver_config=sc, device="cpu", unet_config=cfg, max_batch=B, latent_hw=(hw, hw), text_encoder=hip.text_encoder,
                     engine=eng, scalar_semantics="cuda", **kw)
    return hip, ref


V = dict(prediction_type="v_prediction")
# tolerances: those of the epsilon chains of the same kind in test_gpu_unet.py / test_gpu_configs.py (ddim_cfg++ 3e-3, ddim_inversion_cfg++
# 1.3e-2 on SD; ddim_cfg++ 1.5e-3, ddim_inversion_cfg++ 2.5e-2, euler_cfg++ 2e-3 on SDXL; plain ddim 4e-3)
SD_CHAINS = [("ddim_cfg++", 0.6, V, 3e-3), ("ddim_inversion_cfg++", 0.6, V, 1.3e-2), ("euler_cfg++", 0.6, V, 2e-3),
             # plain CFG multiplies the two halves' independent fp16 errors by omega - 1 and omega, so the tolerance of the existing
             # `ddim` chain (4e-3) holds at ITS guidance scale, 5.0 (at 7.5 this chain measured 4.9e-3: 1.5 x the guidance, 1.5 x the error)
             ("ddim", 5.0, dict(V, zero_terminal_snr=True, timestep_spacing="trailing", guidance_rescale=0.7), 4e-3)]


@pytest.mark.parametrize("name,lam,kw,tol", SD_CHAINS)
def test_sd2_v_chain_vs_mock(E, name, lam, kw, tol):
    """4-step v-prediction chains on TINY_SD2, B = 2: HIP UNet + v kernels vs UNetRef + the CPU emulation"""
    B, hw = 2, 12
    hip, ref = _sd_pair(name, 4, B, hw, **kw)
    uc, c = hip.get_text_embed("bad", ["a cat", "a dog"])
    job = dict(cfg_guidance=lam, prompt_embeds=(uc, c), seeds=[11, 12], return_latents=True)
    if "inversion" in name:
        job["src_latent"] = _rand((B, 4, hw, hw), 3, 0.5)
        job.pop("seeds")
    a = hip.sample(**job)[0]
    job["prompt_embeds"] = (uc.cpu(), c.cpu())
    b = ref.sample(**job)[0]
    rel = _rel_l2(a, b)
    print(f"sd2 v chain {name}: rel-L2 {rel:.3e} (tolerance {tol:.1e})")
    assert bool(torch.isfinite(a.float()).all()) and rel < tol, f"{name}: chain rel-L2 {rel:.3e}"
    names = [v[0] for v in ref.engine.vcalls]
    assert ("cfg_rescale" in names) == ("guidance_rescale" in kw) and ("v_to_eps" in names) == name.startswith("euler")


@pytest.mark.parametrize("name,tol", [("ddim_cfg++", 1.5e-3), ("ddim_inversion_cfg++", 2.5e-2)])
def test_sdxl_v_chain_vs_mock(E, name, tol):
    """the same on TINY_XL (the SDXL solver family: unguarded alpha index, added conditioning)"""
    from cfgpp_amd.latent_sdxl import get_solver
    from cfgpp_amd.unet_config import TINY_XL as cfg
    from cfgpp_amd.weights import synth_state_dict
    from oracle.unet_ref import UNetRef
    from vpred_mock import VPredMockEngine
    B, hw = 2, 16
    sc = types.SimpleNamespace(num_sampling=4)
    hip = get_solver(name, solver_config=sc, device="cuda", unet_config=cfg, max_batch=B, latent_hw=(hw, hw), scalar_semantics="cuda", **V)
    net = UNetRef(cfg, synth_state_dict(cfg, 0))

    def unet(z, t, ehs, te, ti):
        return net(z.float(), t, ehs.float(), {"text_embeds": te.float(), "time_ids": ti.float()})["sample"].half()
    ref = get_solver(name, solver_config=sc, device="cpu", unet_config=cfg, max_batch=B, latent_hw=(hw, hw), text_encoder=hip.text_encoder,
                     engine=VPredMockEngine(unet, (hw, hw)), scalar_semantics="cuda", **V)
    prompts = ["a cat", "a dog"]
    n_e, p_e, p_n, p_p = hip.get_text_embed("bad", prompts, "bad", prompts)
    kw = dict(cfg_guidance=0.6, target_size=(128, 128), original_size=(128, 128), return_latents=True)
    if "inversion" in name:
        pe = (n_e, p_e, p_e, p_n, p_p, p_p)
        kw["src_latent"] = _rand((B, 4, hw, hw), 5, 0.5, H)
    else:
        pe = (n_e, p_e, p_n, p_p)
        kw["seeds"] = [21, 22]
    a = hip.sample(prompt_embeds=pe, **kw)
    b = ref.sample(prompt_embeds=tuple(x.cpu() for x in pe), **kw)
    rel = _rel_l2(a, b)
    print(f"sdxl v chain {name}: rel-L2 {rel:.3e} (tolerance {tol:.1e})")
    assert a.shape == (B, 4, hw, hw) and bool(torch.isfinite(a.float()).all()) and rel < tol, f"{name}: chain rel-L2 {rel:.3e}"


def test_graph_switch_falls_back_to_the_eager_loop_with_v_prediction(E, monkeypatch):
    """CFGPP_GRAPH=1 with a v-prediction model: not an error - the eager loop runs and gives the eager bits"""
    hip, _ = _sd_pair("ddim_cfg++", 4, 2, 12, **V)
    uc, c = hip.get_text_embed("bad", ["a cat", "a dog"])
    job = dict(cfg_guidance=0.6, prompt_embeds=(uc, c), seeds=[1, 2], return_latents=True)
    a = hip.sample(**job)[0].cpu()
    monkeypatch.setenv("CFGPP_GRAPH", "1")
    assert hip.engine.graph_enabled
    b = hip.sample(**job)[0].cpu()
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ symbols
def test_every_symbol_of_the_header_is_exported(E):
    import re
    from cfgpp_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "cfgpp_vpred.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(cfgpp_\w+)\s*\(", hdr))
    assert len(names) == 3
    lib = _lib.load()
    for n in names:
        assert getattr(lib, n) is not None
