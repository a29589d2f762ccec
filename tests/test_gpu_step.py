"""-m gpu: fused step kernels vs the reference's golden vectors and vs the CPU oracle, bit-exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from cfgpp_amd import engine
    return engine


CASES = [("G2/sd_ddim_cfgpp_h", 50, "ddim", 0.6, True, False), ("G2/sd_ddim_cfgpp_f", 50, "ddim", 0.6, True, False),
         ("G2/sd_ddim_cfg_h", 10, "ddim", 7.5, False, False), ("G3/sd_inv_cfgpp", 10, "ddim", 0.6, True, False),
         ("G3/sd_inv_cfg", 10, "ddim", 2.0, False, False), ("G2/xl_ddim_cfgpp", 50, "ddim", 0.6, True, True),
         ("G2/xl_light_ddim_cfgpp", 4, "lightning", 1.0, True, True), ("G3/xl_edit_cfgpp", 10, "ddim", 0.6, True, False)]


@pytest.mark.parametrize("tag,nfe,kind,lam,cfgpp,wrap", CASES)
def test_ddim_family_vs_golden(E, golden, tag, nfe, kind, lam, cfgpp, wrap):
    from cfgpp_amd.coeffs import ddim_coeffs_pinned
    from cfgpp_amd.schedule import SchedulerTables
    g, _ = golden
    tb = SchedulerTables(nfe, kind)
    z, e, z0, zt = T(g[tag + "/unet_z"]), T(g[tag + "/unet_eps"]), T(g[tag + "/z0t"]), T(g[tag + "/zt"])
    off = z.shape[0] - z0.shape[0]
    half = e.dtype == torch.float16
    ts = tb.timesteps.int() if wrap else tb.timesteps

    def run(i, co, tw, rn):
        zi = z[i][0:1].contiguous().cuda()
        z0o = torch.empty_like(zi)
        E.step_ddim(zi, z0o, e[i][0:1].contiguous().cuda(), e[i][1:2].contiguous().cuda(), lam, co, tw, rn)
        return z0o.cpu(), zi.cpu()
    for i, t in enumerate(ts):
        a, b = run(off + i, ddim_coeffs_pinned(tb.ddim_sqrt_coeffs(t, wrap=wrap), eps_half=half), False, cfgpp)
        assert torch.equal(a, z0[i]) and torch.equal(b, zt[i]), f"{tag} step {i}"
    for i, t in enumerate(reversed(tb.timesteps)):
        if i >= off:
            break
        _, b = run(i, ddim_coeffs_pinned(tb.ddim_sqrt_coeffs(t, inversion=True), eps_half=half), cfgpp, False)
        assert torch.equal(b, z[i + 1][0:1]), f"{tag} inversion step {i}"


@pytest.mark.parametrize("variant,xl_form,solver", [(0, False, "dpm2m"), (1, False, "dpm2m"), (2, True, "dpm2m"), (1, False, "euler"), (0, False, "euler")])
def test_kdiff_kernel_vs_emulation_large(E, variant, xl_form, solver):
    """k-diffusion step kernel == its CPU emulation (tests/mock_engine.py, itself pinned to the golden
    trajectories in test_solver_cpu.py) on a full-size fp16 latent batch, incl. the 2M branch."""
    from cfgpp_amd.coeffs import kdiff_coeffs
    from cfgpp_amd.schedule import SchedulerTables
    from mock_engine import emulate_kdiff_input, emulate_step_kdiff
    tb = SchedulerTables(20)
    sig = tb.karras_sigmas()
    g = torch.Generator().manual_seed(3)
    n = (8, 4, 64, 64)
    x = (torch.randn(n, generator=g) * 3).half()
    old = torch.randn(n, generator=g).half()
    for i in (0, 5, 18, 19):
        eu, ec = torch.randn(n, generator=g).half(), torch.randn(n, generator=g).half()
        first = (solver == "euler") or i == 0
        coef, euler = kdiff_coeffs(0.6, sig, i, first, xl_form)
        xr, dr, orr = x.clone(), torch.empty_like(x), old.clone()
        emulate_step_kdiff(xr, dr, orr, eu, ec, coef, variant, xl_form, euler, solver != "euler")
        xd, dd, od = x.clone().cuda(), torch.empty_like(x).cuda(), old.clone().cuda()
        E.step_kdiff(xd, dd, od, eu.cuda(), ec.cuda(), coef, variant, xl_form, euler, solver != "euler")
        assert torch.equal(xd.cpu(), xr) and torch.equal(dd.cpu(), dr) and torch.equal(od.cpu(), orr), f"step {i}"
        xc_r, xc_d = torch.empty_like(x), torch.empty_like(x).cuda()
        emulate_kdiff_input(x, xc_r, 1.7321, 0 if not xl_form else 1)
        E.kdiff_input(x.cuda(), xc_d, 1.7321, 0 if not xl_form else 1)
        assert torch.equal(xc_d.cpu(), xc_r)


def test_ddim_step_full_size_properties(E):
    """BASELINE sizes ([8,4,64,64] and [16,4,128,128]): kernel == oracle on random data, and lambda = 0 with
    identical eps reduces CFG and CFG++ to the same update (size-independent property)."""
    from cfgpp_amd.coeffs import ddim_coeffs_pinned
    from cfgpp_amd.schedule import SchedulerTables
    from oracle import sampler as O
    tb = SchedulerTables(50)
    g = torch.Generator().manual_seed(5)
    for shape in ((8, 4, 64, 64), (16, 4, 128, 128)):
        z = torch.randn(shape, generator=g)
        eu, ec = torch.randn(shape, generator=g).half(), torch.randn(shape, generator=g).half()
        t = tb.timesteps[7]
        s4 = tb.ddim_sqrt_coeffs(t)
        a, b = O.ddim_step(z, eu, ec, 0.6, None, None, False, True, sqrt4=s4)
        zd, z0d = z.clone().cuda(), torch.empty_like(z).cuda()
        E.step_ddim(zd, z0d, eu.cuda(), ec.cuda(), 0.6, ddim_coeffs_pinned(s4), False, True)
        assert torch.equal(z0d.cpu(), a) and torch.equal(zd.cpu(), b)
        z1, z2 = z.clone().cuda(), z.clone().cuda()
        o1, o2 = torch.empty_like(z1), torch.empty_like(z2)
        E.step_ddim(z1, o1, eu.cuda(), eu.cuda(), 0.0, ddim_coeffs_pinned(s4), False, True)
        E.step_ddim(z2, o2, eu.cuda(), eu.cuda(), 0.0, ddim_coeffs_pinned(s4), False, False)
        assert torch.equal(z1, z2) and torch.equal(o1, o2)


def test_denoise_and_lincomb_kernels_vs_emulation(E):
    """building blocks of the ancestral / 2-stage samplers: bit-exact vs the CPU emulation that reproduces the
    reference's golden trajectories (tests/test_solver_cpu.py::test_sd_ancestral_trajectory)."""
    from mock_engine import emulate_kdiff_denoise, emulate_lincomb
    g = torch.Generator().manual_seed(9)
    n = (8, 4, 64, 64)
    x, y, z = ((torch.randn(n, generator=g) * 2).half() for _ in range(3))
    eu, ec = torch.randn(n, generator=g).half(), torch.randn(n, generator=g).half()
    dr, ur = torch.empty_like(x), torch.empty_like(x)
    emulate_kdiff_denoise(x, eu, ec, 0.6, 3.217, dr, ur)
    dd, ud = torch.empty_like(x).cuda(), torch.empty_like(x).cuda()
    E.kdiff_denoise(x.cuda(), eu.cuda(), ec.cuda(), 0.6, 3.217, dd, ud)
    assert torch.equal(dd.cpu(), dr) and torch.equal(ud.cpu(), ur)
    for mode, (a, b) in ((0, (0.7312, -0.2466)), (1, (0.6123, 0.3711)), (2, (1.913, 0.0))):
        outr = torch.empty_like(x)
        emulate_lincomb(outr, x, y, z if mode == 1 else None, a, b, mode)
        outd = torch.empty_like(x).cuda()
        E.lincomb(outd, x.cuda(), y.cuda(), z.cuda() if mode == 1 else None, a, b, mode)
        assert torch.equal(outd.cpu(), outr), f"mode {mode}"
        xin = x.clone().cuda()                      # in-place form (out aliases x), as the solvers use it
        E.lincomb(xin, xin, y.cuda(), z.cuda() if mode == 1 else None, a, b, mode)
        assert torch.equal(xin.cpu(), outr), f"mode {mode} in place"


def test_ancestral_solvers_run_on_gpu():
    """euler_a / dpm++_2s_a (+cfg++) end to end on the HIP engine: finite, right shapes, and deterministic
    given the device RNG seed."""
    import types
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from cfgpp_amd.latent_diffusion import get_solver
    from cfgpp_amd.unet_config import TINY_SD as cfg
    for name, lam in (("euler_a", 7.5), ("euler_a_cfg++", 0.6), ("dpm++_2s_a", 7.5), ("dpm++_2s_a_cfg++", 0.6)):
        s = get_solver(name, solver_config=types.SimpleNamespace(num_sampling=6), device="cuda", unet_config=cfg, max_batch=2)
        outs = []
        for _ in range(2):
            torch.cuda.manual_seed(5)
            den, x = s.sample(cfg_guidance=lam, prompt=["bad", ["a cat", "a dog"]], seeds=[1, 2], return_latents=True)
            outs.append((den.float().cpu(), x.float().cpu()))
        assert outs[0][0].shape == (2, 4, 16, 16) and torch.isfinite(outs[0][1]).all()
        assert torch.equal(outs[0][1], outs[1][1]), name


# ---------------------------------------------------------------------------------------------------- launch edges, guarded buffers
# The tests above run sizes such as [8, 4, 64, 64]: whole blocks, a grid below the cap of 2048 blocks x 256 threads, so every thread
# runs its grid-stride loop body once.  Here: one thread, a partial last block on both sides of a block boundary, and one item more
# than the capped grid has threads (thread 0 takes a second trip) - float4 kernels in units of 4 values.  Every operand lives in an
# allocation with guard elements before and after (tests/test_gpu_small.py: a NaN bit pattern, which also fills every destination
# before the launch), and the guards must hold their bits afterwards.  Same bit-exact CPU emulations as above.
F4_SIZES = (4, 1020, 1024, 1028, 4 * 2048 * 256 + 4)
SC_SIZES = (1, 255, 257, 2048 * 256 + 1)


def _gin(t):
    """a CPU tensor -> (guarded allocation, its device view holding t)"""
    from test_gpu_small import guarded
    buf, v = guarded(tuple(t.shape), t.dtype)
    v.copy_(t.cuda())
    return buf, v


def _gout(n, dtype):
    from test_gpu_small import guarded
    return guarded((n,), dtype)


def _intact(*bufs):
    from test_gpu_small import guards_intact
    return all(guards_intact(b) for b in bufs)


def _same(dev_view, want):
    it = torch.int16 if want.dtype == torch.float16 else torch.int32
    return torch.equal(dev_view.cpu().view(it), want.contiguous().view(it))


@pytest.mark.parametrize("n", F4_SIZES)
@pytest.mark.parametrize("latent,eps", [("f32", "f16"), ("f32", "f32"), ("f16", "f16")])
def test_ddim_step_edges(E, n, latent, eps):
    """ddim_step_kernel<true>, <false> and ddim_step_h_kernel: all four (tweedie, renoise) pairs at the small sizes, CFG++ at the
    size that wraps the grid"""
    from cfgpp_amd.coeffs import ddim_coeffs_pinned
    from cfgpp_amd.schedule import SchedulerTables
    from mock_engine import emulate_step_ddim
    tb = SchedulerTables(50)
    co = ddim_coeffs_pinned(tb.ddim_sqrt_coeffs(tb.timesteps[7]), eps_half=eps == "f16")
    zt, et = (torch.float32 if k == "f32" else torch.float16 for k in (latent, eps))
    g = torch.Generator().manual_seed(n % 9973 + len(latent + eps))
    z = torch.randn(n, generator=g).to(zt)
    eu, ec = torch.randn(n, generator=g).to(et), torch.randn(n, generator=g).to(et)
    flags = [(False, True)] if n > 4096 else [(False, False), (False, True), (True, False), (True, True)]
    for tw, rn in flags:
        zr, z0r = z.clone(), torch.empty_like(z)
        emulate_step_ddim(zr, z0r, eu, ec, 0.6, co, tw, rn)
        (bz, zd), (b0, z0d), (bu, ud), (bc, cd) = _gin(z), _gout(n, zt), _gin(eu), _gin(ec)
        E.step_ddim(zd, z0d, ud, cd, 0.6, co, tw, rn)
        torch.cuda.synchronize()
        assert _intact(bz, b0, bu, bc), (n, tw, rn, "guard elements written")
        assert _same(z0d, z0r) and _same(zd, zr), (n, latent, eps, tw, rn)
        assert _same(ud, eu) and _same(cd, ec)


@pytest.mark.parametrize("n", SC_SIZES)
def test_kdiff_kernels_edges(E, n):
    """kdiff_input (both modes), kdiff_step at the variant / form / solver combinations of test_kdiff_kernel_vs_emulation_large on the
    Euler and the 2M branch, kdiff_denoise"""
    from cfgpp_amd.coeffs import kdiff_coeffs
    from cfgpp_amd.schedule import SchedulerTables
    from mock_engine import emulate_kdiff_denoise, emulate_kdiff_input, emulate_step_kdiff
    sig = SchedulerTables(20).karras_sigmas()
    g = torch.Generator().manual_seed(n % 9973)
    x = (torch.randn(n, generator=g) * 3).half()
    old = torch.randn(n, generator=g).half()
    eu, ec = torch.randn(n, generator=g).half(), torch.randn(n, generator=g).half()
    for mode, s in ((0, 1.7321), (1, 0.5774), (0, -0.5774)):
        xr = torch.empty_like(x)
        emulate_kdiff_input(x, xr, s, mode)
        (bx, xd), (bo, od) = _gin(x), _gout(n, torch.float16)
        E.kdiff_input(xd, od, s, mode)
        torch.cuda.synchronize()
        assert _intact(bx, bo) and _same(od, xr) and _same(xd, x), (n, mode, s)
    for variant, xl_form, solver in [(0, False, "dpm2m"), (1, False, "dpm2m"), (2, True, "dpm2m"), (1, False, "euler"), (0, False, "euler")]:
        for i in (0, 5):
            first = solver == "euler" or i == 0
            coef, euler = kdiff_coeffs(0.6, sig, i, first, xl_form)
            xr, dr, orr = x.clone(), torch.empty_like(x), old.clone()
            emulate_step_kdiff(xr, dr, orr, eu, ec, coef, variant, xl_form, euler, solver != "euler")
            (bx, xd), (bd, dd), (bo, od), (bu, ud), (bc, cd) = _gin(x), _gout(n, torch.float16), _gin(old), _gin(eu), _gin(ec)
            E.step_kdiff(xd, dd, od, ud, cd, coef, variant, xl_form, euler, solver != "euler")
            torch.cuda.synchronize()
            assert _intact(bx, bd, bo, bu, bc), (n, variant, xl_form, solver, i, "guard elements written")
            assert _same(xd, xr) and _same(dd, dr) and _same(od, orr), (n, variant, xl_form, solver, i)
    dr, ur = torch.empty_like(x), torch.empty_like(x)
    emulate_kdiff_denoise(x, eu, ec, 0.6, 3.217, dr, ur)
    (bx, xd), (bu, ud), (bc, cd), (bd, dd), (bn, nd) = _gin(x), _gin(eu), _gin(ec), _gout(n, torch.float16), _gout(n, torch.float16)
    E.kdiff_denoise(xd, ud, cd, 0.6, 3.217, dd, nd)
    torch.cuda.synchronize()
    assert _intact(bx, bu, bc, bd, bn) and _same(dd, dr) and _same(nd, ur) and _same(xd, x), n


@pytest.mark.parametrize("n", SC_SIZES)
def test_lincomb_edges(E, n):
    """lincomb modes 0 - 2, into a fresh destination and in place (out aliases x)"""
    from mock_engine import emulate_lincomb
    g = torch.Generator().manual_seed(n % 9973 + 1)
    x, y, z = ((torch.randn(n, generator=g) * 2).half() for _ in range(3))
    for mode, (a, b) in ((0, (0.7312, -0.2466)), (1, (0.6123, 0.3711)), (2, (1.913, 0.0))):
        want = torch.empty_like(x)
        emulate_lincomb(want, x, y, z if mode == 1 else None, a, b, mode)
        (bx, xd), (by, yd), (bz, zd), (bo, od) = _gin(x), _gin(y), _gin(z), _gout(n, torch.float16)
        E.lincomb(od, xd, yd, zd if mode == 1 else None, a, b, mode)
        torch.cuda.synchronize()
        assert _intact(bx, by, bz, bo) and _same(od, want) and _same(xd, x) and _same(yd, y) and _same(zd, z), (n, mode)
        E.lincomb(xd, xd, yd, zd if mode == 1 else None, a, b, mode)
        torch.cuda.synchronize()
        assert _intact(bx, by, bz) and _same(xd, want) and _same(yd, y) and _same(zd, z), (n, mode, "in place")
