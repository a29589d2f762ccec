"""-m gpu: the panorama kernels (include/cfgpp_panorama.h; csrc/pano_kernels.hip) against the slice model of tests/pano_ref.py
evaluated on torch-CPU, bit for bit - the project's contract for step kernels.

Every case of the table (tests/pano_cases.py) x B in {1, 2} x every divisor Vc x CFG / CFG++ x both signs of the divisor c2 x
lam in {1.0, 7.5}, on random fp16 eps that differ per view.  The destinations are NaN-filled and sit between guard rows."""
import itertools

import pytest
import torch

import pano_ref as R
from pano_cases import CASES, case_id, divisors

pytestmark = pytest.mark.gpu

H, F = torch.float16, torch.float32
GUARD = 256          # elements on either side of every buffer (a multiple of 16 bytes in both dtypes)
C1, C2, C3, C4 = 0.5908203125, 0.8068, 0.8170, 0.5766          # c1 and c4 multiply fp16 eps; any fp32 values exercise the roundings


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _guarded(shape, dtype, fill):
    """a contiguous GPU tensor of ``shape`` holding ``fill`` inside a longer buffer whose two ends hold a sentinel"""
    n = 1
    for d in shape:
        n *= int(d)
    buf = torch.full((n + 2 * GUARD,), 777.0, dtype=dtype, device="cuda")
    t = buf[GUARD:GUARD + n].view(shape)
    if torch.is_tensor(fill):
        t.copy_(fill)
    else:
        t.fill_(fill)
    return buf, t


def _guards_intact(buf):
    return bool((buf[:GUARD] == 777.0).all()) and bool((buf[-GUARD:] == 777.0).all())


def _geometry(case, Vc):
    from cfgpp_amd.panorama import ViewGeometry
    Hp, Wp, h, w, stride, circ = case
    return ViewGeometry(Hp, Wp, h, w, stride, bool(circ), Vc)


def _inputs(case, B, seed):
    """z [B, 4, Hp, Wp] fp32 and per-view eps [V, 2, B, 4, h, w] fp16 (uc, c), fixed seed"""
    Hp, Wp, h, w, _, _ = case
    V = CASES[case][0]
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, 4, Hp, Wp, generator=g)
    eps = torch.randn(V, 2, B, 4, h, w, generator=g).to(H)
    return z, eps


def _chunked(eps_v, Vc):
    """[V, 2, B, ...] -> the engine's layout [V / Vc, 2 * Vc * B, ...]: per chunk the uc rows (row vi * B + b), then the c rows"""
    V, _, B = eps_v.shape[:3]
    e = eps_v.view(V // Vc, Vc, 2, B, *eps_v.shape[3:]).permute(0, 2, 1, 3, 4, 5, 6)
    return e.reshape(V // Vc, 2 * Vc * B, *eps_v.shape[3:]).contiguous()


@pytest.mark.parametrize("case", list(CASES), ids=case_id)
def test_step_views_bit_exact_against_the_slice_model(case):
    need_gpu()
    from cfgpp_amd import engine as E
    V = CASES[case][0]
    combos = 0
    for B in (1, 2):
        z0, eps_v = _inputs(case, B, seed=100 + B)
        assert not torch.equal(eps_v[0], eps_v[-1]) or V == 1
        for Vc in divisors(V):
            g = _geometry(case, Vc)
            eps = _chunked(eps_v, Vc)
            eps_buf, eps_d = _guarded(eps.shape, H, eps)
            for renoise_uc, sign, lam in itertools.product((False, True), (1.0, -1.0), (1.0, 7.5)):
                co = (C1, sign * (C2 if sign > 0 else 1.0 / C2), C3, C4)          # c2 < 0: the kernel multiplies by -c2
                # the model, on torch-CPU
                zv_ref = R.gather(case, z0, B)
                z_ref, z0t_ref = R.step(case, z0, zv_ref, eps, B, Vc, lam, co, False, renoise_uc)
                # the kernel: z in place, z0t and z_views NaN-filled, everything between guards
                z_buf, z_d = _guarded(z0.shape, F, z0)
                z0t_buf, z0t_d = _guarded(z0.shape, F, float("nan"))
                zv_buf, zv_d = _guarded(zv_ref.shape, F, float("nan"))
                E.step_ddim_views(g, z_d, z0t_d, zv_d, eps_d, lam, co, False, renoise_uc)
                torch.cuda.synchronize()
                what = (B, Vc, renoise_uc, sign, lam)
                assert torch.equal(z_d.cpu(), z_ref), what
                assert torch.equal(z0t_d.cpu(), z0t_ref), what
                assert torch.equal(zv_d.cpu(), zv_ref), what
                assert torch.equal(zv_d.cpu(), R.gather(case, z_d.cpu(), B)), what          # the views ARE the new panorama's slices
                assert all(_guards_intact(b) for b in (z_buf, z0t_buf, zv_buf, eps_buf)), what
                assert torch.equal(eps_d.cpu(), eps), what                                   # eps is only read
                combos += 1
    assert combos == 2 * len(divisors(V)) * 8


@pytest.mark.parametrize("case", list(CASES), ids=case_id)
def test_views_gather_equals_the_slices(case):
    need_gpu()
    from cfgpp_amd import engine as E
    for B in (1, 2):
        z0, _ = _inputs(case, B, seed=7)
        want = R.gather(case, z0, B)
        z_buf, z_d = _guarded(z0.shape, F, z0)
        zv_buf, zv_d = _guarded(want.shape, F, float("nan"))
        E.gather_views(_geometry(case, 1), z_d, zv_d)
        torch.cuda.synchronize()
        assert torch.equal(zv_d.cpu(), want) and torch.equal(z_d.cpu(), z0)
        assert _guards_intact(z_buf) and _guards_intact(zv_buf)


@pytest.mark.parametrize("renoise_uc,sign,lam", list(itertools.product((False, True), (1.0, -1.0), (1.0, 7.5))))
def test_one_view_is_cfgpp_step_ddim_on_the_same_buffers(renoise_uc, sign, lam):
    need_gpu()
    from cfgpp_amd import engine as E
    case = (8, 8, 8, 8, 4, 0)
    for B in (1, 2):
        z0, eps_v = _inputs(case, B, seed=31)
        eps = _chunked(eps_v, 1).cuda()
        co = (C1, sign * (C2 if sign > 0 else 1.0 / C2), C3, C4)
        za, z0ta = z0.cuda(), torch.full_like(z0, float("nan")).cuda()
        zva = torch.full((B, 4, 8, 8), float("nan"), device="cuda")
        E.step_ddim_views(_geometry(case, 1), za, z0ta, zva, eps, lam, co, False, renoise_uc)
        zb, z0tb = z0.cuda(), torch.full_like(z0, float("nan")).cuda()
        E.step_ddim(zb, z0tb, eps[0, :B].contiguous(), eps[0, B:].contiguous(), lam, co, False, renoise_uc)
        torch.cuda.synchronize()
        assert torch.equal(za, zb) and torch.equal(z0ta, z0tb) and torch.equal(zva, zb)


def test_library_refuses_bad_geometry_by_name():
    need_gpu()
    from cfgpp_amd import engine as E
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.panorama import ViewGeometry

    class Raw(ViewGeometry):          # the library's own checks: geometry the host code would have refused
        n = 1

        @property
        def n_views(self):
            return self.n

    z, zv = torch.zeros(1, 4, 8, 16, device="cuda"), torch.zeros(1, 4, 8, 8, device="cuda")
    for g, word in ((Raw(8, 16, 8, 8, 6, False), "multiples of 4"), (Raw(8, 16, 8, 8, 12, False), "exceeds the window"),
                    (Raw(8, 16, 8, 8, 4, False, 2), "does not divide the 3 views")):
        with pytest.raises(CfgppError, match=word):
            E.gather_views(g, z, zv)
    with pytest.raises(CfgppError, match="z_views shape"):
        E.gather_views(ViewGeometry(8, 16, 8, 8, 4, False), z, zv)
