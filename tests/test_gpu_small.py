"""-m gpu: every launch path of csrc/small_kernels.hip - conv_in, conv_out (wave-per-pixel and LDS-tiled), the sinusoidal embedding,
the skinny GEMM, f16_to_f32_rows, the fan-out of the shared CFG prefix and the VAE posterior - against the fp64 references of
tests/small_cases.py, per element.

Every destination is allocated with guard elements before and after and prefilled, guards included, with a NaN bit pattern.  After
the call the write set must be finite everywhere (an element the kernel never stores stays NaN) and within the derived bound of
small_cases' docstring; everything outside the write set - conv_in's halo ring, the guards (rows at or beyond R), columns outside
[out_off, out_off + dim) or [0, N), the fan-out's rows [0, h) and >= 2h - must hold the same bits as before; conv_out must have
launched the kernel and instance the case is named after (cfgpp_conv_out_last_launch against small_cases.expected_launch_co).  The
whole-tensor rel-L2 of the older tests is kept.  Sources carry NaN wherever the kernel has no business reading (the addend's halo,
the padding columns of x and addend rows).  tests/test_small_cases_cpu.py shows which faults these conditions catch."""
import numpy as np
import pytest
import torch

import small_cases as S
from test_gpu_configs import need_gpu, record

pytestmark = pytest.mark.gpu

GUARD = 4096                                     # guard elements before and after every destination (16-byte aligned for fp16)
SENT = {torch.float16: (torch.int16, 0x7e57), torch.float32: (torch.int32, 0x7fc0e57a)}          # NaN bit patterns
ids = dict(ids=lambda c: c.id)


def dev():
    import hip_ops as H
    return H.DEV


def guarded(shape, dtype):
    """-> (whole buffer as integers, the view of `shape` the kernel writes): the sentinel everywhere"""
    it, bits = SENT[dtype]
    n = int(np.prod(shape))
    buf = torch.full((2 * GUARD + n,), bits, dtype=it, device=dev())
    return buf, buf[GUARD:GUARD + n].view(dtype).view(*shape)


def guards_intact(buf):
    bits = 0x7e57 if buf.dtype == torch.int16 else 0x7fc0e57a
    return bool((buf[:GUARD] == bits).all()) and bool((buf[-GUARD:] == bits).all())


def untouched(t):
    """elementwise: does t still hold the sentinel bits"""
    it, bits = SENT[t.dtype]
    return t.contiguous().view(it) == bits


def to_dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev(), dtype).contiguous()


def nan_padded(a, ld, dtype=torch.float32):
    """rows of a [rows, n] at stride ld, NaN in the padding columns"""
    t = torch.full((a.shape[0], ld), float("nan"), dtype=dtype, device=dev())
    t[:, :a.shape[1]] = to_dev(a, dtype)
    return t


def judge(group, c, got, ref, rounding, rest, problems, rel_l2=True, **extra):
    """the assertions every bounded case shares; got / ref: numpy arrays of the write set"""
    got = np.asarray(got, dtype=np.float64)
    finite = bool(np.isfinite(got).all())
    q = S.ratio(got, ref, rounding, rest)
    rel = S.rel_l2(got, ref) if finite else float("inf")
    record("small_case", group=group, case=c.id, ratio=q, rel_l2=rel, problems=problems, **extra)
    print(f"{group} {c.id}: ratio {q:.3f} rel_l2 {rel:.3e} {problems} {extra}")
    assert not problems, (c.id, problems)
    assert finite, f"{c.id}: {int((~np.isfinite(got)).sum())} elements of the write set not finite (unwritten or NaN)"
    assert q <= 1.0, f"{c.id}: (|got - ref64| - rounding) / rest = {q:.3f} > 1, {S.violations(got, ref, rounding, rest)} elements outside the bound"
    if rel_l2:
        assert rel < S.REL_L2_BOUND, f"{c.id}: rel-L2 {rel:.3e}"


# ---- conv_in -------------------------------------------------------------------------------------------------------------------
def run_conv_in(c, out):
    import hip_ops as H
    i = S.ci_inputs(c)
    z = to_dev(i.z, torch.float16 if c.z_half else torch.float32)
    wk, bias = to_dev(S.ci_pack_w(i.w), torch.float32), to_dev(i.bias, torch.float32)
    if c.entry == "ex":
        return H.conv_in_ex(z, wk, bias, c.R, c.Cout, pre_w=to_dev(i.pre_w, torch.float32), pre_b=to_dev(i.pre_b, torch.float32),
                            in_scale=c.in_scale, out=out)
    add = None
    if c.add_rows:                                               # the addend in the output's layout, NaN in its halo
        add = torch.full((c.add_rows, c.H + 2, c.W + 2, c.Cout), float("nan"), dtype=torch.float16, device=dev())
        add[:, 1:c.H + 1, 1:c.W + 1] = to_dev(i.add, torch.float16)
    return H.conv_in_add(z, wk, bias, c.R, c.Cout, cond=to_dev(i.cond, torch.float16), addend=add, out=out)


@pytest.mark.parametrize("c", S.CONV_IN, **ids)
def test_conv_in(c):
    """pixel tails, one and several blocks, the second Cout pass, Cz 1 .. 8 with 0 .. 8 condition channels up to the 16 of patch[],
    fp32 and fp16 z, rows r % zB with fewer condition and addend rows, bias on and off, the folded pre-conv with exact and real inputs"""
    need_gpu()
    r = S.ci_reference(c)
    buf, out = guarded((c.R, c.H + 2, c.W + 2, c.Cout), torch.float16)
    run_conv_in(c, out)
    torch.cuda.synchronize()
    problems = [] if guards_intact(buf) else ["guard elements written (rows at or beyond R, or before row 0)"]
    ring = untouched(out)
    ring[:, 1:c.H + 1, 1:c.W + 1] = True
    if not bool(ring.all()):
        problems.append("halo ring written")
    got = out[:, 1:c.H + 1, 1:c.W + 1].double().cpu().numpy()
    judge("conv_in", c, got, r.ref, *S.ci_bound(c, got), problems)


# ---- conv_out ------------------------------------------------------------------------------------------------------------------
def check_conv_out(c, group, tiled):
    import hip_ops as H
    r = S.co_reference(c)
    xp, wk = S.co_device_layout(r.inputs)
    x, w, bias = to_dev(xp, torch.float16), to_dev(wk, torch.float16), to_dev(r.inputs.bias, torch.float32)
    ps, sh, clamp = c.post_op
    lib = H.lib()
    lib.cfgpp_conv_out_set_tiled(tiled)
    try:
        buf, out = guarded((c.R, c.Cout, c.H, c.W), torch.float16 if c.out_half else torch.float32)
        H.conv_out_ex(x, w, bias, out_half=bool(c.out_half), post_scale=ps, post_shift=sh, clamp01=clamp, out=out)
        launch = H.conv_out_last_launch()
        torch.cuda.synchronize()
    finally:
        lib.cfgpp_conv_out_set_tiled(1)
    problems = [] if guards_intact(buf) else ["guard elements written"]
    want = S.expected_launch_co(c, tiled)
    if launch != want:
        problems.append(f"dispatched {launch} (kernel, CO, out_is_half, workgroups), the case is for {want}")
    got = out.double().cpu().numpy()
    judge(group, c, got, r.ref, *S.co_bound(c, got), problems, launch=list(launch))
    if clamp:
        assert got.min() >= 0.0 and got.max() <= 1.0


@pytest.mark.parametrize("c", S.CONV_OUT_WAVE, **ids)
def test_conv_out_wave_per_pixel(c):
    """C = 8 (9 chunks for 64 lanes) .. 512 (576 chunks, 9 passes), 1 .. 4 outputs on the 4-wide instance in fp16 and fp32, 5 and 8 on
    the 8-wide one, pixel counts that are no multiple of the 4 waves of a workgroup, the post-op with both clamp ends binding"""
    need_gpu()
    check_conv_out(c, "conv_out_wave", 1)


@pytest.mark.parametrize("c", S.CONV_OUT_TILED, **ids)
def test_conv_out_tiled_and_the_wave_kernel_on_the_same_map(c):
    """all three instances, 1 .. 4 outputs, maps narrower than a tile in either direction (the halo guard and the store guard do all
    the work), ragged last tiles; every case again with the A/B switch off, each run against the reference"""
    need_gpu()
    check_conv_out(c, "conv_out_tiled", 1)
    check_conv_out(c, "conv_out_tiled_switch_off", 0)


# ---- sinusoid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.SINUSOID, **ids)
def test_sinusoid(c):
    """the vector and the scalar form, dims 2 .. 320, into a row of its own and into SDXL's 2816-wide row at 1280 + 256 k"""
    need_gpu()
    import hip_ops as H
    buf, out = guarded((c.count, c.ld), torch.float32)
    if c.scalar:
        H.sinusoid_ex(None, c.dim, count=c.count, scalar=c.vals[0], out_ld=c.ld, out_off=c.out_off, out=out)
    else:
        H.sinusoid_ex(to_dev(np.array(c.vals), torch.float32), c.dim, out_ld=c.ld, out_off=c.out_off, out=out)
    torch.cuda.synchronize()
    problems = [] if guards_intact(buf) else ["guard elements written"]
    outside = untouched(out)
    outside[:, c.out_off:c.out_off + c.dim] = True
    if not bool(outside.all()):
        problems.append("columns outside [out_off, out_off + dim) written")
    got = out[:, c.out_off:c.out_off + c.dim].double().cpu().numpy()
    judge("sinusoid", c, got, S.sn_ref64(c), *S.sn_bound(c), problems)
    assert np.array_equal(got, S.h16(got))                                 # values rounded through fp16


# ---- skinny GEMM ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.SKINNY, **ids)
def test_skinny_gemm(c):
    """both instances (M = 1, M > 1 with clamped tail rows), odd N (the clamped second column), K = 8 .. 2816 with a partial last
    pass, a broadcast x row, padded x / addend / out rows, the addend with M = 1, all four SiLU combinations saturating on both sides"""
    need_gpu()
    import hip_ops as H
    r = S.sk_reference(c)
    i = r.inputs
    x = to_dev(i.x, torch.float32) if c.ldx != "K+8" else nan_padded(i.x, c.K + 8)
    add = None if not c.add else nan_padded(i.add, c.add_ld)
    buf, out = guarded((c.M, c.N + c.ldo), torch.float32)
    H.skinny_ex(x, c.ldx_v, to_dev(i.w, torch.float16), to_dev(i.bias, torch.float32), c.M, addend=add, add_ld=c.add_ld, ldo=c.N + c.ldo,
                silu_in=c.silu_in, silu_out=c.silu_out, out=out)
    torch.cuda.synchronize()
    problems = [] if guards_intact(buf) else ["guard elements written"]
    if not bool(untouched(out[:, c.N:]).all()):
        problems.append("columns [N, ldo) written")
    judge("skinny", c, out[:, :c.N].double().cpu().numpy(), r.ref, r.rounding, r.rest, problems)


# ---- f16_to_f32_rows, fan-out: exact ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.ROWS, **ids)
def test_f16_to_f32_rows(c):
    need_gpu()
    import hip_ops as H
    x = torch.from_numpy(S.rw_input(c)).to(dev())
    buf, out = guarded((c.rows, c.ld), torch.float32)
    H.f16_to_f32_rows(x, out_ld=c.ld, out_off=c.out_off, out=out)
    torch.cuda.synchronize()
    assert guards_intact(buf)
    outside = untouched(out)
    outside[:, c.out_off:c.out_off + c.cols] = True
    assert bool(outside.all()), "columns outside [out_off, out_off + cols) written"
    assert torch.equal(out[:, c.out_off:c.out_off + c.cols], x.float()), c.id
    record("small_case", group="rows", case=c.id, ratio=0.0, exact=True)


@pytest.mark.parametrize("c", S.FANOUT, **ids)
def test_fanout_rows(c):
    """the unrolled loop alone, the tail loop alone, both; one to three segments of very unequal length; the 2048-block cap"""
    need_gpu()
    import hip_ops as H
    g = torch.Generator(device=dev()).manual_seed(len(c.n16) * 7 + c.h)
    bufs, views, before = [], [], []
    for n in c.n16:
        row = 8 * n
        buf = torch.randint(-32768, 32767, (2 * GUARD + 2 * c.h * row,), dtype=torch.int16, device=dev(), generator=g)
        bufs.append(buf)
        before.append(buf.clone())
        views.append(buf[GUARD:GUARD + 2 * c.h * row].view(torch.float16).view(2 * c.h, row))
    H.fanout_rows(views, c.h)
    torch.cuda.synchronize()
    for k, (buf, old) in enumerate(zip(bufs, before)):
        lo = GUARD + c.h * 8 * c.n16[k]                      # first element of rows [h, 2h)
        assert torch.equal(buf[:lo], old[:lo]), f"{c.id}: segment {k}: rows [0, h) or the guard before them changed"
        assert torch.equal(buf[-GUARD:], old[-GUARD:]), f"{c.id}: segment {k}: rows >= 2h changed"
        assert torch.equal(buf[lo:-GUARD], old[GUARD:lo]), f"{c.id}: segment {k}: rows [h, 2h) are no copy of rows [0, h)"
    record("small_case", group="fanout", case=c.id, ratio=0.0, exact=True, grid=S.fo_grid(c))


# ---- VAE posterior -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.POSTERIOR, **ids)
def test_vae_posterior(c):
    """moments against the quant conv of the fp16-rounded input with the logvar clamp binding at both ends; z against the fp64 formula
    on the returned moments; with moments == null the same z bit for bit"""
    need_gpu()
    import hip_ops as H
    i = S.po_inputs(c)
    co, qw, qb, noise = (to_dev(a, torch.float32) for a in (i.co, i.qw, i.qb, i.noise))
    zbuf, z = guarded((c.B, 4, c.HW), torch.float32)
    mbuf, m = guarded((c.B, 8, c.HW), torch.float32)
    H.vae_posterior(co, qw, qb, noise, c.scale, out=z, out_moments=m)
    zbuf2, z2 = guarded((c.B, 4, c.HW), torch.float32)
    H.vae_posterior(co, qw, qb, noise, c.scale, moments=False, out=z2)
    torch.cuda.synchronize()
    problems = [] if guards_intact(zbuf) and guards_intact(mbuf) and guards_intact(zbuf2) else ["guard elements written"]
    mg, zg = m.double().cpu().numpy(), z.double().cpu().numpy()
    r = S.po_moments_ref(c)
    judge("posterior_moments", c, mg, r.ref, 0.5 * S.ulp16(np.nan_to_num(mg)), r.rest, problems, rel_l2=False)
    assert mg[:, 4:].min() >= -30.0 and mg[:, 4:].max() <= 20.0 and np.array_equal(mg, S.h16(mg))
    if c.clamp:
        assert (mg[:, 4:] == 20.0).any() and (mg[:, 4:] == -30.0).any()
    judge("posterior_z", c, zg, *S.po_z_ref(c, mg), [], rel_l2=False)
    assert torch.equal(z.view(torch.int32), z2.view(torch.int32)), f"{c.id}: z depends on whether moments are returned"


# ---- refusals: the error code with a message, nothing launched, the destination untouched -----------------------------------------
def test_refused_calls_leave_their_destinations_untouched():
    need_gpu()
    import hip_ops as H
    from cfgpp_amd._lib import CfgppError
    f16, f32 = torch.float16, torch.float32
    z = torch.zeros((1, 9, 4, 4), dtype=f32, device=dev())
    w = torch.zeros((9 * 17 * 8,), dtype=f32, device=dev())
    cond = torch.zeros((1, 9, 4, 4), dtype=f16, device=dev())
    buf, out = guarded((1, 6, 6, 8), f16)
    with pytest.raises(CfgppError, match="conv_in: Cin=9"):
        H.conv_in_add(z, w, None, 1, 8, out=out)
    with pytest.raises(CfgppError, match="conv_in: condition of 9 channels"):
        H.conv_in_add(z[:, :8].contiguous(), w, None, 1, 8, cond=cond, out=out)
    lib = H.lib()
    z4, add = z[:, :4].contiguous(), torch.zeros((1, 6, 6, 8), dtype=f16, device=dev())
    assert lib.cfgpp_op_conv_in_add(H.P(z4), 0, None, 0, 0, H.P(add), 0, H.P(out), H.P(w), None, 1, 1, 4, 4, 4, 8, H.stream()) != 0
    assert b"add_rows=0" in lib.cfgpp_last_error()
    assert lib.cfgpp_op_conv_in_add(None, 0, None, 0, 0, None, 0, H.P(out), H.P(w), None, 1, 1, 4, 4, 4, 8, H.stream()) != 0
    assert b"conv_in" in lib.cfgpp_last_error()
    torch.cuda.synchronize()
    assert bool(untouched(out).all()) and guards_intact(buf)

    for (C, Cout, half, msg) in ((64, 9, 0, "Cout=9"), (12, 4, 0, "C=12"), (64, 8, 1, "fp32 only")):
        x = torch.zeros((1, 6, 6, C), dtype=f16, device=dev())
        wk = torch.zeros((Cout, 9, C), dtype=f16, device=dev())
        buf, out = guarded((1, Cout, 4, 4), f16 if half else f32)
        with pytest.raises(CfgppError, match=msg):
            H.conv_out_ex(x, wk, None, out_half=bool(half), out=out)
        torch.cuda.synchronize()
        assert H.conv_out_last_launch() == (0, 0, 0, 0) and bool(untouched(out).all()) and guards_intact(buf)

    buf, out = guarded((2, 8), f32)
    with pytest.raises(CfgppError, match="sinusoid"):
        H.sinusoid_ex(None, 7, count=2, scalar=1.0, out_ld=8, out=out)
    assert lib.cfgpp_op_sinusoid(None, 1.0, H.P(out), 0, 8, 8, 0, H.stream()) != 0
    x = torch.zeros((2, 16), dtype=f32, device=dev())
    with pytest.raises(CfgppError, match="K=12"):
        H.skinny_ex(x, 12, torch.zeros((8, 12), dtype=f16, device=dev()), None, 2, out=out)
    with pytest.raises(CfgppError, match="M=0"):
        H.skinny_ex(x, 8, torch.zeros((8, 8), dtype=f16, device=dev()), None, 0, out=out[:0])
    with pytest.raises(CfgppError, match="ldx=10"):
        H.skinny_ex(x, 10, torch.zeros((8, 8), dtype=f16, device=dev()), None, 2, out=out)
    torch.cuda.synchronize()
    assert bool(untouched(out).all()) and guards_intact(buf)

    buf, seg = guarded((2, 32), f16)
    with pytest.raises(CfgppError, match="16-byte units"):
        H.fanout_rows([seg], 1, row_elems=[12])
    with pytest.raises(CfgppError, match="16-byte units"):
        H.fanout_rows([seg], 1, row_elems=[8], ptrs=[seg.data_ptr() + 8])
    with pytest.raises(CfgppError, match="fanout_rows"):
        H.fanout_rows([seg] * 4, 1)
    torch.cuda.synchronize()
    assert bool(untouched(seg).all()) and guards_intact(buf)
