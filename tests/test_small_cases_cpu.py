"""No GPU: what tests/small_cases.py claims, and what the conditions of tests/test_gpu_small.py can see.

D1  ids are unique; the tables hold every value the issue lists on every axis and reach every instance and branch the launchers of
    csrc/small_kernels.hip can emit (the launch rules restated in small_cases.expected_launch_* / *_branches / fo_paths).
D2  the fp32 models of correct kernels pass every condition on every case.  They read the device's layouts (halo-padded NHWC, packed
    weights), the references torch's conv2d on the NCHW map: a packing mistake of the tests shows here.
D3  a named table of fault models applied to those models: each is caught per element by at least one case; one of them, confined
    to where it would occur at a realistic size, passes the older whole-tensor rel-L2.
D4  the `exact` pre-conv inputs are exact: model and reference agree bitwise on the pre-conv.
D5  refusals that need no device memory return the error code with a message and leave the launch record at zero."""
import ctypes
import math

import numpy as np
import pytest

import small_cases as S


# ---- D1 -----------------------------------------------------------------------------------------------------------------------
def test_ids_are_unique():
    for g, cases in S.GROUPS.items():
        ids = [c.id for c in cases]
        assert len(set(ids)) == len(ids), g


def test_conv_in_table_reaches_every_branch():
    cs = S.CONV_IN
    assert {(c.H, c.W) for c in cs} == {(1, 1), (3, 1), (1, 5), (5, 7), (16, 12)}
    assert {c.Cout for c in cs} == {1, 24, 128, 320}
    assert {c.Cz for c in cs} == {1, 3, 4, 8} and {c.Cc for c in cs} == {0, 5, 8} and max(c.Cin for c in cs) == 16
    rz = {(c.R, c.zB, c.cond_rows, c.add_rows) for c in cs if c.Cc and c.add_rows}
    assert {(c.R, c.zB) for c in cs} == {(r[0], r[1]) for r in S._RZ} and rz & set(S._RZ)
    br = [S.ci_branches(c) for c in cs]
    for key in ("z_half", "tail", "blocks", "second_pass", "bias"):
        assert {bool(b[key]) for b in br} == {False, True}, key
    assert {(b["cond"], b["add"]) for b in br if b["entry"] == "add"} == {(False, False), (False, True), (True, False), (True, True)}
    assert {b["pre"] for b in br} == {0, 1, 2} and all(b["entry"] == "ex" for b in br if b["pre"])
    assert any(b["full_patch"] for b in br) and any(b["cond_and_add_rows_below_zB"] for b in br)
    assert any(b["tail"] and b["second_pass"] and b["blocks"] for b in br)
    assert {c.kind for c in cs} == {"rand", "exact", "real", "scaled"}
    assert all(c.Cin <= 16 and (not c.pre or (c.Cc == 0 and c.add_rows == 0)) for c in cs)


def test_conv_out_tables_reach_every_instance():
    wave, tiled = S.CONV_OUT_WAVE, S.CONV_OUT_TILED
    assert {c.C for c in wave} == {8, 24, 64, 128, 512}
    assert {(c.Cout, c.out_half) for c in wave} >= {(o, h) for o in (1, 2, 3, 4) for h in (0, 1)} | {(5, 0), (8, 0)}
    assert {c.R * c.H * c.W for c in wave} == {1, 9, 35, 240} and {c.post for c in wave} == {0, 1}
    assert {S.expected_launch_co(c)[:3] for c in wave} == {(0, 4, 1), (0, 4, 0), (0, 8, 0)}
    assert any(c.R * c.H * c.W % 4 for c in wave)                                        # pix >= total taken
    assert {(c.H, c.W) for c in tiled} == {(128, 128), (129, 161), (4, 4096), (2048, 8), (136, 152)}
    assert {c.C for c in tiled} == {64, 128} and {c.Cout for c in tiled} == {1, 2, 3, 4} and any(c.post for c in tiled)
    assert {S.expected_launch_co(c)[:3] for c in tiled} == {(1, 4, 1), (1, 3, 0), (1, 4, 0)}
    assert all(S.expected_launch_co(c, tiled=0)[0] == 0 for c in tiled)
    # every instance and kernel conv_out_ex can launch
    assert {S.expected_launch_co(c)[:3] for c in wave + tiled} == {(k, co, h) for (k, co, h) in ((0, 4, 1), (0, 4, 0), (0, 8, 0), (1, 4, 1), (1, 3, 0), (1, 4, 0))}
    # a 3-output call on a 4-wide instance, in both kernels
    assert any(c.Cout == 3 and S.expected_launch_co(c)[1] == 4 for c in wave) and any(c.Cout == 3 and S.expected_launch_co(c)[1] == 4 for c in tiled)


def test_clamp_cases_bind_at_both_ends():
    for c in [c for c in S.CONV_OUT_WAVE + S.CONV_OUT_TILED if c.post]:
        u = S.co_reference(c).unclamped
        if u.size >= 35:
            assert (u < 0).any() and (u > 1).any() and ((u > 0) & (u < 1)).any(), c.id


def test_sinusoid_skinny_rows_fanout_posterior_tables():
    sn = S.SINUSOID
    assert {c.dim for c in sn} == {2, 8, 256, 320} and {c.count for c in sn} == {1, 5, 6} and {c.scalar for c in sn} == {0, 1}
    assert {v for c in sn for v in c.vals} == set(S._SV)
    assert {(c.ld, c.out_off) for c in sn if c.out_ld} == {(2816, 1280), (2816, 2560)} and any(not c.out_ld for c in sn)
    sk = S.SKINNY
    assert {c.M for c in sk} == {1, 2, 4, 5, 8, 64} and {c.N for c in sk} == {1, 2, 7, 9, 64, 1280} and {c.K for c in sk} == {8, 64, 320, 512, 520, 2816}
    for a, b in (("M", "N"), ("M", "K"), ("N", "K")):                                      # pairwise, loosely: every value of one axis meets 2+ of the other
        for v in {getattr(c, a) for c in sk}:
            assert len({getattr(c, b) for c in sk if getattr(c, a) == v}) >= 2, (a, v)
    assert {c.ldx for c in sk} == {"K", "0", "K+8"} and {c.add for c in sk} == {"", "N", "N+4"} and {c.ldo for c in sk} == {0, 3}
    assert {(c.silu_in, c.silu_out) for c in sk} == {(0, 0), (0, 1), (1, 0), (1, 1)} and {c.bias for c in sk} == {0, 1}
    assert any(c.M == 1 and c.add for c in sk) and any(c.ldx == "0" and c.M > 1 for c in sk) and any(c.N % 2 for c in sk)
    assert {S.expected_launch_sk(c)[0] for c in sk} == {1, 4}
    assert all(np.abs(S.sk_inputs(c).x).max() == 20.0 for c in sk)
    assert {(c.rows, c.cols) for c in S.ROWS} >= {(1, 1), (3, 7), (2, 1280), (300, 1024)} and {S.rw_grid(c)[1] for c in S.ROWS} == {False, True}
    assert {(c.ld, c.out_off) for c in S.ROWS if c.out_ld} == {(2816, 1280), (2816, 2560)}
    fo = S.FANOUT
    assert {len(c.n16) for c in fo} == {1, 2, 3} and {c.h for c in fo} == {1, 2}
    assert {n for c in fo for n in c.units} >= {1, 255, 1024, 1025, 4095, 2048 * 1024 + 1} and (1, 5000, 300000) in {c.n16 for c in fo}
    assert {p for c in fo for p in S.fo_paths(c)[0]} == {(True, False), (False, True), (True, True)}
    assert {S.fo_paths(c)[1] for c in fo} == {False, True}
    assert S.fo_paths(S.FO((4095,)))[0] == [(True, True)] and S.fo_grid(S.FO((4095,))) * 256 * 4 - 1 == 4095
    capped = S.FO((2048 * 1024 + 1,))
    assert S.fo_grid(capped) == 2048 and capped.units[0] == 4 * 256 * 2048 + 1
    po = S.POSTERIOR
    assert {(c.B, c.HW) for c in po} == {(1, 1), (3, 35), (2, 256), (1, 300)} and {c.noise for c in po} == {0, 1} and {c.clamp for c in po} == {0, 1}
    assert {c.scale for c in po} == {0.18215, 0.13025}
    for c in (c for c in po if c.clamp):
        m = S.po_moments_ref(c).unclamped[:, 4:]
        assert (m > 20).any() and (m < -30).any()


# ---- D2 -----------------------------------------------------------------------------------------------------------------------
def _ci_ratio(c, got):
    return S.ratio(got, S.ci_reference(c).ref, *S.ci_bound(c, got))


def _co_ratio(c, got):
    return S.ratio(got, S.co_reference(c).ref, *S.co_bound(c, got))


def _sn_window(c, buf):
    return buf[:, c.out_off:c.out_off + c.dim]


def _sn_ratio(c, buf):
    outside = np.delete(buf, np.s_[c.out_off:c.out_off + c.dim], axis=1)
    if not np.isnan(outside).all():                                            # something stored outside [out_off, out_off + dim)
        return math.inf
    return S.ratio(_sn_window(c, buf), S.sn_ref64(c), *S.sn_bound(c))


def _sk_ratio(c, buf):
    r = S.sk_reference(c)
    if not np.isnan(buf[:, c.N:]).all():
        return math.inf
    return S.ratio(buf[:, :c.N], r.ref, r.rounding, r.rest)


def _po_ratios(c, z, m):
    r = S.po_moments_ref(c)
    zr, zround, zrest = S.po_z_ref(c, m)
    return S.ratio(m, r.ref, 0.5 * S.ulp16(np.nan_to_num(m)), r.rest), S.ratio(z, zr, zround, zrest)


def test_conv_in_model_passes_every_condition():
    worst = 0.0
    for c in S.CONV_IN:
        got = S.ci_model32(c)
        q = _ci_ratio(c, got)
        assert q <= 1.0, (c.id, q)
        assert S.rel_l2(got, S.ci_reference(c).ref) < S.REL_L2_BOUND, c.id
        worst = max(worst, q)
    print(f"conv_in: largest ratio of the fp32 model {worst:.3f}")


@pytest.mark.parametrize("c", S.CONV_OUT_WAVE + S.CONV_OUT_TILED, ids=lambda c: c.id)
def test_conv_out_model_passes_every_condition(c):
    kernel = S.expected_launch_co(c)[0]
    got = S.co_model32(c, kernel)
    q = _co_ratio(c, got)
    assert q <= 1.0, (c.id, q)
    assert S.rel_l2(got, S.co_reference(c).ref) < S.REL_L2_BOUND
    if kernel == 1 and c.H * c.W == 16384 and c.R == 1:                          # the wave kernel on a map of the tiled kernel, once
        assert _co_ratio(c, S.co_model32(c, 0)) <= 1.0


def test_sinusoid_skinny_posterior_models_pass_every_condition():
    for c in S.SINUSOID:
        assert _sn_ratio(c, S.sn_model32(c)) <= 1.0, c.id
        assert S.rel_l2(_sn_window(c, S.sn_model32(c)), S.sn_ref64(c)) < S.REL_L2_BOUND
    for c in S.SKINNY:
        buf = S.sk_model32(c)
        assert _sk_ratio(c, buf) <= 1.0, (c.id, _sk_ratio(c, buf))
        assert S.rel_l2(buf[:, :c.N], S.sk_reference(c).ref) < S.REL_L2_BOUND
    for c in S.POSTERIOR:
        qm, qz = _po_ratios(c, *S.po_model32(c))
        assert qm <= 1.0 and qz <= 1.0, (c.id, qm, qz)


def test_fanout_model_copies_every_unit_once():
    for c in S.FANOUT:
        T = 256 * S.fo_grid(c)
        for n in c.units:
            copied, unrolled = S.fo_copied(n, T)
            assert copied.all()
            # the closed form against the kernel's two loops, thread by thread, on the small segments
            if n <= 5000:
                seen = np.zeros(n, dtype=int)
                for i0 in range(min(T, n)):
                    i = i0
                    while i + 3 * T < n:
                        seen[[i, i + T, i + 2 * T, i + 3 * T]] += 1
                        assert unrolled[[i, i + T, i + 2 * T, i + 3 * T]].all()
                        i += 4 * T
                    while i < n:
                        seen[i] += 1
                        assert not unrolled[i]
                        i += T
                assert (seen == 1).all(), (c.id, n)


# ---- D3 -----------------------------------------------------------------------------------------------------------------------
def _case(table, **kw):
    for c in table:
        if all(getattr(c, k) == v for k, v in kw.items()):
            return c
    raise KeyError(kw)


def _ci_fault(c, fault):
    return _ci_ratio(c, S.ci_model32(c)), _ci_ratio(c, S.ci_model32(c, fault))


def _co_fault(c, fault):
    k = S.expected_launch_co(c)[0]
    return _co_ratio(c, S.co_model32(c, k)), _co_ratio(c, S.co_model32(c, k, fault))


def _sn_fault(c, fault):
    return _sn_ratio(c, S.sn_model32(c)), _sn_ratio(c, S.sn_model32(c, fault))


def _sk_fault(c, fault):
    return _sk_ratio(c, S.sk_model32(c)), _sk_ratio(c, S.sk_model32(c, fault))


def _po_fault(c, fault):
    return max(_po_ratios(c, *S.po_model32(c))), max(_po_ratios(c, *S.po_model32(c, fault)))


def _fo_fault(c, fault):
    T = 256 * S.fo_grid(c)
    return 0.0, (0.0 if all(S.fo_copied(n, T, fault)[0].all() for n in c.units) else math.inf)


# issue's name -> (how the fault is applied, the case that must catch it)
FAULTS = {
    "r // zB instead of r % zB": (_ci_fault, "row_div", _case(S.CONV_IN, R=4, zB=2, Cc=0)),
    "tail block of pixels not written": (_ci_fault, "tail", _case(S.CONV_IN, H=5, W=7, Cout=320)),
    "second Cout pass missing": (_ci_fault, "second_pass", _case(S.CONV_IN, H=5, W=7, Cout=320)),
    "cond channel offset off by one": (_ci_fault, "cond_off", _case(S.CONV_IN, H=1, W=5, Cc=5)),
    "one tap's dx mirrored": (_co_fault, "dx_mirrored", _case(S.CONV_OUT_WAVE, C=24, Cout=2)),
    "4th output read on a 3-output call": (_co_fault, "stride_co", _case(S.CONV_OUT_WAVE, C=128, Cout=3)),
    "last 64-channel block skipped": (_co_fault, "last_block", _case(S.CONV_OUT_TILED, C=128, Cout=3)),
    "tile's last row or column dropped": (_co_fault, "last_row", _case(S.CONV_OUT_TILED, H=129, C=64)),
    "sin and cos halves swapped": (_sn_fault, "swapped", _case(S.SINUSOID, dim=8, count=6)),
    "out_off ignored": (_sn_fault, "off_ignored", _case(S.SINUSOID, dim=256, out_off=1280, scalar=0)),
    "frequency with half-1 in place of half": (_sn_fault, "half_minus_one", _case(S.SINUSOID, dim=320, scalar=0, count=5)),
    "skinny: last K chunk dropped": (_sk_fault, "last_chunk", _case(S.SKINNY, K=520, M=5)),
    "skinny: ldx = 0 treated as K": (_sk_fault, "ldx0_as_K", _case(S.SKINNY, ldx="0", M=64)),
    "skinny: addend row 0 for every m": (_sk_fault, "add_row0", _case(S.SKINNY, M=8, add="N")),
    "skinny: silu_out before the addend": (_sk_fault, "silu_before_add", _case(S.SKINNY, M=5, add="N", silu_out=1)),
    "clamp missing": (_po_fault, "no_clamp", _case(S.POSTERIOR, clamp=1, HW=256)),
    "logvar not halved": (_po_fault, "logvar_not_halved", _case(S.POSTERIOR, HW=300, noise=1, clamp=0)),
    "fan-out tail missing": (_fo_fault, "tail", _case(S.FANOUT, n16=(4095,))),
}


def test_the_fault_table_is_the_issues():
    assert len(FAULTS) == 18


@pytest.mark.parametrize("name", list(FAULTS))
def test_faults_are_caught_per_element(name):
    apply, fault, c = FAULTS[name]
    good, bad = apply(c, fault)
    print(f"{name} on {c.id}: ratio of the correct model {good:.3f}, of the faulty one {bad:.3g}")
    assert good <= 1.0 < bad


def test_one_wrong_pixel_at_production_size_passes_rel_l2():
    """rel-L2 is |wrong part| / |whole|: on the few-pixel cases above every fault is a large share of the tensor.  The mirrored tap
    confined to ONE pixel - what a wrong halo or tile-edge index gives - inside the VAE decoder's 3 x 512 x 512 image of the same RMS
    moves rel-L2 by 7e-4: the old bound of 1.5e-3 (1e-2 for the VAE) passes it, the per-element bound does not care how large
    the tensor around the pixel is."""
    c = _case(S.CONV_OUT_WAVE, C=128, Cout=3)
    ref = S.co_reference(c).ref
    good, bad = S.co_model32(c, 0), S.co_model32(c, 0, "dx_mirrored")
    one = good.copy()
    one[1, :, 4, 5] = bad[1, :, 4, 5]
    assert _co_ratio(c, good) <= 1.0 < _co_ratio(c, one)
    rms = math.sqrt(float((ref ** 2).mean()))
    rel_big = float(np.linalg.norm((one - ref)[1, :, 4, 5])) / (rms * math.sqrt(3 * 512 * 512.0))
    print(f"tap 5 mirrored at one pixel: rel-L2 {rel_big:.3e} inside a 3 x 512 x 512 image, {S.rel_l2(one, ref):.3e} on the {c.id} case itself")
    assert rel_big < S.REL_L2_BOUND


# ---- D4 -----------------------------------------------------------------------------------------------------------------------
def test_exact_pre_conv_inputs_are_exact():
    for c in (c for c in S.CONV_IN if c.kind == "exact"):
        i = S.ci_inputs(c)
        v = S.ci_scaled_z(c, i)
        assert np.array_equal(v, i.z * c.in_scale)                              # z * in_scale needs no rounding
        u64 = np.einsum("oj,bjhw->bohw", i.pre_w.astype(np.float64), v) + (i.pre_b.astype(np.float64)[None, :, None, None] if c.pre == 2 else 0.0)
        acc = np.broadcast_to((i.pre_b if c.pre == 2 else np.zeros(c.Cz, np.float32))[None, :, None, None], v.shape).astype(np.float32)
        for j in range(c.Cz):
            # with and without FMA contraction: the product rounded to fp32 first
            prod = (i.pre_w[None, :, j, None, None] * v[:, j:j + 1].astype(np.float32)).astype(np.float32)
            acc = (acc + prod).astype(np.float32)
        assert np.array_equal(acc.astype(np.float64), u64) and np.array_equal(S.h16(u64), u64), c.id


# ---- D5 -----------------------------------------------------------------------------------------------------------------------
def test_refusals_return_the_error_code_before_any_launch():
    """none of these calls may touch the device: the pointers are small integers no kernel could read"""
    from cfgpp_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    out4 = (ctypes.c_int * 4)()

    def refused(rc, word):
        msg = lib.cfgpp_last_error()
        assert rc != 0 and word in msg, (rc, msg)

    refused(lib.cfgpp_op_conv_in_add(p, 0, None, 0, 0, None, 0, p, p, p, 1, 1, 9, 4, 4, 8, None), b"conv_in")                 # Cz = 9
    refused(lib.cfgpp_op_conv_in_add(p, 0, p, 1, 9, None, 0, p, p, p, 1, 1, 8, 4, 4, 8, None), b"conv_in")                   # Cz + Cc = 17
    refused(lib.cfgpp_op_conv_in_add(p, 0, None, 0, 0, p, 0, p, p, p, 1, 1, 4, 4, 4, 8, None), b"add_rows")
    refused(lib.cfgpp_op_conv_in_add(None, 0, None, 0, 0, None, 0, p, p, p, 1, 1, 4, 4, 4, 8, None), b"conv_in")             # null z
    refused(lib.cfgpp_op_conv_in_ex(None, 0, p, p, p, 1, 1, 4, 4, 4, 8, None, None, 1.0, None), b"conv_in")
    for args, word in (((p, p, 0, p, p, 1, 4, 4, 64, 9), b"Cout=9"), ((p, p, 0, p, p, 1, 4, 4, 12, 4), b"C=12"), ((p, p, 1, p, p, 1, 4, 4, 64, 8), b"fp32 only")):
        refused(lib.cfgpp_op_conv_out_ex(*args, 1.0, 0.0, 0, None), word)
        lib.cfgpp_conv_out_last_launch(out4)
        assert tuple(out4) == (0, 0, 0, 0)
    refused(lib.cfgpp_op_sinusoid(None, 1.0, p, 1, 7, 7, 0, None), b"sinusoid")                                                # odd dim
    refused(lib.cfgpp_op_sinusoid(None, 1.0, p, 0, 8, 8, 0, None), b"sinusoid")                                                # count = 0
    refused(lib.cfgpp_op_skinny_gemm(p, 12, p, None, None, 0, p, 8, 1, 8, 12, 0, 0, None), b"K=12")
    refused(lib.cfgpp_op_skinny_gemm(p, 8, p, None, None, 0, p, 8, 0, 8, 8, 0, 0, None), b"M=0")
    refused(lib.cfgpp_op_skinny_gemm(p, 10, p, None, None, 0, p, 8, 2, 8, 8, 0, 0, None), b"ldx=10")
    refused(lib.cfgpp_op_f16_to_f32_rows(None, p, 1, 1, 1, 0, None), b"f16_to_f32_rows")
    refused(lib.cfgpp_op_f16_to_f32_rows(p, p, 0, 1, 1, 0, None), b"f16_to_f32_rows")
    refused(lib.cfgpp_op_f16_to_f32_rows(p, p, 2, 8, 12, 8, None), b"f16_to_f32_rows")
    ptr = lambda *v: (ctypes.c_void_p * len(v))(*v)                              # noqa: E731
    lng = lambda *v: (ctypes.c_long * len(v))(*v)                                # noqa: E731
    refused(lib.cfgpp_op_fanout_rows(ptr(4096), lng(12), 1, 1, None), b"16-byte units")
    refused(lib.cfgpp_op_fanout_rows(ptr(4096 + 8), lng(16), 1, 1, None), b"16-byte units")
    refused(lib.cfgpp_op_fanout_rows(ptr(4096, 4096, 4096, 4096), lng(8, 8, 8, 8), 4, 1, None), b"fanout_rows")
