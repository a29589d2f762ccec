"""No GPU: what tests/cn_cases.py claims, and what the conditions of tests/test_gpu_cn_kernels.py can see.

D1  the table holds every value the issue lists on every axis and the combinations the older chain test never ran.
D2  the fp32 model of a correct kernel passes its bound on every case, halo untouched.
D3  every fault model fails on at least one case; the test names the cases.
D4  refusals return the error code with the launcher's name before anything could be launched."""
import ctypes

import numpy as np

import cn_cases as N


def test_table_reaches_every_branch():
    cs = N.CONV
    assert len({c.id for c in cs}) == len(cs)
    assert {(c.Hi, c.Wi) for c in cs} == set(N.SIZES) and {(c.Ci, c.Co) for c in cs} == set(N.CHANNELS) | {(256, 256)}
    assert {(c.Hi, c.Wi) for c in cs if c.Ci == 256} == {(5, 7)}
    assert {(c.Hi, c.Wi, c.Ci, c.Co) for c in cs} >= {(h, w, ci, co) for h, w in N.SIZES for ci, co in N.CHANNELS}
    for a, vals in (("in_kind", {0, 1, 2}), ("stride", {1, 2}), ("silu", {0, 1}), ("bias", {0, 1}), ("out_pad", {0, 1}), ("R", {1, 3})):
        assert {getattr(c, a) for c in cs} == vals, a
    for a, b in (("in_kind", "stride"), ("in_kind", "silu"), ("in_kind", "out_pad"), ("in_kind", "bias"), ("stride", "silu"), ("stride", "out_pad"),
                 ("silu", "bias"), ("silu", "out_pad"), ("bias", "out_pad"), ("stride", "R"), ("in_kind", "R")):
        have = {(getattr(c, a), getattr(c, b)) for c in cs}
        assert len(have) == len({getattr(c, a) for c in cs}) * len({getattr(c, b) for c in cs}), (a, b, have)
    # what the 7-layer chain never ran: in_kind 1; no SiLU; no bias; a dense last layer; stride 2 on odd and non-square maps
    assert any(c.in_kind == 1 and not c.silu and not c.bias and not c.out_pad for c in cs)
    for hw in ((1, 1), (1, 6), (5, 7), (9, 4)):
        assert any((c.Hi, c.Wi) == hw and c.stride == 2 for c in cs), hw
    for kind in (0, 1, 2):
        assert any(c.in_kind == kind and N.cv_branches(c)["odd_stride2"] and N.cv_branches(c)["non_square"] for c in cs), kind
    br = [N.cv_branches(c) for c in cs]
    assert {b["blocks"] for b in br} == {False, True} and {b["tail"] for b in br} == {False, True}
    assert {(c.Ho, c.Wo) for c in cs if (c.Hi, c.Wi, c.stride) == (9, 4, 2)} == {(5, 2)} and {(c.Ho, c.Wo) for c in cs if (c.Hi, c.Wi, c.stride) == (5, 7, 2)} == {(3, 4)}
    rn = N.RESIDUAL_NCHW
    assert {(c.rows, c.H, c.W, c.C) for c in rn} == {(3, 5, 7, 64), (1, 1, 1, 8)} and {c.scale for c in rn} == {1.0, 0.7}


def test_inputs_are_what_the_docstring_says():
    for c in N.CONV:
        i = N.cv_inputs(c)
        assert i.dev.dtype == (np.float32 if c.in_kind == 2 else np.float16)
        assert i.dev.shape == ((c.R, c.Hi, c.Wi, c.Ci) if c.in_kind == 0 else (c.R, c.Ci, c.Hi, c.Wi))
        if c.in_kind == 2 and i.x.size >= 16:
            assert (i.x != i.x16).any()                                      # the kernel's own rounding is exercised
        assert not np.allclose(i.w, i.w.transpose(0, 1, 3, 2)) or c.Ci * c.Co == 1
        assert (i.bias is None) == (not c.bias)


def test_model_passes_and_every_fault_is_seen():
    seen = {f: [] for f in N.CONV_FAULTS}
    worst = 0.0
    for c in N.CONV:
        q = N.cv_ratio(c, N.cv_model32(c))
        worst = max(worst, q)
        assert q <= 1.0, (c.id, q)
        for f in N.CONV_FAULTS:
            if N.cv_ratio(c, N.cv_model32(c, f)) > 1.0:
                seen[f].append(c.id)
    print(f"model ratio, max over cases: {worst:.3f}")
    print("conv faults seen by:", seen)
    assert all(seen.values()), {f: v for f, v in seen.items() if not v}
    by_id = {c.id: c for c in N.CONV}
    assert all(by_id[i].stride == 2 for i in seen["ho_floor"]) and all(by_id[i].in_kind != 0 for i in seen["plane_hi_hi"])
    assert all(by_id[i].out_pad for i in seen["no_halo_offset"]) and all(by_id[i].bias for i in seen["bias_co_minus_1"])
    # every case a fault can touch sees it
    assert set(seen["ho_floor"]) == {c.id for c in N.CONV if c.stride == 2 and (c.Hi % 2 or c.Wi % 2)}
    assert set(seen["plane_hi_hi"]) == {c.id for c in N.CONV if c.in_kind != 0 and c.Hi != c.Wi and c.R * c.Ci > 1}
    assert set(seen["no_halo_offset"]) == {c.id for c in N.CONV if c.out_pad}
    assert set(seen["bias_co_minus_1"]) == {c.id for c in N.CONV if c.bias and c.Co > 1}
    assert set(seen["pad0"]) == {c.id for c in N.CONV} and set(seen["kykx_swapped"]) >= {c.id for c in N.CONV if min(c.Hi, c.Wi) > 1}


def test_residual_nchw_model_and_faults():
    for c in N.RESIDUAL_NCHW:
        want = N.rn_model(c)
        assert want.shape == (c.rows, c.C, c.H, c.W) and np.isfinite(want).all()
        assert not np.isfinite(N.rn_model(c, "no_halo_offset")).all()
        if c.H * c.W > 1:
            assert not np.array_equal(N.rn_model(c, "nhwc_order"), want)
    a, b = (N.rn_model(c) for c in N.RESIDUAL_NCHW[:2])
    assert not np.array_equal(a, b)


def test_refusals_return_the_error_code_before_any_launch():
    """none of these calls may touch the device: the pointers are small integers no kernel could read"""
    from cfgpp_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)

    def refused(rc, word):
        msg = lib.cfgpp_last_error()
        assert rc != 0 and word in msg, (rc, msg)

    conv = {"Ci257": (p, 0, p, 0, p, p, 1, 257, 8, 4, 4, 1, 1), "Co0": (p, 0, p, 0, p, p, 1, 8, 0, 4, 4, 1, 1), "stride3": (p, 0, p, 0, p, p, 1, 8, 8, 4, 4, 3, 1),
            "in_kind3": (p, 3, p, 0, p, p, 1, 8, 8, 4, 4, 1, 1), "null_in": (None, 0, p, 0, p, p, 1, 8, 8, 4, 4, 1, 1),
            "null_out": (p, 0, None, 0, p, p, 1, 8, 8, 4, 4, 1, 1), "null_w": (p, 0, p, 0, None, p, 1, 8, 8, 4, 4, 1, 1), "R0": (p, 0, p, 0, p, p, 0, 8, 8, 4, 4, 1, 1)}
    assert set(conv) == set(N.CONV_REFUSED)
    for name, args in conv.items():
        refused(lib.cfgpp_op_cn_conv3x3(*args, None), b"cn_conv3x3")
    assert b"Ci=257" in (lib.cfgpp_op_cn_conv3x3(*conv["Ci257"], None), lib.cfgpp_last_error())[1]
    assert b"stride 3" in (lib.cfgpp_op_cn_conv3x3(*conv["stride3"], None), lib.cfgpp_last_error())[1]
    rn = {"rows0": (p, p, 0, 4, 4, 8, 1.0), "C0": (p, p, 1, 4, 4, 0, 1.0), "null_src": (None, p, 1, 4, 4, 8, 1.0), "null_out": (p, None, 1, 4, 4, 8, 1.0)}
    assert set(rn) == set(N.RESIDUAL_NCHW_REFUSED)
    for name, args in rn.items():
        refused(lib.cfgpp_op_residual_nchw(*args, None), b"residual_nchw")
