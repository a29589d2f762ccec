"""-m gpu: cn_conv3x3_kernel and cn_residual_nchw_kernel of csrc/controlnet_kernels.hip, alone, against the fp64 references of
tests/cn_cases.py per element: every input layout, both strides on odd and non-square maps, SiLU and bias on and off, dense and
halo-padded destinations.  Harness of tests/test_gpu_vit_attention.py: the destination is NaN-filled between sentinel guard rows -
a padded destination's halo must still hold the NaN bits afterwards -, a second launch must be bit-identical, refusals raise by name
and leave the destination untouched.  tests/test_cn_cases_cpu.py shows which faults these conditions catch."""
import numpy as np
import pytest
import torch

import cn_cases as N
from test_gpu_attention import guarded, guards_intact
from test_gpu_configs import need_gpu, record
from test_gpu_tower_kernels import dev, guarded32, twice

pytestmark = pytest.mark.gpu

ids = dict(ids=lambda c: c.id)
NAN16 = 0x7e57                                   # the NaN payload of tests/test_gpu_small.py: not the NaN any arithmetic produces


@pytest.mark.parametrize("c", N.CONV, **ids)
def test_cn_conv3x3(c):
    need_gpu()
    import hip_ops as H
    r = N.cv_reference(c)
    i = r.inputs
    x = dev(i.dev, torch.float32 if c.in_kind == 2 else torch.float16)
    wk, bias = dev(i.wk, torch.float32), (dev(i.bias, torch.float32) if c.bias else None)
    _, Hd, Wd, Co = N.cv_dest_shape(c)
    bits = []

    def call(o):
        H.cn_conv3x3(x, c.in_kind, o, c.out_pad, wk, bias, c.R, c.Ci, c.Co, c.Hi, c.Wi, c.stride, c.silu)
        bits.append(o.view(torch.int16).cpu().view(c.R, Hd, Wd, Co))

    def make():
        buf, o = guarded(c.R, Hd * Wd, Co)
        o.view(torch.int16).fill_(NAN16)                          # a NaN with a payload of its own between the sentinel guard rows
        return buf, o, Co
    dest, problems = twice(make, call)
    dest = dest.reshape(c.R, Hd, Wd, Co)
    if c.out_pad:                                                 # the halo by bits: still the payload the buffer was filled with
        halo = torch.ones((c.R, Hd, Wd, Co), dtype=torch.bool)
        halo[:, 1:c.Ho + 1, 1:c.Wo + 1] = False
        if not bool((bits[0][halo] == NAN16).all()):
            problems.append("halo written")
    got = N.cv_interior(c, dest)
    q = N.cv_ratio(c, dest)
    record("cn_case", group="cn_conv3x3", case=c.id, silu=c.silu, ratio=q, problems=problems)
    print(f"cn_conv3x3 {c.id}: ratio {q:.3f} {problems}")
    assert not problems, (c.id, problems)
    assert np.isfinite(got).all(), f"{c.id}: {int((~np.isfinite(got)).sum())} elements of the write set not finite (unwritten or NaN)"
    assert q <= 1.0, f"{c.id}: (|got - ref64| - rounding) / rest = {q:.3f} > 1, {N.violations(got, r.ref, *N.cv_bound(c, got))} elements outside the bound"


@pytest.mark.parametrize("c", N.RESIDUAL_NCHW, **ids)
def test_residual_nchw(c):
    need_gpu()
    import hip_ops as H
    src = dev(N.rn_input(c), torch.float16)
    width = c.H * c.W
    got, problems = twice(lambda: guarded32(c.rows * c.C, width) + (width,), lambda o: H.residual_nchw(src, o, c.rows, c.H, c.W, c.C, c.scale))
    want = N.rn_model(c)
    got = got.reshape(want.shape)
    ok = bool(np.isfinite(got).all()) and np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
    record("cn_case", group="residual_nchw", case=c.id, exact=ok, problems=problems)
    assert not problems, (c.id, problems)
    assert ok, f"{c.id}: {int((got != want).sum())} elements differ from ((v.float() * scale).half()).float()"


@pytest.mark.parametrize("name,Ci,stride,in_kind,null,msg", [("Ci257", 257, 1, 0, "", "Ci=257"), ("stride3", 8, 3, 0, "", "stride 3"), ("in_kind3", 8, 1, 3, "", "in_kind 3"),
                                                            ("null_in", 8, 1, 0, "in", "bad args"), ("null_w", 8, 1, 0, "w", "bad args")])
def test_cn_conv3x3_refusals_launch_nothing(name, Ci, stride, in_kind, null, msg):
    need_gpu()
    import hip_ops as H
    from cfgpp_amd._lib import CfgppError
    x = torch.ones((1, 4, 4, 257), dtype=torch.float16, device=H.DEV)
    wk = torch.ones((9, 257, 8), dtype=torch.float32, device=H.DEV)
    buf, o = guarded(1, 16, 8)
    with pytest.raises(CfgppError, match="cn_conv3x3.*" + msg):
        H.cn_conv3x3(None if null == "in" else x, in_kind, o, 0, None if null == "w" else wk, None, 1, Ci, 8, 4, 4, stride, 1)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()) and guards_intact(buf, 8)


def test_residual_nchw_refusals_launch_nothing():
    need_gpu()
    import hip_ops as H
    from cfgpp_amd._lib import CfgppError
    src = torch.ones((1, 3, 3, 8), dtype=torch.float16, device=H.DEV)
    buf, o = guarded32(8, 1)
    for args in ((None, o, 1, 1, 1, 8, 1.0), (src, o, 0, 1, 1, 8, 1.0), (src, o, 1, 1, 1, 0, 1.0)):
        with pytest.raises(CfgppError, match="residual_nchw"):
            H.residual_nchw(*args)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()) and guards_intact(buf, 1)
