"""The FreeU op (csrc/freeu_kernel.hip) through cfgpp_op_freeu on the GPU: every case of tests/freeu_cases.py against the fp64
reference, per element, to the bound derived there; NaN-filled guard rows around both tensors, the halo, the untouched half of the
hidden tensor and a tensor the call does not pass stay bit-identical; the dispatch is the expected one; two runs give the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import freeu_cases as FC

pytestmark = pytest.mark.gpu
ids = dict(ids=lambda c: c.id)
GUARD = 2           # batch rows of NaN in front of and behind each tensor


@pytest.fixture(scope="module")
def ops():
    import hip_ops as ops
    return ops


def _padded(interior, dev):
    """interior NHWC fp16 numpy [rows, H, W, C] -> (flat NaN-guarded buffer, view of the halo-padded tensor inside it)"""
    rows, H, W, Cc = interior.shape
    buf = torch.full((rows + 2 * GUARD, H + 2, W + 2, Cc), float("nan"), dtype=torch.float16, device=dev)
    t = buf[GUARD:GUARD + rows]
    t.zero_()
    t[:, 1:H + 1, 1:W + 1, :] = torch.from_numpy(interior).to(dev)
    return buf, t


def _run(ops, c, hid_t, skip_t):
    lib = ops.lib()
    rc = lib.cfgpp_op_freeu(hid_t.data_ptr() if c.half != "skip" else None, c.C_h, skip_t.data_ptr() if c.half != "hidden" else None, c.C_s,
                            c.rows, c.H, c.W, c.b, c.s, ops.stream())
    from cfgpp_amd import _lib
    assert rc == 0, _lib.last_error()
    out = (C.c_int * 5)()
    lib.cfgpp_freeu_last_launch(out)
    return list(out)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


@pytest.mark.parametrize("c", FC.CASES, **ids)
def test_op_against_fp64(c, ops):
    hidden, skip = FC.make_inputs(c)
    ref_h, ref_k = FC.reference(c, hidden, skip)
    hbuf, ht = _padded(hidden, ops.DEV)
    kbuf, kt = _padded(skip, ops.DEV)
    h0, k0 = _bits(hbuf), _bits(kbuf)
    launch = _run(ops, c, ht, kt)
    torch.cuda.synchronize()
    assert launch[:4] == FC.expected_launch(c), f"{c.id}: launched {launch}, expected {FC.expected_launch(c)}"
    h1, k1 = _bits(hbuf), _bits(kbuf)
    for name, a, b0 in (("hidden", h1, h0), ("skip", k1, k0)):
        assert torch.equal(a[:GUARD], b0[:GUARD]) and torch.equal(a[-GUARD:], b0[-GUARD:]), f"{c.id}: guard rows of {name} written"
    assert ops.halo_is_zero(ht) and ops.halo_is_zero(kt), f"{c.id}: halo written"
    got_h = ht[:, 1:-1, 1:-1, :].cpu().numpy()
    got_k = kt[:, 1:-1, 1:-1, :].cpu().numpy()
    if c.half == "skip" or c.b == 1.0:
        assert got_h.tobytes() == hidden.tobytes(), f"{c.id}: hidden changed"
    if c.half == "hidden" or c.s == 1.0:
        assert got_k.tobytes() == skip.tobytes(), f"{c.id}: skip changed"
    assert got_h[..., c.C_h // 2:].tobytes() == np.ascontiguousarray(hidden[..., c.C_h // 2:]).tobytes(), f"{c.id}: second half of hidden changed"
    rh, rk = FC.worst_ratio(c, got_h, got_k, hidden, skip, ref_h, ref_k)
    print(f"{c.id}: hidden {rh:.3f} x bound, skip {rk:.3f} x bound, launch {launch}")
    assert rh <= 1.0 and rk <= 1.0, f"{c.id}: hidden {rh:.3f} x, skip {rk:.3f} x the bound"
    if c.half != "skip":
        share = FC.hidden_mismatch_share(c, got_h, ref_h)
        assert share <= FC.MISMATCH_CAP, f"{c.id}: {share:.2e} of the scaled hidden elements are not the correctly rounded product"
    # a second run from the same inputs: the same bits
    hbuf2, ht2 = _padded(hidden, ops.DEV)
    kbuf2, kt2 = _padded(skip, ops.DEV)
    _run(ops, c, ht2, kt2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(hbuf2), h1) and torch.equal(_bits(kbuf2), k1), f"{c.id}: two runs differ"


def test_negative_zero_survives_unit_scales(ops):
    """s = 1, b = 1: the kernel runs and stores the input's bits, -0 included"""
    c = FC.Case(6, 10, 64, 64, 3, 1.0, 1.0, seed=11)
    hidden, skip = FC.make_inputs(c)
    hidden[0, 0, 0, 0] = np.float16(-0.0)
    skip[1, 2, 3, 4] = np.float16(-0.0)
    hbuf, ht = _padded(hidden, ops.DEV)
    kbuf, kt = _padded(skip, ops.DEV)
    launch = _run(ops, c, ht, kt)
    torch.cuda.synchronize()
    assert launch[0] == 1 and launch[2] > 0 and launch[3] > 0
    assert ht[:, 1:-1, 1:-1, :].cpu().numpy().tobytes() == hidden.tobytes()
    assert kt[:, 1:-1, 1:-1, :].cpu().numpy().tobytes() == skip.tobytes()


@pytest.mark.parametrize("r", FC.REFUSED, ids=lambda r: r["word"] + f"-{r['H']}x{r['W']}")
def test_refusals_name_the_reason(r, ops):
    from cfgpp_amd import _lib
    lib = ops.lib()
    t = torch.zeros((1, r["H"] + 2, r["W"] + 2, 128), dtype=torch.float16, device=ops.DEV)
    rc = lib.cfgpp_op_freeu(t.data_ptr(), r["C_h"], t.data_ptr(), r["C_s"], 1, r["H"], r["W"], r.get("b", 1.5), r.get("s", 0.2), ops.stream())
    assert rc != 0 and r["word"] in _lib.last_error(), _lib.last_error()
    out = (C.c_int * 5)()
    lib.cfgpp_freeu_last_launch(out)
    assert list(out) == [0, 0, 0, 0, 0]
    torch.cuda.synchronize()
    assert not bool(t.any())
    rc = lib.cfgpp_op_freeu(None, 64, None, 64, 1, 8, 8, 1.5, 0.2, ops.stream())
    assert rc != 0 and "both tensors are null" in _lib.last_error()
