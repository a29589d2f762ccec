"""The 2x2 phase form of `nearest-2x upsample -> conv3x3` (IGemmArgs::amode 4) through the single-op entry points: the fold kernel
and cfgpp_op_upsample_conv3x3, which dispatches as the engines' plan builder does.

Bound, per output element, against an fp64 evaluation of the ORIGINAL op (upsample, then the 3x3 conv with the unfolded fp16
weights):  0.5 ulp16 + (2^-11 + K 2^-23) S,  S = sum_k |x_k| |w'_k| in fp64 over the issued K = 4 C products - one rounding of
each folded weight (2^-11 relative), fp32 accumulation over K terms, one rounding of the result to fp16.  ulp16 is taken at the
stored fp16 value (the binade the final rounding happened in).  Derived, not measured; no extra factor.  The 9-tap fallback gets
the same formula without the 2^-11 S term, with S over its own 9 C products."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import hip_ops as H  # noqa: E402
from upsample_phase_ref import fold, fold_packed_fp16, phase_conv, upsample_conv_ref  # noqa: E402


def _ulp16(v: np.ndarray) -> np.ndarray:
    a = np.abs(v.astype(np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)


class Case:
    """inputs, device buffers and fp64 references of one shape, built once"""

    def __init__(self, Hs, Ws, rows, C, N, seed):
        g = torch.Generator().manual_seed(seed)
        self.Hs, self.Ws, self.rows, self.C, self.N = Hs, Ws, rows, C, N
        self.x = torch.randn((rows, C, Hs, Ws), generator=g).half()
        self.w = (torch.randn((N, C, 3, 3), generator=g) * (9 * C) ** -0.5).half()
        self.xp = H.to_pn(self.x)
        self.w9 = H.pack_conv3(self.w)
        self.w4 = torch.full((4, N, 4 * C), float("nan"), dtype=torch.float16, device=H.DEV)
        H.check(H.lib().cfgpp_op_fold_upsample(H.P(self.w9), H.P(self.w4), N, C, H.stream()), "cfgpp_op_fold_upsample")
        xd, wd = self.x.double(), self.w.double()
        self.ref = F.conv2d(F.interpolate(xd, scale_factor=2, mode="nearest"), wd, padding=1).numpy()
        wf16 = fold(self.w.numpy(), dtype=np.float32).astype(np.float16)
        self.S4 = phase_conv(self.x.numpy(), wf16, absolute=True)
        self.S9 = upsample_conv_ref(np.abs(self.x.numpy()), np.abs(self.w.numpy()))

    def run(self, gstat=None):
        """-> (interior [rows, N, 2Hs, 2Ws] float64, raw padded buffer)"""
        out = torch.full((self.rows, 2 * self.Hs + 2, 2 * self.Ws + 2, self.N), float("nan"), dtype=torch.float16, device=H.DEV)
        lib = H.lib()
        if gstat is not None:
            lib.cfgpp_op_igemm_set_gstat(H.P(gstat))
        try:
            H.check(lib.cfgpp_op_upsample_conv3x3(H.P(self.xp), self.C, self.Hs, self.Ws, H.P(self.w9), H.P(self.w4), self.rows, self.N,
                                                  None, H.P(out), H.stream()), "cfgpp_op_upsample_conv3x3")
        finally:
            if gstat is not None:
                lib.cfgpp_op_igemm_set_gstat(None)
        torch.cuda.synchronize()
        return out[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).double().cpu().numpy(), out

    def check(self, got, amode):
        K = (4 if amode == 4 else 9) * self.C
        S = self.S4 if amode == 4 else self.S9
        bound = 0.5 * _ulp16(got) + ((2.0 ** -11 if amode == 4 else 0.0) + K * 2.0 ** -23) * S
        err = np.abs(got - self.ref)
        worst = float((err / bound).max())
        print(f"source {self.Hs}x{self.Ws} rows {self.rows} {self.C}->{self.N} amode {amode}: max err {err.max():.3e}, worst err / bound {worst:.3f}")
        assert np.isfinite(got).all()
        assert worst <= 1.0, worst


def _halo_untouched(buf):
    return bool(torch.isnan(buf[:, 0]).all() and torch.isnan(buf[:, -1]).all() and torch.isnan(buf[:, :, 0]).all() and torch.isnan(buf[:, :, -1]).all())


_CASES = {}


def _case(*key):
    if key not in _CASES:
        _CASES[key] = Case(*key)
    return _CASES[key]


@pytest.mark.parametrize("Hs,Ws,rows,C,N", [
    (8, 8, 2, 64, 64),          # M per phase = 128 < BM: the per-phase tail
    (16, 16, 1, 64, 64),        # exactly one 256-row tile per phase
    (8, 12, 3, 128, 320),       # W not a power of two, N no multiple of 256, two 64-channel K chunks, several samples per tile
])
def test_phase_form_against_fp64(Hs, Ws, rows, C, N):
    c = _case(Hs, Ws, rows, C, N, 1)
    got, buf = c.run()
    assert H.lib().cfgpp_igemm_last_amode() == 4
    assert _halo_untouched(buf)
    c.check(got, 4)
    got2, buf2 = c.run()
    assert torch.equal(buf.view(torch.int16), buf2.view(torch.int16))          # a second launch: the same bits, halo NaNs included


def test_phase_form_writes_producer_statistics():
    """source 32 x 32, 2 rows, 64 -> 128: GroupNorm from the statistics the phase launch wrote (slot n * nb + phase * HsWs / 32 + block)
    equals GroupNorm recomputed from the stored output, to the bound test_groupnorm_from_producer_statistics uses (rel-L2 6e-4)"""
    c = _case(32, 32, 2, 64, 128, 2)
    gst = torch.full((2 * 64 * 64 // 32, 128, 2), float("nan"), dtype=torch.float32, device=H.DEV)
    got, buf = c.run(gstat=gst)
    assert H.lib().cfgpp_igemm_last_amode() == 4
    assert int(H.lib().cfgpp_op_igemm_gstat_written()) == 1
    assert _halo_untouched(buf)
    c.check(got, 4)
    assert bool(torch.isfinite(gst).all())                                    # every slot of every sample filled
    y = torch.nan_to_num(buf, nan=0.0)                                        # zero halo, as the engines' activation buffers have
    g = torch.Generator().manual_seed(5)
    gamma, beta = 1 + 0.1 * torch.randn(128, generator=g), 0.1 * torch.randn(128, generator=g)
    ref = F.silu(F.group_norm(H.from_pn(y), 32, gamma, beta, 1e-5))
    out = H.groupnorm_pre(y, None, gst, None, gamma.to(H.DEV), beta.to(H.DEV), 32, 1e-5, 1)
    st = H.err_stats(H.from_pn(out), ref)
    print("groupnorm from the phase launch's statistics:", st)
    assert st["finite"] and st["rel_l2"] < 6e-4, st
    # and the pairs against their definition: the 32 pixels of (sample n, phase, block) in (i, j) order
    yi = torch.from_numpy(got)                                               # [n, N, 64, 64]
    for n, phase, blk in ((0, 0, 0), (1, 3, 31), (1, 2, 7)):
        py, px = phase >> 1, phase & 1
        rows32 = yi[n, :, py::2, px::2].reshape(128, -1)[:, blk * 32:(blk + 1) * 32]
        pair = gst[n * 128 + phase * 32 + blk].double().cpu()
        assert float((pair[:, 0] - rows32.mean(1)).abs().max()) < 2e-5
        m2 = ((rows32 - rows32.mean(1, keepdim=True)) ** 2).sum(1)
        assert float(((pair[:, 1] - m2).abs() / (m2 + 1e-6)).max()) < 1e-3


# every tile config that carries the phase form; 18 / 19 (16x16x32 MFMA) sum k in another order: right, but not the same bits
_SAME_BITS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 21, 22, 23)


def test_every_supporting_config_and_one_that_does_not():
    c = _case(8, 12, 3, 128, 320, 1)
    lib = H.lib()
    base, _ = c.run()
    try:
        for cfg in _SAME_BITS + (18, 19):
            lib.cfgpp_igemm_force_config(cfg)
            got, buf = c.run()
            assert lib.cfgpp_igemm_last_amode() == 4 and lib.cfgpp_igemm_last_config_ran() == 1, cfg
            assert _halo_untouched(buf), cfg
            if cfg in _SAME_BITS:
                assert np.array_equal(got, base), cfg
            else:
                c.check(got, 4)
        for cfg in (24, 20):                                                  # one wave per SIMD / 64 x 160 waves on 32-deep K-tiles: no phase form
            lib.cfgpp_igemm_force_config(cfg)
            got, buf = c.run()
            assert lib.cfgpp_igemm_last_amode() == 4 and lib.cfgpp_igemm_last_config_ran() == 0, cfg
            assert _halo_untouched(buf) and np.array_equal(got, base), cfg   # (another tile ran it)
    finally:
        lib.cfgpp_igemm_force_config(0)


def test_small_maps_keep_the_nine_tap_form():
    c = _case(6, 6, 2, 64, 64, 3)
    got, buf = c.run()
    assert H.lib().cfgpp_igemm_last_amode() == 3
    assert _halo_untouched(buf)
    c.check(got, 3)


def test_switch_off_keeps_the_nine_tap_form():
    c = _case(8, 8, 2, 64, 64, 1)
    lib = H.lib()
    lib.cfgpp_igemm_set_upsample_phase(0)
    try:
        got, buf = c.run()
        assert lib.cfgpp_igemm_last_amode() == 3
    finally:
        lib.cfgpp_igemm_set_upsample_phase(1)
    c.check(got, 3)


def test_fold_kernel_bit_equal_to_its_restatement():
    c = _case(8, 12, 3, 128, 320, 1)
    want = fold_packed_fp16(c.w9.cpu().numpy(), c.N, c.C)
    got = c.w4.cpu().numpy()
    assert np.array_equal(got.view(np.int16), want.view(np.int16))
