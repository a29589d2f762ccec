"""The identity behind the 2x2 phase form of the upsampler convolutions (IGemmArgs::amode 4), on the CPU in float64:
conv3x3(pad 1)(nearest-2x(x)) == four 2x2 convolutions over the source map with folded weights, borders included."""
import numpy as np
import pytest

from upsample_phase_ref import TAPS, fold, fold_packed_fp16, out_pixel, phase_conv, stat_slot, upsample_conv_ref

SHAPES = [(1, 1), (2, 3), (8, 8), (8, 12)]


def _case(Hs, Ws, n=2, C=3, O=2):
    rng = np.random.default_rng(100 * Hs + Ws)
    x = rng.standard_normal((n, C, Hs, Ws))
    # every tap weight distinct (and no two sums of taps equal by accident): a swapped or dropped tap changes the result
    w = (1.0 + np.arange(O * C * 9, dtype=np.float64).reshape(O, C, 3, 3) * 0.37) * rng.choice([-1.0, 1.0], size=(O, C, 3, 3))
    return x, w


@pytest.mark.parametrize("Hs,Ws", SHAPES)
def test_four_phase_convs_equal_the_upsampled_conv(Hs, Ws):
    x, w = _case(Hs, Ws)
    ref = upsample_conv_ref(x, w)
    got = phase_conv(x, fold(w))
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("Hs,Ws", SHAPES)
def test_a_wrong_tap_set_is_seen(Hs, Ws):
    """p = 1 with a = 0 <- {t = 0} (tap 1 dropped): off by orders of magnitude more than the 1e-12 of the right fold"""
    x, w = _case(Hs, Ws)
    wrong = dict(TAPS)
    wrong[(1, 0)] = (0,)
    ref = upsample_conv_ref(x, w)
    got = phase_conv(x, fold(w, taps=wrong))
    assert np.abs(got - ref).max() > 1e-3 * np.abs(ref).max()


def test_output_map_covers_every_pixel_once():
    for Hs, Ws in SHAPES:
        seen = np.zeros((2 * Hs + 2, 2 * Ws + 2), dtype=int)
        for phase in range(4):
            for i in range(Hs):
                for j in range(Ws):
                    r, c = out_pixel(phase, i, j)
                    seen[r, c] += 1
        assert (seen[1:-1, 1:-1] == 1).all() and seen[0].sum() == 0 and seen[-1].sum() == 0 and seen[:, 0].sum() == 0 and seen[:, -1].sum() == 0


@pytest.mark.parametrize("HsWs", [32, 64, 1024, 96])
def test_statistics_slots_are_a_bijection_per_sample(HsWs):
    bps, nb = HsWs // 32, 4 * HsWs // 32
    for n in range(3):
        slots = sorted(stat_slot(n, ph, blk, HsWs) for ph in range(4) for blk in range(bps))
        assert slots == list(range(n * nb, (n + 1) * nb))
    # the kernel's form: in-phase block index bi = n * bps + blk  ->  bi + (3 n + phase) * bps
    for n in range(3):
        for ph in range(4):
            for blk in range(bps):
                bi = n * bps + blk
                assert bi + (3 * (bi // bps) + ph) * bps == stat_slot(n, ph, blk, HsWs)


def test_packed_fold_matches_the_plain_fold():
    O, I = 4, 128
    rng = np.random.default_rng(7)
    w = rng.standard_normal((O, I, 3, 3)).astype(np.float16)
    packed = np.ascontiguousarray(w.transpose(0, 2, 3, 1).reshape(O, 9, I // 64, 64).transpose(0, 2, 1, 3)).reshape(O, 9 * I)
    got = fold_packed_fp16(packed, O, I).reshape(4, O, I // 64, 2, 2, 64)
    want = fold(w, dtype=np.float32).astype(np.float16)          # [4, O, I, 2, 2]
    for cb in range(I // 64):
        assert np.array_equal(got[:, :, cb].transpose(0, 1, 4, 2, 3), want[:, :, cb * 64:(cb + 1) * 64])
