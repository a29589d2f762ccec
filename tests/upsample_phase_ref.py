"""Python restatement of the 2x2 phase form of `nearest-2x upsample -> conv3x3` (IGemmArgs::amode 4, csrc/igemm.h): the weight
fold (csrc/lora_kernels.hip fold_upsample_kernel) and the row / output-pixel / statistics-slot maps (csrc/igemm_device.h).  Shared
by tests/test_upsample_phase_cpu.py and tests/test_gpu_upsample_phase.py."""
from __future__ import annotations

import numpy as np

# 1-D: output y = 2i + p, 2-tap index a reads source row i + p - 1 + a and carries these taps t (dy = t - 1) of the 3-tap kernel
TAPS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}


def fold(w: np.ndarray, taps=TAPS, dtype=np.float64) -> np.ndarray:
    """w [O, I, 3, 3] -> [4 phases = 2 py + px, O, I, 2, 2]: W'[py, px][a, b] = sum_{t in T(py, a)} sum_{s in T(px, b)} W[t, s],
    summed in `dtype` in the kernel's order (t ascending, then s ascending)"""
    O, I = w.shape[:2]
    out = np.zeros((4, O, I, 2, 2), dtype=dtype)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    acc = np.zeros((O, I), dtype=dtype)
                    for t in taps[(py, a)]:
                        for s in taps[(px, b)]:
                            acc = (acc + w[:, :, t, s].astype(dtype)).astype(dtype)
                    out[2 * py + px, :, :, a, b] = acc
    return out


def fold_packed_fp16(w9_packed: np.ndarray, O: int, I: int) -> np.ndarray:
    """the device fold on the repacked layout: w9 [O][I/64][9][64] fp16 -> w4 [4][O][I/64][4][64] fp16, fp32 sums rounded once"""
    w = w9_packed.reshape(O, I // 64, 3, 3, 64).transpose(0, 1, 4, 2, 3).reshape(O, I, 3, 3)          # -> [O, I, 3, 3]
    f = fold(w, dtype=np.float32).astype(np.float16)                                                  # [4, O, I, 2, 2]
    return np.ascontiguousarray(f.reshape(4, O, I // 64, 64, 4).transpose(0, 1, 2, 4, 3)).reshape(4, O, 4 * I)


def upsample_conv_ref(x: np.ndarray, w: np.ndarray) -> np.ndarray:
    """x [n, C, Hs, Ws], w [O, C, 3, 3] -> conv3x3(pad 1)(nearest-2x(x)) in float64, [n, O, 2Hs, 2Ws]"""
    n, C, Hs, Ws = x.shape
    up = np.repeat(np.repeat(x.astype(np.float64), 2, axis=2), 2, axis=3)
    upp = np.pad(up, ((0, 0), (0, 0), (1, 1), (1, 1)))
    out = np.zeros((n, w.shape[0], 2 * Hs, 2 * Ws))
    for t in range(3):
        for s in range(3):
            out += np.einsum("oc,nchw->nohw", w[:, :, t, s].astype(np.float64), upp[:, :, t:t + 2 * Hs, s:s + 2 * Ws])
    return out


def src_pixel(phase: int, i: int, j: int, a: int, b: int):
    """padded source pixel (row, column) that tap (a, b) of row (phase, n, i, j) reads (+1 halo offset included)"""
    return i + (phase >> 1) + a, j + (phase & 1) + b


def out_pixel(phase: int, i: int, j: int):
    """padded output pixel (row, column) of row (phase, n, i, j)"""
    return 2 * i + (phase >> 1) + 1, 2 * j + (phase & 1) + 1


def phase_conv(x: np.ndarray, wf: np.ndarray, absolute: bool = False) -> np.ndarray:
    """the four 2x2 convs through the row / pixel maps above: x [n, C, Hs, Ws], wf [4, O, C, 2, 2] -> [n, O, 2Hs, 2Ws] (float64).
    absolute: sum |x| |w'| instead (the S of the error bound)"""
    n, C, Hs, Ws = x.shape
    xs = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)))
    wf = wf.astype(np.float64)
    if absolute:
        xs, wf = np.abs(xs), np.abs(wf)
    outp = np.zeros((n, wf.shape[1], 2 * Hs + 2, 2 * Ws + 2))
    ii, jj = np.arange(Hs), np.arange(Ws)
    for phase in range(4):
        acc = np.zeros((n, wf.shape[1], Hs, Ws))
        for a in range(2):
            for b in range(2):
                r0, c0 = src_pixel(phase, 0, 0, a, b)
                acc += np.einsum("oc,nchw->nohw", wf[phase, :, :, a, b], xs[:, :, r0:r0 + Hs, c0:c0 + Ws])
        ro, co = out_pixel(phase, ii, jj)
        outp[:, :, ro[:, None], co[None, :]] = acc
    return outp[:, :, 1:-1, 1:-1]


def stat_slot(n: int, phase: int, block: int, HsWs: int) -> int:
    """slot of the {mean, M2} pairs of 32-row block `block` of (sample n, phase): a sample owns nb = 4 * HsWs / 32 slots"""
    bps = HsWs // 32
    return n * 4 * bps + phase * bps + block
