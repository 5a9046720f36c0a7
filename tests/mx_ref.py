"""The MXFP4 W4A4 contract of include/atom_hip.h restated in numpy (float64), on the plain layout.

One block of 32 values v: amax = max|v|; amax == 0 -> scale byte 127, codes 0; else e = clamp(floor(log2 amax) - emax, -127, 127)
(emax 2 for E2M1, 8 for E4M3), scale byte e + 127, code = |v| / 2^e rounded to the nearest grid value, ties to the even code, saturated
at the largest finite one (6 / 448); sign bit where v < 0.  Plain operand = (codes u8 [rows, (K-128)/2] low nibble first, scales u8
[rows, (K-128)/32], keeper codes u8 [rows, 128], keeper scales u8 [rows, 4]).  GEMM = the float64 product of the dequantised operands."""
import numpy as np

FMT = {"e2m1": (1, 1, 7, 2, 8), "e4m3": (3, 7, 0x7E, 8, 0x80)}      # mantissa bits, bias, largest finite code, emax, sign bit


def decode(codes, fmt):
    mb, bias, _, _, sign = FMT[fmt]
    c = np.asarray(codes).astype(np.int64)
    ex, man = (c & (sign - 1)) >> mb, c & ((1 << mb) - 1)
    mag = np.where(ex == 0, man * 2.0 ** (1 - bias - mb), (man + (1 << mb)) * 2.0 ** (ex - bias - mb))
    return np.where(c & sign, -mag, mag)


def quantise(v, fmt):
    """float [rows, 32 B] -> (codes u8 [rows, 32 B], scale bytes u8 [rows, B])"""
    _, _, maxc, emax, sign = FMT[fmt]
    grid = decode(np.arange(maxc + 1), fmt)
    b = np.asarray(v, dtype=np.float64).reshape(len(v), -1, 32)
    amax = np.abs(b).max(-1)
    e = np.where(amax > 0, np.clip(np.frexp(amax)[1] - 1 - emax, -127, 127), 0)
    y = np.abs(b) / 2.0 ** e[..., None]
    hi = np.clip(np.searchsorted(grid, y), 1, maxc)
    lo = hi - 1
    up = (grid[hi] - y < y - grid[lo]) | ((grid[hi] - y == y - grid[lo]) & (hi % 2 == 0))
    code = np.where(up, hi, lo) | np.where(b < 0, sign, 0)
    return code.reshape(len(v), -1).astype(np.uint8), (e + 127).astype(np.uint8)


def pack4(codes):
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)


def unpack4(packed):
    return np.stack([packed & 15, packed >> 4], axis=-1).reshape(len(packed), -1)


def quantise_plain(xr):
    """reordered fp16 [rows, K] -> the plain operand"""
    c4, s4 = quantise(xr[:, :-128], "e2m1")
    c8, s8 = quantise(xr[:, -128:], "e4m3")
    return pack4(c4), s4, c8, s8


def dequant(plain):
    codes, scales, k8, s8 = plain
    v4 = decode(unpack4(codes), "e2m1") * np.repeat(2.0 ** (scales.astype(np.float64) - 127), 32, axis=1)
    v8 = decode(k8, "e4m3") * np.repeat(2.0 ** (s8.astype(np.float64) - 127), 32, axis=1)
    return np.concatenate([v4, v8], axis=1)


def gemm_ref(a, w):
    return dequant(a).astype(np.float64) @ dequant(w).astype(np.float64).T


def block_abs_sum(a, w):
    """S[m][n] = the sum over the 32-channel blocks of |that block's contribution|"""
    da, dw = dequant(a), dequant(w)
    return sum(np.abs(da[:, k:k + 32] @ dw[:, k:k + 32].T) for k in range(0, da.shape[1], 32))
