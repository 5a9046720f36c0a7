"""The MXFP6 activation of include/atom_hip.h ("MXFP6 activations, W4A6") in numpy (float64) on the plain layout: tests/mx_ref.py with an
E2M3 row in the format table, and the 6-bit packing (a block's 32 codes = one 192-bit little-endian string)."""
import numpy as np

from tests import mx_ref as R

R.FMT.setdefault("e2m3", (3, 1, 31, 2, 0x20))                # mantissa bits, bias, largest finite code, emax, sign bit


def pack6(codes):
    bits = np.unpackbits(np.asarray(codes, dtype=np.uint8)[..., None], axis=-1, bitorder="little")[..., :6]
    return np.packbits(bits.reshape(len(codes), -1), axis=-1, bitorder="little")


def unpack6(packed):
    bits = np.unpackbits(np.asarray(packed, dtype=np.uint8), axis=-1, bitorder="little").reshape(len(packed), -1, 6)
    return np.packbits(np.pad(bits, ((0, 0), (0, 0), (0, 2))), axis=-1, bitorder="little")[..., 0]


def quantise_plain(xr):
    """reordered values [rows, K] -> the plain MXFP6 operand"""
    c6, s6 = R.quantise(xr[:, :-128], "e2m3")
    c8, s8 = R.quantise(xr[:, -128:], "e4m3")
    return pack6(c6), s6, c8, s8


def dequant(plain):
    codes, scales, k8, s8 = plain
    v6 = R.decode(unpack6(codes), "e2m3") * np.repeat(2.0 ** (scales.astype(np.float64) - 127), 32, axis=1)
    v8 = R.decode(k8, "e4m3") * np.repeat(2.0 ** (s8.astype(np.float64) - 127), 32, axis=1)
    return np.concatenate([v6, v8], axis=1)
