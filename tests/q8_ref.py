"""numpy float32 reference of the row-wise int8 (Q8) table format (include/trs_abi.h): a row of E columns is
S = round_up(E + 8, 16) bytes -- E codes, fp32 scale, fp32 bias (little endian), zero padding."""
import numpy as np


def stride(E):
    return (E + 8 + 15) // 16 * 16


def _f32_bytes(v, V):
    return np.ascontiguousarray(np.asarray(v, dtype='<f4').reshape(V, 1)).view(np.uint8)


def pack(codes, scale, bias):
    """codes (V, E) in 0..255, scale / bias (V,) -> the (V, S) uint8 rows"""
    V, E = codes.shape
    q = np.zeros((V, stride(E)), np.uint8)
    q[:, :E] = codes
    q[:, E:E + 4] = _f32_bytes(scale, V)
    q[:, E + 4:E + 8] = _f32_bytes(bias, V)
    return q


def tails(q, E):
    """(scale, bias), each (V, 1) float32"""
    return tuple(np.ascontiguousarray(q[:, E + o:E + o + 4]).view('<f4') for o in (0, 4))


def dequant(q, E):
    """x[e] = float(c[e]) * scale + bias in float32, the product and the sum each rounded"""
    scale, bias = tails(q, E)
    return (q[:, :E].astype(np.float32) * scale).astype(np.float32) + bias


def quantize(x):
    """bias = min, scale = (max - bias) / 255, c = clamp(rint((x - bias) / scale), 0, 255), all float32; scale == 0: codes
    0; a min or max of -0 counts as +0"""
    x = np.asarray(x, np.float32)
    zero = np.float32(0)
    bias = x.min(1, keepdims=True) + zero
    scale = ((x.max(1, keepdims=True) + zero) - bias) / np.float32(255)
    with np.errstate(divide='ignore', invalid='ignore'):
        c = np.rint((x - bias) / scale)
    c = np.where(scale == 0, zero, np.clip(c, 0, 255))
    return pack(c.astype(np.uint8), scale, bias)


def recon_bound(x, scale):
    """|deq(quantize(x)) - x| <= (0.5 + 2^-15) * scale + 2^-23 * max|x_row|, per row (V, 1)"""
    return (0.5 + 2.0 ** -15) * scale.astype(np.float64) + 2.0 ** -23 * np.abs(x).max(1, keepdims=True).astype(np.float64)
