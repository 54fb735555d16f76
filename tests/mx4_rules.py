"""MXFP4 TABLES (include/param_amd.h) restated in numpy float64, where every step of the rule is exact: the stored value of a row's
columns, and the quantiser.  Host only."""
import numpy as np

BLOCK = 32
MAGNITUDES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
VALUES = np.concatenate([MAGNITUDES, -MAGNITUDES])      # by code; code 8 is -0.0


def row_bytes(dim):
    return (dim // 2 + dim // BLOCK + 7) // 8 * 8


def dequant(table, dim):
    """fp32 ``[rows, dim]`` of a uint8 table ``[rows, row_bytes(dim)]``: ``e2m1(code) * 2^(x - 127)``, NaN where the block's x is 255"""
    tab = np.asarray(table, dtype=np.uint8)
    codes = np.stack([tab[:, :dim // 2] & 15, tab[:, :dim // 2] >> 4], axis=2).reshape(tab.shape[0], dim)
    x = np.repeat(tab[:, dim // 2:dim // 2 + dim // BLOCK].astype(np.int64), BLOCK, axis=1)
    v = VALUES[codes] * 2.0 ** (x - 127).astype(np.float64)
    return np.where(x == 255, np.nan, v).astype(np.float32)


def quantize(src):
    """uint8 ``[rows, row_bytes(dim)]`` of a ``[rows, dim]`` array of fp32-representable values; a NaN block's code bytes are zero"""
    x64 = np.asarray(src, dtype=np.float32).astype(np.float64)
    n, dim = x64.shape
    blocks = x64.reshape(n, dim // BLOCK, BLOCK)
    bad = ~np.isfinite(blocks).all(axis=2)
    amax = np.abs(np.where(np.isfinite(blocks), blocks, 0.0)).max(axis=2)
    q = np.frexp(amax)[1].astype(np.int64) - 1                      # floor(log2 amax); amax == 0 gives -1, below the clamp or not: fixed next
    x = np.where(amax == 0, 2, np.clip(q - 2 + 127, 2, 252))
    y = np.abs(blocks) * 2.0 ** (127 - x)[:, :, None].astype(np.float64)
    dist = np.abs(y[..., None] - MAGNITUDES)
    near = dist == dist.min(axis=-1, keepdims=True)                 # one magnitude, or the two neighbours of a midpoint
    even = near & (np.arange(8) % 2 == 0)
    code = np.where(even.any(axis=-1), even.argmax(axis=-1), near.argmax(axis=-1)) | (np.signbit(blocks) << 3)
    code = np.where(bad[:, :, None], 0, code).reshape(n, dim).astype(np.uint8)
    out = np.zeros((n, row_bytes(dim)), dtype=np.uint8)
    out[:, :dim // 2] = code[:, 0::2] | (code[:, 1::2] << 4)
    out[:, dim // 2:dim // 2 + dim // BLOCK] = np.where(bad, 255, x)
    return out
