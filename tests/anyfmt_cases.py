"""Tables and requests the mixed-format tests share (tests/test_anyfmt_host.py, tests/test_gpu_anyfmt.py): seeded tables of every format
as the BYTES the module stores (tests/anyfmt_rules.py: ``Table``), and ragged requests with empty bags."""
import numpy as np

from tests import anyfmt_rules as A
from tests import embedding_rules as E
from tests import f8_rules as F8

SEVEN = list(A.FORMATS)
# each format twice and never next to itself, T = 14
FOURTEEN = SEVEN + SEVEN[3:] + SEVEN[:3]


def table_bytes(fmt, rows, dim, rng):
    """uint8 ``[rows, row_bytes]`` of a seeded table: float formats hold normal values (row 0: zeros), FP8 finite codes, quantised rows
    random codes behind a scale in [0.01, 0.1] and a bias in [-1, 1] (fp32 tails for 8 bits, fp16 tails for 4)"""
    if fmt in ("fp32", "bf16", "fp16"):
        x = (rng.standard_normal((rows, dim)) * 2).astype(np.float32)
        x[0] = 0.0
        return np.ascontiguousarray(E.to_bits(x, A._KIND[fmt])).view(np.uint8).reshape(rows, -1)
    if fmt.startswith("fp8"):
        return F8.finite_codes(rng, A._F8[fmt], (rows, dim))
    scale = rng.uniform(0.01, 0.1, (rows, 1))
    bias = rng.uniform(-1.0, 1.0, (rows, 1))
    tails = np.concatenate([scale, bias], axis=1)
    if fmt == "int8":
        codes = rng.integers(0, 256, (rows, dim), dtype=np.uint8)
        return np.concatenate([codes, tails.astype(np.float32).view(np.uint8).reshape(rows, 8)], axis=1)
    codes = rng.integers(0, 16, (rows, dim), dtype=np.uint8)
    packed = (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)
    return np.concatenate([packed, tails.astype(np.float16).view(np.uint8).reshape(rows, 4)], axis=1)


def tables(formats, rows, dims, seed, exps=None):
    """list of ``anyfmt_rules.Table``; ``exps``: None (0 everywhere) or one exponent per table (used for the FP8 tables)"""
    rng = np.random.default_rng(seed)
    out = []
    for t, (f, r, d) in enumerate(zip(formats, rows, dims)):
        e = int(exps[t]) if exps is not None and f.startswith("fp8") else 0
        out.append(A.make_table(f, table_bytes(f, r, d, rng), d, e))
    return out


def request(seed, rows, B, max_len=9, weights=True):
    """(indices int64, offsets int64 ``[T * B + 1]``, per-sample weights fp32 or None): ragged bags of 0 .. max_len lookups; the first bag
    of table 0 and the last bag of the last table are empty"""
    rng = np.random.default_rng(seed)
    T = len(rows)
    lens = rng.integers(0, max_len + 1, T * B)
    lens[0] = lens[-1] = 0
    ends = np.cumsum(lens)
    off = np.concatenate([[0], ends]).astype(np.int64)
    per_table = np.repeat(np.asarray(rows, dtype=np.int64), [int(lens[t * B:(t + 1) * B].sum()) for t in range(T)])
    idx = (rng.random(int(ends[-1])) * per_table).astype(np.int64)
    psw = (rng.standard_normal(idx.size) * 1.5).astype(np.float32) if weights else None
    return idx, off, psw


def rows_for(T, seed, lo=50, hi=300):
    return [int(r) for r in np.random.default_rng(seed).integers(lo, hi + 1, T)]
