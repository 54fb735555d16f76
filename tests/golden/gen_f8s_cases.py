"""Writes tests/golden/f8s_cases.npz from torch's CPU engine and ``np.frexp`` alone (no kernel of this project, no rule of
tests/f8s_rules.py), for both formats ``fmt`` and both kinds of exponent ``kind`` (``row``, ``table``):

* ``src_<fmt>``: fp32 rows ``[14, 16]`` -- rows of the uniform init of 10 M rows (|x| <= 3.2e-4), rows of mixed magnitudes, a row whose
  largest magnitude has mantissa exactly 1.75 and one with the next fp32 above it, a row of zeros, a row with NaN and +-Inf next to
  finite values, a row without a finite element, fp32 subnormals, a row beyond the exponent clamp (2^100);
* ``rowexp_<fmt>``: from ``np.frexp`` of the largest finite magnitude; ``codes_<kind>_<fmt>``: ``torch.ldexp(src, -s).to(float8)`` with
  ``s`` the row's exponent, or for ``table`` the largest exponent of rows 0 .. 9 (the 2^100 row then overflows: the cast's business);
* ``deq_<kind>_<fmt>``: ``torch.ldexp(codes.to(float32), s)``; over it ``torch.nn.functional.embedding_bag`` -- sum, sum with
  ``padding_idx``, weighted sum, mean, mean with ``padding_idx``, over the rows that are finite -- their bf16 / fp16 casts (uint16
  patterns) for sum and mean, and ``torch.nn.functional.embedding`` of every row.

Run from the repository root: ``python tests/golden/gen_f8s_cases.py``."""
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
K = {"e4m3": 8, "e5m2": 15}
PAD = 5
LENS = (3, 0, 1, 4, 2, 5, 2, 3)          # bag 4 is all padding, bag 1 empty
FINITE_ROWS = 10                          # rows 0 .. 9 hold finite values only: what the pooled cases look up


def source(rng):
    x = np.zeros((14, 16), dtype=np.float32)
    x[0:3] = rng.uniform(-3.2e-4, 3.2e-4, (3, 16))
    x[3:6] = rng.standard_normal((3, 16)) * np.exp2(rng.integers(-20, 20, (3, 1)))
    x[6] = rng.uniform(-1, 1, 16) * 3.0
    x[6, 3] = -3.5                        # amax = 1.75 * 2^1 exactly
    x[7] = x[6]
    x[7, 3] = np.nextafter(np.float32(3.5), np.float32(4.0))
    x[8] = 0.0
    x[8, 1] = -0.0
    x[9] = rng.standard_normal(16) * 1e-41          # fp32 subnormals
    x[10] = rng.standard_normal(16)
    x[10, :3] = [np.nan, np.inf, -np.inf]
    x[11] = np.tile([np.inf, np.nan], 8)
    x[12] = rng.standard_normal(16) * 2.0 ** 100
    x[13] = rng.standard_normal(16) * 2.0 ** -100
    return x


def exponents(x, k):
    a = np.where(np.isfinite(x), np.abs(x), np.float32(0)).max(axis=1).astype(np.float64)
    m, q = np.frexp(a)                    # a = m * 2^q, 0.5 <= m < 1
    e = (q - 1) - k + (2 * m > 1.75)
    return np.where(a == 0, -64, np.clip(e, -64, 64)).astype(np.int8)


def bits16(t, dt):
    return t.to(dt).view(torch.int16).numpy().view(np.uint16)


def main():
    rng = np.random.default_rng(2026)
    out = {"pad": np.int64(PAD)}
    x = source(rng)
    off = np.concatenate([[0], np.cumsum(LENS)])[:-1].astype(np.int64)
    n = int(sum(LENS))
    idx = rng.integers(0, FINITE_ROWS, n).astype(np.int64)
    idx[0], idx[2] = PAD, PAD             # bag 0: padded first and last
    idx[8:10] = PAD                       # bag 4: all padding
    psw = rng.standard_normal(n).astype(np.float32)
    ti, to, tw = torch.from_numpy(idx), torch.from_numpy(off), torch.from_numpy(psw)
    out["indices"], out["offsets"], out["psw"] = idx, off, psw
    for fmt, dt in DTYPES.items():
        out[f"src_{fmt}"] = x
        e = exponents(x, K[fmt])
        out[f"rowexp_{fmt}"] = e
        for kind, s in (("row", e.astype(np.int32)), ("table", np.full(14, e[:FINITE_ROWS].max(), dtype=np.int32))):
            ts = torch.from_numpy(s)
            codes = torch.ldexp(torch.from_numpy(x), -ts[:, None]).to(dt)
            W = torch.ldexp(codes.to(torch.float32), ts[:, None])
            tag = f"{kind}_{fmt}"
            out[f"codes_{tag}"], out[f"deq_{tag}"] = codes.view(torch.uint8).numpy(), W.numpy()
            out[f"sum_{tag}"] = F.embedding_bag(ti, W, to, mode="sum").numpy()
            out[f"sum_pad_{tag}"] = F.embedding_bag(ti, W, to, mode="sum", padding_idx=PAD).numpy()
            out[f"weighted_{tag}"] = F.embedding_bag(ti, W, to, mode="sum", per_sample_weights=tw).numpy()
            out[f"mean_{tag}"] = F.embedding_bag(ti, W, to, mode="mean").numpy()
            out[f"mean_pad_{tag}"] = F.embedding_bag(ti, W, to, mode="mean", padding_idx=PAD).numpy()
            for name, dt16 in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
                out[f"sum_{name}_{tag}"] = bits16(torch.from_numpy(out[f"sum_{tag}"]), dt16)
                out[f"mean_pad_{name}_{tag}"] = bits16(torch.from_numpy(out[f"mean_pad_{tag}"]), dt16)
            out[f"rows_{tag}"] = F.embedding(torch.arange(14), W).numpy()
    np.savez_compressed(os.path.join(HERE, "f8s_cases.npz"), **out)
    print("wrote f8s_cases.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
