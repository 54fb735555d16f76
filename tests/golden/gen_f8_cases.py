"""Writes tests/golden/f8_cases.npz from torch's CPU engine alone (no kernel of this project, no rule of tests/f8_rules.py):

* ``dec_<fmt>``: the 256 fp32 values ``torch.arange(256, dtype=uint8).view(float8).to(float32)`` of both formats;
* per format one table of codes ``[24, 16]`` -- random codes, and rows holding -0.0, subnormals, the largest values, +-Inf (e5m2) and
  NaN -- one request of 8 bags (an empty bag, an all-padding bag, a bag of one, padded lookups first and last in a bag), and
  ``torch.nn.functional.embedding_bag`` over ``table.to(float32)`` for: sum, sum with ``padding_idx``, weighted sum (over the finite rows:
  a weight times Inf is left to the GPU tests' own rule), mean, mean with ``padding_idx``.

Run from the repository root: ``python tests/golden/gen_f8_cases.py``."""
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
PAD = 5
# rows 0 .. 15 random finite codes; 16: -0.0 / +0.0; 17: subnormals; 18: largest finite; 19: NaN codes; 20: +-Inf (e5m2; e4m3: 448s);
# 21 .. 23 random finite
LENS = (3, 0, 1, 4, 2, 5, 2, 3)          # bag 4 is all padding, bag 1 empty


def finite_codes(rng, fmt, shape):
    c = rng.integers(0, 256, shape, dtype=np.uint8)
    bad = (c & 0x7f) == 0x7f if fmt == "e4m3" else (c & 0x7f) >= 0x7c
    return np.where(bad, c & 0x3f, c).astype(np.uint8)


def table(fmt, rng):
    t = finite_codes(rng, fmt, (24, 16))
    t[16] = np.tile([0x80, 0x00], 8)
    t[17] = np.tile([0x01, 0x81, 0x03, 0x07 if fmt == "e4m3" else 0x02], 4)
    t[18] = np.tile([0x7e, 0xfe] if fmt == "e4m3" else [0x7b, 0xfb], 8)
    t[19] = np.tile([0x7f, 0xff] if fmt == "e4m3" else [0x7d, 0xfe], 8)
    t[20] = np.tile([0x7e, 0x7e] if fmt == "e4m3" else [0x7c, 0xfc], 8)
    return t


def main():
    rng = np.random.default_rng(2025)
    out = {}
    for fmt, dt in DTYPES.items():
        out[f"dec_{fmt}"] = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(dt).to(torch.float32).numpy()
        tab = table(fmt, rng)
        W = torch.from_numpy(tab).view(dt).to(torch.float32)
        off = np.concatenate([[0], np.cumsum(LENS)])[:-1].astype(np.int64)
        n = int(sum(LENS))
        idx = rng.integers(0, 16, n).astype(np.int64)
        idx[0], idx[2] = PAD, PAD                      # bag 0: padded first and last
        idx[8:10] = PAD                                # bag 4: all padding
        idx[10:15] = [16, 17, 18, 21, 16]              # bag 5: signed zeros, subnormals, the largest values
        idx[15:17] = [19, 3]                           # bag 6: NaN
        idx[17:20] = [20, 20, 22]                      # bag 7: Inf + Inf (e5m2) / 448 + 448 (e4m3)
        psw = rng.standard_normal(n).astype(np.float32)
        fin_idx = np.where(idx >= 19, idx - 19, idx)   # the weighted case stays on finite rows (19, 20 -> 0, 1)
        ti, to = torch.from_numpy(idx), torch.from_numpy(off)
        out[f"table_{fmt}"], out[f"indices_{fmt}"], out[f"offsets_{fmt}"], out[f"psw_{fmt}"] = tab, idx, off, psw
        out[f"indices_weighted_{fmt}"] = fin_idx
        out[f"sum_{fmt}"] = F.embedding_bag(ti, W, to, mode="sum").numpy()
        out[f"sum_pad_{fmt}"] = F.embedding_bag(ti, W, to, mode="sum", padding_idx=PAD).numpy()
        out[f"weighted_{fmt}"] = F.embedding_bag(torch.from_numpy(fin_idx), W, to, mode="sum", per_sample_weights=torch.from_numpy(psw)).numpy()
        out[f"weighted_pad_{fmt}"] = F.embedding_bag(torch.from_numpy(fin_idx), W, to, mode="sum", per_sample_weights=torch.from_numpy(psw),
                                                     padding_idx=PAD).numpy()
        out[f"mean_{fmt}"] = F.embedding_bag(ti, W, to, mode="mean").numpy()
        out[f"mean_pad_{fmt}"] = F.embedding_bag(ti, W, to, mode="mean", padding_idx=PAD).numpy()
    out["pad"] = np.int64(PAD)
    np.savez_compressed(os.path.join(HERE, "f8_cases.npz"), **out)
    print("wrote f8_cases.npz:", sorted(out))


if __name__ == "__main__":
    main()
