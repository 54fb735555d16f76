#!/usr/bin/env python3
"""Writes tests/golden/max_cases.npz: the inputs of the MAX POOLING rule's special cases and what torch's CPU
``nn.functional.embedding_bag(..., mode="max")`` gives for them -- output, ``max_indices`` and ``weight.grad`` -- on fp32, bf16 and fp16
tables, with and without ``padding_idx``, for the 1-D (indices + offsets) and the 2-D (``[B, L]``) form.  Run from the repository root:
``python tests/golden/gen_max_cases.py`` (CPU only; recorded with torch 2.10).

One table of 12 rows x 8 columns.  Every weight is a multiple of 1/8 below 32 in magnitude, so the same values are exact in all three
dtypes; the special rows are listed in ``weight()``.  ``g_rand`` is the fp32 gradient; ``g_exact`` (multiples of 1/4, |g| <= 4) is
the gradient of the 16-bit cases: every sum of a few of them is exact in bf16 and fp16, so the comparison does not depend on where a
16-bit accumulation rounds."""
import os

import numpy as np
import torch

R, D, PAD = 12, 8, 3
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
# the bags of the 1-D form, in order (tests/test_max_host.py asserts what each one is there for)
BAGS = [
    [],                    # 0: empty
    [3, 3],                # 1: padding only
    [3, 6, 7],             # 2: padding first, then two all-negative rows
    [9],                   # 3: a bag of one
    [0, 9, 10],            # 4: column 0's first kept value is NaN
    [9, 0, 10],            # 5: column 0 has a NaN only later
    [1, 2],                # 6: column 1: -0.0 before +0.0
    [2, 1],                # 7: ... and the reverse
    [4, 5],                # 8: column 2: equal maxima from two different rows
    [8],                   # 9: a row of -Inf
    [9, 10, 9],            # 10: a row twice in one bag
    [9, 11, 5, 10, 6],     # 11: five lookups; row 9 is in several bags
]
# the 2-D form: 5 bags of 3
INPUT_2D = [[3, 6, 7], [0, 9, 10], [9, 0, 3], [3, 3, 3], [4, 5, 9]]


def weight():
    rng = np.random.default_rng(20261021)
    w = (rng.integers(-80, 81, size=(R, D)) / 8.0).astype(np.float32)
    w[0, 0] = np.nan
    w[1, 1], w[2, 1] = -0.0, 0.0
    w[PAD] = 31.0                      # the padding row would win every column it is in
    w[4, 2] = w[5, 2] = 12.5           # a tie that is the maximum of bag 8 (and larger than anything random)
    w[4, 3], w[5, 3] = 1.0, 2.0
    w[6] = -np.abs(w[6]) - 0.125
    w[7] = -np.abs(w[7]) - 0.125
    w[8] = -np.inf
    return w


def table_bits(w32, dtype):
    """the table in ``dtype`` as stored bits (uint32 / uint16).  Stored in the file and read back by the tests: how a NaN converts to
    16 bits is the converting code's choice (a vectorised and a scalar cast give different payloads), and the cases must not depend on it."""
    t = torch.from_numpy(w32).to(dtype)
    return t.view(torch.int32 if dtype == torch.float32 else torch.int16).numpy().view(np.uint32 if dtype == torch.float32 else np.uint16)


def table_from_bits(bits, dtype):
    return torch.from_numpy(bits.view(np.int32 if dtype == torch.float32 else np.int16).copy()).view(dtype)


def torch_case(wbits, dtype, idx, off, pad, grad):
    """(out widened to fp32, max_indices int32, weight.grad widened to fp32) of torch's CPU kernels"""
    w = table_from_bits(wbits, dtype).requires_grad_(True)
    args = (torch.from_numpy(idx),) if off is None else (torch.from_numpy(idx), torch.from_numpy(off))
    out = torch.nn.functional.embedding_bag(args[0], w, *args[1:], mode="max", padding_idx=pad)
    out.backward(torch.from_numpy(grad).to(dtype))
    flat = args[0].reshape(-1)
    o = torch.from_numpy(off) if off is not None else torch.arange(idx.shape[0], dtype=torch.int64) * idx.shape[1]
    mi = torch.ops.aten._embedding_bag(w.detach(), flat, o, False, 2, False, None, False, -1 if pad is None else pad)[3]
    return out.detach().float().numpy(), mi.to(torch.int32).numpy(), w.grad.float().numpy()


def main():
    rng = np.random.default_rng(7)
    w = weight()
    idx1 = np.array([r for bag in BAGS for r in bag], dtype=np.int64)
    off1 = np.cumsum([0] + [len(b) for b in BAGS[:-1]]).astype(np.int64)
    idx2 = np.array(INPUT_2D, dtype=np.int64)
    data = {"idx1": idx1, "off1": off1, "idx2": idx2, "pad": np.int64(PAD)}
    for dname, dt in DTYPES.items():
        data[f"w_{dname}"] = table_bits(w, dt)
    for form, idx, off in (("1d", idx1, off1), ("2d", idx2, None)):
        nb = len(BAGS) if form == "1d" else idx2.shape[0]
        data[f"{form}_g_rand"] = rng.standard_normal((nb, D)).astype(np.float32)
        data[f"{form}_g_exact"] = (rng.integers(-16, 17, size=(nb, D)) / 4.0).astype(np.float32)
        for pname, pad in (("pad", PAD), ("nopad", None)):
            for dname, dt in DTYPES.items():
                g = data[f"{form}_g_rand" if dname == "f32" else f"{form}_g_exact"]
                out, mi, wg = torch_case(data[f"w_{dname}"], dt, idx, off, pad, g)
                data[f"{form}_{pname}_{dname}_out"], data[f"{form}_{pname}_{dname}_arg"], data[f"{form}_{pname}_{dname}_wgrad"] = out, mi, wg
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "max_cases.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes, torch", torch.__version__)


if __name__ == "__main__":
    main()
