"""tests/golden/max_cases.npz (written by tests/golden/gen_max_cases.py) as the max-pooling tests read it: one table of 12 rows x 8
columns in fp32, bf16 and fp16 -- built from the stored BITS, so that no test depends on how this host converts a NaN to 16 bits --,
the 1-D and the 2-D request, and what torch's CPU kernels gave: ``out`` (widened to fp32), ``max_indices`` and ``weight.grad`` (widened)."""
import os

import numpy as np
import torch

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "max_cases.npz")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
ROWS, DIM = 12, 8
_Z = None


def z():
    global _Z
    if _Z is None:
        _Z = dict(np.load(PATH))
    return _Z


def pad():
    return int(z()["pad"])


def table(dname):
    """the table as a torch CPU tensor of that dtype (a fresh copy)"""
    b = z()["w_" + dname]
    return torch.from_numpy(b.view(np.int32 if dname == "f32" else np.int16).copy()).view(DTYPES[dname])


def table32(dname):
    """... widened exactly to fp32, as numpy (what tests/max_rules.py takes)"""
    return table(dname).float().numpy()


def request(form):
    """(indices flat int64, offsets int64 [B], B, the 2-D input or None)"""
    if form == "1d":
        return z()["idx1"], z()["off1"], int(z()["off1"].size), None
    i2 = z()["idx2"]
    return i2.reshape(-1), np.arange(i2.shape[0], dtype=np.int64) * i2.shape[1], int(i2.shape[0]), i2


def grad(form, dname):
    return z()[f"{form}_g_rand" if dname == "f32" else f"{form}_g_exact"]


def torch_result(form, pname, dname):
    """(out fp32, max_indices int32, weight.grad fp32) as recorded"""
    k = f"{form}_{pname}_{dname}_"
    return z()[k + "out"], z()[k + "arg"], z()[k + "wgrad"]


def bags(form):
    """the request's bags as lists of row indices"""
    idx, off, B, _ = request(form)
    end = list(off[1:]) + [idx.size]
    return [list(map(int, idx[int(s):int(e)])) for s, e in zip(off, end)]
