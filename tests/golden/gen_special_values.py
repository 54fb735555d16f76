"""Writes tests/golden/special_values.npz: what torch computes ON THE CPU for the shared special values of tests/special_values.py.

  fwd_{kind}_{D}_{u|w}   ``torch.nn.functional.embedding_bag(mode="sum")`` over the special table (fp32; bf16 / fp16 table bits widened by
                         torch's own ``.float()``), the named bags and ragged bags, unweighted / weighted (tests.special_values.forward_request)
  q{bits}_{dim}, d{bits}_{dim}   ``quantized::embedding_bag_{byte,4bit,2bit}_prepack`` / ``_unpack`` of the finite edge rows followed by the
                         mixed-zero rows, dims 8, 32, 128
  ada_w_{case}, ada_s_{case}     ``torch.optim.Adagrad`` after two steps on the special gradients (eps x weight decay cases)

Inputs are rebuilt from the builders (seeded), not stored: a builder change shows up as a mismatch.  Run from the repository root:
``python tests/golden/gen_special_values.py``; the file is reproduced byte for byte (fixed zip timestamps).
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import special_values as S      # noqa: E402

FWD_DIMS, QUANT_DIMS = (8, 64, 128), (8, 32, 128)
FWD_ROWS, FWD_B = 48, 40
ADA_CASES = [(eps, wd) for eps in (1e-10, 1e-5, 0.0) for wd in (0.0, 0.01)]
ADA_LR = 0.05
PACK = {8: ("embedding_bag_byte_prepack", "embedding_bag_byte_unpack"), 4: ("embedding_bag_4bit_prepack", "embedding_bag_4bit_unpack"),
        2: ("embedding_bag_2bit_prepack", "embedding_bag_2bit_unpack")}


def fwd_case(kind, D, weighted):
    """(table as stored, table widened to fp32, idx, off, psw, named bags) of one forward fixture: one table, ragged bags"""
    rng = np.random.default_rng(100 * D + 10 * S.KINDS.index(kind) + weighted)
    store, w = S.special_table(FWD_ROWS, D, rng, kind)
    idx, off, psw, named = S.forward_request(kind, [FWD_ROWS], FWD_B, rng, None, weighted)
    return store, w, idx, off, psw, named


def torch_widen(store, kind):
    if kind == "f32":
        return torch.from_numpy(store.copy())
    t = torch.from_numpy(store.view(np.int16).copy())
    return t.view(torch.bfloat16 if kind == "bf16" else torch.float16).float()


def torch_fwd(w_t, idx, off, psw):
    return torch.nn.functional.embedding_bag(torch.from_numpy(idx), w_t, torch.from_numpy(off[:-1].copy()), mode="sum",
                                             per_sample_weights=None if psw is None else torch.from_numpy(psw)).numpy()


def quant_rows(dim):
    return np.concatenate([S.quant_edge_rows(dim)[0], S.quant_mixed_zero_rows(dim)], axis=0)


def adagrad_inputs():
    """(w0, s0, [g step 1, g step 2]): one weight per (special gradient, starting state) pair; states 0, a subnormal, 1, FLT_MAX; the second
    step's gradients are the first's moved on by one (so -0 is followed by +0: a zero sum on a zero state)"""
    g = np.concatenate([S.F32_SPECIALS, np.array([1e-30, -1e-30, 1e-20, 1e19, -1e19, 1e-38, 5e-39], S.F32)])
    s0 = np.array([0.0, 1e-40, 1.0, S.FLT_MAX], S.F32)
    G, S0 = np.meshgrid(g, s0, indexing="ij")
    w0 = np.broadcast_to(np.array([0.5, -1.25, 0.0, 3.0], S.F32), G.shape)
    return np.ascontiguousarray(w0, dtype=S.F32), np.ascontiguousarray(S0, dtype=S.F32), [np.ascontiguousarray(G, dtype=S.F32), np.ascontiguousarray(np.roll(G, 1, axis=0), dtype=S.F32)]


def torch_adagrad(w0, s0, grads, eps, wd):
    p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.Adagrad([p], lr=ADA_LR, eps=eps, initial_accumulator_value=0.0, lr_decay=0.0, weight_decay=wd)
    opt.state[p]["sum"] = torch.from_numpy(s0.copy())
    opt.state[p]["step"] = torch.tensor(0.0)
    for g in grads:
        p.grad = torch.from_numpy(g.copy())
        opt.step()
    return p.detach().numpy().copy(), opt.state[p]["sum"].numpy().copy()


def generate():
    out = {}
    for kind in S.KINDS:
        for D in FWD_DIMS:
            for weighted in (False, True):
                store, _, idx, off, psw, _ = fwd_case(kind, D, weighted)
                out[f"fwd_{kind}_{D}_{'w' if weighted else 'u'}"] = torch_fwd(torch_widen(store, kind), idx, off, psw)
    for dim in QUANT_DIMS:
        x = torch.from_numpy(quant_rows(dim))
        for bits, (pack, unpack) in PACK.items():
            q = getattr(torch.ops.quantized, pack)(x)
            out[f"q{bits}_{dim}"] = q.numpy()
            out[f"d{bits}_{dim}"] = getattr(torch.ops.quantized, unpack)(q).numpy()
    w0, s0, grads = adagrad_inputs()
    for k, (eps, wd) in enumerate(ADA_CASES):
        out[f"ada_w_{k}"], out[f"ada_s_{k}"] = torch_adagrad(w0, s0, grads, eps, wd)
    return out


def write(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "special_values.npz")
    write(dst, generate())
    print(dst, os.path.getsize(dst), "bytes")
