"""pm_sparse_rows_adam on the GPU, BIT FOR BIT against the numpy restatement of its rule (tests/sparse_adam_rules.py): whole tables and
whole state arrays, so rows that are not listed are checked too; then SparseAdamMI355 end to end behind the sparse=True modules."""
import numpy as np
import pytest
import torch

import param_amd
from tests import sparse_adam_rules as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
# dims: one lane, a sub-wave group, a full row, column passes whose last is not full.  U: an empty table; 257 + 300 + 40 slots: tile 0
# ends inside table 1, tile 1 straddles tables 1 | 2, tile 2 straddles 2 | 3; table 3 has every row listed
MIXED = ((4, 8, 128, 520), (7, 300, 1000, 40), (0, 257, 300, 40))
MANY = ((8,) * 300, (1,) * 300, (1,) * 300)            # 300 one-row tables: the prefix is searched in global memory


_bits = lambda x: np.ascontiguousarray(x).view(np.uint32)      # noqa: E731


def _row_ids(rng, rows, u):
    """u distinct rows in random order, the table's first and last row among them"""
    ids = rng.permutation(rows)[:u]
    if u >= 2:
        ids = np.concatenate(([0, rows - 1], ids[(ids != 0) & (ids != rows - 1)]))[:u]
    return rng.permutation(ids).astype(np.int64)


@pytest.mark.parametrize("dims,rows,listed", [MIXED, MANY], ids=["mixed", "many"])
@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_rows_kernel_matches_the_restatement_on_bits(dtype, wd, maximize, dims, rows, listed):
    rng = np.random.default_rng(3)
    hyper = {"lr": 1.0e-2, "betas": (0.9, 0.999), "eps": 1.0e-8, "weight_decay": wd, "maximize": maximize}
    T = len(dims)
    w = [R.round_to_table(rng.standard_normal((rows[t], dims[t])).astype(np.float32), dtype) for t in range(T)]
    m, v = [np.zeros_like(x) for x in w], [np.zeros_like(x) for x in w]
    d_w = [torch.from_numpy(x).to(DEV).to(TORCH[dtype]) for x in w]
    d_m, d_v = [torch.zeros(x.shape, device=DEV) for x in w], [torch.zeros(x.shape, device=DEV) for x in w]
    for step in (1, 2, 3):
        ids = [_row_ids(rng, rows[t], listed[t]) for t in range(T)]
        g = [rng.standard_normal((listed[t], dims[t])).astype(np.float32) for t in range(T)]
        grads = [(torch.from_numpy(ids[t]).to(DEV), torch.from_numpy(g[t]).to(DEV)) for t in range(T)]
        param_amd.sparse_adam_rows_(d_w, grads, d_m, d_v, step, hyper["lr"], hyper["betas"], hyper["eps"], wd, maximize)
        for t in range(T):
            w[t], m[t], v[t] = R.sparse_adam_step(w[t], ids[t], g[t], m[t], v[t], step, hyper, dtype)
    for t in range(T):
        for got, want in ((d_w[t].float(), w[t]), (d_m[t], m[t]), (d_v[t], v[t])):
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (t, dims[t])


@pytest.mark.parametrize("kind", ["bag", "embedding"])
def test_optimizer_steps_the_sparse_modules(kind):
    torch.manual_seed(0)
    hyper = {"lr": 1.0e-2, "betas": (0.9, 0.999), "eps": 1.0e-8, "weight_decay": 0.0}
    if kind == "bag":
        mod = param_amd.EmbeddingBagMI355(50, 16, sparse=True, device=DEV)
        args = (torch.tensor([3, 3, 49, 0, 7, 3, 7, 20], device=DEV), torch.tensor([0, 3, 5], device=DEV))      # duplicate lookups
    else:
        mod = param_amd.EmbeddingMI355(50, 16, sparse=True, device=DEV)
        args = (torch.tensor([[3, 3, 49], [0, 7, 20]], device=DEV),)
    opt = param_amd.SparseAdamMI355(mod.parameters(), lr=hyper["lr"])
    w = mod.weight.detach().cpu().numpy().copy()
    m, v = np.zeros_like(w), np.zeros_like(w)
    for step in (1, 2):
        opt.zero_grad(set_to_none=True)
        out = mod(*args)
        (out * torch.randn_like(out)).sum().backward()
        g = mod.weight.grad
        assert g.is_sparse and g.is_coalesced()
        ids, vals = g._indices()[0].cpu().numpy(), g._values().cpu().numpy()
        opt.step()
        w, m, v = R.sparse_adam_step(w, ids, vals, m, v, step, hyper)
        assert np.array_equal(_bits(mod.weight.detach().cpu().numpy()), _bits(w))        # rows never looked up keep their bits
        assert np.array_equal(_bits(opt.state[mod.weight]["exp_avg_sq"].cpu().numpy()), _bits(v))


def test_dense_gradient_raises_torchs_error():
    p = torch.nn.Parameter(torch.zeros(8, 4, device=DEV))
    p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="SparseAdam does not support dense gradients"):
        param_amd.SparseAdamMI355([p]).step()
