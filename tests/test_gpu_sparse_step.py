"""pm_sparse_rows_sgd / pm_sparse_rows_adagrad on the GPU, BIT FOR BIT against the numpy restatement of their rules
(tests/sparse_step_rules.py): whole tables and whole state arrays, so rows that are not listed are checked too; then the two optimizer
classes end to end behind the sparse=True modules."""
import numpy as np
import pytest
import torch

import param_amd
from tests import sparse_step_rules as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
HYPER = {"lr": 3.0e-2, "lr_decay": 0.1, "eps": 1.0e-10}
# dims: one lane and no butterfly, two lanes, a group of 4 with one idle lane, a 32-lane group, two sweeps whose last pass is not full.
# U: an empty table; 257 + 5 + 300 + 40 slots: tiles end inside tables and straddle table borders; the last table has every row listed
MIXED = ((4, 8, 12, 128, 520), (7, 300, 300, 1000, 40), (0, 257, 5, 300, 40))
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
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("rule", ["sgd", "adagrad", "rowwise"])
def test_rows_kernel_matches_the_restatement_on_bits(rule, dtype, maximize, dims, rows, listed):
    rng = np.random.default_rng(3)
    hyper = dict(HYPER, maximize=maximize)
    T, rowwise = len(dims), rule == "rowwise"
    w = [R.round_to_table(rng.standard_normal((rows[t], dims[t])).astype(np.float32), dtype) for t in range(T)]
    s = [np.full(x.shape[:1] if rowwise else x.shape, 0.25, dtype=np.float32) for x in w]
    d_w = [torch.from_numpy(x).to(DEV).to(TORCH[dtype]) for x in w]
    d_s = [torch.from_numpy(x).to(DEV) for x in s]
    for step in (1, 2, 3):
        ids = [_row_ids(rng, rows[t], listed[t]) for t in range(T)]
        g = [rng.standard_normal((listed[t], dims[t])).astype(np.float32) for t in range(T)]
        grads = [(torch.from_numpy(ids[t]).to(DEV), torch.from_numpy(g[t]).to(DEV)) for t in range(T)]
        if rule == "sgd":
            param_amd.sparse_sgd_rows_(d_w, grads, hyper["lr"], maximize)
            w = [R.sgd_step(w[t], ids[t], g[t], hyper, dtype) for t in range(T)]
        else:
            param_amd.sparse_adagrad_rows_(d_w, grads, d_s, step, hyper["lr"], hyper["lr_decay"], hyper["eps"], maximize, rowwise)
            for t in range(T):
                w[t], s[t] = R.adagrad_step(w[t], ids[t], g[t], s[t], step, hyper, dtype, rowwise)
    for t in range(T):
        for got, want in ((d_w[t].float(), w[t]), (d_s[t], s[t])):
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (t, dims[t])


@pytest.mark.parametrize("kind", ["bag", "embedding"])
@pytest.mark.parametrize("rule", ["sgd", "adagrad", "rowwise"])
def test_optimizers_step_the_sparse_modules(rule, kind):
    torch.manual_seed(0)
    if kind == "bag":
        mod = param_amd.EmbeddingBagMI355(50, 16, sparse=True, device=DEV)
        args = (torch.tensor([3, 3, 49, 0, 7, 3, 7, 20], device=DEV), torch.tensor([0, 3, 5], device=DEV))      # duplicate lookups
    else:
        mod = param_amd.EmbeddingMI355(50, 16, sparse=True, device=DEV)
        args = (torch.tensor([[3, 3, 49], [0, 7, 20]], device=DEV),)
    hyper = dict(HYPER, initial_accumulator_value=0.5)
    opt = (param_amd.SparseSGDMI355(mod.parameters(), lr=hyper["lr"]) if rule == "sgd" else
           param_amd.SparseAdagradMI355(mod.parameters(), rowwise=rule == "rowwise", **hyper))
    w = mod.weight.detach().cpu().numpy().copy()
    s = np.full(w.shape[:1] if rule == "rowwise" else w.shape, 0.5, dtype=np.float32)
    for step in (1, 2):
        opt.zero_grad(set_to_none=True)
        out = mod(*args)
        (out * torch.randn_like(out)).sum().backward()
        g = mod.weight.grad
        assert g.is_sparse and g.is_coalesced()
        ids, vals = g._indices()[0].cpu().numpy(), g._values().cpu().numpy()
        opt.step()
        if rule == "sgd":
            w = R.sgd_step(w, ids, vals, hyper)
        else:
            w, s = R.adagrad_step(w, ids, vals, s, step, hyper, rowwise=rule == "rowwise")
            assert np.array_equal(_bits(opt.state[mod.weight]["sum"].cpu().numpy()), _bits(s))
        assert np.array_equal(_bits(mod.weight.detach().cpu().numpy()), _bits(w))        # rows never looked up keep their bits


@pytest.mark.parametrize("cls", ["SparseAdagradMI355", "SparseSGDMI355"])
def test_dense_gradient_raises_torchs_error(cls):
    p = torch.nn.Parameter(torch.zeros(8, 4, device=DEV))
    p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="does not support dense gradients"):
        getattr(param_amd, cls)([p], lr=0.1).step()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_adagrad_steps_after_loading_torchs_state_dict(dtype):
    """torch.optim.Adagrad takes a step, SparseAdagradMI355 loads its state_dict (groups without `rowwise`, a `sum` of the parameter's
    dtype) and takes the next one: the restatement's bits, carried from torch's state"""
    rng = np.random.default_rng(5)
    hyper = dict(HYPER, initial_accumulator_value=0.5)
    p = torch.nn.Parameter(torch.from_numpy(rng.standard_normal((40, 16)).astype(np.float32)).to(DEV).to(TORCH[dtype]))
    ref, ours = torch.optim.Adagrad([p], **hyper), param_amd.SparseAdagradMI355([p], **hyper)
    ids = np.array([39, 0, 7, 21])
    for step, opt in ((1, ref), (2, ours)):
        g = rng.standard_normal((ids.size, 16)).astype(np.float32)
        p.grad = torch.sparse_coo_tensor(torch.from_numpy(ids)[None].to(DEV), torch.from_numpy(g).to(DEV).to(TORCH[dtype]), (40, 16)).coalesce()
        w, s = p.detach().float().cpu().numpy(), opt.state[p]["sum"].float().cpu().numpy()
        opt.step()
        if step == 1:
            ours.load_state_dict(ref.state_dict())
    assert ours.state[p]["sum"].dtype == torch.float32 and int(ours.state[p]["step"]) == 2
    rows, g = p.grad._indices()[0].cpu().numpy(), p.grad._values().float().cpu().numpy()    # coalesced: rows ascending, the dtype's values
    w, s = R.adagrad_step(w, rows, g, s, 2, hyper, dtype)
    assert np.array_equal(_bits(p.detach().float().cpu().numpy()), _bits(w))
    assert np.array_equal(_bits(ours.state[p]["sum"].cpu().numpy()), _bits(s))
