"""The direct backward of max pooling without a GPU: its numpy restatement (tests/max_direct_rules.py) against ``max_rules.dense_grad``
and torch's CPU autograd of ``F.embedding_bag(mode="max")`` on bits, and the refusals the host layer makes before it needs a device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import max_direct_rules as R
from tests import max_rules as M


def test_restatement_is_torch_cpu_autograd_and_the_dense_rule():
    rng = np.random.default_rng(3)
    rows, dims, B = (40, 17, 300), (8, 16, 8), 24
    idx, off = [], []
    for r in rows:
        for b in range(B):
            off.append(len(idx))
            bag = list(map(int, rng.integers(0, min(r, 12), size=(0, 1, 2, 3, 5)[b % 5])))
            idx += bag[:1] * (b % 3 == 0) + bag      # some bags hold a row twice
    idx, off = np.array(idx, np.int64), np.array(off, np.int64)
    tabs = [(rng.integers(-8, 9, size=(r, d)) / 8.0).astype(np.float32) for r, d in zip(rows, dims)]      # few values: ties
    grads = [rng.standard_normal((B, d)).astype(np.float32) for d in dims]
    _, args = M.forward(tabs, idx, off, B)
    want = M.dense_grad(rows, dims, grads, args)
    for t, (G, won, _, _, n) in enumerate(R.sums(rows, dims, idx, off, B, grads, args)):
        assert n.max() > 1 and n.max() <= R.EXACT_RUN and not won.all()
        got = R.apply(np.zeros(G.shape, np.uint32), "f32", G, won, 1.0)
        assert np.array_equal(got, M.bits(want[t])), t
        w = torch.from_numpy(tabs[t]).requires_grad_()
        lo, hi = off[t * B], (off[(t + 1) * B] if t + 1 < len(rows) else idx.size)
        out = F.embedding_bag(torch.from_numpy(idx[lo:hi]), w, torch.from_numpy(off[t * B:(t + 1) * B] - lo), mode="max")
        out.backward(torch.from_numpy(grads[t]))
        assert np.array_equal(got, M.bits(w.grad.numpy())), t


def test_host_refusals():
    import param_amd

    i, o, g = torch.zeros(6, dtype=torch.int64), torch.arange(7, dtype=torch.int64), torch.zeros(2, 24)
    s = param_amd.BatchedEmbeddingBagMI355([64, 64, 64], 8, device="cpu", init=None)
    m = param_amd.MaxBatchedEmbeddingBagMI355([64, 64, 64], 8, device="cpu", init=None)
    for call in (lambda: s.dense_grad(g, i, o, method="direct"), lambda: s.scatter_add_(g, i, o, 1.0, method="direct")):
        with pytest.raises(ValueError, match="direct backward of max pooling"):
            call()
    for call in (lambda: m.dense_grad(g, i, o, method="atomic"), lambda: m.scatter_add_(g, i, o, 1.0, method="atomic"),
                 lambda: m.scatter_add_(g, i, o, 1.0, method="direct", presorted=True),
                 lambda: m.scatter_add_(g, i, o, 1.0, torch.ones(6), method="direct")):
        with pytest.raises(ValueError, match="not taken|per_sample_weights"):
            call()
