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


# ---- the constructed requests of tests/max_direct_cases.py: what they claim, and that they tell a wrong rule from the right one ----------

def _wrong(c, t, row, mistake):
    """row ``row`` of table t's fp32 sum under a deliberately wrong rule, over the case's slice: ``"repeat"`` counts a bag again when its
    repeat is the first pair of a piece (a kernel that forgot the pair in front of a piece); ``"combine"`` adds the pieces onto +0.0
    instead of starting from the first piece that has a term"""
    from tests import max_direct_cases as C

    s, n = c.run(t, row)
    bags, g, a = c.pairs[s:s + n, 2], c.grads[t], c.args[t]
    total, won = np.zeros(c.dims[t], np.float32), np.zeros(c.dims[t], bool)
    for p0 in range(0, n, C.PIECE):
        acc, has = np.zeros(c.dims[t], np.float32), np.zeros(c.dims[t], bool)
        for k in range(p0, min(p0 + C.PIECE, n)):
            if k and bags[k - 1] == bags[k] and not (mistake == "repeat" and k == p0):
                continue
            hit = a[bags[k]] == row
            acc = np.where(hit, np.where(has, acc + g[bags[k]], g[bags[k]]), acc)
            has |= hit
        start = won | (mistake == "combine")
        total = np.where(has, np.where(start, total + acc, acc), total)
        won |= has
    return total, won


def test_constructed_requests_hold_their_claims_and_discriminate():
    from tests import max_direct_cases as C

    cases = {"repeat100": C.repeat(263), "repeat768": C.repeat(85), "nothing": C.nothing(), "far": C.far(), "zero": C.zero(), "sliced": C.sliced(),
             "mixed": C.mixed()}      # (the builders assert the sorted positions and run lengths they are named for)
    for name, c in cases.items():
        b0, nb = c.slice
        res = R.sums(C.ROWS, c.dims, c.idx, c.off, c.B, c.grads, c.args, b0, nb)
        for (t, row), n in c.hot().items():
            assert (res[t][4][row] <= n).all()
            right = _wrong(c, t, row, None)                          # the helper with no mistake is the rule
            assert np.array_equal(M.bits(right[0][right[1]]), M.bits(res[t][0][row][right[1]])) and np.array_equal(right[1], res[t][1][row]), name
    # a repeat across a piece cut, inside a tile and on a tile border: counting it twice changes bits in every column
    for c in (C.repeat(263), C.repeat(85)):
        s, _ = c.run(1, 7)
        assert [(s + k) % C.PIECE == s % C.PIECE for k in c.repeats(1, 7)] == [True, True]
        G = R.sums(C.ROWS, c.dims, c.idx, c.off, c.B, c.grads, c.args)[1][0][7]
        assert (M.bits(_wrong(c, 1, 7, "repeat")[0]) != M.bits(G)).all()
    assert (C.repeat(85).run(1, 7)[0] + 256) % C.TILE == 0 and (C.repeat(263).run(1, 7)[0] + 256) % C.TILE == 356
    # pieces that win nothing: a combine that starts from +0.0 gives +0.0 where the rule gives -0.0 (column 0); every other column has the
    # same bits under both (x + 0.0 == x unless x is -0.0), so the difference shows in a destination that holds -0.0 and nowhere else
    c = C.nothing()
    G, won = R.sums(C.ROWS, c.dims, c.idx, c.off, c.B, c.grads, c.args)[1][:2]
    bad = _wrong(c, 1, 7, "combine")[0]
    assert M.bits(G[7])[0] == 0x80000000 and M.bits(bad)[0] == 0 and np.array_equal(M.bits(G[7])[1:], M.bits(bad)[1:]) and won[7, :7].all() and not won[7, 7]
    dst = np.full((1, 8), 0x80000000, np.uint32)
    assert R.apply(dst, "f32", G[7:8], won[7:8], -0.5)[0, 0] == 0 and R.apply(dst, "f32", bad[None], won[7:8], -0.5)[0, 0] == 0x80000000
    assert not R.sums(C.ROWS, c.dims, c.idx, c.off, c.B, c.grads, c.args)[2][1][3].any()
