"""The update paths of 16-bit tables on a real MI355X against the C oracle: fused row-wise Adagrad on bf16 / fp16 tables with the
round-to-nearest store (B1) and with the stochastic store (B3), and the in-place scatter-add into fp16 tables (B2).

Bars (tests/lowp_rules.py says where each number comes from):
  * Adagrad, round to nearest: every element of every touched row lies within ``ulp16(w_pre) / 2 + b`` of the oracle's fp32 value
    before rounding, ``b = 2e-5 * |w_pre| + 2e-6`` (scale-free form for the small-valued tables); rows looked up more than 256
    times are held to the fuzz test's derived bound instead of b.  State: ``allclose(rtol=2e-5, atol=1e-12)``.  Untouched rows
    and their state keep their bits, a second module fed the same steps ends bit-identical.
  * every step is judged on its own: the oracle starts from the bits and the state the DEVICE held before the step.  A stored
    16-bit value may legitimately differ from the oracle's by one spacing where the fp32 values straddle a midpoint; carried
    into the next step such a difference is no longer an error of that step.
  * fp16 scatter-add: bit-equal to ``bwd_f16`` on rows with at most 256 lookups.
  * stochastic store: both neighbours only, round-up frequency calibrated in ten bins of the position between the neighbours,
    decisions of a column pair and of two steps uncorrelated, same step reproducible.
"""
import numpy as np
import pytest
import torch

from oracle import embbag_oracle as O
from tests import lowp_rules as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CODE = {torch.bfloat16: O.BF16, torch.float16: O.F16}
WD = {None: 0, "l2": 1, "decouple": 2}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    import param_amd

    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    param_amd.load_library()  # raises loudly if libparam_amd.so is missing: no fallback
    yield


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).copy()


def _widen(bits, code):
    return (O.bf16_bits_to_f32 if code == O.BF16 else O.f16_bits_to_f32)(bits)


def _request(rng, rows, B, spec):
    """TBE request on the host (int64, offsets [T*B+1]).  spec[t]: ("fixed", L) | ("ragged", L) -- 0 .. 2L lookups per bag, an
    eighth of the bags empty | ("empty",) -- a table nobody looks up | ("hot", L, row, n) -- fixed L with n lookups of one row
    spread over the bags | ("zipf", L, alpha) -- the benchmark's skew model, duplicates kept"""
    from param_amd.indices import zipf_indices

    lens, parts = [], []
    for t, (kind, *a) in enumerate(spec):
        if kind == "empty":
            ln = np.zeros(B, np.int64)
        elif kind == "ragged":
            ln = rng.integers(0, 2 * a[0] + 1, size=B)
            ln[rng.integers(0, B, size=max(1, B // 8))] = 0
        else:
            ln = np.full(B, a[0], np.int64)
        n = int(ln.sum())
        if kind == "zipf":
            ix = zipf_indices(a[1], rows[t], n, 1, dedupe=False, generator=torch.Generator().manual_seed(int(rng.integers(1 << 30)))).numpy()
        else:
            ix = rng.integers(0, rows[t], size=n)
        if kind == "hot":
            ix[rng.permutation(n)[:a[2]]] = a[1]
        lens.append(ln)
        parts.append(ix.astype(np.int64))
    off = np.zeros(len(rows) * B + 1, np.int64)
    off[1:] = np.cumsum(np.concatenate(lens))
    return np.concatenate(parts), off


def _table_grad(grad, t, m, B):
    """[B, D_t] gradient rows of table t for the module's layout"""
    if m.layout == "bd":
        c0 = sum(m.dims[:t])
        return grad[:, c0:c0 + m.dims[t]]
    if m.layout == "tbd":
        return grad[t]
    return grad[:, t].reshape(B, m.dims[t])


def _grad_shape(m, B):
    if m.layout == "bd":
        return (B, sum(m.dims))
    if m.layout == "tbd":
        return (len(m.rows), B, m.dims[0])
    return (B // m.block_bags, len(m.rows), m.block_bags, m.dims[0])


def _module(rows, dims, dtype, W_bits, **kw):
    """a module whose tables hold exactly the given bit patterns (host-made: every input of a case is reproducible off the device)"""
    from param_amd import BatchedEmbeddingBagMI355

    m = BatchedEmbeddingBagMI355(rows, dims, dtype=dtype, device=DEV, init=None, **kw)
    for t, b in enumerate(W_bits):
        m.table(t).view(torch.int16).copy_(_t(b.view(np.int16)))
    return m


def _init_bits(rng, rows, dims, dtype, scale=1.0):
    return [_bits(torch.from_numpy((rng.standard_normal((r, d)) * scale).astype(np.float32)).to(dtype)) for r, d in zip(rows, dims)]


def check_adagrad_step(coracle, m, before, grad_h, idx_h, off_h, psw_h, B, scale_free=False, tag=None):
    """One round-to-nearest Adagrad step of module ``m`` against the oracle started from ``before`` = [(table bits, state)] as the
    device held them.  Returns the number of elements checked under the cold rule and under the hot-row rule."""
    code = CODE[m.weights.dtype]
    lr, eps, wd, mode = m.learning_rate, m.eps, m.weight_decay, WD[m.weight_decay_mode]
    n_cold = n_hot = 0
    for t in range(len(m.rows)):
        s, e = off_h[t * B], off_h[(t + 1) * B]
        loc = off_h[t * B:(t + 1) * B] - s
        it = idx_h[s:e]
        g = np.ascontiguousarray(_table_grad(grad_h, t, m, B))
        pw = None if psw_h is None else psw_h[s:e]
        old_bits, old_mom = before[t]
        exp_bits, exp_mom = old_bits.copy(), old_mom.copy()
        _, _, w_pre = coracle.bwd_rowwise_adagrad(exp_bits, exp_mom, it, loc, g, pw, lr=lr, eps=eps, weight_decay=wd,
                                                  weight_decay_mode=mode, dtype=code)
        got_bits, gm = _bits(m.table(t)), m.momentum_table(t).cpu().numpy()
        cnt = np.bincount(it, minlength=m.rows[t])
        touched, hot = cnt > 0, cnt > R.EXACT_RUN
        cold = touched & ~hot
        assert np.array_equal(got_bits[~touched], old_bits[~touched]) and np.array_equal(gm[~touched], old_mom[~touched]), (tag, t)
        got, w_old, wp = _widen(got_bits, code).astype(np.float64), _widen(old_bits, code).astype(np.float64), w_pre.astype(np.float64)
        assert np.isfinite(got[touched]).all(), (tag, t)
        b = R.tol_b(wp, w_old if scale_free else None)
        ratio = R.nearest_ratio(got[cold], wp[cold], code, b[cold])
        assert ratio.size == 0 or ratio.max() <= 1.0, (tag, t, "worst |got - w_pre| / (ulp / 2 + b)", float(ratio.max()))
        assert np.allclose(gm, exp_mom, rtol=2e-5, atol=1e-12), (tag, t, "state")
        n_cold += int(cold.sum()) * m.dims[t]
        if hot.any():
            # the gradient sum of such a row is formed from ordered chunk partials: bound derived from an fp64 evaluation, plus
            # half a spacing for the store
            assert not scale_free
            W64, m64, bound_w, bound_m = R.adagrad_fp64(w_old, old_mom, it, loc, g, pw, lr, eps, wd, mode)
            lim = bound_w + 3e-5 * np.abs(W64) + 3e-6 + O.ulp16(W64, code) / 2
            assert (np.abs(got[hot] - W64[hot]) <= lim[hot]).all(), (tag, t, "hot rows")
            assert (np.abs(gm[hot] - m64[hot]) <= bound_m[hot] + 3e-5 * m64[hot] + 1e-10).all(), (tag, t, "hot rows, state")
            n_hot += int(hot.sum()) * m.dims[t]
    return n_cold, n_hot


def run_adagrad_case(coracle, dtype, rows, dims, spec, B, *, layout="bd", idt=torch.int64, weighted=False, wd_mode=None, lr=0.05,
                     scale=1.0, seed=0, block_bags=None, steps=2, tag=None):
    rng = np.random.default_rng(seed)
    dims_l = [dims] * len(rows) if isinstance(dims, int) else list(dims)
    W0 = _init_bits(rng, rows, dims_l, dtype, scale)
    kw = dict(layout=layout, learning_rate=lr, optimizer="rowwise_adagrad", eps=1e-6 if scale == 1.0 else 1e-8, block_bags=block_bags,
              weight_decay=0.02 if wd_mode else 0.0, weight_decay_mode=wd_mode)
    ma, mb = _module(rows, dims_l, dtype, W0, **kw), _module(rows, dims_l, dtype, W0, **kw)
    checked = [0, 0]
    for step in range(steps):
        idx_h, off_h = _request(rng, rows, B, spec)
        psw_h = rng.standard_normal(len(idx_h)).astype(np.float32) if weighted else None          # both signs
        grad_h = rng.standard_normal(_grad_shape(ma, B)).astype(np.float32)
        before = [(_bits(ma.table(t)), ma.momentum_table(t).cpu().numpy().copy()) for t in range(len(rows))]
        for m in (ma, mb):
            m.adagrad_step_(_t(grad_h), _t(idx_h, idt), _t(off_h, idt), None if psw_h is None else _t(psw_h), batch=B)
        c, h = check_adagrad_step(coracle, ma, before, grad_h, idx_h, off_h, psw_h, B, scale_free=scale != 1.0, tag=(tag, step))
        checked[0] += c
        checked[1] += h
        if step == 1:
            assert any(mom.any() for _, mom in before)                       # the second step started from a non-zero state
    # (table by table: the slab's padding between tables is never written)
    assert all(np.array_equal(_bits(ma.table(t)), _bits(mb.table(t))) for t in range(len(rows))) and torch.equal(ma.momentum, mb.momentum), tag
    return checked


# ----------------------------------------------------------------------------- B1. Adagrad, round to nearest
MIXED = ([3000, 500, 40, 2000], [16, 32, 64, 128])
ADAGRAD_CASES = {
    # name: (rows, dims, request spec per table, B, keyword arguments)
    "mixed_ragged_weighted_i32": (*MIXED, [("ragged", 6), ("ragged", 3), ("empty",), ("ragged", 10)], 256,
                                  dict(idt=torch.int32, weighted=True)),
    "mixed_ragged_weighted_l2": (*MIXED, [("ragged", 6), ("ragged", 3), ("empty",), ("ragged", 10)], 256,
                                 dict(weighted=True, wd_mode="l2")),
    "mixed_fixed_decouple": (*MIXED, [("fixed", 4), ("hot", 5, 11, 400), ("fixed", 1), ("fixed", 8)], 256, dict(wd_mode="decouple")),
    "tbd_zipf_hot": ([50000, 3000, 700], 64, [("zipf", 10, 1.2), ("hot", 6, 3, 450), ("empty",)], 512, dict(layout="tbd", wd_mode="decouple")),
    "tbd_ragged_weighted_i32_l2": ([1000, 1000, 1000], 32, [("ragged", 5), ("empty",), ("ragged", 9)], 192,
                                   dict(layout="tbd", idt=torch.int32, weighted=True, wd_mode="l2")),
    "blocked_hot": ([1500, 700, 90], 64, [("fixed", 7), ("hot", 4, 5, 300), ("fixed", 2)], 256, dict(layout="blocked", block_bags=64)),
    "blocked_ragged_weighted_i32": ([1500, 700, 90, 300], 24, [("ragged", 4), ("ragged", 8), ("empty",), ("ragged", 2)], 128,
                                    dict(layout="blocked", block_bags=32, idt=torch.int32, weighted=True, wd_mode="l2")),
    # values AND results below fp16's normal range (2^-14 = 6.1e-5): the Adagrad step is about lr in size whatever the weights are
    "small_values": ([3000, 600], [64, 128], [("ragged", 6), ("fixed", 9)], 256, dict(scale=1e-5, lr=1e-6)),
    "small_values_weighted_decouple": ([2000, 50], 32, [("ragged", 8), ("empty",)], 256,
                                       dict(scale=1e-5, lr=1e-6, weighted=True, wd_mode="decouple", idt=torch.int32)),
}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("case", sorted(ADAGRAD_CASES))
def test_adagrad_16bit_tables_vs_oracle(coracle, case, dtype):
    rows, dims, spec, B, kw = ADAGRAD_CASES[case]
    cold, hot = run_adagrad_case(coracle, dtype, rows, dims, spec, B, seed=sorted(ADAGRAD_CASES).index(case), tag=case, **kw)
    assert cold > 10000 and (hot > 0) == any(s[0] == "hot" for s in spec), (cold, hot)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("D", [8, 24, 56, 64, 128, 256, 512])
def test_adagrad_16bit_tables_every_dim(coracle, D, dtype):
    """one common dim per case (lane groups with idle lanes: 24, 56), a hot row (chunk-partial path), weight decay modes and index
    types taking turns"""
    k = [8, 24, 56, 64, 128, 256, 512].index(D)
    cold, hot = run_adagrad_case(coracle, dtype, [2000, 300], D, [("hot", 8, 7, 300), ("ragged", 5)], 128, seed=100 + k,
                                 idt=(torch.int64, torch.int32)[k % 2], weighted=k % 3 == 1, wd_mode=(None, "l2", "decouple")[k % 3],
                                 tag=D)
    assert cold > 10000 and hot == 2 * D


def test_small_valued_case_is_below_the_fp16_normal_range(coracle):
    """the inputs of the small-valued cases do what their name says: old values and fp32 results mostly in 2^-24 .. 2^-14"""
    rng = np.random.default_rng(sorted(ADAGRAD_CASES).index("small_values"))
    rows, dims, spec, B, kw = ADAGRAD_CASES["small_values"]
    W0 = _init_bits(rng, rows, dims, torch.float16, kw["scale"])
    idx_h, off_h = _request(rng, rows, B, spec)
    grad_h = rng.standard_normal((B, sum(dims))).astype(np.float32)
    s, e = off_h[0], off_h[B]
    bits, mom = W0[0].copy(), np.zeros(rows[0], np.float32)
    _, _, w_pre = coracle.bwd_rowwise_adagrad(bits, mom, idx_h[s:e], off_h[:B], grad_h[:, :dims[0]].copy(), None, lr=kw["lr"], eps=1e-8,
                                              dtype=O.F16)
    touched = np.bincount(idx_h[s:e], minlength=rows[0]) > 0
    for v in (O.f16_bits_to_f32(W0[0])[touched], w_pre[touched]):
        a = np.abs(v)
        assert ((a < 2.0 ** -14) & (a >= 2.0 ** -24)).mean() > 0.9


# ----------------------------------------------------------------------------- B2. fp16 in-place scatter-add
def _check_scatter_f16(coracle, m, before_bits, grad_h, idx_h, off_h, psw_h, B, alpha, b0=0, b1=None, tag=None):
    """bag slice [b0, b1) of the request applied to fp16 tables: rows with at most 256 lookups bit-equal to the oracle, hotter rows
    within the sorted backward's bound for ordered chunk partials (tests/test_gpu_fuzz.py) plus half a spacing.  Returns the
    expected bits (for a following slice)."""
    b1 = B if b1 is None else b1
    exp_all = []
    for t in range(len(m.rows)):
        s, e = off_h[t * B + b0], off_h[t * B + b1]
        loc = off_h[t * B + b0:t * B + b1] - s
        it = idx_h[s:e]
        g = np.ascontiguousarray(_table_grad(grad_h, t, m, B)[b0:b1])
        pw = None if psw_h is None else psw_h[s:e]
        exp = coracle.bwd_f16(before_bits[t].copy(), it, loc, g, pw, alpha=alpha)
        got = _bits(m.table(t))
        cnt = np.bincount(it, minlength=m.rows[t])
        cold = cnt <= R.EXACT_RUN
        assert np.array_equal(got[cold], exp[cold]), (tag, t)
        if (~cold).any():
            hot = ~cold
            start, end = O.bag_bounds(loc, b1 - b0, e - s)
            bag_of = np.repeat(np.arange(b1 - b0), end - start)
            contrib = alpha * g.astype(np.float64)[bag_of] * (1.0 if pw is None else pw.astype(np.float64)[:, None])
            w_old = O.f16_bits_to_f32(before_bits[t]).astype(np.float64)
            truth, mag = w_old.copy(), np.abs(w_old)
            np.add.at(truth, it, contrib)
            np.add.at(mag, it, np.abs(contrib))
            tol = np.maximum(1e-5, (256 + cnt[:, None] / 32) * 2.0 ** -24) * mag + O.ulp16(truth, O.F16) / 2
            assert (np.abs(O.f16_bits_to_f32(got).astype(np.float64) - truth)[hot] <= tol[hot]).all(), (tag, t, "hot rows")
            exp[hot] = got[hot]
        exp_all.append(exp)
    return exp_all


@pytest.mark.parametrize("D", [8, 64, 128, 512])
def test_fp16_scatter_add_vs_oracle(coracle, D):
    k = [8, 64, 128, 512].index(D)
    rng = np.random.default_rng(200 + k)
    rows, B, weighted = [1500, 400, 60], 192, k % 2 == 0
    W0 = _init_bits(rng, rows, [D] * 3, torch.float16)
    m = _module(rows, D, torch.float16, W0, fused_update=False)
    idx_h, off_h = _request(rng, rows, B, [("ragged", 6), ("hot", 5, 9, 330), ("empty",)])
    psw_h = rng.standard_normal(len(idx_h)).astype(np.float32) if weighted else None
    grad_h = rng.standard_normal((B, 3 * D)).astype(np.float32)
    idt = (torch.int64, torch.int32)[k % 2]
    m.scatter_add_(_t(grad_h), _t(idx_h, idt), _t(off_h, idt), alpha=-0.125, per_sample_weights=None if psw_h is None else _t(psw_h), batch=B)
    exp = _check_scatter_f16(coracle, m, W0, grad_h, idx_h, off_h, psw_h, B, -0.125, tag=D)
    assert not np.array_equal(exp[0], W0[0]) and np.array_equal(exp[2], W0[2])


@pytest.mark.parametrize("layout", ["bd", "tbd"])
def test_fp16_scatter_add_two_batch_slices(coracle, layout):
    """a batch applied as two bag_begin / bag_count slices: two updates, each rounded once (the second starts from the first's bits)"""
    rng = np.random.default_rng(210 + (layout == "tbd"))
    rows, D, B, cut = [900, 2500], 64, 160, 57
    W0 = _init_bits(rng, rows, [D, D], torch.float16)
    m = _module(rows, D, torch.float16, W0, fused_update=False, layout=layout)
    idx_h, off_h = _request(rng, rows, B, [("ragged", 7), ("fixed", 3)])
    psw_h = rng.standard_normal(len(idx_h)).astype(np.float32)
    grad_h = rng.standard_normal(_grad_shape(m, B)).astype(np.float32)
    args = (_t(grad_h), _t(idx_h), _t(off_h))
    m.scatter_add_(*args, alpha=0.25, per_sample_weights=_t(psw_h), batch=B, bag_begin=0, bag_count=cut)
    mid = _check_scatter_f16(coracle, m, W0, grad_h, idx_h, off_h, psw_h, B, 0.25, 0, cut, tag=(layout, 0))
    m.scatter_add_(*args, alpha=0.25, per_sample_weights=_t(psw_h), batch=B, bag_begin=cut, bag_count=B - cut)
    _check_scatter_f16(coracle, m, mid, grad_h, idx_h, off_h, psw_h, B, 0.25, cut, B, tag=(layout, 1))


def test_fp16_scatter_add_subnormal_results_and_overflow(coracle):
    """results that land below fp16's normal range are rounded on the subnormal grid, results beyond 65504 become +-Inf, as the
    oracle's software conversion does"""
    rng = np.random.default_rng(220)
    rows, D, B = [800, 800], 64, 128
    small = _init_bits(rng, [rows[0]], [D], torch.float16, 1e-5)[0]
    big = _bits(torch.from_numpy((rng.choice([-1.0, 1.0], (rows[1], D)) * rng.uniform(55000, 65504, (rows[1], D))).astype(np.float32)).to(torch.float16))
    # one request per regime (alpha is per call): table 1 / table 0 has no lookups in the other's call
    for which, alpha in ((0, -1e-6), (1, 3000.0)):
        m = _module(rows, D, torch.float16, [small, big], fused_update=False)
        spec = [("ragged", 5), ("empty",)] if which == 0 else [("empty",), ("ragged", 5)]
        idx_h, off_h = _request(rng, rows, B, spec)
        grad_h = rng.standard_normal((B, 2 * D)).astype(np.float32)
        m.scatter_add_(_t(grad_h), _t(idx_h), _t(off_h), alpha=alpha, batch=B)
        exp = _check_scatter_f16(coracle, m, [small, big], grad_h, idx_h, off_h, None, B, alpha, tag=which)
        v = O.f16_bits_to_f32(exp[which])
        changed = exp[which] != (small, big)[which]
        if which == 0:
            a = np.abs(v[changed])
            assert changed.mean() > 0.3 and ((a < 2.0 ** -14) & (a > 0)).mean() > 0.9
        else:
            assert np.isinf(v).sum() > 1000 and (v == np.inf).any() and (v == -np.inf).any() and not np.isnan(v).any()


# ----------------------------------------------------------------------------- B3. the stochastic store
SR_ROWS, SR_DIMS, SR_B = [4000, 3000, 50, 2000], [64, 32, 16, 128], 1024
SR_SPEC = [("ragged", 8), ("ragged", 6), ("empty",), ("ragged", 5)]


def _sr_run(coracle, dtype, rows, dims, spec, B, *, scale=1.0, lr=0.05, seed=300, sr_step=0, weighted=True, wd_mode="l2"):
    """one stochastic Adagrad step on host-made inputs -> (stored values, w_pre, b, column index) over the touched elements, fp64,
    tables concatenated; plus the raw table bits"""
    rng = np.random.default_rng(seed)
    W0 = _init_bits(rng, rows, dims, dtype, scale)
    m = _module(rows, dims, dtype, W0, learning_rate=lr, optimizer="rowwise_adagrad", eps=1e-6 if scale == 1.0 else 1e-8,
                weight_decay=0.02 if wd_mode else 0.0, weight_decay_mode=wd_mode, stochastic_rounding=True)
    m._sr_step = sr_step
    idx_h, off_h = _request(rng, rows, B, spec)
    psw_h = rng.standard_normal(len(idx_h)).astype(np.float32) if weighted else None
    grad_h = rng.standard_normal((B, sum(dims))).astype(np.float32)
    m.adagrad_step_(_t(grad_h), _t(idx_h), _t(off_h), None if psw_h is None else _t(psw_h), batch=B)
    code = CODE[dtype]
    got, pre, bb, col, raw = [], [], [], [], []
    for t in range(len(rows)):
        s, e = off_h[t * B], off_h[(t + 1) * B]
        it = idx_h[s:e]
        cnt = np.bincount(it, minlength=rows[t])
        assert cnt.max(initial=0) <= R.EXACT_RUN                               # every row in the oracle's own summation order
        bits, mom = W0[t].copy(), np.zeros(rows[t], np.float32)
        _, _, w_pre = coracle.bwd_rowwise_adagrad(bits, mom, it, off_h[t * B:(t + 1) * B] - s, np.ascontiguousarray(_table_grad(grad_h, t, m, B)),
                                                  None if psw_h is None else psw_h[s:e], lr=lr, eps=m.eps, weight_decay=m.weight_decay,
                                                  weight_decay_mode=WD[wd_mode], dtype=code)
        tb = _bits(m.table(t))
        raw.append(tb)
        touched = cnt > 0
        assert np.array_equal(tb[~touched], W0[t][~touched])
        assert np.allclose(m.momentum_table(t).cpu().numpy(), mom, rtol=2e-5, atol=1e-12)
        wp, w_old = w_pre[touched].astype(np.float64), _widen(W0[t], code)[touched].astype(np.float64)
        got.append(_widen(tb, code)[touched].astype(np.float64).ravel())
        pre.append(wp.ravel())
        bb.append(R.tol_b(wp, w_old if scale != 1.0 else None).ravel())
        col.append(np.broadcast_to(np.arange(dims[t]), wp.shape).ravel())
    return np.concatenate(got), np.concatenate(pre), np.concatenate(bb), np.concatenate(col), raw


def _assert_calibrated(p, up, slack, tag):
    rows = R.calibration(p, up, slack)
    table = R.calibration_table(rows)
    print(f"\n{tag}: {p.size} elements\n{table}")
    assert all(n > 0 and abs(o - e) <= lim for n, e, o, lim in rows), f"{tag}\n{table}"


@pytest.mark.parametrize("dtype,cap", [(torch.bfloat16, 0.05), (torch.float16, 0.15)], ids=["bf16", "f16"])
def test_stochastic_rounding_neighbours_calibration_independence(coracle, dtype, cap):
    """General inputs (mixed dims, ragged bags, signed per-sample weights, L2 weight decay, a table nobody looks up), every touched
    row at most 256 lookups.  Share of elements the calibration drops because the oracle's w_pre lies within b of a grid value
    (a property of these inputs, computed from the oracle alone; caps 5 % / 15 %): bf16 1.2 %, fp16 8.9 %."""
    code = CODE[dtype]
    got, wp, b, col, raw = _sr_run(coracle, dtype, SR_ROWS, SR_DIMS, SR_SPEC, SR_B)
    assert got.size >= 200000
    p, slack, up, inside = R.round_up_stats(got, wp, code, b)
    assert inside.all(), (int((~inside).sum()), "stored values that are no neighbour of w_pre")
    keep = (p > slack) & (p < 1 - slack)
    print(f"\ndropped by the calibration: {1 - keep.mean():.4f}")
    assert 1 - keep.mean() <= cap
    _assert_calibrated(p[keep], up[keep], slack[keep], f"{dtype} calibration")
    # the two elements of a column pair share one 32-bit draw (its low and its high half): their decisions are independent
    c = up.astype(np.float64) - p
    even = np.flatnonzero((col % 2 == 0))
    even = even[keep[even] & keep[even + 1]]                                    # (rows are whole and dims even: even + 1 is the pair's other column)
    assert (col[even + 1] == col[even] + 1).all() and even.size > 50000
    r_pair = R.correlation(c[even], c[even + 1])
    # a new step gives new decisions; the same step the same bits
    got2, wp2, _, _, raw2 = _sr_run(coracle, dtype, SR_ROWS, SR_DIMS, SR_SPEC, SR_B, sr_step=1)
    assert np.array_equal(wp2, wp)
    _, _, up2, inside2 = R.round_up_stats(got2, wp, code, b)
    assert inside2.all()
    r_step = R.correlation(c[keep], (up2.astype(np.float64) - p)[keep])
    print(f"correlation within a column pair {r_pair:+.4f} (limit {5 / np.sqrt(even.size):.4f}), between two steps {r_step:+.4f} "
          f"(limit {5 / np.sqrt(keep.sum()):.4f})")
    assert abs(r_pair) <= 5 / np.sqrt(even.size) and abs(r_step) <= 5 / np.sqrt(keep.sum())
    assert (up2 != up)[keep].mean() > 0.1
    *_, raw3 = _sr_run(coracle, dtype, SR_ROWS, SR_DIMS, SR_SPEC, SR_B)
    assert all(np.array_equal(x, y) for x, y in zip(raw, raw3))


def test_stochastic_rounding_fp16_below_the_normal_range(coracle):
    """fp16 values and results in 2^-24 .. 2^-14, where the grid has the one spacing 2^-24 (a fifth of a DLRM-initialised 10 M-row
    table lies there).  Before the fix of f32_to_f16_sr (random bits added, low bits cleared, then a conversion that rounds to
    NEAREST where it is inexact) the ten bins read 0.0001 0.0003 0.0041 0.0305 0.2044 0.7969 0.9674 0.9963 0.9997 0.9999 on an
    MI355X against expected 0.05 .. 0.95: round-to-nearest in all but name."""
    got, wp, b, _, _ = _sr_run(coracle, torch.float16, [4000, 1500], [64, 32], [("ragged", 8), ("fixed", 4)], SR_B, scale=1e-5, lr=1e-6,
                               seed=310, wd_mode="decouple")
    p, slack, up, inside = R.round_up_stats(got, wp, O.F16, b)
    assert inside.all(), int((~inside).sum())
    sub = np.abs(wp) < 2.0 ** -14
    assert sub.mean() > 0.9 and sub.sum() >= 200000
    keep = sub & (p > slack) & (p < 1 - slack)
    assert 1 - keep.sum() / sub.sum() <= 0.15
    _assert_calibrated(p[keep], up[keep], slack[keep], "fp16 below 2^-14")
