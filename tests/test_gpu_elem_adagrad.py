"""Fused exact element-wise Adagrad (``optimizer="adagrad"``, C calls ``pm_embbag_bwd_*_adagrad_elem``) on a real MI355X.

What is pinned to what (tests/elem_adagrad_rules.py says where each number comes from):
  * NONE and L2 weight decay: to ``torch.optim.Adagrad`` on the CPU (a real third-party implementation), three fused steps, general
    columns, mixed dims; and to the numpy restatement that tests/test_elem_adagrad_host.py pins to torch, for general gradients.
    Bars: state ``rtol 1e-6``, weights ``rtol 2e-6, atol 1e-7``; rows looked up more than 256 times add the first-order bound of
    a gradient sum formed in another order.
  * DECOUPLE and the stochastic store: restated only -- no third-party implementation of either is at hand.
  * 16-bit tables, round to nearest: ``lowp_rules.nearest_ratio <= 1`` with ``lowp_rules.tol_b``.
  * sorted / presorted / hybrid bag-major / LDS left-over paths: the same bits.
"""
import numpy as np
import pytest
import torch

from oracle import embbag_oracle as O
from tests import elem_adagrad_rules as E
from tests import lowp_rules as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CODE = {torch.bfloat16: O.BF16, torch.float16: O.F16}
WD = {None: E.WD_NONE, "l2": E.WD_L2, "decouple": E.WD_DECOUPLE}


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


def _module(rows, dims, dtype=torch.float32, W=None, **kw):
    """a module whose tables hold exactly the given values (fp32 arrays, or uint16 bit patterns for 16-bit tables)"""
    from param_amd import BatchedEmbeddingBagMI355

    kw.setdefault("optimizer", "adagrad")
    m = BatchedEmbeddingBagMI355(rows, dims, dtype=dtype, device=DEV, init=None if W is not None else "normal", **kw)
    if W is not None:
        for t, w in enumerate(W):
            if dtype == torch.float32:
                m.table(t).copy_(_t(w))
            else:
                m.table(t).view(torch.int16).copy_(_t(w.view(np.int16)))
    return m


def _request(rng, rows, B, spec):
    """TBE request on the host (int64, offsets [T*B+1]).  spec[t]: ("fixed", L) | ("ragged", L) -- 0 .. 2L lookups per bag, an
    eighth of the bags empty | ("empty",) | ("hot", L, row, n) -- fixed L with n lookups of one row spread over the bags |
    ("zipf", L) -- Zipf(1.4) duplicates, the table's last five rows never hit"""
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
            ix = np.minimum(rng.zipf(1.4, n) - 1, rows[t] - 6)
        else:
            ix = rng.integers(0, rows[t], size=n)
        if kind == "hot":
            ix[rng.permutation(n)[:a[2]]] = a[1]
        lens.append(ln)
        parts.append(ix.astype(np.int64))
    off = np.zeros(len(rows) * B + 1, np.int64)
    off[1:] = np.cumsum(np.concatenate(lens))
    return np.concatenate(parts), off


def _table_slice(idx_h, off_h, t, B):
    s, e = off_h[t * B], off_h[(t + 1) * B]
    return idx_h[s:e], off_h[t * B:(t + 1) * B] - s, s, e


def _tables_f32(m):
    return [m.table(t).float().cpu().numpy().copy() for t in range(len(m.rows))]


def _state(m):
    return [m.momentum_table(t).cpu().numpy().copy() for t in range(len(m.rows))]


# ----------------------------------------------------------------------------- 1. the torch pin on the device
@pytest.mark.parametrize("wd_mode,wd", [(None, 0.0), ("l2", 0.01)], ids=["none", "l2"])
def test_three_fused_steps_equal_torch_adagrad(wd_mode, wd):
    """Two tables of different widths (16 and 64: the mixed-dim launch), general columns, Zipf(1.4) duplicates, dyadic bag
    gradients (per-row sums exact in any order), the last five rows never hit.  torch.optim.Adagrad on the CPU is fed the summed
    gradients of the touched rows (state injected through ``opt.state[p]["sum"]``, so that L2 decay reaches touched rows only)."""
    rng = np.random.default_rng(21)
    rows, dims, B, L, lr, eps = [300, 50], [16, 64], 64, 5, 0.05, 1e-6
    W0 = [rng.standard_normal((r, d)).astype(np.float32) for r, d in zip(rows, dims)]
    m = _module(rows, dims, W=W0, learning_rate=lr, eps=eps, weight_decay=wd, weight_decay_mode=wd_mode)
    Wt, St = [w.copy() for w in W0], [np.zeros_like(w) for w in W0]
    most = 0
    for step in range(3):
        idx_h, off_h = _request(rng, rows, B, [("zipf", L), ("zipf", L)])
        g_h = (rng.integers(-8, 9, (B, sum(dims))) / 4.0).astype(np.float32)
        m.adagrad_step_(_t(g_h), _t(idx_h), _t(off_h))
        for t, (r, d) in enumerate(zip(rows, dims)):
            it, loc, _, _ = _table_slice(idx_h, off_h, t, B)
            c0 = sum(dims[:t])
            G = np.zeros((r, d), np.float32)
            np.add.at(G, it, g_h[np.repeat(np.arange(B), L), c0:c0 + d])
            hit = np.unique(it)
            most = max(most, int(np.bincount(it).max()))
            p = torch.nn.Parameter(torch.from_numpy(Wt[t][hit].copy()))
            opt = torch.optim.Adagrad([p], lr=lr, eps=eps, initial_accumulator_value=0.0, lr_decay=0.0, weight_decay=wd)
            opt.state[p]["sum"] = torch.from_numpy(St[t][hit].copy())
            p.grad = torch.from_numpy(G[hit].copy())
            opt.step()
            Wt[t][hit], St[t][hit] = p.detach().numpy(), opt.state[p]["sum"].numpy()
    assert most >= 30
    for t in range(2):
        gw, gs = m.table(t).cpu().numpy(), m.momentum_table(t).cpu().numpy()
        ds = np.abs(gs - St[t]) / np.maximum(np.abs(St[t]), 1e-30)
        dw = np.abs(gw - Wt[t]) / (E.W_RTOL * np.abs(Wt[t]) + E.W_ATOL)
        print(f"{wd_mode} table {t}: state max rel diff {ds.max():.3g} (bar {E.STATE_RTOL}), weights max diff / bar {dw.max():.3g}")
        assert np.allclose(gs, St[t], rtol=E.STATE_RTOL, atol=0), t
        assert np.allclose(gw, Wt[t], rtol=E.W_RTOL, atol=E.W_ATOL), t
        assert np.array_equal(gw[-5:], W0[t][-5:]) and not gs[-5:].any()
        assert (gs[:5] > 0).any() and not np.array_equal(gw[:5], W0[t][:5])


# ----------------------------------------------------------------------------- 2. general gradients, fp32 tables
def _check_step_f32(m, before, g_h, idx_h, off_h, psw_h, B, tag, fp64_only=False):
    """one step of fp32-table module ``m`` started from ``before`` = (tables, states) as the device held them.  Rows looked up at
    most 256 times: the fp32 restatement applied to the sequential fp32 gradient sum, at the torch pin's bars.  Hotter rows (and
    every row when ``fp64_only``): the fp64 restatement with the first-order bound of a sum formed in another order.
    Returns (elements under the cold rule, under the hot rule)."""
    lr, eps, wd, code = m.learning_rate, m.eps, m.weight_decay, WD[m.weight_decay_mode]
    n_cold = n_hot = 0
    got_w, got_s = _tables_f32(m), _state(m)
    for t, (r, d) in enumerate(zip(m.rows, m.dims)):
        it, loc, s, e = _table_slice(idx_h, off_h, t, B)
        c0 = sum(m.dims[:t])
        g = np.ascontiguousarray(g_h[:, c0:c0 + d])
        pw = None if psw_h is None else psw_h[s:e]
        w_old, s_old = before[0][t], before[1][t]
        W64, S64, dw, ds, count = E.step_fp64(w_old, s_old, it, loc, g, pw, lr, eps, wd, code)
        touched, hot = count > 0, count > E.EXACT_RUN
        assert np.array_equal(got_w[t][~touched], w_old[~touched]) and np.array_equal(got_s[t][~touched], s_old[~touched]), (tag, t)
        assert np.isfinite(got_w[t]).all() and np.isfinite(got_s[t]).all(), (tag, t)
        cold = touched & ~hot
        if fp64_only:
            hot, cold = touched, np.zeros_like(touched)
        if cold.any():
            G, c32 = E.grad_sum_f32(r, it, loc, g, pw)
            assert np.array_equal(c32, count)
            w_exp, s_exp = E.step_f32(w_old, s_old, G, touched, lr, eps, wd, code)
            assert np.allclose(got_s[t][cold], s_exp[cold], rtol=E.STATE_RTOL, atol=0), (tag, t, "state")
            assert np.allclose(got_w[t][cold], w_exp[cold], rtol=E.W_RTOL, atol=E.W_ATOL), (tag, t, "weights")
            n_cold += int(cold.sum()) * d
        if hot.any():
            lim_w = dw + E.W_RTOL * np.abs(W64) + E.W_ATOL
            lim_s = ds + E.STATE_RTOL * S64
            assert (np.abs(got_w[t] - W64)[hot] <= lim_w[hot]).all(), (tag, t, "hot rows, weights")
            assert (np.abs(got_s[t] - S64)[hot] <= lim_s[hot]).all(), (tag, t, "hot rows, state")
            n_hot += int(hot.sum()) * d
    return n_cold, n_hot


GENERAL_ROWS = [2000, 300, 3, 40]
GENERAL_SPEC = [("ragged", 6), ("hot", 8, 7, 300), ("fixed", 40), ("empty",)]      # table 2: 3 rows, ~20 000 lookups (whole tiles in one run)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("D", [4, 16, 64, 128, 256])
def test_general_gradients_vs_restatement_fp32_tables(D, weighted, seed):
    """ragged and empty bags, a row of 300 lookups, a 3-row table of 20 480 lookups, a table nobody looks up; int32 / int64 indices
    and the weight-decay modes none / l2 taking turns; two steps, the second from a non-zero state"""
    k = [4, 16, 64, 128, 256].index(D) + seed
    rng = np.random.default_rng(1000 + 10 * D + seed)
    B, idt, wd_mode = 512, (torch.int64, torch.int32)[k % 2], (None, "l2")[(k // 2) % 2]
    W0 = [rng.standard_normal((r, D)).astype(np.float32) for r in GENERAL_ROWS]
    m = _module(GENERAL_ROWS, D, W=W0, learning_rate=0.05, eps=1e-6, weight_decay=0.01 if wd_mode else 0.0, weight_decay_mode=wd_mode)
    total = [0, 0]
    for step in range(2):
        idx_h, off_h = _request(rng, GENERAL_ROWS, B, GENERAL_SPEC)
        psw_h = rng.standard_normal(len(idx_h)).astype(np.float32) if weighted else None
        g_h = rng.standard_normal((B, len(GENERAL_ROWS) * D)).astype(np.float32)
        before = (_tables_f32(m), _state(m))
        m.adagrad_step_(_t(g_h), _t(idx_h, idt), _t(off_h, idt), None if psw_h is None else _t(psw_h), batch=B)
        c, h = _check_step_f32(m, before, g_h, idx_h, off_h, psw_h, B, (D, weighted, seed, step))
        total[0] += c
        total[1] += h
    assert total[0] > 1000 * D and total[1] >= 2 * 4 * D, total      # (the hot row and the 3-row table's rows, both steps)
    assert any(s.any() for s in before[1])


# ----------------------------------------------------------------------------- 3. all paths give the same bits
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_presorted_equals_fused_and_two_runs_are_bit_identical(dtype):
    rng = np.random.default_rng(31)
    rows, dims, B = [5000, 800, 60], [64, 128, 32], 256
    idx_h, off_h = _request(rng, rows, B, [("ragged", 6), ("hot", 5, 3, 400), ("fixed", 9)])
    g_h = rng.standard_normal((B, sum(dims))).astype(np.float32)
    idx, off, g = _t(idx_h), _t(off_h), _t(g_h)
    res = []
    for how in ("fused", "presorted", "fused"):
        m = _module(rows, dims, dtype=dtype, seed=4, learning_rate=0.05, weight_decay=0.01, weight_decay_mode="l2")
        for _ in range(2):
            if how == "presorted":
                m.sort_indices(idx, off, batch=B)
                m.adagrad_step_(g, idx, off, batch=B, presorted=True)
            else:
                m.adagrad_step_(g, idx, off, batch=B)
        res.append((m.weights.data.clone(), m.momentum.clone()))
        assert m.momentum.numel() == sum(r * d for r, d in zip(rows, dims)) and bool(m.momentum.any())
    for other in res[1:]:
        assert torch.equal(res[0][0].view(torch.uint8), other[0].view(torch.uint8)) and torch.equal(res[0][1], other[1])


@pytest.mark.parametrize("dtype,D,rows_t,B,L,expect_lds", [(torch.float32, 128, 300_000, 1024, 12, True), (torch.bfloat16, 64, 300_000, 1024, 12, True),
                                                           (torch.float32, 32, 330_000, 4096, 20, False)], ids=["f32_lds", "bf16_lds", "f32_sorted_rest"])
def test_hybrid_bag_major_path_equals_the_sorted_path(dtype, D, rows_t, B, L, expect_lds):
    """A uniform request in which some rows repeat, with the hybrid backward forced on every eligible table: the bag-major kernel
    applies the rows looked up once, the LDS left-over kernel (or, for the longer list, the key sort + sorted apply + fix-up) the
    repeats.  Same bits as the hybrid-off (sorted) route, tables and state, after two steps."""
    import param_amd
    from param_amd.indices import tbe_request

    rows = [rows_t] * 3      # (81 920 lookups into 330 K rows: ~18 K flagged per table, more than the LDS kernel takes)
    idx, off = tbe_request(rows, B, L, alpha=0.0, device=DEV, seed=8)
    n_rep = sum(int((np.bincount(idx.cpu().numpy()[t * B * L:(t + 1) * B * L]) > 1).sum()) for t in range(3))
    assert n_rep > 50                                                     # some rows repeat
    grad = torch.randn((B, len(rows) * D), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    res = {}
    try:
        param_amd.set_hybrid_min_tiles(0)
        for tag, hyb in (("hybrid", 2), ("sorted", 0)):
            param_amd.set_hybrid_tuning(hyb, 0)
            m = _module(rows, D, dtype=dtype, seed=6, learning_rate=0.05, eps=1e-8, weight_decay=0.01, weight_decay_mode="l2")
            for _ in range(2):
                m.adagrad_step_(grad, idx, off, batch=B)
            st = m.sort_status(idx, off, batch=B)
            if tag == "hybrid":
                assert st["hybrid_tables"] == 3 and st["hybrid_launched"], st
                if expect_lds:
                    assert st["lds_pairs"] > 0 and st["lds_tables"] == 3, st
                else:
                    assert st["pairs_sorted"] > 0 and st["lds_tables"] == 0, st      # too long for the LDS kernel: key sort + sorted apply
            else:
                assert st["hybrid_tables"] == 0 and st["pairs_sorted"] == idx.numel(), st
            res[tag] = (m.weights.data.clone(), m.momentum.clone())
            del m
    finally:
        param_amd.set_hybrid_tuning()
        param_amd.set_hybrid_min_tiles()
    assert torch.equal(res["hybrid"][0].view(torch.uint8), res["sorted"][0].view(torch.uint8))
    assert torch.equal(res["hybrid"][1], res["sorted"][1]) and bool(res["hybrid"][1].any())


# ----------------------------------------------------------------------------- 4. bf16 and fp16 tables
def _init_bits(rng, rows, dims, dtype):
    return [_bits(torch.from_numpy(rng.standard_normal((r, d)).astype(np.float32)).to(dtype)) for r, d in zip(rows, dims)]


def _w_pre(m, W_bits, S_old, g_h, idx_h, off_h, psw_h, B, code):
    """per table: (fp32 value before rounding, new state, touched) from the restatement; every row within the exact-sum range"""
    out = []
    for t, (r, d) in enumerate(zip(m.rows, m.dims)):
        it, loc, s, e = _table_slice(idx_h, off_h, t, B)
        c0 = sum(m.dims[:t])
        G, count = E.grad_sum_f32(r, it, loc, np.ascontiguousarray(g_h[:, c0:c0 + d]), None if psw_h is None else psw_h[s:e])
        assert count.max(initial=0) <= E.EXACT_RUN
        w_pre, s_new = E.step_f32(_widen(W_bits[t], code), S_old[t], G, count > 0, m.learning_rate, m.eps, m.weight_decay, WD[m.weight_decay_mode])
        out.append((w_pre, s_new, count > 0))
    return out


LOWP_ROWS, LOWP_DIMS, LOWP_B = [4000, 3000, 50, 2000], [64, 32, 16, 128], 1024
LOWP_SPEC = [("ragged", 8), ("ragged", 6), ("empty",), ("ragged", 5)]


@pytest.mark.parametrize("wd_mode", [None, "l2"], ids=["none", "l2"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_16bit_tables_round_to_nearest(dtype, wd_mode):
    """mixed dims, ragged bags, signed per-sample weights, two steps each judged from the bits and the state the device held before
    it: every element within ``ulp16(w_pre) / 2 + b`` of the restatement's fp32 value before rounding; state at the fp32 bar"""
    code = CODE[dtype]
    rng = np.random.default_rng(40 + code)
    W0 = _init_bits(rng, LOWP_ROWS, LOWP_DIMS, dtype)
    m = _module(LOWP_ROWS, LOWP_DIMS, dtype=dtype, W=W0, learning_rate=0.05, eps=1e-6, weight_decay=0.02 if wd_mode else 0.0,
                weight_decay_mode=wd_mode)
    n = 0
    for step in range(2):
        idx_h, off_h = _request(rng, LOWP_ROWS, LOWP_B, LOWP_SPEC)
        psw_h = rng.standard_normal(len(idx_h)).astype(np.float32)
        g_h = rng.standard_normal((LOWP_B, sum(LOWP_DIMS))).astype(np.float32)
        bits0, s0 = [_bits(m.table(t)) for t in range(4)], _state(m)
        m.adagrad_step_(_t(g_h), _t(idx_h), _t(off_h), _t(psw_h), batch=LOWP_B)
        for t, (w_pre, s_new, touched) in enumerate(_w_pre(m, bits0, s0, g_h, idx_h, off_h, psw_h, LOWP_B, code)):
            got_bits, gs = _bits(m.table(t)), m.momentum_table(t).cpu().numpy()
            assert np.array_equal(got_bits[~touched], bits0[t][~touched]) and np.array_equal(gs[~touched], s0[t][~touched]), (step, t)
            got, wp = _widen(got_bits, code).astype(np.float64)[touched], w_pre.astype(np.float64)[touched]
            ratio = R.nearest_ratio(got, wp, code, R.tol_b(wp))
            assert ratio.size == 0 or ratio.max() <= 1.0, (step, t, float(ratio.max()))
            assert np.allclose(gs, s_new, rtol=E.STATE_RTOL, atol=0), (step, t, "state")
            n += got.size
    assert n > 200000


def _sr_run(dtype, sr_step):
    """one stochastic step on host-made inputs -> (stored values, w_pre, b) over the touched elements (fp64, tables concatenated)
    and the raw table bits"""
    code = CODE[dtype]
    rng = np.random.default_rng(300)
    W0 = _init_bits(rng, LOWP_ROWS, LOWP_DIMS, dtype)
    m = _module(LOWP_ROWS, LOWP_DIMS, dtype=dtype, W=W0, learning_rate=0.05, eps=1e-6, weight_decay=0.02, weight_decay_mode="l2",
                stochastic_rounding=True)
    m._sr_step = sr_step
    idx_h, off_h = _request(rng, LOWP_ROWS, LOWP_B, LOWP_SPEC)
    psw_h = rng.standard_normal(len(idx_h)).astype(np.float32)
    g_h = rng.standard_normal((LOWP_B, sum(LOWP_DIMS))).astype(np.float32)
    s0 = [np.zeros((r, d), np.float32) for r, d in zip(LOWP_ROWS, LOWP_DIMS)]
    m.adagrad_step_(_t(g_h), _t(idx_h), _t(off_h), _t(psw_h), batch=LOWP_B)
    got, pre, raw = [], [], []
    for t, (w_pre, s_new, touched) in enumerate(_w_pre(m, W0, s0, g_h, idx_h, off_h, psw_h, LOWP_B, code)):
        tb = _bits(m.table(t))
        raw.append(tb)
        assert np.array_equal(tb[~touched], W0[t][~touched])
        assert np.allclose(m.momentum_table(t).cpu().numpy(), s_new, rtol=E.STATE_RTOL, atol=0)      # the state is fp32: nothing stochastic
        got.append(_widen(tb, code)[touched].astype(np.float64).ravel())
        pre.append(w_pre[touched].astype(np.float64).ravel())
    got, pre = np.concatenate(got), np.concatenate(pre)
    return got, pre, R.tol_b(pre), raw


@pytest.mark.parametrize("dtype,cap", [(torch.bfloat16, 0.05), (torch.float16, 0.15)], ids=["bf16", "f16"])
def test_16bit_tables_stochastic_rounding(dtype, cap):
    """The stochastic store (restated only: no third-party implementation pins it): every stored value is one of the two neighbours
    of the restatement's fp32 value (interval of ``round_up_stats``), the round-up frequency is calibrated in ten bins over at
    least 2e5 elements with no MISS, the same step gives the same bits and the next step other decisions.  (Caps on the share
    the calibration drops because w_pre lies within b of a grid value: those of tests/test_gpu_lowp_update.py.)"""
    code = CODE[dtype]
    got, wp, b, raw = _sr_run(dtype, 0)
    assert got.size >= 200000
    p, slack, up, inside = R.round_up_stats(got, wp, code, b)
    assert inside.all(), (int((~inside).sum()), "stored values that are no neighbour of w_pre")
    keep = (p > slack) & (p < 1 - slack)
    print(f"\ndropped by the calibration: {1 - keep.mean():.4f}")
    assert 1 - keep.mean() <= cap and keep.sum() >= 200000
    rows = R.calibration(p[keep], up[keep], slack[keep])
    table = R.calibration_table(rows)
    print(f"{dtype}: {int(keep.sum())} elements\n{table}")
    assert "MISS" not in table and all(n > 0 for n, *_ in rows), table
    got2, wp2, _, raw2 = _sr_run(dtype, 1)                                   # the next step: same w_pre, other draws
    assert np.array_equal(wp2, wp)
    _, _, up2, inside2 = R.round_up_stats(got2, wp, code, b)
    assert inside2.all() and (up2 != up)[keep].mean() > 0.1
    *_, raw3 = _sr_run(dtype, 0)                                             # the same step: the same bits
    assert all(np.array_equal(x, y) for x, y in zip(raw, raw3))


# ----------------------------------------------------------------------------- 5. DECOUPLE
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_decoupled_weight_decay_vs_fp64_restatement(weighted):
    """``weight_decay_mode="decouple"``: ``w = (1 - lr * wd) * w - lr * G / (sqrt(s) + eps)``, ``s += G * G``.  NO third-party
    implementation pins this mode (torch.optim.Adagrad has L2 only; fbgemm is not at hand): it is compared with the fp64 restatement
    of tests/elem_adagrad_rules.py alone, at the torch pin's bars plus the first-order bound of an fp32 gradient sum."""
    rng = np.random.default_rng(50 + weighted)
    rows, dims, B = [2000, 300, 3], [64, 16, 128], 512
    W0 = [rng.standard_normal((r, d)).astype(np.float32) for r, d in zip(rows, dims)]
    m = _module(rows, dims, W=W0, learning_rate=0.05, eps=1e-6, weight_decay=0.02, weight_decay_mode="decouple")
    n = 0
    for step in range(2):
        idx_h, off_h = _request(rng, rows, B, [("ragged", 6), ("hot", 8, 7, 300), ("fixed", 40)])
        psw_h = rng.standard_normal(len(idx_h)).astype(np.float32) if weighted else None
        g_h = rng.standard_normal((B, sum(dims))).astype(np.float32)
        before = (_tables_f32(m), _state(m))
        m.adagrad_step_(_t(g_h), _t(idx_h), _t(off_h), None if psw_h is None else _t(psw_h), batch=B)
        n += _check_step_f32(m, before, g_h, idx_h, off_h, psw_h, B, ("decouple", weighted, step), fp64_only=True)[1]
    assert n > 100000
    # the decay is really the decoupled one: a touched row whose gradient sum is zero shrinks by exactly (1 - lr * wd)
    m2 = _module([8], [16], W=[np.ones((8, 16), np.float32)], learning_rate=0.5, eps=1e-6, weight_decay=0.25, weight_decay_mode="decouple")
    m2.adagrad_step_(torch.zeros(2, 16, device=DEV), _t(np.array([1, 5], np.int64)), _t(np.array([0, 1, 2], np.int64)), batch=2)
    w = m2.table(0).cpu().numpy()
    assert (w[[1, 5]] == np.float32(1.0 - 0.5 * 0.25)).all() and (np.delete(w, [1, 5], axis=0) == 1.0).all() and not m2.momentum.any()


# ----------------------------------------------------------------------------- 6. more than 1024 tables
def test_1100_tables_in_one_call_equal_the_per_table_application():
    rng = np.random.default_rng(60)
    T, D, B, L = 1100, 8, 16, 3
    rows = [int(r) for r in rng.integers(20, 50, T)]
    W0 = [rng.standard_normal((r, D)).astype(np.float32) for r in rows]
    idx_h = np.concatenate([rng.integers(0, r, B * L) for r in rows]).astype(np.int64)
    off_h = np.arange(T * B + 1, dtype=np.int64) * L
    g_h = rng.standard_normal((B, T * D)).astype(np.float32)
    kw = dict(learning_rate=0.05, eps=1e-6, weight_decay=0.01, weight_decay_mode="l2")
    m = _module(rows, D, W=W0, **kw)
    idx, off, g = _t(idx_h), _t(off_h), _t(g_h)
    for _ in range(2):
        m.adagrad_step_(g, idx, off, batch=B)
    with pytest.raises(ValueError, match="presorted=True takes requests of at most 1024 tables"):
        m.adagrad_step_(g, idx, off, batch=B, presorted=True)
    got_w, got_s = _tables_f32(m), _state(m)
    one_off = _t(np.arange(B + 1, dtype=np.int64) * L)
    for t in range(T):
        one = _module([rows[t]], [D], W=[W0[t]], **kw)
        gt = g[:, t * D:(t + 1) * D].contiguous()
        for _ in range(2):
            one.adagrad_step_(gt, idx[t * B * L:(t + 1) * B * L], one_off, batch=B)
        assert np.array_equal(one.table(0).cpu().numpy(), got_w[t]) and np.array_equal(one.momentum_table(0).cpu().numpy(), got_s[t]), t
        assert got_s[t].any()


# ----------------------------------------------------------------------------- 7. autograd and the operator
def test_backward_of_the_module_equals_adagrad_step():
    rng = np.random.default_rng(70)
    rows, dims, B = [900, 200], [32, 64], 128
    idx_h, off_h = _request(rng, rows, B, [("ragged", 5), ("fixed", 4)])
    g_h = rng.standard_normal((B, sum(dims))).astype(np.float32)
    psw_h = rng.standard_normal(len(idx_h)).astype(np.float32)
    kw = dict(seed=3, learning_rate=0.05, eps=1e-6, weight_decay=0.01, weight_decay_mode="l2", fused_update=True)
    a, b = _module(rows, dims, **kw), _module(rows, dims, **kw)
    idx, off, g, psw = _t(idx_h), _t(off_h), _t(g_h), _t(psw_h)
    w_before = a.weights.data.clone()
    for _ in range(2):
        a(idx, off, psw).backward(g)
        b.adagrad_step_(g, idx, off, psw)
    assert torch.equal(a.weights.data, b.weights.data) and torch.equal(a.momentum, b.momentum)
    assert not torch.equal(a.weights.data, w_before) and bool(a.momentum.any())


def test_operator_builds_and_steps_as_the_reference_unit_test_constructs_it():
    """the three ``build(...)`` calls of the reference's unit test of this operator (fp16 tables, ``"exact_adagrad"``) and its
    ``embedding_specs`` assertions; then ``forward`` + ``backward`` change exactly the rows the request touches"""
    from param_amd.compute.python.split_table_batched_embeddings_ops import SplitTableBatchedEmbeddingBagsCodegenOp, generate_batched_request

    op = SplitTableBatchedEmbeddingBagsCodegenOp()
    op.device = "cuda"
    op.cleanup()
    op.build(1, [1000], [64], 0, False, "fp16", "exact_adagrad")
    assert op.op.embedding_specs[0][0] == 1000 and op.op.embedding_specs[0][1] == 64
    op.build(1, 2000, 128, 0, False, "fp16", "exact_adagrad")
    assert op.op.embedding_specs[0][0] == 2000 and op.op.embedding_specs[0][1] == 128
    op.build(2, [1000, 2000], [64, 128], 0, False, "fp16", "exact_adagrad")
    assert op.op.embedding_specs[0][0] == 1000 and op.op.embedding_specs[1][0] == 2000
    assert op.op.embedding_specs[0][1] == 64 and op.op.embedding_specs[1][1] == 128
    assert op.op.optimizer == "adagrad" and op.op.weights.dtype == torch.float16
    B, L = 32, 4
    torch.manual_seed(0)
    idx, off, _ = generate_batched_request(2, [1000, 2000], B, L, alpha=1.0, device=DEV)
    before = [_bits(op.op.table(t)) for t in range(2)]
    out = op.forward(idx, off)
    assert tuple(out.shape) == (B, 64 + 128)
    op.backward()                                   # grad = ones_like(fwd_out)
    torch.cuda.synchronize()
    idx_h = idx.cpu().numpy()
    for t, r in enumerate((1000, 2000)):
        touched = np.bincount(idx_h[t * B * L:(t + 1) * B * L], minlength=r) > 0
        after, st = _bits(op.op.table(t)), op.op.momentum_table(t).cpu().numpy()
        assert tuple(st.shape) == (r, (64, 128)[t])
        changed = (after != before[t]).any(axis=1)
        assert np.array_equal(changed, touched), t                               # (lr 0.01 >> fp16 spacing of U(-1/sqrt(n), 1/sqrt(n)) weights)
        assert np.array_equal(st.any(axis=1), touched) and (st[touched] > 0).all(), t
    op.cleanup()
