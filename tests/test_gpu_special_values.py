"""NaN, Inf, signed zeros and subnormals through the kernels on a real MI355X (``pytest -m gpu``).

Inputs come from tests/special_values.py: tables, gradients and per-sample weights in which some rows are constant specials, some
mix specials with ordinary values inside one 16-byte lane load, and the rest are ordinary.  What is compared how:

  * ``same_bits`` (NaN at the same places, every other bit equal, the sign of zero and of Inf included) against the oracle, which
    tests/test_special_values_host.py pins to torch's CPU results on these very values: every forward kernel, the stand-alone
    quantisers, the backward and both Adagrad flavours' fp32 tables on rows looked up at most ``EXACT_RUN`` times;
  * ``same_class`` (NaN, +Inf, -Inf at the same places, finite values within the existing named bars -- the fuzz test's
    ``tol_sorted``, ``lowp_rules.tol_b``, the fuzz test's Adagrad bars) for rows beyond ``EXACT_RUN``, whose inputs have one class
    in any order of addition (pinned on the host), and for row-wise Adagrad, whose reduction order differs from the oracle's;
  * at most the sign bit of the bias field on quantiser rows whose minimum is zero with both zero signs present.

The alternates-only atomic backward (``method="atomic"``) is left out: it is built on unsafe floating-point atomics and is a
baseline, not the product.  ``scatter_add_`` has no stochastic store: the stochastic-rounding tests cover both Adagrad flavours.
Every backward and Adagrad test asserts the route it took (``sort_status``); the forward kernel is the library's choice
(``pm_embbag_plan`` reports it; tests/test_gpu_plan_sweep.py runs every choice), so the forward tests name their requests.  Every test asserts the number of special elements it compared.
"""
import numpy as np
import pytest
import torch

from oracle import embbag_oracle as O
from oracle import rowquant as orq
from tests import elem_adagrad_rules as E
from tests import lowp_rules as R
from tests import special_values as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CODE = {"f32": None, "bf16": O.BF16, "f16": O.F16}
WD = {None: E.WD_NONE, "l2": E.WD_L2, "decouple": E.WD_DECOUPLE}
WD_ROW = {None: 0, "l2": 1, "decouple": 2}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    import param_amd

    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    param_amd.load_library()
    param_amd.set_hybrid_min_tiles(0)          # the hybrid tests drive its kernels with small requests (as tests/test_gpu_rest.py)
    yield
    param_amd.set_hybrid_min_tiles()
    param_amd.set_hybrid_tuning()
    param_amd.set_hybrid_rest()


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _module(rows, dims, kind, stores, **kw):
    """a module whose tables hold exactly ``stores`` (fp32 values, or uint16 bits copied through an int16 view)"""
    from param_amd import BatchedEmbeddingBagMI355

    m = BatchedEmbeddingBagMI355(rows, dims, dtype=TD[kind], device=DEV, init=None, **kw)
    _fill(m, kind, stores)
    return m


def _fill(m, kind, stores):
    for t, w in enumerate(stores):
        if kind == "f32":
            m.table(t).copy_(_t(w))
        else:
            m.table(t).view(torch.int16).copy_(_t(w.view(np.int16)))


def _read(m, t, kind):
    if kind == "f32":
        return m.table(t).cpu().numpy().copy()
    return m.table(t).contiguous().view(torch.int16).cpu().numpy().view(np.uint16).copy()


def _f32(a, kind):
    return a if kind == "f32" else S.widen16(a, kind)


def _slice(idx, off, t, B):
    s, e = off[t * B], off[(t + 1) * B]
    return idx[s:e], off[t * B:(t + 1) * B] - s, s, e


def _assert_same_bits(got, want, what, kind="f32"):
    assert S.same_bits(got, want, kind), (what, S.first_difference(got, want, kind))


# ============================================================================= forward
def _forward_case(kind, dims, L, seed):
    rng = np.random.default_rng(seed)
    T = len(dims)
    rows = [2 * S.n_special_rows(kind) + 40 + 3 * t for t in range(T)]
    both = [S.special_table(r, d, rng, kind) for r, d in zip(rows, dims)]
    return rows, [b[0] for b in both], [b[1] for b in both], rng


@pytest.mark.parametrize("route,dims,L", [("fixed_pooling", [16] * 3, 5), ("fixed_pooling", [128] * 3, 3), ("fixed_pooling", [512] * 3, 4),
                                          ("ragged", [16] * 3, None), ("ragged", [128] * 3, None), ("ragged", [512] * 3, None),
                                          ("mixed_dims", [16, 64, 128], None), ("mixed_dims", [16, 64, 128], 3)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
@pytest.mark.parametrize("kind", S.KINDS)
def test_forward_every_kernel_same_bits_as_the_oracle(coracle, kind, route, dims, L):
    """The requests that make the library choose its forward kernels -- fixed pooling (tile kernel, staged output), ragged bags (tile
    kernel, or the flat-walk kernel where the request is staged: short bags at small D), mixed dims (flat-walk kernel, lane group per
    table).  The choice is the library's (launch_plan.h); ``pm_embbag_plan`` reports it, and at B = 257 it is the small-request corner
    of the plan: staged tiles of ONE bag per lane group (32 / 8 / 4 bags at D = 16 / 128 / 512, unroll 4 / 2 / 4) for fixed pooling, the
    flat walk for the ragged requests at D = 16 and 128, plain 4-bag tiles at unroll 8 at D = 512 -- never a tile of more bags than
    lane groups, so never the longest-bag-first instance.  The ids name the REQUEST, not the kernel.  The variants the product takes
    at benchmark size (32-bag staged and ordered tiles, every unroll) are run by tests/test_gpu_plan_sweep.py, on ordinary values.
    T = 3; int32 and int64
    indices, weighted (weights 0, -0, +-Inf, NaN, 1e-30, 1e-40 among ordinary ones) and unweighted, layouts ``bd`` and ``tbd``.
    fp16 tables: their subnormals must widen exactly (the oracle's widening is torch's).  The named bags are asserted one by one."""
    T, B = 3, 257
    rows, stores, tabs, rng = _forward_case(kind, dims, L, 7 * len(dims) + sum(dims) + (L or 0))
    layouts = ("bd", "tbd") if len(set(dims)) == 1 else ("bd",)
    n_cmp = 0
    for layout in layouts:
        m = _module(rows, dims, kind, stores, layout=layout, fused_update=False)
        for weighted in (False, True):
            idx, off, psw, named = S.forward_request(kind, rows, B, rng, L, weighted)
            exp = coracle.fwd_batched(stores, idx, off, B, psw=psw, dtype=CODE[kind], layout=layout)
            for idt in (torch.int64, torch.int32):
                got = m.lookup(_t(idx, idt), _t(off, idt), None if psw is None else _t(psw), batch=B).cpu().numpy()
                _assert_same_bits(got, exp, (route, layout, weighted, idt))
                n_cmp += int(S.is_special(exp).sum())
            for t in range(T):
                c0 = sum(dims[:t])
                for b, (name, rr, _, expected) in enumerate(named):
                    row = got[b, c0:c0 + dims[t]] if layout == "bd" else got[t, b]
                    S.check_named_bag(name, expected, row, [tabs[t][r] for r in rr])
            assert not (np.signbit(exp) & (exp == 0)).any() or weighted        # a sum started at +0 gives no -0 (a weighted one can underflow to it)
    # the named bags alone: 5 special results per table (4 for fp16, whose subnormal sum is a normal fp32 value), each D wide
    assert n_cmp >= len(layouts) * 2 * 2 * (5 if kind != "f16" else 4) * sum(dims), n_cmp
    assert n_cmp >= len(layouts) * 4 * 90 * sum(dims), n_cmp                       # and the drawn bags: 90 special pooled rows per lookup call


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("kind", S.KINDS)
def test_forward_split_bag_kernel_same_bits_on_order_free_bags(coracle, kind, weighted):
    """``split_bags=True`` (one workgroup per bag, partial sums) adds in another order than the oracle, so ordinary values agree
    to rounding only; these 8 bags of 300 .. 3000 lookups are built so that the order cannot matter (``special_values.
    long_bag_request``): bits are comparable all the same.  A partial sum that starts from its first row instead of +0 would turn
    the all -0 bag into -0."""
    rng = np.random.default_rng(11)
    D, rows = 64, 2 * S.n_special_rows(kind) + 60
    store, w = S.dyadic_table(rows, D, rng, kind)
    idx, off, psw = S.long_bag_request(kind, rows, rng, weighted)
    exp = coracle.fwd_batched([store], idx, off, 8, psw=psw, dtype=CODE[kind])
    with np.errstate(all="ignore"):                                       # the premise: another order, the same bits
        rev = np.concatenate([np.arange(off[b], off[b + 1])[::-1] for b in range(8)])
        assert S.same_bits(coracle.fwd_batched([store], idx[rev], off, 8, psw=None if psw is None else psw[rev], dtype=CODE[kind]), exp)
    m = _module([rows], [D], kind, [store], fused_update=False)
    for idt in (torch.int64, torch.int32):
        got = m.lookup(_t(idx, idt), _t(off, idt), None if psw is None else _t(psw), batch=8, split_bags=True).cpu().numpy()
        _assert_same_bits(got, exp, (kind, weighted, idt))
        assert (got[3].view(np.uint32) == 0).all(), "the bag of -0 rows must pool to +0"
        assert np.isnan(got[6]).all() and np.isnan(got[2]).all()
        assert np.isposinf(got[5]).all() if kind != "f16" else (got[5] == np.float32(300 * 65504.0)).all()
        assert (got[4] == np.float32(500 * float(_f32(store, kind)[S.special_index(kind)["sub_a"], 0]))).all() and (got[4] != 0).all()
    assert int(S.is_special(exp).sum()) >= 4 * D


@pytest.mark.parametrize("bits", (16, 8, 4, 2))
@pytest.mark.parametrize("kind", S.KINDS)
def test_forward_quantised_output_on_the_special_request(coracle, kind, bits):
    """``lookup_quantized`` on the forward requests above (fixed pooling: the kernel's own output burst; ragged: forward + quantiser),
    judged on the bags whose pooled row is finite (rows with non-finite elements are undefined at 8 / 4 / 2 bits: DESIGN) against
    ``quantize_rows(oracle forward)``, byte for byte.  Unweighted sums start at +0 and hold no -0, so no row can mix zero signs."""
    T, B, n_rows, n_sub = 3, 257, 0, 0
    for D, L in ((16, 5), (128, 3), (16, None), (128, None)):
        rows, stores, _, rng = _forward_case(kind, [D] * T, L, 100 + D + (L or 0))
        for layout in ("bd", "tbd"):
            m = _module(rows, [D] * T, kind, stores, layout=layout, fused_update=False)
            idx, off, _, _ = S.forward_request(kind, rows, B, rng, L, False)
            exp = coracle.fwd_batched(stores, idx, off, B, dtype=CODE[kind], layout=layout).reshape(-1, D)
            assert not (np.signbit(exp) & (exp == 0)).any()
            ok = np.isfinite(exp).all(axis=1)
            with np.errstate(all="ignore"):
                want = orq.quantize_rows(exp[ok], bits)
            got = m.lookup_quantized(_t(idx), _t(off), bits, batch=B).cpu().numpy().reshape(-1, orq.row_bytes(D, bits))
            bad = np.flatnonzero((got[ok] != want).any(axis=1))
            assert bad.size == 0, (D, L, layout, bad[:5], exp[ok][bad[:1]], got[ok][bad[:1]], want[bad[:1]])
            n_rows += int(ok.sum())
            n_sub += int(S.is_special(exp[ok]).sum())
    assert n_rows >= 8 * T * B // 2 and n_sub >= 8 * T * 3 * 16, (n_rows, n_sub)


# ============================================================================= the stand-alone quantisers
@pytest.mark.parametrize("bits", (8, 4, 2))
@pytest.mark.parametrize("dim", (8, 96, 128))
def test_quantisers_byte_exact_on_the_finite_edge_rows(dim, bits):
    """all-subnormal rows, all -0, a range beyond fp32, one ulp at 1.0, one subnormal outlier, negative subnormals, +-30000, a
    1e-9 range at 5, zero with a single 1e-44, -0 below positive values: quantise and dequantise, byte for byte against the oracle
    (pinned to torch's prepack operators on these rows).  Rows that mix both zero signs at the minimum: the kernels' lane reduction
    takes -0 where torch takes the first zero -- that rule is asserted, and those rows are compared with the one sign bit of the
    bias field masked, everything else byte for byte, and their dequantised values equal as numbers (DESIGN, parity section)."""
    from param_amd import quant

    x, names = S.quant_edge_rows(dim)
    mz = S.quant_mixed_zero_rows(dim)
    reps = 70                                                        # more than one block of rows
    xx = np.concatenate([x] * reps + [mz] * reps, axis=0)
    n_edge = len(x) * reps
    q = quant.quantize_rows(_t(xx), dim, bits)
    got = q.cpu().numpy()
    want = orq.quantize_rows(xx, bits)
    for i in range(len(x)):
        assert np.array_equal(got[i], want[i]), (names[i], got[i][-8:], want[i][-8:])
    assert np.array_equal(got[:n_edge], want[:n_edge])
    mask = np.full(want.shape[1], 0xFF, np.uint8)
    mask[-1] = 0x7F                                                   # the bias field ends the row; its top bit is its sign
    assert np.array_equal(got[n_edge:] & mask, want[n_edge:] & mask), "mixed-zero rows differ beyond the bias sign"
    # the kernels' rule, pinned: a zero minimum with a -0 among the zeros is stored as -0 (fminf), wherever the first zero sits
    assert ((got[n_edge:, -1] & 0x80) == 0x80).all(), "a mixed-zero row whose bias is not -0"
    assert int((got[n_edge:, -1] != want[n_edge:, -1]).sum()) == 2 * reps            # the two rows of four whose FIRST zero is +0
    d = quant.dequantize_rows(q, dim, bits).cpu().numpy()
    dw = orq.dequantize_rows(want, dim, bits)
    _assert_same_bits(d[:n_edge], dw[:n_edge], "dequantise")
    assert np.array_equal(d[n_edge:], dw[n_edge:])                    # equal as numbers (-0 == +0)
    # and the oracle's own bytes dequantise to the oracle's values on the device
    _assert_same_bits(quant.dequantize_rows(_t(want), dim, bits).cpu().numpy(), dw, "dequantise the oracle's bytes")
    assert int(S.is_special(xx[:n_edge]).sum()) >= reps * 5 * dim


def test_quantiser_16_bits_on_the_full_special_set():
    from param_amd import quant

    for dim in (8, 96, 128):
        x = np.concatenate(list(S.special_rows_f32(dim)) * 40, axis=0)
        got = quant.quantize_rows(_t(x), dim, 16)
        want = orq.quantize_rows(x, 16).view(np.uint16)
        _assert_same_bits(got.cpu().numpy().view(np.uint16), want, dim, "f16")
        _assert_same_bits(quant.dequantize_rows(got, dim, 16).cpu().numpy(), orq.dequantize_rows(want.view(np.uint8), dim, 16), dim)
        assert int(S.is_special(want, "f16").sum()) >= 40 * 14 * dim


# ============================================================================= backward and in-place update
def _truth_mag(shape, idx_t, loc, g, pw, B):
    """fp64 sum of the contributions per row and of their magnitudes"""
    start, end = O.bag_bounds(loc, B, len(idx_t))
    bag_of = np.repeat(np.arange(B), end - start)
    with np.errstate(all="ignore"):
        contrib = g.astype(np.float64)[bag_of] * (1.0 if pw is None else pw.astype(np.float64)[:, None])
        truth, mag = np.zeros(shape), np.zeros(shape)
        np.add.at(truth, idx_t, contrib)
        np.add.at(mag, idx_t, np.abs(contrib))
    return truth, mag


def _tol_factor(cnt):
    """the relative part of the fuzz test's ``tol_sorted``: 1e-5, widened for rows of very many lookups"""
    return np.maximum(1e-5, (256 + cnt.astype(np.float64)[:, None] / 32) * 2.0 ** -24)


def _hot_in_place_check(got, want, before, idx_t, loc, g, pw, B, alpha, kind, what):
    """in-place update, rows beyond the exact-run limit: the oracle's class; finite values within the bar of
    tests/test_gpu_join_tiles.py's in-place test -- one rounding of the table's type (``ulp16 / 2``; fp32: inside the relative
    term) plus ``tol_sorted``'s factor times (|alpha| * sum |contribution| + |old value|).  ``got`` / ``want`` / ``before``: fp32.
    Returns the number of finite elements whose value was compared."""
    cnt = np.bincount(idx_t, minlength=want.shape[0])
    hot = cnt > R.EXACT_RUN
    truth, mag = _truth_mag(want.shape, idx_t, loc, g, pw, B)
    fin = np.isfinite(want)
    with np.errstate(all="ignore"):
        exact = before.astype(np.float64) + alpha * truth
        lim = _tol_factor(cnt) * (abs(alpha) * mag + np.abs(before)) + 1e-30
        if kind != "f32":
            lim = lim + O.ulp16(np.where(fin, exact, 0.0), CODE[kind]) / 2
    lim = np.where(fin, lim, 0.0)
    assert S.same_class(got[hot], np.where(fin, exact, want)[hot], 0.0, lim[hot]), (what, "rows beyond the exact-run limit, in place")
    return int((fin & hot[:, None]).sum())


def _hot_check(got, ref, idx_t, loc, g, pw, B, what):
    """rows within the exact-run limit: the oracle's bits.  Beyond: the oracle's class, finite values within the fuzz test's
    ``tol_sorted`` of the fp64 sum.  Returns (special elements compared bit for bit, elements compared by class)."""
    rows = ref.shape[0]
    cnt = np.bincount(idx_t, minlength=rows)
    cold = cnt <= R.EXACT_RUN
    _assert_same_bits(got[cold], ref[cold], (what, "rows within the exact-run limit"))
    hot = ~cold
    if hot.any():
        truth, mag = _truth_mag(ref.shape, idx_t, loc, g, pw, B)
        tol_sorted = _tol_factor(cnt) * np.where(np.isfinite(mag), mag, 0.0) + 1e-30
        fin = np.isfinite(ref)
        assert S.same_class(got[hot], np.where(fin, truth, ref)[hot], 0.0, tol_sorted[hot]), (what, "rows beyond the exact-run limit")
    return int(S.is_special(ref[cold]).sum()), int(hot.sum()) * ref.shape[1]


def _bwd_oracle(coracle, kind, store, idx_t, loc, g, pw, alpha):
    if kind == "f32":
        return coracle.bwd_f32(store.copy(), idx_t, loc, g, pw, alpha=alpha)
    return (coracle.bwd_bf16 if kind == "bf16" else coracle.bwd_f16)(store.copy(), idx_t, loc, g, pw, alpha=alpha)


def _backward_case(kind, dims, B, seed, hot=True, extra_rows=60):
    rng = np.random.default_rng(seed)
    rows = [2 * S.n_special_rows(kind) + extra_rows + 5 * t for t in range(len(dims))]
    both = [S.special_table(r, d, rng, kind) for r, d in zip(rows, dims)]
    idx, off, psw = S.backward_request(kind, rows, B, rng, hot)
    g = np.concatenate([S.special_grad(B, d, rng) for d in dims], axis=1)
    return rows, [b[0] for b in both], idx, off, psw, g


@pytest.mark.parametrize("kind", S.KINDS)
def test_backward_plain_sorted_route(coracle, kind):
    """``dense_grad``, ``sparse_grad`` (row lists and values) and the in-place ``scatter_add_`` (16-bit tables: widened, fp32 sum,
    ONE rounding) on the sorted apply: special gradient rows and mixed rows, special table rows, special per-sample weights;
    cancelling huge values only on rows within the exact-run limit, where the oracle's order is the kernel's."""
    dims, B = [64, 16], 600
    rows, stores, idx, off, psw, g = _backward_case(kind, dims, B, 21)
    m = _module(rows, dims, kind, stores, fused_update=False)
    i_t, o_t, p_t, g_t = _t(idx), _t(off), _t(psw), _t(g)
    dense = m.dense_grad(g_t, i_t, o_t, p_t, batch=B)
    st = m.sort_status(i_t, o_t, p_t, batch=B)
    assert st["hybrid_tables"] == 0 and st["pairs_sorted"] == len(idx), st
    dense_plain = m.dense_grad(g_t, _t(idx, torch.int32), _t(off, torch.int32), None, batch=B)
    sparse = m.sparse_grad(g_t, i_t, o_t, p_t, batch=B)
    m.scatter_add_(g_t, i_t, o_t, alpha=-0.125, per_sample_weights=p_t, batch=B)
    n_bits = n_class = n_hot_val = 0
    for t in range(len(dims)):
        it, loc, s, e = _slice(idx, off, t, B)
        c0 = sum(dims[:t])
        gt = np.ascontiguousarray(g[:, c0:c0 + dims[t]])
        cnt = np.bincount(it, minlength=rows[t])
        assert (cnt[-S.N_HOT:] > R.EXACT_RUN).all() and cnt[:-S.N_HOT].max() <= R.EXACT_RUN
        for got, pw, tag in ((dense[t], psw[s:e], "dense_grad weighted"), (dense_plain[t], None, "dense_grad plain")):
            ref = coracle.bwd_f32(np.zeros((rows[t], dims[t]), np.float32), it, loc, gt, pw)
            a, b = _hot_check(got.cpu().numpy(), ref, it, loc, gt, pw, B, (tag, t))
            n_bits, n_class = n_bits + a, n_class + b
        ref = coracle.bwd_f32(np.zeros((rows[t], dims[t]), np.float32), it, loc, gt, psw[s:e])
        r_t, v_t = sparse[t]
        hit = np.flatnonzero(cnt > 0)
        assert np.array_equal(r_t.cpu().numpy(), hit), ("sparse_grad row list", t)
        a, b = _hot_check(v_t.cpu().numpy(), ref[hit], np.searchsorted(hit, it), loc, gt, psw[s:e], B, ("sparse_grad values", t))
        n_bits, n_class = n_bits + a, n_class + b
        want = _bwd_oracle(coracle, kind, stores[t], it, loc, gt, psw[s:e], -0.125)
        got = _read(m, t, kind)
        cold = cnt <= R.EXACT_RUN
        _assert_same_bits(got[cold], want[cold], ("in place", t), kind)
        n_hot_val += _hot_in_place_check(_f32(got, kind), _f32(want, kind), _f32(stores[t], kind), it, loc, gt, psw[s:e], B, -0.125, kind, t)
        assert np.array_equal(got[cnt == 0], stores[t][cnt == 0])
        n_bits += int(S.is_special(want[cold], kind).sum())
    assert n_bits >= 3 * 25 * sum(dims) and n_class == 3 * S.N_HOT * sum(dims), (n_bits, n_class)
    # in place, by value: the subnormal-only hot row whole, the ordinary columns of the mixed Inf and NaN bags' rows, and the 3e38
    # row -- whole where 3 * 0.125 * 3e38 is finite in the table's type (fp32, bf16), its ordinary columns under fp16
    assert n_hot_val == sum(dims) * (5 if kind == "f16" else 6) // 2, n_hot_val


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_backward_runs_across_tile_borders_with_fix_up(coracle, weighted):
    """3-, 11- and 3000-row tables (shapes of tests/test_gpu_join_tiles.py): rows of ~16 K lookups span many tiles of the sorted
    order and are finished by the fix-up kernel from per-tile partial sums; ``dense_grad`` and the in-place ``scatter_add_``.  Gradient columns of one class in any order
    (``special_values.column_grad``; pinned on the host); the 3000-row table's rows keep the oracle's bits."""
    from param_amd import BatchedEmbeddingBagMI355

    rows, dims, B, L = [3, 11, 3000], [128, 64, 32], 2048, 24
    rng = np.random.default_rng(33 + weighted)
    m = BatchedEmbeddingBagMI355(rows, dims, device=DEV, init="normal", seed=1, fused_update=False)
    idx = np.concatenate([rng.integers(0, r, B * L) for r in rows]).astype(np.int64)
    off = np.arange(len(rows) * B + 1, dtype=np.int64) * L
    g = np.concatenate([S.column_grad(B, d, rng) for d in dims], axis=1)
    psw = S.hot_weights(len(idx), rng) if weighted else None
    dense = m.dense_grad(_t(g), _t(idx), _t(off), None if psw is None else _t(psw), batch=B)
    st = m.sort_status(_t(idx), _t(off), None if psw is None else _t(psw), batch=B)
    assert st["hybrid_tables"] == 0 and st["pairs_sorted"] == len(idx), st
    before = [_read(m, t, "f32") for t in range(3)]
    m.scatter_add_(_t(g), _t(idx), _t(off), alpha=-0.125, per_sample_weights=None if psw is None else _t(psw), batch=B)
    st = m.sort_status(_t(idx), _t(off), None if psw is None else _t(psw), batch=B)
    assert st["hybrid_tables"] == 0 and st["pairs_sorted"] == len(idx), st
    assert int(np.bincount(idx[:B * L], minlength=3).min()) > 8 * 1024            # table 0: every row spans more than 8 tiles
    n_bits = n_class = n_hot_val = 0
    for t in range(3):
        it, loc, s, e = _slice(idx, off, t, B)
        c0 = sum(dims[:t])
        gt = np.ascontiguousarray(g[:, c0:c0 + dims[t]])
        pw = None if psw is None else psw[s:e]
        ref = coracle.bwd_f32(np.zeros((rows[t], dims[t]), np.float32), it, loc, gt, pw)
        a, b = _hot_check(dense[t].cpu().numpy(), ref, it, loc, gt, pw, B, t)
        n_bits, n_class = n_bits + a, n_class + b
        want = coracle.bwd_f32(before[t].copy(), it, loc, gt, pw, alpha=-0.125)
        got_w = _read(m, t, "f32")
        cold = np.bincount(it, minlength=rows[t]) <= R.EXACT_RUN
        _assert_same_bits(got_w[cold], want[cold], ("in place", t))
        n_hot_val += _hot_in_place_check(got_w, want, before[t], it, loc, gt, pw, B, -0.125, "f32", t)
        if t < 2:                                                      # per column class, as built: +Inf, NaN, +Inf (overflow), -Inf
            got = dense[t].cpu().numpy()
            k = np.arange(dims[t]) % 6
            assert np.isposinf(got[:, (k == 1) | (k == 3)]).all() and np.isnan(got[:, k == 2]).all() and np.isneginf(got[:, k == 5]).all()
            assert np.isfinite(got[:, (k == 0) | (k == 4)]).all() and S.is_subnormal(got[:, k == 4]).any()
    assert n_class == 3 * 128 + 11 * 64 and n_bits >= 3000 * 32 // 3, (n_bits, n_class)
    assert n_hot_val == 3 * (22 + 21) + 11 * (11 + 10), n_hot_val          # the ordinary and the subnormal columns (d % 6 in (0, 4)) of every hot row


def _hybrid_case(kind, seed, T=2, D=32, B=1024, L=12, n_rows=300_000):
    """the smallest shape the hybrid route takes (tests/test_gpu_hybrid.py, test_gpu_rest.py): unweighted, fixed pooling, lookups
    <= rows / 4; a tenth of the lookups go to the special table rows, which therefore repeat and are left to the LDS kernel"""
    rng = np.random.default_rng(seed)
    rows = [n_rows] * T
    n2 = 2 * S.n_special_rows(kind)
    stores = [S.special_table(r, D, rng, kind)[0] for r in rows]
    idx = np.concatenate([np.where(rng.random(B * L) < 0.1, rng.integers(0, n2, B * L), rng.integers(0, r, B * L)) for r in rows]).astype(np.int64)
    for t in range(T):                                            # row n2 + 1: looked up twice, by the bags of 1e-45 and of 1e-40 gradients
        idx[t * B * L + 5 * L] = idx[t * B * L + 7 * L] = n2 + 1
    off = np.arange(T * B + 1, dtype=np.int64) * L
    g = np.concatenate([S.special_grad(B, D, rng) for _ in rows], axis=1)
    return rows, stores, idx, off, g


def _assert_hybrid_lds(st, T):
    assert st["hybrid_tables"] == T and st["hybrid_launched"] and st["lds_tables"] == T and st["lds_pairs"] > 0 and st["pairs_sorted"] == 0, st


@pytest.mark.parametrize("kind", S.KINDS)
def test_backward_hybrid_bag_major_and_lds_leftovers(coracle, kind):
    """The hybrid route forced on: rows looked up once are applied by the bag-major kernel, the flagged repeats -- every special
    table row among them -- sorted and walked in LDS.  Every row keeps the sequential oracle's bits (the LDS walk is sequential
    whatever the run length).  The route takes unweighted requests only."""
    import param_amd

    T, D, B = 2, 32, 1024
    rows, stores, idx, off, g = _hybrid_case(kind, 44)
    try:
        param_amd.set_hybrid_tuning(2, 0)
        param_amd.set_hybrid_rest(1)
        m = _module(rows, [D] * T, kind, stores, fused_update=False)
        dense = [d.cpu().numpy() for d in m.dense_grad(_t(g), _t(idx), _t(off), batch=B)]      # into zeros: subnormal sums stay subnormal
        _assert_hybrid_lds(m.sort_status(_t(idx), _t(off), batch=B), T)
        m.scatter_add_(_t(g), _t(idx), _t(off), alpha=-0.125, batch=B)
        _assert_hybrid_lds(m.sort_status(_t(idx), _t(off), batch=B), T)
    finally:
        param_amd.set_hybrid_tuning()
        param_amd.set_hybrid_rest()
    n_bits = 0
    for t in range(T):
        it, loc, s, e = _slice(idx, off, t, B)
        gt = np.ascontiguousarray(g[:, t * D:(t + 1) * D])
        want = _bwd_oracle(coracle, kind, stores[t], it, loc, gt, None, -0.125)
        got = _read(m, t, kind)
        _assert_same_bits(got, want, ("hybrid", t), kind)
        cnt = np.bincount(it, minlength=rows[t])
        ref = coracle.bwd_f32(np.zeros((rows[t], D), np.float32), it, loc, gt)
        _assert_same_bits(dense[t], ref, ("hybrid, dense_grad", t))
        n_bits += int(S.is_special(want[cnt > 0], kind).sum())
        assert int(S.is_special(want[cnt == 1], kind).sum()) >= 20 * D        # the bag-major kernel saw special gradients too
        sub2 = 2 * S.n_special_rows(kind) + 1                     # a repeated row (left to the LDS kernel) whose sum is subnormal
        assert int(S.is_subnormal(ref[cnt == 1]).sum()) >= 2 * D and cnt[sub2] == 2 and S.is_subnormal(ref[sub2]).all(), t
    assert n_bits >= T * 60 * D, n_bits


# ============================================================================= Adagrad, both flavours
def _elem_expect(m, kind, stores, s_old, g, idx, off, psw, B):
    """per table (w_pre fp32, s_new, touched, cold) from the restatement the host test pins to torch.optim.Adagrad"""
    out = []
    for t, (r, d) in enumerate(zip(m.rows, m.dims)):
        it, loc, s, e = _slice(idx, off, t, B)
        c0 = sum(m.dims[:t])
        with np.errstate(all="ignore"):
            G, cnt = E.grad_sum_f32(r, it, loc, np.ascontiguousarray(g[:, c0:c0 + d]), None if psw is None else psw[s:e])
            w_pre, s_new = E.step_f32(_f32(stores[t], kind), s_old[t], G, cnt > 0, m.learning_rate, m.eps, m.weight_decay, WD[m.weight_decay_mode])
        out.append((w_pre, s_new, cnt > 0, (cnt > 0) & (cnt <= R.EXACT_RUN)))
    return out


def _seed_states(m, rows):
    """a state that starts at a subnormal and one that starts at the largest finite value, on rows the request touches"""
    s_old = []
    for t, r in enumerate(rows):
        st = m.momentum_table(t)
        st.zero_()
        st[3] = 1e-40
        st[20] = float(S.FLT_MAX)
        s_old.append(st.cpu().numpy().copy())
    return s_old


@pytest.mark.parametrize("route", ["sorted", "hybrid_lds"])
@pytest.mark.parametrize("wd_mode", [None, "l2", "decouple"], ids=["none", "l2", "decouple"])
def test_elementwise_adagrad_fp32_tables_same_bits(wd_mode, route):
    """``optimizer="adagrad"`` through ``adagrad_step_`` and through the fused ``.backward()``: tables and state bit for bit equal
    to ``elem_adagrad_rules.step_f32`` on rows within the exact-run limit (torch.optim.Adagrad pins that restatement on special
    gradients in tests/test_special_values_host.py); on the rows beyond, the restatement's class and finite values within
    ``elem_adagrad_rules.step_fp64``'s bound plus the torch pin's bars; states that start at a
    subnormal and at FLT_MAX; untouched rows untouched.  Routes: sorted apply; hybrid bag-major with LDS left-overs."""
    import param_amd

    if route == "sorted":
        dims, B = [64, 16], 600
        rows, stores, idx, off, psw, g = _backward_case("f32", dims, B, 51, extra_rows=1500)
    else:
        dims, B, psw = [32, 32], 1024, None
        rows, stores, idx, off, g = _hybrid_case("f32", 52)
    p_t = None if psw is None else _t(psw)
    kw = dict(optimizer="adagrad", learning_rate=0.05, eps=1e-6, weight_decay=0.01 if wd_mode else 0.0, weight_decay_mode=wd_mode)
    res = {}
    try:
        if route != "sorted":
            param_amd.set_hybrid_tuning(2, 0)
            param_amd.set_hybrid_rest(1)
        for how in ("step", "backward"):
            m = _module(rows, dims, "f32", stores, fused_update=True, **kw)
            s_old = _seed_states(m, rows)
            if how == "step":
                m.adagrad_step_(_t(g), _t(idx), _t(off), p_t, batch=B)
            else:
                m(_t(idx), _t(off), p_t).backward(_t(g))
            st = m.sort_status(_t(idx), _t(off), p_t, batch=B)
            if route == "sorted":
                assert st["hybrid_tables"] == 0 and st["pairs_sorted"] == len(idx), st
            else:
                _assert_hybrid_lds(st, 2)
            res[how] = ([_read(m, t, "f32") for t in range(2)], [m.momentum_table(t).cpu().numpy().copy() for t in range(2)])
    finally:
        param_amd.set_hybrid_tuning()
        param_amd.set_hybrid_rest()
    n_bits = n_hot_val = 0
    for t, (w_exp, s_exp, touched, cold) in enumerate(_elem_expect(m, "f32", stores, s_old, g, idx, off, psw, B)):
        for how in ("step", "backward"):
            gw, gs = res[how][0][t], res[how][1][t]
            _assert_same_bits(gs[cold], s_exp[cold], (how, "state", t))
            _assert_same_bits(gw[cold], w_exp[cold], (how, "weights", t))
            assert np.array_equal(gw[~touched], stores[t][~touched]) and np.array_equal(gs[~touched], s_old[t][~touched])
            hot = touched & ~cold
            if hot.any():      # the restatement's class; finite values within the fp64 evaluation's bound for a sum formed in another order
                it, loc, s, e = _slice(idx, off, t, B)
                gt = np.ascontiguousarray(g[:, sum(dims[:t]):sum(dims[:t + 1])])
                with np.errstate(all="ignore"):
                    W64, S64, dw, ds, _ = E.step_fp64(stores[t], s_old[t], it, loc, gt, None if psw is None else psw[s:e], kw["learning_rate"], kw["eps"], kw["weight_decay"],
                                                      WD[wd_mode])
                    fw, fs = np.isfinite(w_exp), np.isfinite(s_exp)
                    lim_w = np.where(fw, dw + E.W_RTOL * np.abs(W64) + E.W_ATOL, 0.0)
                    lim_s = np.where(fs, ds + E.STATE_RTOL * S64, 0.0)
                assert S.same_class(gw[hot], np.where(fw, W64, w_exp)[hot], 0.0, lim_w[hot]), (how, "hot rows, weights", t)
                assert S.same_class(gs[hot], np.where(fs, S64, s_exp)[hot], 0.0, lim_s[hot]), (how, "hot rows, state", t)
                n_hot_val += int(fw[hot].sum())
        n_bits += int(S.is_special(w_exp[cold]).sum()) + int(S.is_special(s_exp[cold]).sum())
        assert touched[3] and touched[20] and (s_exp[3] != s_old[t][3]).any() and not (s_exp[20] < S.FLT_MAX).any()
    assert n_bits >= 2 * 20 * sum(dims), n_bits
    assert n_hot_val >= (2 * sum(dims) if route == "sorted" else 0), n_hot_val      # (the hybrid request has no row beyond the limit)


def test_elementwise_adagrad_eps_zero_and_a_zero_gradient_sum_give_nan_as_torch():
    rows, D = [40], 16
    W = [np.full((40, 16), 0.25, np.float32)]
    m = _module(rows, [D], "f32", W, optimizer="adagrad", learning_rate=0.05, eps=0.0)
    g = np.zeros((2, D), np.float32)
    g[1] = 2.0
    g[0, 1::2] = -0.0
    m.adagrad_step_(_t(g), _t(np.array([5, 9], np.int64)), _t(np.array([0, 1, 2], np.int64)), batch=2)
    w, s = m.table(0).cpu().numpy(), m.momentum_table(0).cpu().numpy()
    assert np.isnan(w[5]).all() and (s[5].view(np.uint32) == 0).all()                  # 0 / (sqrt(0) + 0)
    assert (w[9] == np.float32(0.25) - np.float32(0.05)).all() and (s[9] == 4.0).all()
    assert np.array_equal(np.delete(w, [5, 9], axis=0), np.delete(W[0], [5, 9], axis=0))
    p = torch.nn.Parameter(torch.full((1, D), 0.25))
    opt = torch.optim.Adagrad([p], lr=0.05, eps=0.0)
    p.grad = torch.from_numpy(g[:1].copy())
    opt.step()
    assert torch.isnan(p).all()


@pytest.mark.parametrize("route", ["sorted", "hybrid_lds"])
@pytest.mark.parametrize("wd_mode", [None, "l2", "decouple"], ids=["none", "l2", "decouple"])
@pytest.mark.parametrize("kind,flavour", [("f32", "rowwise_adagrad"), ("bf16", "rowwise_adagrad"), ("f16", "rowwise_adagrad"),
                                          ("bf16", "adagrad"), ("f16", "adagrad")])
def test_adagrad_16bit_and_rowwise_class_and_nearest(coracle, kind, flavour, wd_mode, route):
    """Row-wise Adagrad on every table type and element-wise Adagrad on 16-bit tables, through ``adagrad_step_`` and through the
    fused ``.backward()``, on the sorted route and on the hybrid route (bag-major kernel for rows looked up once, LDS left-over
    kernel for the repeats: their own reduction and store code); rows within the exact-run limit.  Finite values before rounding:
    ``lowp_rules.nearest_ratio <= 1`` with ``tol_b`` (16-bit tables) or the fuzz test's bars (fp32, row-wise); everything else by
    class.  A touched row whose gradient sum is zero keeps its bits and its state (no weight decay, eps > 0) -- bit for bit, -0
    included.  (fp32 tables under element-wise Adagrad are held to the bit by test_elementwise_adagrad_fp32_tables_same_bits.)"""
    import param_amd

    lr, eps, wd = 0.05, 1e-6, 0.01 if wd_mode else 0.0
    if route == "sorted":
        dims, B = [64, 16], 600
        rows, stores, idx, off, psw, g = _backward_case(kind, dims, B, 61, hot=False, extra_rows=1500)
        zero_rows = [[r - 5, r - 6] for r in rows]                 # looked up once, by the +0 / the -0 gradient bag
    else:
        dims, B, psw = [32, 32], 1024, None
        rows, stores, idx, off, g = _hybrid_case(kind, 62)
        zero_rows = []
        for t in range(2):                                          # rows whose every lookup comes from bag 0 (+0) or bag 1 (-0)
            it, loc, s, e = _slice(idx, off, t, B)
            last_bag = np.full(rows[t], -1)
            np.maximum.at(last_bag, it, np.repeat(np.arange(B), 12))
            zero_rows.append(np.flatnonzero((last_bag >= 0) & (last_bag <= 1)).tolist())
            assert len(zero_rows[t]) >= 4
    p_t = None if psw is None else _t(psw)
    res = {}
    try:
        if route != "sorted":
            param_amd.set_hybrid_tuning(2, 0)
            param_amd.set_hybrid_rest(1)
        for how in ("step", "backward"):
            m = _module(rows, dims, kind, stores, optimizer=flavour, learning_rate=lr, eps=eps, weight_decay=wd, weight_decay_mode=wd_mode,
                        fused_update=True)
            s_old = _seed_states(m, rows)
            if how == "step":
                m.adagrad_step_(_t(g), _t(idx), _t(off), p_t, batch=B)
            else:
                m(_t(idx), _t(off), p_t).backward(_t(g))
            st = m.sort_status(_t(idx), _t(off), p_t, batch=B)
            if route == "sorted":
                assert st["hybrid_tables"] == 0 and st["pairs_sorted"] == len(idx), st
            else:
                _assert_hybrid_lds(st, 2)
            res[how] = ([_read(m, t, kind) for t in range(2)], [m.momentum_table(t).cpu().numpy().copy() for t in range(2)])
    finally:
        param_amd.set_hybrid_tuning()
        param_amd.set_hybrid_rest()
    if flavour == "adagrad":
        expect = _elem_expect(m, kind, stores, s_old, g, idx, off, psw, B)
    else:
        expect = []
        for t in range(2):
            it, loc, s, e = _slice(idx, off, t, B)
            gt = np.ascontiguousarray(g[:, sum(dims[:t]):sum(dims[:t + 1])])
            pw = None if psw is None else psw[s:e]
            mom = s_old[t].copy()
            if kind == "f32":
                w_pre, _ = coracle.bwd_rowwise_adagrad(stores[t].copy(), mom, it, loc, gt, pw, lr=lr, eps=eps, weight_decay=wd,
                                                       weight_decay_mode=WD_ROW[wd_mode])
            else:
                _, _, w_pre = coracle.bwd_rowwise_adagrad(stores[t].copy(), mom, it, loc, gt, pw, lr=lr, eps=eps, weight_decay=wd,
                                                          weight_decay_mode=WD_ROW[wd_mode], dtype=CODE[kind])
            touched = np.bincount(it, minlength=rows[t]) > 0
            expect.append((w_pre, mom, touched, touched))
    n_fin = n_cls = 0
    for how in ("step", "backward"):
        for t, (w_pre, s_exp, touched, cold) in enumerate(expect):
            got_store, gs = res[how][0][t], res[how][1][t]
            got = _f32(got_store, kind)
            assert np.array_equal(got_store[~touched], stores[t][~touched]) and np.array_equal(gs[~touched], s_old[t][~touched]), (how, t)
            # state: element-wise is exact arithmetic per element (the restatement's bits); row-wise reduces a row in another order
            if flavour == "adagrad":
                _assert_same_bits(gs[cold], s_exp[cold], (how, "state", t))
            else:
                assert S.same_class(gs[cold], s_exp[cold], 3e-5, 1e-10), (how, "state", t)
            wp, gg = w_pre[cold].astype(np.float64), got[cold].astype(np.float64)
            top = O.max16(CODE[kind]) if kind != "f32" else float(S.FLT_MAX)
            fin = np.isfinite(wp) & (np.abs(wp) < top)
            if flavour == "rowwise_adagrad":                       # a row whose state is not finite is compared by class alone
                fin &= np.isfinite(s_exp[cold])[:, None]
            if kind == "f32":
                assert np.allclose(gg[fin], wp[fin], rtol=3e-5, atol=3e-6), (how, "weights", t)
            else:
                ratio = R.nearest_ratio(gg[fin], wp[fin], CODE[kind], R.tol_b(wp[fin]))
                assert ratio.max() <= 1.0, (how, "weights", t, float(ratio.max()))
            if flavour == "adagrad":                                # at or past the largest finite value: it, or the Inf above it
                edge = np.isfinite(wp) & ~fin & np.isfinite(gg)
                assert (np.abs(gg[edge]) >= top).all(), (how, t)
            rest = ~np.isfinite(wp)
            assert S.same_nonfinite(gg[rest], wp[rest]), (how, "class", t, S.first_difference(gg[rest].astype(np.float32), wp[rest].astype(np.float32)))
            n_fin, n_cls = n_fin + int(fin.sum()), n_cls + int(rest.sum())
            if wd_mode is None:
                for r in zero_rows[t]:
                    assert touched[r] and np.array_equal(got_store[r], stores[t][r]) and np.array_equal(gs[r], s_old[t][r]), (how, t, r)
    assert n_fin >= 2 * 100 * sum(dims) and n_cls >= 2 * 4 * sum(dims), (n_fin, n_cls)


# ============================================================================= stochastic rounding
def _sr_case(kind, flavour):
    rng = np.random.default_rng(71)
    D, B = 16, 80
    n2 = 2 * S.n_special_rows(kind)
    rows = n2 + 30
    store, w = S.special_table(rows, D, rng, kind)
    assert rows <= B
    idx = np.arange(rows, dtype=np.int64)                          # bag b looks up row b, once; the bags from `rows` on are empty
    off = np.minimum(np.arange(B + 1, dtype=np.int64), rows)
    return rows, D, B, store, w, idx, off, rng


@pytest.mark.parametrize("flavour", ["adagrad", "rowwise_adagrad"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_stochastic_rounding_keeps_specials_and_representable_values_over_64_seeds(coracle, kind, flavour):
    """One small request, 64 seeds.  (1) A zero update leaves a table of representable values -- +-0, the subnormals, the largest
    finite, +-Inf; NaN stays NaN -- bit-identical for every seed.  (2) A real update: NaN stays NaN, Inf keeps its sign, every stored value is one
    of the two neighbours of the value before rounding (``down16`` / ``up16``: above the largest finite value that neighbour is
    Inf), and both neighbours do occur.  Element-wise, where the restatement's value before rounding IS the kernel's, a value the
    table type holds exactly must be stored as it is; row-wise the oracle's value is only within ``tol_b`` of the kernel's, so there
    the neighbours are those of that interval and exactness is shown by part (1) alone."""
    code = CODE[kind]
    rows, D, B, store, w, idx, off, rng = _sr_case(kind, flavour)
    lr, eps = 0.05, 1e-6
    m = _module([rows], [D], kind, [store], optimizer=flavour, learning_rate=lr, eps=eps, stochastic_rounding=True)
    i_t, o_t = _t(idx), _t(off)
    zero = torch.zeros(B, D, device=DEV)
    touched = np.bincount(idx, minlength=rows) > 0
    assert touched[:2 * S.n_special_rows(kind)].all()
    for seed in range(64):
        _fill(m, kind, [store])
        m.momentum_table(0).zero_()
        m._sr_step = seed
        m.adagrad_step_(zero, i_t, o_t, batch=B)
        _assert_same_bits(_read(m, 0, kind), store, ("zero update", seed), kind)
    assert not m.momentum_table(0).any()
    # (2) finite special and ordinary gradients (an Inf or NaN gradient makes a NaN row: covered by the class tests above).  An
    # Adagrad step is at most about lr long: the second learning rate is the one that carries the largest finite rows past the end.
    g = S.special_grad(B, D, rng, specials=S.F32_FINITE_SPECIALS)
    g[g > 1e30] = 100.0
    g[g < -1e30] = -100.0                                             # (lr * g must stay finite under the second learning rate)
    past_the_end = 0
    for lr in (0.05, 1e36 if kind == "bf16" else 16.0):
        m.learning_rate = lr
        if flavour == "adagrad":
            with np.errstate(all="ignore"):
                G, cnt = E.grad_sum_f32(rows, idx, off[:-1], g)
                w_pre, _ = E.step_f32(w, np.zeros((rows, D), np.float32), G, cnt > 0, lr, eps)
            b = np.zeros(w_pre.shape)                                      # the restatement's bits are the kernel's
        else:
            _, _, w_pre = coracle.bwd_rowwise_adagrad(store.copy(), np.zeros(rows, np.float32), idx, off[:-1], g, lr=lr, eps=eps, dtype=code)
            with np.errstate(all="ignore"):
                b = R.tol_b(np.where(np.isfinite(w_pre), w_pre, 0.0))
        wp = w_pre.astype(np.float64)
        with np.errstate(all="ignore"):
            lo, hi = O.down16(wp - b, code), O.up16(wp + b, code)
            exact = np.isfinite(wp) & (O.down16(wp, code) == wp) & (flavour == "adagrad")
        nan, inf = np.isnan(wp), np.isinf(wp)
        rest = ~nan & ~inf
        went_up, went_down = np.zeros(wp.shape, bool), np.zeros(wp.shape, bool)
        for seed in range(64):
            _fill(m, kind, [store])
            m.momentum_table(0).zero_()
            m._sr_step = seed
            m.adagrad_step_(_t(g), i_t, o_t, batch=B)
            bits = _read(m, 0, kind)
            got = S.widen16(bits, kind).astype(np.float64)
            assert np.array_equal(bits[~touched], store[~touched])
            assert np.isnan(got[nan]).all() and np.array_equal(got[inf], wp[inf]), (lr, seed)
            assert np.array_equal(got[exact], wp[exact]) and np.array_equal(np.signbit(got[exact]), np.signbit(wp[exact])), (lr, seed)
            assert ((got[rest] >= lo[rest]) & (got[rest] <= hi[rest])).all(), (lr, seed, "a stored value that is no neighbour of the value before rounding")
            went_up |= rest & (got > wp)
            went_down |= rest & (got < wp)
        between = rest & (lo != hi) & touched[:, None]
        if lr == 0.05:
            assert between.sum() >= 20 * D and (went_up & went_down)[between].mean() > 0.5
            assert int(nan.sum()) >= D and int(inf.sum()) >= 2 * D and (flavour != "adagrad" or int(exact.sum()) >= 1)
        past = rest & (np.abs(wp) > O.max16(code))                    # stored as the largest finite value or as the Inf above it
        past_the_end += int(past.sum())
        assert np.isinf(np.where(wp > 0, hi, lo)[past]).all()
    assert past_the_end >= 1, "no value before rounding lay past the largest finite value of the table type"
