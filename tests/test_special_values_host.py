"""NaN, Inf, signed zeros and subnormals through the CHECKERS (no device): the oracle's forward (C and numpy forms), the element-wise
Adagrad restatement and the row-wise quantiser restatement against what torch computes on the CPU -- committed
(tests/golden/special_values.npz, written by tests/golden/gen_special_values.py) and live -- with ``special_values.same_bits``:
NaN at the same places, every other bit equal (the sign of zero and of Inf included).  Row-wise Adagrad restates fbgemm, which is not
at hand: property checks of the oracle only.  The last tests pin what the GPU tests of tests/test_gpu_special_values.py rely on for
rows beyond the exact-run limit: inputs whose sum has the same class in any order.
"""
import os

import numpy as np
import pytest
import torch

from oracle import embbag_oracle as O
from oracle import rowquant as orq
from tests import elem_adagrad_rules as E
from tests import lowp_rules as R
from tests import special_values as S
from tests.golden import gen_special_values as GEN

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "special_values.npz"))
CODE = {"f32": O.F32, "bf16": O.BF16, "f16": O.F16}


def test_the_committed_file_is_what_the_generator_writes_with_this_torch():
    now = GEN.generate()
    assert sorted(now) == sorted(GOLD.files)
    for k in GOLD.files:
        if now[k].dtype == np.uint8:
            assert np.array_equal(now[k], GOLD[k]), k
        else:
            assert S.same_bits(now[k], GOLD[k]), k


def test_same_bits_and_same_class_see_what_they_must():
    a = np.array([0.0, -0.0, np.inf, np.nan, 1e-45, 1.0], np.float32)
    assert S.same_bits(a, a.copy())
    other_nan = a.copy()
    other_nan.view(np.uint32)[3] = 0xFFC00001                     # another payload, another sign: still a NaN
    assert S.same_bits(a, other_nan)
    for i, v in ((0, -0.0), (1, 0.0), (2, -np.inf), (3, 1.0), (4, 0.0), (5, np.nan)):
        b = a.copy()
        b[i] = v
        assert not S.same_bits(a, b), i
        assert S.first_difference(a, b)[0] == (i,)
    h = S.F16_BITS.copy()
    assert S.same_bits(h, h.copy(), "f16") and not S.same_bits(h, np.where(h == 0x8000, 0, h).astype(np.uint16), "f16")
    assert S.same_bits(np.array([0x7E00], np.uint16), np.array([0xFE01], np.uint16), "f16")
    assert S.same_bits(np.array([0x7FC0], np.uint16), np.array([0x7F81], np.uint16), "bf16")
    assert not S.same_bits(np.array([0x7E00], np.uint16), np.array([0x7E01], np.uint16), "bf16")      # finite in bf16: bits count
    assert S.same_class(a, a, 0.0, 0.0) and S.same_class([1.0, np.inf], [1.0 + 1e-7, np.inf], 1e-6, 0.0)
    assert not S.same_class([1.0, np.inf], [1.0, -np.inf], 1.0, 1.0) and not S.same_class([np.nan], [np.inf], 1.0, 1.0)
    assert not S.same_class([1.0], [1.1], 1e-6, 0.0) and not S.same_class([3e38], [np.inf], 1.0, 1.0)
    assert S.is_special(S.F32_SPECIALS[:S.N_SPECIAL]).all() and not S.is_special(S.F32_SPECIALS[S.N_SPECIAL:]).any()
    assert S.is_special(S.BF16_BITS, "bf16").all() and S.is_special(S.F16_BITS, "f16").all()
    # the 16-bit neighbours: the grid value above the largest finite one is Inf
    for code, bits in ((O.BF16, S.BF16_BITS), (O.F16, S.F16_BITS)):
        top = float(S.widen16(bits[8:9], "bf16" if code == O.BF16 else "f16")[0])
        assert O.up16(top, code) == top and O.down16(top, code) == top
        assert O.up16(top * (1 + 1e-6), code) == np.inf and O.down16(top * (1 + 1e-6), code) == top
        assert O.down16(-top * (1 + 1e-6), code) == -np.inf and O.up16(-top * (1 + 1e-6), code) == -top
        assert O.up16(np.inf, code) == np.inf and O.down16(-np.inf, code) == -np.inf and np.isnan(O.up16(np.nan, code))


# ----------------------------------------------------------------------------- forward
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("D", GEN.FWD_DIMS)
@pytest.mark.parametrize("kind", S.KINDS)
def test_oracle_forward_equals_torch_on_the_special_table(coracle, kind, D, weighted):
    store, w, idx, off, psw, named = GEN.fwd_case(kind, D, weighted)
    gold = GOLD[f"fwd_{kind}_{D}_{'w' if weighted else 'u'}"]
    live = GEN.torch_fwd(GEN.torch_widen(store, kind), idx, off, psw)
    assert S.same_bits(live, gold), S.first_difference(live, gold)
    c = coracle.fwd(store, idx, off[:-1], psw, dtype=CODE[kind])
    assert S.same_bits(c, gold), ("C oracle", S.first_difference(c, gold))
    assert np.array_equal(S.widen16(store, kind), w, equal_nan=True) if kind != "f32" else True
    with np.errstate(all="ignore"):
        n = O.embbag_fwd_np(w, idx, off[:-1], psw)
    assert S.same_bits(n, gold), ("numpy oracle", S.first_difference(n, gold))
    for b, (name, rows, _, expected) in enumerate(named):
        S.check_named_bag(name, expected, gold[b], [w[r] for r in rows])
    n_nan, n_inf, n_sub, n_zero = int(np.isnan(gold).sum()), int(np.isinf(gold).sum()), int(S.is_subnormal(gold).sum()), int((gold == 0).sum())
    assert n_nan >= D and n_inf >= 2 * D and n_zero >= 4 * D and (n_sub >= D or kind == "f16"), (n_nan, n_inf, n_sub, n_zero)


# ----------------------------------------------------------------------------- element-wise Adagrad
@pytest.mark.parametrize("case", range(len(GEN.ADA_CASES)))
def test_step_f32_equals_torch_adagrad_on_the_special_gradients(case):
    """bit for bit, two steps.  torch forms ``g + wd * w`` and ``s + g * g`` fused (one rounding each); the restatement does so
    under ``torch_fused=True`` and is then torch's bits; left at its default (the kernels' arithmetic: the products rounded first) it
    stays within the torch pin's bars ``STATE_RTOL`` / ``W_RTOL`` / ``W_ATOL`` and has the same class everywhere."""
    eps, wd = GEN.ADA_CASES[case]
    w0, s0, grads = GEN.adagrad_inputs()
    w, s = w0.copy(), s0.copy()
    with np.errstate(all="ignore"):
        for g in grads:
            w, s = E.step_f32(w, s, g, np.ones(len(w), bool), GEN.ADA_LR, eps, wd, E.WD_L2 if wd else E.WD_NONE, torch_fused=True)
    lw, ls = GEN.torch_adagrad(w0, s0, grads, eps, wd)
    assert S.same_bits(lw, GOLD[f"ada_w_{case}"]) and S.same_bits(ls, GOLD[f"ada_s_{case}"])
    assert S.same_bits(s, ls), ("state", S.first_difference(s, ls))
    assert S.same_bits(w, lw), ("weights", S.first_difference(w, lw))
    assert np.isnan(lw).sum() >= 8 and S.is_special(grads[0]).sum() >= 4 * S.N_SPECIAL
    w2, s2 = w0.copy(), s0.copy()
    with np.errstate(all="ignore"):
        for g in grads:
            w2, s2 = E.step_f32(w2, s2, g, np.ones(len(w2), bool), GEN.ADA_LR, eps, wd, E.WD_L2 if wd else E.WD_NONE)
    assert S.same_class(s2, ls, E.STATE_RTOL, 0.0) and S.same_class(w2, lw, E.W_RTOL, E.W_ATOL)
    if eps == 0.0 and wd == 0.0:                           # a zero gradient on a zero state: 0 / 0, as torch gives
        zero_g = (grads[0] == 0) & (grads[1] == 0) & (s0 == 0)
        assert zero_g.any() and np.isnan(lw[zero_g]).all() and np.isnan(w[zero_g]).all()


# ----------------------------------------------------------------------------- the quantiser
@pytest.mark.parametrize("bits", (8, 4, 2))
@pytest.mark.parametrize("dim", GEN.QUANT_DIMS)
def test_rowquant_oracle_equals_torch_on_the_edge_rows(dim, bits):
    x = GEN.quant_rows(dim)
    n_edge = len(S.quant_edge_rows(dim)[1])
    pack, unpack = (getattr(torch.ops.quantized, n) for n in GEN.PACK[bits])
    live = pack(torch.from_numpy(x)).numpy()
    assert np.array_equal(live, GOLD[f"q{bits}_{dim}"])
    q = orq.quantize_rows(x, bits)
    for i in range(len(x)):
        name = S.quant_edge_rows(dim)[1][i] if i < n_edge else f"mixed_zero_{i - n_edge}"
        assert np.array_equal(q[i], live[i]), (name, q[i][-8:], live[i][-8:])
    d = orq.dequantize_rows(live, dim, bits)
    assert S.same_bits(d, unpack(torch.from_numpy(live)).numpy()) and S.same_bits(d, GOLD[f"d{bits}_{dim}"])


@pytest.mark.parametrize("bits", (8, 4, 2))
def test_rowquant_bias_carries_the_sign_of_the_first_zero(bits):
    """the rows numpy's ``min`` got wrong: minimum zero, both zero signs present.  torch (std::min_element) keeps the first."""
    for dim in (8, 32, 96, 128):
        x = S.quant_mixed_zero_rows(dim)
        q = orq.quantize_rows(x, bits)
        live = getattr(torch.ops.quantized, GEN.PACK[bits][0])(torch.from_numpy(x)).numpy()
        assert np.array_equal(q, live), (dim, q[:, -8:], live[:, -8:])
        first_zero = np.array([row[np.flatnonzero(row == 0)[0]] for row in x])
        assert np.array_equal(q[:, -1] >> 7, np.signbit(first_zero).astype(np.uint8)), dim      # the bias field's top byte ends the row
        assert set((q[:, -1] >> 7).tolist()) == {0, 1}
        if bits == 8:
            assert not q[:2, dim:dim + 4].any()                                                   # a zero range is +0, never -0


def test_rowquant_16_bits_is_torchs_cast_on_the_full_special_set():
    x = np.concatenate(S.special_rows_f32(8), axis=0)
    want = torch.from_numpy(x).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    got = orq.quantize_rows(x, 16).view(np.uint16)
    assert S.same_bits(got, want, "f16")
    assert S.same_bits(orq.dequantize_rows(got.view(np.uint8), 8, 16), torch.from_numpy(x).to(torch.float16).float().numpy())
    assert S.is_nan(got, "f16").sum() == 8 + 4 and (got == 0x8000).sum() >= 8 and (got == 0xFC00).sum() >= 8 * 3


# ----------------------------------------------------------------------------- row-wise Adagrad: properties of the oracle
@pytest.mark.parametrize("wd_code", [0, 1, 2])
@pytest.mark.parametrize("kind", S.KINDS)
def test_rowwise_adagrad_oracle_zero_gradient_row_and_nonfinite_gradients(coracle, kind, wd_code):
    """(a) a touched row whose gradient sum is all zeros (of either sign) keeps weights and state bit for bit at eps > 0 without
    weight decay; (b) Inf and NaN gradients land where an fp64 evaluation says they must (``same_class``, bars ``lowp_rules.tol_b``
    and the fuzz test's state bar)"""
    rng = np.random.default_rng(5)
    D, B, lr, eps, wd = 16, 2 * S.N_SPECIAL + 6, 0.05, 1e-6, 0.01 if wd_code else 0.0
    rows = 2 * S.n_special_rows(kind) + 40
    store, w = S.special_table(rows, D, rng, kind)
    g = S.special_grad(B, D, rng)
    # bag b looks up row (rows - 1 - b) (an ordinary table row) and special row b % (2n): one lookup per row or two
    idx = np.stack([rows - 1 - np.arange(B), np.arange(B) % (2 * S.n_special_rows(kind))], axis=1).reshape(-1).astype(np.int64)
    off = np.arange(B, dtype=np.int64) * 2
    mom0 = rng.uniform(0.5, 2.0, rows).astype(np.float32)
    mom0[rows - 1], mom0[rows - 2] = 1e-40, S.FLT_MAX
    mom = mom0.copy()
    if kind == "f32":
        W = w.copy()
        coracle.bwd_rowwise_adagrad(W, mom, idx, off, g, lr=lr, eps=eps, weight_decay=wd, weight_decay_mode=wd_code)
        got = W
    else:
        Wb = store.copy()
        coracle.bwd_rowwise_adagrad(Wb, mom, idx, off, g, lr=lr, eps=eps, weight_decay=wd, weight_decay_mode=wd_code, dtype=CODE[kind])
        got = S.widen16(Wb, kind)
    if wd_code == 0:
        for b in (0, 1):                                                    # the +0 and the -0 gradient bags
            r = rows - 1 - b
            assert S.same_bits(got[r], w[r]) and mom[r] == mom0[r], b
    # the same step in fp64 with fp32's range: a state that overflows fp32 is Inf (then mult = 0)
    with np.errstate(all="ignore"):
        G = np.zeros((rows, D))
        np.add.at(G, idx, g.astype(np.float64)[np.repeat(np.arange(B), 2)])
        gx = G + wd * w if wd_code == 1 else G
        m64 = (mom0 + (gx ** 2).mean(1)).astype(np.float32).astype(np.float64)
        mult = lr / (np.sqrt(m64) + eps)
        corr = 1.0 - (mult * wd if wd_code == 1 else np.full_like(mult, lr * wd if wd_code == 2 else 0.0))
        W64 = corr[:, None] * w - mult[:, None] * G
        touched = np.bincount(idx, minlength=rows) > 0
        W64, m64 = np.where(touched[:, None], W64, w), np.where(touched, m64, mom0)
        W32 = W64.astype(np.float32)
    assert S.same_class(mom, m64, 3e-5, 1e-10), S.first_difference(mom, m64.astype(np.float32))
    fin = np.isfinite(W64)
    half = 0 if kind == "f32" else O.ulp16(np.where(fin, W64, 0.0), CODE[kind]) / 2
    # (near the top of fp32 a finite fp64 value may round to Inf in fp32: W32 is the class, W64 the value)
    assert S.same_class(got, W32, 0.0, R.tol_b(np.where(fin, W64, 0.0)) + half), S.first_difference(got, W32)
    assert np.isnan(got).sum() >= 3 * D and np.isnan(m64).sum() >= 3 and np.isinf(m64).sum() >= 6 and touched.sum() >= B


# ----------------------------------------------------------------------------- what the GPU tests assume of their hot rows
def test_one_sign_inputs_have_one_class_in_any_order(coracle):
    """Rows beyond the exact-run limit are summed by the kernels in another order than the oracle's.  The inputs the GPU tests give
    such rows (``special_values.column_grad``: per column +Inf, NaN, -Inf or +3e38 sprinkled over ordinary values, or subnormals
    only; weights >= 0) must give a sum whose class does not depend on the order: the oracle's lookup-order fp32 result, the same
    lookups in reverse and in a shuffled order, and the fp64 sum rounded to fp32 agree in class, and where finite within ``tol_sorted``."""
    rng = np.random.default_rng(9)
    B, D, rows, L = 2048, 24, 3, 4
    g = S.column_grad(B, D, rng)
    idx = rng.integers(0, rows, B * L).astype(np.int64)
    off = np.arange(B, dtype=np.int64) * L
    psw = S.hot_weights(B * L, rng)
    ref = coracle.bwd_f32(np.zeros((rows, D), np.float32), idx, off, g, psw)
    bag_of = np.repeat(np.arange(B), L)
    with np.errstate(all="ignore"):
        contrib32 = (psw[:, None] * g[bag_of]).astype(np.float32)
        contrib = g.astype(np.float64)[bag_of] * psw.astype(np.float64)[:, None]
        truth, mag = np.zeros((rows, D)), np.zeros((rows, D))
        np.add.at(truth, idx, contrib)
        np.add.at(mag, idx, np.abs(contrib))
        t32 = truth.astype(np.float32)
        for order in (np.arange(B * L)[::-1], rng.permutation(B * L)):
            acc = np.zeros((rows, D), np.float32)
            for j in order:
                acc[idx[j]] = acc[idx[j]] + contrib32[j]
            assert S.same_class(acc, ref, 0.0, np.where(np.isfinite(mag), 1e-5 * mag, 0.0) + 1e-30)
    cnt = np.bincount(idx, minlength=rows).astype(np.float64)[:, None]
    assert cnt.min() > R.EXACT_RUN
    tol = np.maximum(1e-5, (256 + cnt / 32) * 2.0 ** -24) * np.where(np.isfinite(mag), mag, 0.0) + 1e-30
    assert S.same_class(ref, t32, 0.0, tol)
    cls = [int(f(ref).sum()) for f in (np.isnan, np.isposinf, np.isneginf)]
    assert cls == [rows * 4, rows * 8, rows * 4] and int((np.isfinite(ref) & (ref != 0)).sum()) == rows * 8, cls
