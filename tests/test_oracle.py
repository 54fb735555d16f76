"""Pin the oracle (oracle/) against the committed torch golden vectors (CPU only).

The reference's own tests pin nothing at the EmbeddingBag boundary, so the
goldens are outputs of torch.nn.EmbeddingBag -- the engine the reference calls -- generated
by tests/golden/gen_golden.py in the build container.
"""
import numpy as np
import pytest

from oracle import embbag_oracle as O


def _single(meta):
    return [n for n, m in meta.items() if "tables" not in m]


def _psw(data, name):
    return data[f"{name}.psw"] if f"{name}.psw" in data.files else None


def test_c_oracle_forward_bit_exact(cases, coracle):
    data, meta = cases
    for name in _single(meta):
        out = coracle.fwd(data[f"{name}.W"], data[f"{name}.idx"], data[f"{name}.off"], _psw(data, name))
        assert np.array_equal(out, data[f"{name}.out"]), name


def test_numpy_oracle_forward_bit_exact(cases):
    data, meta = cases
    for name in _single(meta):
        if meta[name]["n_idx"] > 4000:
            continue  # python loop: keep the CPU suite fast
        out = O.embbag_fwd_np(data[f"{name}.W"], data[f"{name}.idx"], data[f"{name}.off"], _psw(data, name))
        assert np.array_equal(out, data[f"{name}.out"]), name


def test_c_oracle_batched_bit_exact(cases, coracle):
    data, meta = cases
    for name, m in meta.items():
        if "tables" not in m:
            continue
        tabs = [data[f"{name}.W{t}"] for t in range(m["tables"])]
        out = coracle.fwd_batched(tabs, data[f"{name}.idx"], data[f"{name}.off"], m["bags"])
        assert np.array_equal(out, data[f"{name}.out"]), name
        out_np = O.embbag_fwd_batched_np(tabs, data[f"{name}.idx"], data[f"{name}.off"], m["bags"])
        assert np.array_equal(out_np, data[f"{name}.out"]), name
        if len({t.shape[1] for t in tabs}) == 1:  # [T,B,D] layout = same numbers, stacked
            tbd = coracle.fwd_batched(tabs, data[f"{name}.idx"], data[f"{name}.off"], m["bags"], layout="tbd")
            D = tabs[0].shape[1]
            for t in range(len(tabs)):
                assert np.array_equal(tbd[t], data[f"{name}.out"][:, t * D:(t + 1) * D])


def _bwd_tol(data, name):
    """1e-5 relative to the magnitude of what was accumulated into each row element:
    sum_j |alpha*psw_j*grad[bag(j),d]| (torch's dense backward adds in a different order)."""
    idx, off, grad = data[f"{name}.idx"], data[f"{name}.off"], data[f"{name}.grad"]
    psw = _psw(data, name)
    W = data[f"{name}.W"]
    mag = np.zeros(W.shape, dtype=np.float64)
    start, end = O.bag_bounds(off, len(off), len(idx))
    for b in range(len(off)):
        for j in range(start[b], end[b]):
            mag[idx[j]] += np.abs(grad[b].astype(np.float64)) * (1.0 if psw is None else abs(float(psw[j])))
    return 1e-5 * mag + 1e-30


def test_c_oracle_backward_matches_torch_dense_grad(cases, coracle):
    data, meta = cases
    for name in _single(meta):
        W = data[f"{name}.W"]
        dW = coracle.bwd_f32(np.zeros_like(W), data[f"{name}.idx"], data[f"{name}.off"],
                             data[f"{name}.grad"], _psw(data, name))
        err = np.abs(dW.astype(np.float64) - data[f"{name}.dW"].astype(np.float64))
        assert (err <= _bwd_tol(data, name)).all(), (name, err.max())
        # rows never looked up stay exactly zero
        touched = np.zeros(W.shape[0], dtype=bool)
        touched[data[f"{name}.idx"]] = True
        assert not dW[~touched].any()


def test_numpy_backward_equals_c_backward(cases, coracle):
    data, meta = cases
    for name in ("u_d32", "ragged_d56", "psw_d64", "gather_l1"):
        W = data[f"{name}.W"]
        a = coracle.bwd_f32(np.zeros_like(W), data[f"{name}.idx"], data[f"{name}.off"], data[f"{name}.grad"],
                            _psw(data, name), alpha=-0.05)
        b = O.embbag_bwd_np(W.shape[0], data[f"{name}.idx"], data[f"{name}.off"], data[f"{name}.grad"],
                            _psw(data, name), alpha=-0.05)
        assert np.array_equal(a, b), name


def test_16bit_tables_widen_then_fp32_accumulate(cases, coracle):
    data, _ = cases
    out = coracle.fwd(data["bf16_d128.W_bits"], data["bf16_d128.idx"], data["bf16_d128.off"], dtype=O.BF16)
    assert np.array_equal(out, data["bf16_d128.out"])
    assert np.array_equal(O.bf16_bits_to_f32(data["bf16_d128.W_bits"]), data["bf16_d128.W"])
    out = coracle.fwd(data["f16_d64.W_f16"], data["f16_d64.idx"], data["f16_d64.off"])
    assert np.array_equal(out, data["f16_d64.out"])


def test_int32_twin_is_same_request(cases, coracle):
    data, _ = cases
    assert np.array_equal(data["u_d32.idx_i32"].astype(np.int64), data["u_d32.idx"])
    out = coracle.fwd(data["u_d32.W"], data["u_d32.idx_i32"], data["u_d32.off_i32"])
    assert np.array_equal(out, data["u_d32.out"])


def test_bf16_backward_rounds_once(coracle):
    rng = np.random.default_rng(3)
    W = rng.standard_normal((50, 16)).astype(np.float32)
    bits = O.f32_to_bf16_bits(W)
    idx = rng.integers(0, 50, 60)
    off = np.arange(6) * 10
    grad = rng.standard_normal((6, 16)).astype(np.float32)
    expect = O.f32_to_bf16_bits(O.embbag_bwd_np(50, idx, off, grad, alpha=-0.1, dst=O.bf16_bits_to_f32(bits).copy()))
    got = coracle.bwd_bf16(bits.copy(), idx, off, grad, alpha=-0.1)
    assert np.array_equal(got, expect)


def test_error_behaviour(coracle):
    W = np.zeros((4, 8), dtype=np.float32)
    with pytest.raises(IndexError):
        coracle.fwd(W, np.array([0, 4]), np.array([0]))
    with pytest.raises(IndexError):
        coracle.fwd(W, np.array([-1]), np.array([0]))
    with pytest.raises(ValueError):
        coracle.fwd(W, np.array([0, 1, 2]), np.array([2, 1]))
    with pytest.raises(IndexError):
        O.embbag_fwd_np(W, np.array([9]), np.array([0]))


def test_oracle_rowwise_adagrad_weight_decay_modes(coracle):
    """the oracle's weight-decay rules (fbgemm rowwise_adagrad as published; parity unpinned) against an fp64 form"""
    rng = np.random.default_rng(4)
    R, D, B, L, lr, eps, wd = 50, 16, 12, 4, 0.1, 1e-6, 0.05
    idx = rng.integers(0, R, B * L).astype(np.int64)
    off = np.arange(B, dtype=np.int64) * L
    g = rng.standard_normal((B, D)).astype(np.float32)
    for mode in (0, 1, 2):
        W = rng.standard_normal((R, D)).astype(np.float32)
        mom = rng.uniform(0, 1, R).astype(np.float32)
        W0, m0 = W.astype(np.float64), mom.astype(np.float64)
        coracle.bwd_rowwise_adagrad(W, mom, idx, off, g, None, lr=lr, eps=eps, weight_decay=wd, weight_decay_mode=mode)
        G = np.zeros((R, D))
        np.add.at(G, idx, g.astype(np.float64)[np.repeat(np.arange(B), L)])
        touched = np.bincount(idx, minlength=R) > 0
        gx = G + wd * W0 if mode == 1 else G
        m64 = m0 + (gx ** 2).mean(1)
        mult = lr / (np.sqrt(m64) + eps)
        corr = np.ones(R) - (mult * wd if mode == 1 else lr * wd if mode == 2 else 0.0)
        W64 = corr[:, None] * W0 - mult[:, None] * G
        assert np.allclose(W[touched], W64[touched], rtol=1e-5, atol=1e-6) and np.allclose(mom[touched], m64[touched], rtol=1e-6)
        assert np.array_equal(W[~touched], W0[~touched].astype(np.float32)) and np.array_equal(mom[~touched], m0[~touched].astype(np.float32))


def _torch_adagrad_steps(w0, grads, lr, eps):
    """torch.optim.Adagrad (a real third-party implementation) on a [R, 1] parameter: per row, state += g^2,
    w -= lr * g / (sqrt(state) + eps) -- what row-wise Adagrad reduces to when every column of a row carries the same
    gradient (the row mean of G^2 is then g^2)"""
    import torch

    p = torch.nn.Parameter(torch.from_numpy(w0.astype(np.float32)).reshape(-1, 1).clone())
    opt = torch.optim.Adagrad([p], lr=lr, eps=eps, initial_accumulator_value=0.0, lr_decay=0.0, weight_decay=0.0)
    for g in grads:
        p.grad = torch.from_numpy(g.astype(np.float32)).reshape(-1, 1)
        opt.step()
    return p.detach().numpy().reshape(-1), opt.state[p]["sum"].numpy().reshape(-1)


def test_oracle_rowwise_adagrad_pinned_to_torch_adagrad_where_rowwise_is_elementwise(coracle):
    """A PARTIAL pin of the f2 oracle to a real implementation: fbgemm is absent, but with all columns of a row equal
    (table and gradient) exact row-wise Adagrad IS torch.optim.Adagrad per row -- same state, same step.  Three steps, rows
    hit 0 .. 5 times per step (the summed gradient is what the optimizer sees), unhit rows untouched.  This pins where the
    square root, eps, the learning rate's sign and the accumulation sit; the row MEAN over unequal columns and the weight
    decay modes stay checked against fp64 forms only (parity unpinned for those, as the oracle header says)."""
    rng = np.random.default_rng(11)
    R, D, B, L, lr, eps = 40, 8, 16, 3, 0.07, 1e-5
    w_col = rng.standard_normal(R).astype(np.float32)
    W = np.repeat(w_col[:, None], D, axis=1).copy()
    mom = np.zeros(R, np.float32)
    off = np.arange(B, dtype=np.int64) * L
    per_step = []
    for step in range(3):
        idx = rng.integers(0, R - 5, B * L).astype(np.int64)          # the last 5 rows are never hit
        g_bag = (rng.integers(-8, 9, B) / 4.0).astype(np.float32)     # dyadic: row sums are exact in fp32, any order
        g = np.repeat(g_bag[:, None], D, axis=1).copy()
        coracle.bwd_rowwise_adagrad(W, mom, idx, off, g, None, lr=lr, eps=eps)
        G = np.zeros(R, np.float32)
        np.add.at(G, idx, g_bag[np.repeat(np.arange(B), L)])
        per_step.append(G)
    w_t, s_t = _torch_adagrad_steps(w_col, per_step, lr, eps)
    assert np.allclose(mom, s_t, rtol=1e-6, atol=0) and np.allclose(W, w_t[:, None], rtol=2e-6, atol=1e-7)
    assert np.array_equal(W[-5:], np.repeat(w_col[-5:, None], D, axis=1)) and not mom[-5:].any()
    assert all(np.array_equal(W[:, 0], W[:, d]) for d in range(1, D))


def test_oracle_rowwise_adagrad_pinned_to_fbgemm_fixture(coracle, golden_dir):
    """fbgemm_gpu's OWN EXACT_ROWWISE_ADAGRAD outputs (tests/golden/gen_adagrad_fbgemm.py writes the fixture wherever
    fbgemm_gpu is importable -- it is not in the build image, so this test normally skips and the oracle's header says
    PARITY UNPINNED): two steps, weight decay none / L2 / decoupled, duplicates inside and across bags."""
    import os

    path = os.path.join(golden_dir, "adagrad_fbgemm.npz")
    if not os.path.exists(path):
        pytest.skip("no fbgemm_gpu fixture: fbgemm_gpu was not importable where the goldens were generated (parity unpinned)")
    z = np.load(path)
    for tag, mode in (("none", 0), ("l2", 1), ("decouple", 2)):
        rows = [int(r) for r in z[f"{tag}.rows"]]
        D, B, L, lr, eps, wd = z[f"{tag}.hp"]
        D, B, L = int(D), int(B), int(L)
        idx, off, grads = z[f"{tag}.idx"], z[f"{tag}.off"], z[f"{tag}.grads"]
        for t, r in enumerate(rows):
            W, mom = z[f"{tag}.W0.{t}"].copy(), np.zeros(r, np.float32)
            s, e = off[t * B], off[(t + 1) * B]
            for g in grads:
                coracle.bwd_rowwise_adagrad(W, mom, idx[s:e], off[t * B:(t + 1) * B] - s, np.ascontiguousarray(g[:, t * D:(t + 1) * D]),
                                            None, lr=float(lr), eps=float(eps), weight_decay=float(wd), weight_decay_mode=mode)
            assert np.allclose(W, z[f"{tag}.W.{t}"], rtol=2e-5, atol=1e-6), (tag, t)
            assert np.allclose(mom, z[f"{tag}.mom.{t}"], rtol=2e-5, atol=1e-7), (tag, t)


def test_c_oracle_against_live_torch_on_random_requests(coracle):
    """Beside the committed goldens: 40 random requests (ragged bags incl. empty first / middle / last ones, repeated indices,
    per-sample weights, int32 and int64 indices, D from 4 to 160) through torch's CPU EmbeddingBag(sum) -- the engine the
    reference calls -- live: forward bit for bit, dense gradient (autograd of the same op, ``sparse=False``) within 1e-5 of the
    summed magnitudes (it is exact except for the order of additions into rows looked up many times)"""
    import torch

    rng = np.random.default_rng(20260928)
    for case in range(40):
        rows, D, B = int(rng.integers(1, 400)), int(rng.choice([4, 8, 32, 56, 128, 160])), int(rng.integers(1, 40))
        lens = rng.integers(0, 9, size=B)
        if case % 4 == 0:
            lens[0] = 0
        if case % 5 == 0:
            lens[-1] = 0
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        n = int(lens.sum())
        idx = rng.integers(0, rows, size=n).astype(np.int64 if case % 2 else np.int32)
        psw = rng.standard_normal(n).astype(np.float32) if case % 3 == 0 else None
        W = rng.standard_normal((rows, D)).astype(np.float32)
        grad = rng.standard_normal((B, D)).astype(np.float32)
        Wt = torch.tensor(W, requires_grad=True)
        out_t = torch.nn.functional.embedding_bag(torch.from_numpy(idx), Wt, torch.from_numpy(off).to(torch.from_numpy(idx).dtype),
                                                  mode="sum", per_sample_weights=None if psw is None else torch.from_numpy(psw))
        out = coracle.fwd(W, idx, off, psw)
        assert np.array_equal(out, out_t.detach().numpy()), case
        out_t.backward(torch.from_numpy(grad))
        dW = coracle.bwd_f32(np.zeros_like(W), idx, off, grad, psw)
        mag = np.zeros(W.shape, dtype=np.float64)
        start, end = O.bag_bounds(off, B, n)
        for b in range(B):
            for j in range(start[b], end[b]):
                mag[idx[j]] += np.abs(grad[b].astype(np.float64)) * (1.0 if psw is None else abs(float(psw[j])))
        assert (np.abs(dW.astype(np.float64) - Wt.grad.numpy().astype(np.float64)) <= 1e-5 * mag + 1e-30).all(), case


# ----------------------------------------------------------------------------- the 16-bit update routines
def _same_f16(x32, coracle):
    import torch

    got = coracle.f32_to_f16_bits(x32)
    exp = torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(np.asarray(x32, dtype=np.float32))
    assert np.array_equal(got[~nan], exp[~nan])
    assert np.isnan(got[nan].view(np.float16)).all() and np.isnan(exp[nan].view(np.float16)).all()
    assert np.array_equal(got[nan] & 0x8000, exp[nan] & 0x8000)            # a NaN keeps its sign


def test_f32_to_f16_software_rounding_equals_torch(coracle):
    """round-to-nearest-even fp32 -> fp16 of the oracle against torch's conversion, bit for bit: every fp16 value widened
    (exact), every midpoint between two neighbouring fp16 values (ties) and both fp32 neighbours of every midpoint, +-0, values
    below 2^-25, above 65504, Inf, NaN"""
    allbits = np.arange(1 << 16, dtype=np.uint16)
    wide = O.f16_bits_to_f32(allbits)
    _same_f16(wide, coracle)
    fin = np.isfinite(wide)
    assert np.array_equal(coracle.f32_to_f16_bits(wide[fin]), allbits[fin])          # widening then rounding is the identity
    # midpoints: consecutive positive finite patterns are neighbours (subnormals included); the midpoint of two fp16 values has at
    # most 12 significant bits, exact in fp32.  The midpoint above 65504 (65520) rounds to infinity.
    pos = O.f16_bits_to_f32(np.arange(0, 0x7c00, dtype=np.uint16)).astype(np.float64)
    mid = np.concatenate([(pos[:-1] + pos[1:]) / 2, [65520.0]])
    mid32 = mid.astype(np.float32)
    assert np.array_equal(mid32.astype(np.float64), mid)
    for sign in (1.0, -1.0):
        m = (sign * mid32).astype(np.float32)
        _same_f16(m, coracle)
        _same_f16(np.nextafter(m, np.float32(np.inf)), coracle)
        _same_f16(np.nextafter(m, np.float32(-np.inf)), coracle)
    tiny = np.float32(2.0 ** -25)
    edge = np.array([0.0, -0.0, tiny, -tiny, np.nextafter(tiny, np.float32(0)), np.nextafter(tiny, np.float32(1)), 1e-9, -1e-9, 1e-30,
                     1e-40, -1e-45, 65504.0, 65519.996, 65520.0, 65536.0, 1e6, -1e6, 3e38, np.inf, -np.inf, np.nan, -np.nan],
                    dtype=np.float32)
    _same_f16(edge, coracle)
    nans = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0x7f802000], dtype=np.uint32).view(np.float32)
    _same_f16(nans, coracle)
    rng = np.random.default_rng(0)
    _same_f16(rng.integers(0, 1 << 32, 2_000_000, dtype=np.uint64).astype(np.uint32).view(np.float32), coracle)


def test_f16_backward_rounds_once(coracle):
    """bwd_f16 accumulates a row's whole update in fp32 on the widened value and rounds once: the case is built so that rounding
    after every add gives other bits"""
    import torch

    rng = np.random.default_rng(3)
    W = rng.standard_normal((50, 16)).astype(np.float32)
    f16 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.float16)          # noqa: E731
    bits = f16(W).view(torch.int16).numpy().view(np.uint16)
    idx = rng.integers(0, 50, 60)
    off = np.arange(6) * 10
    grad = rng.standard_normal((6, 16)).astype(np.float32)
    once = O.embbag_bwd_np(50, idx, off, grad, alpha=-0.1, dst=O.f16_bits_to_f32(bits).copy())
    expect = f16(once).view(torch.int16).numpy().view(np.uint16)
    got = coracle.bwd_f16(bits.copy(), idx, off, grad, alpha=-0.1)
    assert np.array_equal(got, expect)
    each = O.f16_bits_to_f32(bits).copy()
    for b in range(6):
        for j in range(off[b], off[b] + 10):
            each[idx[j]] = f16(each[idx[j]] + (np.float32(-0.1) * grad[b]).astype(np.float32)).float().numpy()
    assert not np.array_equal(f16(each).view(torch.int16).numpy().view(np.uint16), expect)


@pytest.mark.parametrize("code", [O.BF16, O.F16])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_oracle_rowwise_adagrad_16bit_tables(coracle, code, mode):
    """the 16-bit Adagrad routine against an fp64 numpy evaluation of the same formulas followed by torch's own conversion, under
    the interval rule the GPU kernels are held to (tests/lowp_rules.py): duplicates, per-sample weights of both signs, two steps;
    W_pre is the fp32 routine's own result on the widened table, the stored bits its single rounding"""
    import torch

    from tests import lowp_rules as R

    tdt = torch.bfloat16 if code == O.BF16 else torch.float16
    widen = O.bf16_bits_to_f32 if code == O.BF16 else O.f16_bits_to_f32
    to_bits = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(tdt).view(torch.int16).numpy().view(np.uint16)   # noqa: E731
    rng = np.random.default_rng(40 + mode)
    Rr, D, B, L, lr, eps, wd = 300, 24, 64, 12, 0.05, 1e-6, 0.02
    bits = to_bits(rng.standard_normal((Rr, D)))
    mom = np.zeros(Rr, np.float32)
    for step in range(2):
        idx = rng.integers(0, Rr // 2, B * L).astype(np.int64)            # duplicates; the upper half is never looked up
        off = np.arange(B, dtype=np.int64) * L
        g = rng.standard_normal((B, D)).astype(np.float32)
        psw = rng.standard_normal(B * L).astype(np.float32)
        old_bits, m0 = bits.copy(), mom.copy()
        w_old = widen(old_bits)
        f32_W, f32_m = w_old.copy(), m0.copy()
        coracle.bwd_rowwise_adagrad(f32_W, f32_m, idx, off, g, psw, lr=lr, eps=eps, weight_decay=wd, weight_decay_mode=mode)
        _, _, w_pre = coracle.bwd_rowwise_adagrad(bits, mom, idx, off, g, psw, lr=lr, eps=eps, weight_decay=wd,
                                                  weight_decay_mode=mode, dtype=code)
        touched = np.bincount(idx, minlength=Rr) > 0
        assert touched[:Rr // 2].sum() > 100 and not touched[Rr // 2:].any()
        assert np.array_equal(w_pre[touched], f32_W[touched]) and np.array_equal(mom, f32_m)      # one arithmetic
        assert np.array_equal(bits[touched], to_bits(w_pre[touched]))                             # rounded once, to nearest even
        assert np.array_equal(bits[~touched], old_bits[~touched]) and np.array_equal(mom[~touched], m0[~touched])
        W64, m64, _, _ = R.adagrad_fp64(w_old, m0, idx, off, g, psw, lr, eps, wd, mode)
        ref = widen(to_bits(W64.astype(np.float32)))              # (fp64 -> fp32 -> 16 bit; the interval rule absorbs the double rounding)
        ratio = R.nearest_ratio(widen(bits)[touched], W64[touched], code, R.tol_b(W64[touched]))
        assert ratio.max() <= 1.0, ratio.max()
        assert (np.abs(widen(bits)[touched] - ref[touched]) <= O.ulp16(W64[touched], code)).all()
        assert np.allclose(mom[touched], m64[touched], rtol=2e-5, atol=1e-12)


def test_ulp16_and_neighbours():
    for code, tdt_bits in ((O.BF16, O.bf16_bits_to_f32), (O.F16, O.f16_bits_to_f32)):
        top = 0x7f80 if code == O.BF16 else 0x7c00
        vals = tdt_bits(np.arange(0, top, dtype=np.uint16)).astype(np.float64)
        gaps = np.diff(vals)
        assert np.array_equal(O.ulp16(vals[:-1], code), gaps)                       # the spacing above every grid value
        mid = (vals[:-1] + vals[1:]) / 2
        assert np.array_equal(O.down16(mid, code), vals[:-1]) and np.array_equal(O.up16(mid, code), vals[1:])
        assert np.array_equal(O.down16(vals, code), vals) and np.array_equal(O.up16(-vals, code), -vals)
