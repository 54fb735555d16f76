"""The arithmetic rule of ``pm_embbag_psw_grad`` (include/param_amd.h), restated in numpy, and the bar its results are held to.

For lookup j of bag (t, b):  ``out[j] = sum_c grad(t, b)[c] * table_t[indices[j], c]``, evaluated as the kernel evaluates it:

* table elements widened to fp32 (exact); every product rounded to fp32 on its own, every add rounded to fp32 on its own (numpy's
  float32 ``*`` and ``+``: no fused multiply-add);
* lane l owns columns ``[l V, (l + 1) V)`` -- V = 4 for fp32 tables, 8 for 16-bit tables -- and adds its V products to +0 in
  ascending column order;
* the lane partials are combined by an xor butterfly with masks 1, 2, 4, ... over the lanes padded with +0 to a power of two.
  A partial is never -0 (it starts at +0), so further +0 lanes change nothing: the value is the same for every group width.

The bar is the standard gamma_D bound of an fp32 dot product of D terms in ANY summation order (Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1: |fl(x.y) - x.y| <= gamma_D sum |x_c y_c|, gamma_D = D u / (1 - D u) <= (D + 1) u for D u << 1, u = 2^-24),
plus D denormal quanta for products that underflow:

    bar_j = (D + 1) * 2^-24 * sum_c |g_c * w_c|   (fp64)   +   D * 2^-149

Derived, not tuned: torch's CPU kernel and the restatement both stay well inside it (tests/test_psw_grad_host.py prints by how much).
"""
import numpy as np

U32 = 2.0 ** -24
DENORM = 2.0 ** -149


def vec_of(dtype_name: str) -> int:
    """columns per lane: one 16-byte row load"""
    return 4 if dtype_name in ("float32", "fp32", "f32") else 8


def to_bf16_values(x: np.ndarray) -> np.ndarray:
    """fp32 values a bf16 table can hold (low 16 bits cleared), as fp32"""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def to_fp16_values(x: np.ndarray) -> np.ndarray:
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def dot_rule(G: np.ndarray, W: np.ndarray, V: int) -> np.ndarray:
    """G, W: fp32 ``[n, D]`` (gradient row and table row of each lookup) -> fp32 ``[n]`` by the rule above"""
    G, W = np.asarray(G, dtype=np.float32), np.asarray(W, dtype=np.float32)
    n, D = G.shape
    assert W.shape == (n, D) and D % V == 0
    with np.errstate(all="ignore"):
        prod = G * W                                             # fp32 products, each rounded once
        lanes = 1
        while lanes * V < D:
            lanes *= 2
        pad = np.zeros((n, lanes * V), dtype=np.float32)         # lanes past D / V hold +0
        pad[:, :D] = prod
        pad = pad.reshape(n, lanes, V)
        part = np.zeros((n, lanes), dtype=np.float32)
        for k in range(V):                                       # ascending column order, from +0
            part = part + pad[:, :, k]
        lane = np.arange(lanes)
        m = 1
        while m < lanes:                                         # xor butterfly, low mask first
            part = part + part[:, lane ^ m]
            m *= 2
    return part[:, 0].astype(np.float32) if n else np.zeros(0, dtype=np.float32)


def dot_fp64_and_bar(G: np.ndarray, W: np.ndarray):
    """exact-enough value (fp64) and bar per lookup"""
    G, W = np.asarray(G, dtype=np.float64), np.asarray(W, dtype=np.float64)
    D = G.shape[1]
    with np.errstate(all="ignore"):
        p = G * W
        return p.sum(axis=1), (D + 1) * U32 * np.abs(p).sum(axis=1) + D * DENORM


def lookups_of_request(off, T: int, B: int, N: int, bag_begin: int = 0, bag_count=None):
    """positions j, tables t and bags b of the lookups inside the bag slice (offsets of T*B or T*B+1 entries; the last bag ends at N)"""
    off = np.asarray(off, dtype=np.int64)[:T * B]
    ends = np.append(off[1:], N)
    bag = np.repeat(np.arange(T * B, dtype=np.int64), ends - off)
    pos = off[0] + np.arange(bag.size, dtype=np.int64)
    t, b = bag // B, bag % B
    hi = B if bag_count is None else bag_begin + bag_count
    keep = (b >= bag_begin) & (b < hi)
    return pos[keep], t[keep], b[keep]


def restate(tables, idx, off, B: int, grads, V: int, bag_begin: int = 0, bag_count=None):
    """tables: list of fp32-valued ``[rows_t, D_t]`` arrays; grads: list of fp32 ``[B, D_t]`` (table t's gradient rows).
    -> (out fp32 [N] by the rule, zero where not written; written mask [N]; fp64 value [N]; bar [N])"""
    idx = np.asarray(idx, dtype=np.int64)
    N, T = idx.size, len(tables)
    out, exact, bar = np.zeros(N, dtype=np.float32), np.zeros(N), np.zeros(N)
    written = np.zeros(N, dtype=bool)
    pos, t_of, b_of = lookups_of_request(off, T, B, N, bag_begin, bag_count)
    for t in range(T):
        sel = t_of == t
        if not sel.any():
            continue
        j = pos[sel]
        G = np.asarray(grads[t], dtype=np.float32)[b_of[sel]]
        W = np.asarray(tables[t], dtype=np.float32)[idx[j]]
        out[j] = dot_rule(G, W, V)
        exact[j], bar[j] = dot_fp64_and_bar(G, W)
        written[j] = True
    return out, written, exact, bar


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """bit for bit, except that NaN positions must coincide instead of NaN bits"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def within_bar(x: np.ndarray, exact: np.ndarray, bar: np.ndarray) -> bool:
    """every finite entry within its bar of the fp64 value (entries whose fp64 value is not finite are the special-value tests')"""
    fin = np.isfinite(exact) & np.isfinite(bar)
    return bool((np.abs(np.asarray(x, dtype=np.float64)[fin] - exact[fin]) <= bar[fin]).all())
