"""MXFP4 tables without a device: what the five C calls and the module's constructor refuse, that empty requests are PM_OK, and the plan
values at D = 128 and D = 2048 (include/param_amd.h, "MXFP4 TABLES")."""
import ctypes

import pytest

from param_amd import _lib

OK, INVALID, UNSUPPORTED = _lib.PM_OK, _lib.PM_ERR_INVALID, _lib.PM_ERR_UNSUPPORTED
F32, BF16 = _lib.PM_F32, _lib.PM_BF16


def _request(T=2, B=4, N=24, max_dim=32, min_dim=0, weighted=False, wd=_lib.PM_MX4, **fields):
    op = _lib.pm_embbag_batch()
    op.num_tables, op.weight_dtype, op.index_dtype, op.max_dim, op.min_dim = T, wd, _lib.PM_I64, max_dim, min_dim
    op.batch, op.num_indices, op.bag_begin, op.bag_count = B, N, 0, B
    op.tables = op.rows = op.dims = op.out_offsets = op.indices = op.offsets = 64      # non-null dummies, never dereferenced on the host
    op.out_stride = max_dim * T
    op.per_sample_weights = 64 if weighted else None
    for k, v in fields.items():
        setattr(op, k, v)
    return op


# (request fields, call arguments, return code, a word of pm_last_error); "both": the pooled and the un-pooled call refuse it alike
REFUSALS = (
    ("both", dict(wd=_lib.PM_F8E4M3), {}, INVALID, "PM_MX4"),
    ("both", dict(max_dim=48), {}, UNSUPPORTED, "multiple of 32"),
    ("both", dict(max_dim=64, min_dim=16), {}, UNSUPPORTED, "multiple of 32"),
    ("both", dict(max_dim=2080), {}, UNSUPPORTED, "at most 2048"),
    ("both", dict(table_group=2), {}, UNSUPPORTED, "blocked"),
    ("both", dict(grad_block_shift=1, batch=4), {}, UNSUPPORTED, "blocked"),
    ("both", {}, dict(odt=_lib.PM_F8E4M3), INVALID, "out_dtype"),
    ("pooled", {}, dict(mean=2), INVALID, "mean"),
    ("pooled", dict(weighted=True), dict(mean=1), UNSUPPORTED, "weight"),
    ("gather", dict(weighted=True), {}, UNSUPPORTED, "unweighted"),
    ("gather", {}, dict(stride=16), INVALID, "out_row_stride"),
    ("both", {}, dict(out=None), INVALID, "NULL"),
    ("both", {}, dict(out=72), INVALID, "aligned"),
    ("both", {}, dict(out=68, odt=BF16), INVALID, "aligned"),
)


@pytest.mark.parametrize("who, fields, args, rc, word", REFUSALS)
def test_lookups_refuse_on_the_host(who, fields, args, rc, word):
    L = _lib.load()
    op = _request(**fields)
    odt, out = args.get("odt", F32), args.get("out", 64)
    calls = {"pooled": lambda: L.pm_embbag_fwd_mx4(ctypes.byref(op), args.get("mean", 0), odt, out, None),
             "gather": lambda: L.pm_embedding_gather_mx4(ctypes.byref(op), odt, out, args.get("stride", op.max_dim), None)}
    for name in (("pooled", "gather") if who == "both" else (who,)):
        assert calls[name]() == rc and word in L.pm_last_error().decode(), (name, L.pm_last_error().decode())
    # the plan queries refuse what is the request's (not the call's out / mean / stride)
    if not args or "odt" in args and "out" not in args:
        assert L.pm_embbag_mx4_plan(ctypes.byref(op), odt, (ctypes.c_int32 * 12)()) == (rc if who != "gather" else OK)
        if "odt" not in args:
            assert L.pm_embedding_gather_mx4_plan(ctypes.byref(op), (ctypes.c_int64 * 8)()) == (rc if who != "pooled" else OK)


def test_null_request_and_every_other_entry_point_refuses_the_dtype():
    L = _lib.load()
    assert L.pm_embbag_fwd_mx4(None, 0, F32, 64, None) == INVALID and L.pm_embedding_gather_mx4(None, F32, 64, 32, None) == INVALID
    assert L.pm_embbag_mx4_plan(ctypes.byref(_request()), F32, None) == INVALID
    op = _request()
    assert L.pm_embbag_fwd(ctypes.byref(op), 64, None) == INVALID
    assert L.pm_embedding_gather(ctypes.byref(op), F32, 64, 32, None) == INVALID
    assert L.pm_embbag_fwd_f8(ctypes.byref(op), None, 0, F32, 64, None) == INVALID


def test_empty_requests_are_ok():
    L = _lib.load()
    empty = _request(bag_count=0)
    assert L.pm_embbag_fwd_mx4(ctypes.byref(empty), 0, F32, None, None) == OK
    assert L.pm_embedding_gather_mx4(ctypes.byref(empty), F32, None, 32, None) == OK
    none = _request(N=0, indices=None)
    assert L.pm_embedding_gather_mx4(ctypes.byref(none), F32, None, 32, None) == OK
    assert L.pm_rows_quantize_mx4(None, F32, 0, 32, 32, None, None) == OK


QUANTISER = (
    (dict(src_dtype=_lib.PM_MX4), INVALID, "src_dtype"), (dict(n_rows=-1), INVALID, "negative"), (dict(dim=48), UNSUPPORTED, "multiple of 32"),
    (dict(dim=0), UNSUPPORTED, "multiple of 32"), (dict(dim=2080, stride=2080), UNSUPPORTED, "at most 2048"), (dict(stride=32), INVALID, "src_row_stride"),
    (dict(stride=66), INVALID, "16-byte"), (dict(src=None), INVALID, "NULL"), (dict(src=72), INVALID, "aligned"), (dict(dst=None), INVALID, "NULL"),
    (dict(dst=68), INVALID, "8-byte"),
)


@pytest.mark.parametrize("args, rc, word", QUANTISER)
def test_quantiser_refuses_on_the_host(args, rc, word):
    L = _lib.load()
    a = dict(src=64, src_dtype=F32, n_rows=3, dim=64, stride=64, dst=64)
    a.update(args)
    assert L.pm_rows_quantize_mx4(a["src"], a["src_dtype"], a["n_rows"], a["dim"], a["stride"], a["dst"], None) == rc
    assert word in L.pm_last_error().decode()


def test_plans_at_128_and_2048():
    try:
        for dim, lanes, gather_lanes, passes in ((128, 8, 32, 1), (2048, 64, 64, 8)):
            op = _request(T=8, B=4096, N=8 * 4096 * 20, max_dim=dim)
            for knob, unroll in ((0, 2), (1, 2), (2, 2), (3, 2), (4, 4), (8, 4)):      # the rounding: below 4 -> 2, from 4 on -> 4; default 2
                _lib.set_tuning(unroll=knob)
                p = _lib.embbag_mx4_plan(op, F32)
                assert p["unroll"] == unroll, (dim, knob, p)
            _lib.set_tuning()
            p, p16 = _lib.embbag_mx4_plan(op, F32), _lib.embbag_mx4_plan(op, BF16)
            # the FP8 kernel's tiling for a lane of 16 columns: 256 / lanes lane groups, tiles of whole lane-group rounds whose rows fit the
            # 16 KiB burst (a 16-bit output fits twice the bags); D = 2048 is two column passes of the 64-lane group
            ng = 256 // lanes
            assert p["bags_per_block"] % ng == 0 and p["bags_per_block"] * dim * 4 <= max(16384, ng * dim * 4)
            assert p16["bags_per_block"] >= p["bags_per_block"] and p["tiles_per_table"] == -(-4096 // p["bags_per_block"])
            assert p["ordered"] == 0 and p["nt_loads"] == 0 and p["flat_bags"] == 0
            assert (dim + lanes * 16 - 1) // (lanes * 16) == (2 if dim == 2048 else 1)
            g = _lib.embedding_gather_mx4_plan(op)
            assert (g["vec"], g["group_lanes"], g["tile"], g["col_passes"], g["unroll"]) == (4, gather_lanes, 256, passes, 8)
            assert g["grid"] == -(-op.num_indices // 256)
            # the pooled lane group is the one the FP8 plan has for the same width
            op8 = _request(T=8, B=4096, N=8 * 4096 * 20, max_dim=dim, wd=_lib.PM_F8E4M3)
            f8 = _lib.embbag_f8_plan(op8, F32)
            assert {k: p[k] for k in p if k != "unroll"} == {k: f8[k] for k in f8 if k != "unroll"}
    finally:
        _lib.set_tuning()


def test_module_constructor_and_row_bytes():
    import param_amd
    from param_amd import mx4_bag

    assert [mx4_bag.row_bytes(d) for d in (32, 64, 96, 128, 160, 2048)] == [24, 40, 56, 72, 88, 1088]
    M = param_amd.MX4BatchedEmbeddingBagMI355
    for kw, word in ((dict(dims=[48]), "multiple of 32"), (dict(dims=[16]), "multiple of 32"), (dict(dims=[2080]), "2048"),
                     (dict(layout="blocked"), "blocked"), (dict(layout="dense"), "layout"), (dict(pooling_mode="max"), "sum or mean"),
                     (dict(rows=[2 ** 31]), "rows <"), (dict(rows=[4, 4], dims=[32, 64], layout="tbd"), "common"), (dict(rows=[]), "at least one")):
        a = dict(rows=[4], dims=[32], device="cpu")
        a.update(kw)
        with pytest.raises(ValueError, match=word):
            M(**a)
