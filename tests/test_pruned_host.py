"""PRUNED TABLES on the CPU: tests/pruned_rules.py (delete the pruned lookups, remap the rest, then tests/qmixed_rules.py) against torch's
CPU operators called with ``pruned_weights=True`` -- live, and through the committed fixture tests/golden/pruned_cases.npz
(tests/pruned_cases.py writes it); what the constructors accept and refuse about ``index_remapping``; the ``state_dict`` keys;
``from_float(keep=)``; the no-CPU-fallback errors; every host-side refusal of the two C calls; and the compiled kernels' metadata."""
import ctypes
import os

import numpy as np
import pytest
import torch

from param_amd import _lib
from tests import pruned_cases as PC
from tests import pruned_rules as P
from tests import qmixed_rules as M
from tests import qrows_cases as C
from tests import qrows_rules as R
from tests.test_isa_properties import _kernel_resources, bundles  # noqa: F401
from tests.test_qmixed_host import _request

HERE = os.path.dirname(os.path.abspath(__file__))
NP_IT = {"i32": np.int32, "i64": np.int64}


# ---- the rule against torch ------------------------------------------------------------------------------------------------------------

def test_the_request_prunes_what_it_says():
    idx, off, psw = PC.request()
    rm, lens = PC.remap(), np.array(PC.LENS)
    pruned = rm[idx] < 0
    ends = np.concatenate([off[1:], [idx.size]])
    per_bag = [pruned[a:b] for a, b in zip(off, ends)]
    assert rm.shape == (C.ROWS,) and rm.dtype == np.int32 and (np.sort(rm[rm >= 0]) == np.arange((rm >= 0).sum())).all()
    assert 0.3 <= (rm < 0).mean() <= 0.7 and 0.3 <= pruned.mean() <= 0.7
    assert per_bag[PC.ALL_PRUNED].all() and lens[PC.ALL_PRUNED] > 0 and not per_bag[PC.NONE_PRUNED].any() and lens[PC.NONE_PRUNED] > 0
    assert [len(b) for b in per_bag] == list(PC.LENS) and lens[0] == lens[5] == 0
    assert pruned[PC.INF_AT] and np.isinf(psw[PC.INF_AT]) and not per_bag[1].all()      # the +Inf weight sits on a pruned lookup of a live bag


@pytest.mark.parametrize("bits,it,weighted", PC.case_names())
def test_rule_equals_torch_pruned_operators(bits, it, weighted):
    """live and through the fixture; and torch's own un-pruned operator over the compacted request gives the same bits"""
    idx, off, psw = PC.request()
    q, rm, B = PC.physical_table(bits), PC.remap(), len(PC.LENS)
    w = psw if weighted else None
    want = P.forward([q], [PC.DIM], (bits,), [rm], idx.astype(NP_IT[it]), off.astype(NP_IT[it]), B, w)[0]
    live = PC.torch_lookup_pruned(q, bits, rm, idx.astype(NP_IT[it]), off.astype(NP_IT[it]), w)
    assert want.shape == (B, PC.DIM) and R.same_f32(live, want)
    assert R.same_f32(np.load(PC.PATH)[PC.key(bits, it, weighted)], want)
    cidx, coff, cw, kept = P.compact([rm], idx, off, B, w)
    assert kept.sum() == cidx.size < idx.size and coff.shape == off.shape
    assert R.same_f32(C.torch_lookup(q, bits, cidx.astype(NP_IT[it]), coff.astype(NP_IT[it]), cw), want)
    # empty and all-pruned bags: +0.0; the bag whose pruned lookup weighs +Inf stays finite
    for b in (0, 5, PC.ALL_PRUNED):
        assert not want[b].any() and not np.signbit(want[b]).any(), b
    assert np.isfinite(want).all() and want[1].any() and want[PC.NONE_PRUNED].any()
    # a kept row's bytes are the unpruned table's: the physical table is the kept rows of the whole prepack
    assert np.array_equal(C.torch_prepack(C.float_table(PC.DIM), bits)[PC.keep()], q)


@pytest.mark.parametrize("bits", C.BITS)
def test_unpooled_rule_equals_torch_over_bags_of_one(bits):
    idx, off, _ = PC.request()
    q, rm, B = PC.physical_table(bits), PC.remap(), len(PC.LENS)
    want, written = P.gather([q], PC.DIM, (bits,), [rm], idx, off, B)
    live = PC.torch_lookup_pruned(q, bits, rm, idx, np.arange(idx.size, dtype=np.int64))
    assert written.all() and R.same_f32(live, want) and R.same_f32(np.load(PC.PATH)[f"rows_{bits}"], want)
    pruned = rm[idx] < 0
    assert pruned.any() and not want[pruned].any() and not np.signbit(want[pruned]).any() and want[~pruned].any(axis=1).all()
    # a batch slice: pruned positions inside it are written (zeros), positions outside it are not
    _, sl = P.gather([q], PC.DIM, (bits,), [rm], idx, off, B, bag_begin=2, bag_count=2)
    assert sl.sum() == PC.LENS[2] + PC.LENS[3] and sl[off[2]:off[4]].all()
    # an un-pruned table between two pruned ones is the identity
    three = P.forward([q, q, q], [PC.DIM] * 3, (bits,) * 3, [rm, None, rm], np.concatenate([idx, idx % q.shape[0], idx]),
                      np.concatenate([off, off + idx.size, off + 2 * idx.size]), B)
    assert R.same_f32(three[0], three[2]) and R.same_f32(three[1], M.forward([q], [PC.DIM], (bits,), idx % q.shape[0], off, B)[0])


# ---- the modules without a device ------------------------------------------------------------------------------------------------------

def test_constructor_accepts_and_refuses_on_cpu():
    from param_amd import QuantizedBatchedEmbeddingBagMI355 as QB
    from param_amd import QuantizedEmbeddingBagMI355 as QE
    from param_amd import QuantizedEmbeddingMI355 as QS

    r0 = torch.tensor([0, -1, 1, -1, 2, -1, -1], dtype=torch.int32)
    r2 = torch.tensor([-1, 0, -1, 1], dtype=torch.int64)
    m = QB([3, 7, 2], [8, 128, 24], [8, 4, 8], device="cpu", index_remapping=[r0, None, r2])
    assert m.pruned and m.rows == [3, 7, 2] and m.logical_rows == [7, 7, 4] and m.bitwidth is None
    assert [tuple(m.table(t).shape) for t in range(3)] == [(3, 16), (7, 68), (2, 32)]      # the storage is the physical rows
    assert torch.equal(m.index_remapping(0), r0) and m.index_remapping(1) is None and torch.equal(m.index_remapping(2), r2.int())
    assert m.index_remapping(0).dtype == m.index_remapping(2).dtype == torch.int32
    assert m.index_remap.tolist() == r0.tolist() + r2.tolist() and m.index_remap_offsets.tolist() == [0, 7, 7, 11]
    assert m.index_remap.dtype == torch.int32 and m.index_remap_offsets.dtype == torch.int64
    # state_dict: two more buffers of a pruned module, round-tripped; the keys of a module without a pruned table are what they were
    assert list(m.state_dict()) == ["weights", "index_remap", "index_remap_offsets"] and not list(m.parameters())
    for plain in (QB([3, 7, 2], [8, 128, 24], [8, 4, 8], device="cpu"), QB([3, 7, 2], [8, 128, 24], [8, 4, 8], device="cpu", index_remapping=None),
                  QB([3, 7, 2], [8, 128, 24], [8, 4, 8], device="cpu", index_remapping=[None, None, None])):
        assert list(plain.state_dict()) == ["weights"] and not plain.pruned and plain.logical_rows == plain.rows == [3, 7, 2]
        assert all(plain.index_remapping(t) is None for t in range(3)) and not hasattr(plain, "index_remap")
    twin = QB([3, 7, 2], [8, 128, 24], [8, 4, 8], device="cpu", index_remapping=[torch.zeros(7, dtype=torch.int32), None, torch.zeros(4, dtype=torch.int32)])
    m.table(1).fill_(7)
    twin.load_state_dict(m.state_dict())
    assert torch.equal(twin.index_remap, m.index_remap) and torch.equal(twin.weights, m.weights) and torch.equal(twin.index_remapping(2), r2.int())
    # tables of one format: the int stays, the module is pruned all the same
    u = QB([3, 7], [8, 128], 4, device="cpu", index_remapping=[r0, None])
    assert u.bitwidth == 4 and u.bitwidths == [4, 4] and u.pruned
    # a table all of whose rows are pruned has no storage; the slab keeps the bytes the un-pooled lookup reads
    z = QB([0], [8], 8, device="cpu", index_remapping=[torch.full((5,), -1, dtype=torch.int32)])
    assert z.rows == [0] and z.logical_rows == [5] and z.weights.numel() >= 8
    # the single-table modules take one tensor
    e = QE(3, 8, bitwidth=8, device="cpu", index_remapping=r0)
    s = QS(2, 24, bitwidth=4, device="cpu", index_remapping=r2)
    assert e.pruned and e.logical_rows == [7] and e.num_embeddings == 3 and s.pruned and s.logical_rows == [4] and s.num_embeddings == 2
    assert not QE(3, 8, device="cpu").pruned and list(QS(3, 8, device="cpu").state_dict()) == ["weights"]
    # refusals, before anything is allocated (rows that could not be allocated prove it)
    huge, ok = [2**30, 2**30], torch.tensor([0, -1], dtype=torch.int32)
    for remap, text in (([ok], "one entry per table"), ([ok, ok, ok], "one entry per table"), ([], "one entry per table"),
                        ([torch.tensor([0, -2], dtype=torch.int32), None], r"values must lie in \[-1"),
                        ([None, torch.tensor([2**30, 0], dtype=torch.int64)], r"values must lie in \[-1"),
                        ([torch.zeros(0, dtype=torch.int32), None], "at least one"), ([torch.zeros((2, 2), dtype=torch.int32), None], "1-D")):
        with pytest.raises(ValueError, match=text):
            QB(huge, [1024, 1024], [8, 4], device="cpu", index_remapping=remap)
    for remap in (True, False, 3, "remap", ok, [True, None], [ok.bool(), None], [ok.float(), None], [[0, -1], None]):
        with pytest.raises(TypeError, match="index_remapping"):
            QB(huge, [1024, 1024], [8, 4], device="cpu", index_remapping=remap)
    for dims in ([4, 128], [128, 12], [20, 20]):                    # (8-bit dims that are multiples of 4: fine without a remap)
        with pytest.raises(ValueError, match="multiple of 8"):
            QB(huge, dims, 8, device="cpu", index_remapping=[ok, None])
    assert not QB([5, 5], [4, 20], 8, device="cpu").pruned
    with pytest.raises(ValueError, match=r"values must lie in \[-1, rows\[0\]\) = \[-1, 3\)"):
        QE(3, 8, device="cpu", index_remapping=torch.tensor([0, 3], dtype=torch.int32))
    with pytest.raises(TypeError, match="index_remapping"):
        QS(3, 8, device="cpu", index_remapping=True)


def test_no_cpu_fallback_of_a_pruned_module():
    from param_amd import QuantizedBatchedEmbeddingBagMI355 as QB
    from param_amd import QuantizedEmbeddingBagMI355 as QE
    from param_amd import QuantizedEmbeddingMI355 as QS

    r = torch.tensor([0, -1, 1, -1], dtype=torch.int32)
    m = QB([2, 2], [24, 24], [4, 8], device="cpu", layout="tbd", index_remapping=[r, None])
    idx, off = torch.zeros(4, dtype=torch.int64), torch.zeros(5, dtype=torch.int64)
    for call in (m.lookup, m.plan, m.lookup_sequence, m.sequence_plan, m.forward):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(idx, off, batch=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.sanitize_(idx, off, batch=2)
    with pytest.raises(TypeError, match="int64 or both int32"):
        m.lookup(idx.float(), off)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        QE(2, 8, device="cpu", index_remapping=r)(idx, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        QS(2, 8, device="cpu", index_remapping=r)(idx.view(2, 2))


def test_from_float_keep_builds_the_remap(monkeypatch):
    from param_amd import QuantizedBatchedEmbeddingBagMI355 as QB
    from param_amd import QuantizedEmbeddingBagMI355 as QE
    from param_amd import QuantizedEmbeddingMI355 as QS
    from param_amd.quantized_bag import _keep_remap

    k0 = torch.tensor([True, False, False, True, True, False])
    assert _keep_remap(k0, 6, 0).tolist() == [0, -1, -1, 1, 2, -1] and _keep_remap(k0, 6, 0).dtype == torch.int32
    assert np.array_equal(_keep_remap(torch.from_numpy(PC.keep()), C.ROWS, 0).numpy(), PC.remap())
    xs = [torch.arange(6 * 8, dtype=torch.float32).view(6, 8), torch.ones(5, 128), torch.arange(4 * 8, dtype=torch.float32).view(4, 8)]
    k2 = torch.tensor([False, False, False, False])
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # accepted; the quantising kernel then needs a device
        QB.from_float(xs, bitwidth=[8, 4, 8], keep=[k0, None, k2], device="cpu")
    got = []
    monkeypatch.setattr(QB, "quantize_from_", lambda self, t, x: got.append((t, x.clone())))      # (the kernel's part: tests/test_gpu_pruned.py)
    m = QB.from_float(xs, bitwidth=[8, 4, 8], keep=[k0, None, k2], device="cpu")
    assert m.pruned and m.rows == [3, 5, 0] and m.logical_rows == [6, 5, 4]
    assert m.index_remapping(0).tolist() == [0, -1, -1, 1, 2, -1] and m.index_remapping(1) is None and m.index_remapping(2).tolist() == [-1] * 4
    assert [t for t, _ in got] == [0, 1, 2] and torch.equal(got[0][1], xs[0][[0, 3, 4]]) and torch.equal(got[1][1], xs[1]) and got[2][1].shape == (0, 8)
    plain = QB.from_float(xs, bitwidth=[8, 4, 8], device="cpu")
    assert not plain.pruned and plain.rows == [6, 5, 4] and not QB.from_float(xs, bitwidth=8, keep=[None] * 3, device="cpu").pruned
    for keep, text in (([k0, None], "one None or bool mask per table"), (k0, "one None or bool mask per table"), ([k0[:5], None, None], r"keep\[0\]"),
                       ([k0.int(), None, None], r"keep\[0\]"), ([None, None, [False] * 4], r"keep\[2\]")):
        with pytest.raises(ValueError, match=text):
            QB.from_float(xs, bitwidth=8, keep=keep, device="cpu")
    with pytest.raises(ValueError, match="multiple of 8"):
        QB.from_float([torch.zeros(6, 12)], bitwidth=8, keep=[k0], device="cpu")
    # the single-table modules: one mask
    bag = torch.nn.EmbeddingBag(6, 8, mode="sum")
    e = QE.from_float(bag, bitwidth=4, keep=k0, device="cpu")
    assert e.pruned and e.num_embeddings == 3 and e.logical_rows == [6] and e.index_remapping(0).tolist() == [0, -1, -1, 1, 2, -1]
    assert torch.equal(got[-1][1], bag.weight.detach()[[0, 3, 4]])
    s = QS.from_float(torch.nn.Embedding(6, 8), keep=k0, device="cpu")
    assert s.pruned and s.num_embeddings == 3 and s.index_remapping(0).tolist() == [0, -1, -1, 1, 2, -1]
    assert not QS.from_float(torch.nn.Embedding(6, 8), device="cpu").pruned


# ---- the C calls without a device ------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_exported_and_bound():
    names = ("pm_embbag_fwd_qrows_pruned", "pm_embedding_gather_qrows_pruned")
    header = open(os.path.join(os.path.dirname(HERE), "include", "param_amd.h")).read()
    L, A = _lib.load(), _lib.load_alternates()
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name) and hasattr(A, name) and f"int {name}(" in header, name
    assert "PRUNED TABLES" in header and L.pm_abi_version() == 8 and ctypes.sizeof(_lib.pm_embbag_batch) == 144
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert L.pm_embbag_fwd_qrows_pruned.argtypes[1:] == [vp, vp, vp, i32, vp, vp]
    assert L.pm_embedding_gather_qrows_pruned.argtypes[1:] == [vp, vp, vp, i32, vp, i64, vp]


def test_argument_validation_without_gpu():
    """every refusal is made on the host, before any HIP call (the dummy pointers are never dereferenced)"""
    L = _lib.load()
    INVALID, UNSUPPORTED, OK, F32 = _lib.PM_ERR_INVALID, _lib.PM_ERR_UNSUPPORTED, _lib.PM_OK, _lib.PM_F32
    ref = lambda op: None if op is None else ctypes.byref(op)      # noqa: E731

    def fwd(op, odt=F32, out=64, bits=64, remap=64, roff=64, **_):
        return L.pm_embbag_fwd_qrows_pruned(ref(op), bits, remap, roff, odt, out, None)

    def gather(op, odt=F32, out=64, bits=64, remap=64, roff=64, stride=None):
        stride = (op.max_dim if op is not None else 8) if stride is None else stride
        return L.pm_embedding_gather_qrows_pruned(ref(op), bits, remap, roff, odt, out, stride, None)

    err = L.pm_last_error
    for call in (fwd, gather):
        # everything the per-table-format calls refuse, in their words
        assert call(None) == INVALID and b"op is NULL" in err()
        for field, val, text in (("num_tables", 0, b"num_tables"), ("index_dtype", 3, b"index_dtype"), ("bag_count", 5, b"bag_begin/bag_count"),
                                 ("offsets", None, b"offsets"), ("indices", None, b"indices"), ("tables", None, b"tables"),
                                 ("fixed_pooling", 5, b"fixed_pooling")):
            op = _request()
            setattr(op, field, val)
            assert call(op) == INVALID and text in err(), field
        op = _request()
        op.out_stride = 18
        assert call(op) == UNSUPPORTED and b"out_stride" in err()
        for d in (4, 12, 20, 6, 1020):
            assert call(_request(max_dim=d)) == UNSUPPORTED and b"multiple of 8" in err(), d
        for d in (4, 12, 20):
            assert call(_request(max_dim=128, min_dim=d)) == UNSUPPORTED and b"multiple of 8" in err(), d
        assert call(_request(max_dim=4104)) == UNSUPPORTED and b"at most 4096" in err()
        for field, val in (("table_group", 2), ("grad_block_shift", 1)):
            op = _request()
            setattr(op, field, val)
            assert call(op) == UNSUPPORTED and b"blocked layouts" in err(), field
        assert call(_request(), bits=None) == INVALID and b"table_bits is NULL" in err()
        for odt in (-1, 3, _lib.PM_I32, _lib.PM_I64):
            assert call(_request(), odt=odt) == INVALID and b"out_dtype" in err()
        # the call's own: both remap arrays are required, also by a request with nothing to do
        assert call(_request(), roff=None) == INVALID and b"remap_offsets is NULL" in err()
        assert call(_request(), remap=None) == INVALID and b"remap is NULL" in err()
        assert call(_request(), remap=None, roff=None) == INVALID and b"remap_offsets is NULL" in err()
        empty = _request()
        empty.bag_count = 0
        assert call(empty, roff=None, out=None) == INVALID and call(empty, remap=None, out=None) == INVALID
        # `out`
        assert call(_request(), out=None) == INVALID and b"out is NULL" in err()
        assert call(_request(), out=72) == INVALID and b"16-byte aligned" in err()
        assert call(_request(), odt=_lib.PM_BF16, out=68) == INVALID and b"8-byte aligned" in err()
        assert call(_request(), odt=_lib.PM_F16, out=68) == INVALID and b"8-byte aligned" in err()
        # nothing to do: PM_OK without a launch, whatever `out` is
        assert call(empty, out=None) == OK and call(empty, odt=_lib.PM_F16, out=None) == OK and call(_request(B=0, N=0), out=None) == OK
    assert gather(_request(weighted=True)) == UNSUPPORTED and b"per_sample_weights must be NULL" in err()
    for stride in (4, 7, 10, -8):
        assert gather(_request(), stride=stride) == INVALID and b"out_row_stride" in err(), stride
    none = _request(N=0)
    none.indices = None
    assert gather(none, out=None) == OK


# ---- the compiled kernels --------------------------------------------------------------------------------------------------------------

def test_no_instance_of_the_new_kernels_uses_scratch(bundles):  # noqa: F811
    """code-object metadata (llvm-readelf --notes; no GPU): the launcher ladders name 4 lane-group widths x weighted or not x 3 output
    types x 2 depths of the pooled kernel and 3 output types x 4 widths x 4 depths of the un-pooled one; none has a private segment;
    the un-pooled kernel's LDS is the per-table-format kernel's four arrays (the remap needs none); two waves per SIMD at least"""
    res = _kernel_resources(bundles)
    pooled = {n: v for n, v in res.items() if "18qpruned_fwd_kernel" in n}
    gather = {n: v for n, v in res.items() if "21qpruned_gather_kernel" in n}
    assert len(pooled) == 4 * 2 * 3 * 2 and len(gather) == 3 * 4 * 4, (len(pooled), len(gather))
    for name, (vgpr, _sgpr, scratch, lds) in pooled.items():
        assert scratch == 0 and lds == 0 and vgpr <= 128, (name, vgpr, scratch, lds)          # (the tile's LDS is dynamic)
    for name, (vgpr, _sgpr, scratch, lds) in gather.items():
        assert scratch == 0 and lds == 256 * 8 + 256 * 4 + 256 * 8 + 256 * 4 and vgpr <= 256, (name, vgpr, scratch, lds)
    # the per-table-format kernels keep their names and counts
    assert len([n for n in res if "17qmixed_fwd_kernel" in n]) == 4 * 2 * 3 * 2 and len([n for n in res if "20qmixed_gather_kernel" in n]) == 3 * 4 * 4
