"""The seeded cases that pin the UN-POOLED rule over row-quantised tables to torch's CPU operators: shared by tests/golden/gen_qgather.py
(writes tests/golden/qgather_cases.npz from the operators), tests/test_qgather_host.py (the numpy rule against the operators, live and
through the fixture) and tests/test_gpu_qgather.py (the fixture through the modules).  Tables: ``qrows_cases.float_table`` prepacked by
torch (37 rows; rows 0 .. 2 constant); one list of 16 lookups with repeats serves every case.  Cases: bits x D."""
import numpy as np

from tests import qrows_cases as C

BITS = C.BITS
DIMS = (8, 24, 128)                # the fixture's widths (both formats take them); the live comparison runs qrows_cases.DIMS
N = 16


def indices():
    """int64 ``[N]``: the constant rows, the special rows of ``float_table``, then seeded rows -- row 3 and row 36 come twice"""
    rng = np.random.default_rng(C.SEED + 1)
    idx = np.concatenate([[0, 1, 2, 3, 4, 5, 36, 3, 36], rng.integers(0, C.ROWS, N - 9)]).astype(np.int64)
    assert idx.size == N
    return idx


def key(bits, dim):
    return f"out_{bits}_{dim}"


def torch_rows(q, bits, idx):
    """fp32 ``[len(idx), D]``: torch's ``quantized::embedding_bag_{byte,4bit}_rowwise_offsets`` over bags of one (``offsets = arange``)"""
    idx = np.asarray(idx)
    return C.torch_lookup(q, bits, idx, np.arange(idx.size, dtype=idx.dtype))


def torch_embedding(x, idx):
    """(fp32 ``[len(idx), D]``, the packed uint8 rows, codes, scale, bias): the forward of a ``torch.ao.nn.quantized.Embedding`` made from
    the fp32 table ``x`` with ``float_qparams_weight_only_qconfig`` (``quantized::embedding_byte``), and its weight as the rule reads it --
    codes from ``int_repr``, scale from ``q_per_channel_scales().float()``, bias ``fl32(-scale * zero_point)``"""
    import torch
    import torch.ao.nn.quantized as nnq
    from torch.ao.quantization import float_qparams_weight_only_qconfig

    emb = torch.nn.Embedding(x.shape[0], x.shape[1])
    emb.weight.data.copy_(torch.from_numpy(x))
    emb.qconfig = float_qparams_weight_only_qconfig
    q = nnq.Embedding.from_float(emb)
    w = q.weight()
    codes = w.int_repr().numpy().astype(np.uint8)
    scale = w.q_per_channel_scales().float().numpy()
    zp = w.q_per_channel_zero_points().float().numpy()
    bias = (-scale * zp).astype(np.float32)
    packed = np.concatenate([codes, np.stack([scale, bias], axis=1).astype(np.float32).view(np.uint8).reshape(-1, 8)], axis=1)
    return q(torch.from_numpy(np.asarray(idx))).numpy(), packed


# ---- requests whose plan tests/qgather_plan_host.json pins (tests/test_qgather_host.py; ``pm_embedding_gather_qrows_plan`` needs no device)
# name: (bits, T, N, max_dim, pm_set_tuning's unroll, xcd_affine)
PLAN_REQUESTS = {
    "bench_8bit_d128": (8, 16, 16 * 8192 * 20, 128, 0, -1),
    "bench_4bit_d128": (4, 16, 16 * 8192 * 20, 128, 0, -1),
    "d4_8bit_one_table": (8, 1, 1000, 4, 0, -1),
    "d8_4bit_one_table": (4, 1, 1000, 8, 0, -1),
    "d8_8bit": (8, 16, 4097, 8, 0, -1),
    "d1024_8bit": (8, 1, 777, 1024, 0, -1),
    "d1024_4bit": (4, 16, 777, 1024, 0, -1),
    "d4096_8bit": (8, 1, 300, 4096, 0, -1),
    "d4096_4bit": (4, 1, 300, 4096, 0, -1),
    "t300_8bit_borders_in_global_memory": (8, 300, 5000, 128, 0, -1),
    "t300_4bit_borders_in_global_memory": (4, 300, 5000, 128, 0, -1),
    "t255_borders_in_lds": (8, 255, 5000, 128, 0, -1),
    "xcd_affine_off": (8, 16, 100000, 128, 0, 0),
    "one_position": (4, 16, 1, 128, 0, -1),
    "unroll_1": (8, 16, 100000, 128, 1, -1),
    "unroll_2": (4, 16, 100000, 128, 2, -1),
    "unroll_3": (8, 16, 100000, 128, 3, -1),
    "unroll_4": (4, 16, 100000, 128, 4, -1),
    "unroll_6": (8, 16, 100000, 128, 6, -1),
    "unroll_8": (4, 16, 100000, 128, 8, -1),
}
