"""The seeded single-table cases that pin the ROW-QUANTISED TABLES rule to torch's CPU operators: shared by
tests/golden/gen_qrows.py (writes tests/golden/qrows_cases.npz from the operators), tests/test_qrows_host.py (the numpy rule against the
operators, live and through the fixture) and tests/test_gpu_qrows.py (the fixture through the module).

One request serves every case: bags of 0, 5, 0, 300, 2, 1, 0 lookups -- empty first, middle and last, one bag of 300 -- into a table of 37
rows, so indices repeat; rows 0 .. 2 of every table are constant (range zero).  Cases: bits x D x index dtype x weighted."""
import numpy as np

BITS = (8, 4)
DIMS = (4, 8, 20, 24, 128)
ROWS = 37
LENS = (0, 5, 0, 300, 2, 1, 0)
SEED = 20261020


def float_table(dim):
    """fp32 ``[ROWS, dim]``, seeded per width"""
    rng = np.random.default_rng(SEED + dim)
    x = (rng.standard_normal((ROWS, dim)) * (rng.random((ROWS, 1)) * 10 + 0.01)).astype(np.float32)
    x[0], x[1], x[2] = 1.5, 0.0, -7.0                                # range zero
    x[3] = np.arange(dim, dtype=np.float32)
    x[4] = (rng.standard_normal(dim) * 1e-6).astype(np.float32)      # an fp16 scale underflows
    x[5] = (rng.standard_normal(dim) * 1e4).astype(np.float32)
    return x


def request():
    """(indices int64 [N], offsets int64 [B], per_sample_weights fp32 [N]); ``include_last_offset=False``"""
    rng = np.random.default_rng(SEED)
    lens = np.array(LENS, dtype=np.int64)
    n = int(lens.sum())
    idx = rng.integers(0, ROWS, n).astype(np.int64)
    idx[:3] = (0, 1, 2)                                              # the constant rows are looked up
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    psw = (rng.standard_normal(n) * 2).astype(np.float32)
    psw[5] = 0.0
    return idx, off, psw


def case_names():
    return [(bits, dim, it, w) for bits in BITS for dim in DIMS for it in ("i32", "i64") for w in (False, True)]


def key(bits, dim, it, weighted):
    return f"out_{bits}_{dim}_{it}_{'w' if weighted else 'u'}"


def special_request():
    """bags over the four rows of ``qrows_rules.special_rows``: each alone, the first two together, an empty bag"""
    return np.array([0, 1, 2, 3, 0, 1], dtype=np.int64), np.array([0, 1, 2, 3, 4, 6], dtype=np.int64)


def torch_prepack(x, bits):
    """uint8 rows of the fp32 array ``x``: torch's ``quantized::embedding_bag_{byte,4bit}_prepack``"""
    import torch

    op = torch.ops.quantized.embedding_bag_byte_prepack if bits == 8 else torch.ops.quantized.embedding_bag_4bit_prepack
    return op(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).numpy()


def torch_lookup(q, bits, indices, offsets, psw=None, include_last_offset=False):
    """fp32 ``[B, D]``: torch's ``quantized::embedding_bag_{byte,4bit}_rowwise_offsets`` on the CPU"""
    import torch

    op = torch.ops.quantized.embedding_bag_byte_rowwise_offsets if bits == 8 else torch.ops.quantized.embedding_bag_4bit_rowwise_offsets
    return op(torch.from_numpy(np.ascontiguousarray(q)), torch.from_numpy(np.ascontiguousarray(indices)),
              torch.from_numpy(np.ascontiguousarray(offsets)), False, 0, False,
              None if psw is None else torch.from_numpy(np.ascontiguousarray(psw, dtype=np.float32)), None, include_last_offset).numpy()


# ---- requests whose plan tests/qrows_plan_host.json pins (tests/test_qrows_host.py; ``pm_embbag_qrows_plan`` needs no device) -----------
# name: (bits, T, B, N, max_dim, min_dim, weighted, (bag_begin, bag_count) | None, out dtype, pm_set_tuning's (unroll, bags_per_block),
#        pm_set_forward_tuning's stage_out)
PLAN_REQUESTS = {
    "even_8bit_d128": (8, 16, 8192, 16 * 8192 * 20, 128, 128, False, None, "fp32", (0, 0), -1),
    "even_4bit_d128": (4, 16, 8192, 16 * 8192 * 20, 128, 128, False, None, "fp32", (0, 0), -1),
    "ragged_mixed_8bit": (8, 3, 5, 337, 128, 4, False, None, "fp32", (0, 0), -1),
    "ragged_mixed_4bit_weighted": (4, 3, 5, 337, 128, 8, True, None, "fp32", (0, 0), -1),
    "weighted_even": (8, 8, 512, 8 * 512 * 10, 64, 64, True, None, "fp32", (0, 0), -1),
    "batch_slice": (8, 4, 1000, 4 * 1000 * 7, 32, 32, False, (300, 250), "fp32", (0, 0), -1),
    "tile_longer_than_index_tile": (8, 1, 4, 6000, 128, 128, False, None, "fp32", (0, 0), -1),
    "out_fp16": (4, 16, 8192, 16 * 8192 * 20, 128, 128, False, None, "fp16", (0, 0), -1),
    "out_bf16_unroll2": (8, 16, 8192, 16 * 8192 * 20, 256, 256, False, None, "bf16", (2, 0), -1),
    "d4": (8, 2, 64, 2 * 64 * 3, 4, 4, False, None, "fp32", (0, 0), -1),
    "d1024_8bit": (8, 2, 64, 2 * 64 * 3, 1024, 1024, False, None, "fp32", (0, 0), -1),
    "d1024_4bit_fp16": (4, 2, 64, 2 * 64 * 3, 1024, 1024, False, None, "fp16", (0, 0), -1),
    "forced_tile_no_burst": (8, 1, 2, 6, 128, 128, False, None, "fp32", (8, 64), 0),
}
