"""The cases behind tests/golden/pruned_cases.npz: torch's CPU operators ``quantized::embedding_bag_{byte,4bit}_rowwise_offsets`` called
with ``pruned_weights=True`` and a ``compressed_indices_mapping`` over ONE pruned table, 8- and 4-bit, weighted and not, int32 and
int64 indices, pooled and -- as bags of one -- un-pooled.  ``python -m tests.pruned_cases`` writes the fixture anew (a few KB);
tests/test_pruned_host.py compares tests/pruned_rules.py with it and with the operators live.

The table is ``qrows_cases.float_table(DIM)``: ROWS logical rows of which ``keep()`` keeps about half; the physical table is the kept
rows prepacked by torch, the remap sends the kept rows to consecutive physical rows and the dropped ones to -1.  The request has empty
bags, a bag that is all pruned, a bag with nothing pruned, and a pruned lookup whose weight is +Inf (its bag stays finite)."""
import os

import numpy as np

from tests import qrows_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "pruned_cases.npz")
DIM = 24
LENS = (0, 5, 4, 30, 3, 0, 6)        # bag 2: all pruned; bag 4: nothing pruned; bags 0 and 5: empty
ALL_PRUNED, NONE_PRUNED, INF_AT = 2, 4, 0


def keep():
    """bool ``[ROWS]``: the rows that stay (seeded; rows 0 .. 5, ``float_table``'s special rows, alternate)"""
    rng = np.random.default_rng(C.SEED + 77)
    k = rng.random(C.ROWS) < 0.5
    k[:6] = (True, False, True, False, True, True)
    return k


def remap(k=None):
    """int32 ``[ROWS]``: kept rows -> consecutive physical rows in order, dropped rows -> -1"""
    k = keep() if k is None else np.asarray(k, dtype=bool)
    return np.where(k, np.cumsum(k) - 1, -1).astype(np.int32)


def request():
    """(indices int64 [N] over the LOGICAL rows, offsets int64 [B], per_sample_weights fp32 [N]); ``include_last_offset=False``"""
    rng = np.random.default_rng(C.SEED + 78)
    k = keep()
    kept, dropped = np.nonzero(k)[0], np.nonzero(~k)[0]
    lens = np.array(LENS, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    idx = rng.integers(0, C.ROWS, int(lens.sum())).astype(np.int64)
    psw = (rng.standard_normal(idx.size) * 2).astype(np.float32)
    idx[0], idx[1] = dropped[0], kept[0]                             # bag 1 begins with a pruned lookup of weight +Inf, then a kept one
    psw[INF_AT] = np.inf
    a = off[ALL_PRUNED]
    idx[a:a + lens[ALL_PRUNED]] = rng.choice(dropped, lens[ALL_PRUNED])
    a = off[NONE_PRUNED]
    idx[a:a + lens[NONE_PRUNED]] = rng.choice(kept, lens[NONE_PRUNED])
    return idx, off, psw


def physical_table(bits):
    """uint8 ``[kept rows, row_bytes]``: the kept rows of ``float_table(DIM)`` prepacked by torch (a kept row's bytes are what the
    unpruned table's prepack holds for it: the formats are row-wise)"""
    return C.torch_prepack(C.float_table(DIM)[keep()], bits)


def torch_lookup_pruned(q, bits, mapping, indices, offsets, psw=None):
    """fp32 ``[B, D]``: the operator with ``pruned_weights=True`` and ``compressed_indices_mapping=mapping`` (int32), on the CPU"""
    import torch

    op = torch.ops.quantized.embedding_bag_byte_rowwise_offsets if bits == 8 else torch.ops.quantized.embedding_bag_4bit_rowwise_offsets
    return op(torch.from_numpy(np.ascontiguousarray(q)), torch.from_numpy(np.ascontiguousarray(indices)),
              torch.from_numpy(np.ascontiguousarray(offsets)), False, 0, True,
              None if psw is None else torch.from_numpy(np.ascontiguousarray(psw, dtype=np.float32)),
              torch.from_numpy(np.ascontiguousarray(mapping, dtype=np.int32)), False).numpy()


def case_names():
    return [(bits, it, w) for bits in C.BITS for it in ("i32", "i64") for w in (False, True)]


def key(bits, it, weighted):
    return f"out_{bits}_{it}_{'w' if weighted else 'u'}"


def cases():
    """{name: array}: the operators' pooled outputs per case, and per format the un-pooled rows (bags of one)"""
    idx, off, psw = request()
    out = {}
    for bits in C.BITS:
        q = physical_table(bits)
        for it in ("i32", "i64"):
            dt = np.int32 if it == "i32" else np.int64
            for w in (False, True):
                out[key(bits, it, w)] = torch_lookup_pruned(q, bits, remap(), idx.astype(dt), off.astype(dt), psw if w else None)
        out[f"rows_{bits}"] = torch_lookup_pruned(q, bits, remap(), idx, np.arange(idx.size, dtype=np.int64))
    return out


if __name__ == "__main__":
    np.savez_compressed(PATH, **cases())
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
