"""Generates tests/golden/qgather_cases.npz: outputs of torch's CPU operators for UN-POOLED lookups over row-quantised tables --
quantized::embedding_bag_{byte,4bit}_rowwise_offsets over bags of one (offsets = arange) on the seeded inputs of tests/qgather_cases.py
and on the hand-built signed-zero rows of tests/qgather_rules.signed_zero_rows, and the forward of a torch.ao.nn.quantized.Embedding
(quantized::embedding_byte).  Nothing in the file comes from this project's arithmetic.  They pin tests/qgather_rules.py
(tests/test_qgather_host.py) and, through it, the kernel.
Run from the repository root:  python tests/golden/gen_qgather.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import qgather_cases as G  # noqa: E402
from tests import qgather_rules as Q  # noqa: E402
from tests import qrows_cases as C  # noqa: E402

OUT = os.path.join(HERE, "qgather_cases.npz")


def main():
    out = {}
    idx = G.indices()
    out["indices"] = idx
    for bits in G.BITS:
        for dim in G.DIMS:
            q = C.torch_prepack(C.float_table(dim), bits)
            out[f"q_{bits}_{dim}"] = q
            out[G.key(bits, dim)] = G.torch_rows(q, bits, idx)
        sz = Q.signed_zero_rows(8, bits)                             # (layout only: the bytes are data, the results below are torch's)
        out[f"zeros_q_{bits}"] = sz
        out[f"zeros_out_{bits}"] = G.torch_rows(sz, bits, np.arange(sz.shape[0], dtype=np.int64))
    emb, packed = G.torch_embedding(C.float_table(24), idx)
    out["embedding_q_8_24"], out["embedding_out_8_24"] = packed, emb
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; torch", torch.__version__)


if __name__ == "__main__":
    main()
