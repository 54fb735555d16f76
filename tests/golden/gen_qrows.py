"""Generates tests/golden/qrows_cases.npz: outputs of torch's CPU lookup operators over row-quantised tables
(quantized::embedding_bag_{byte,4bit}_rowwise_offsets over quantized::embedding_bag_{byte,4bit}_prepack) on the seeded inputs of
tests/qrows_cases.py, and over the hand-built rows with Inf / NaN tails of tests/qrows_rules.special_rows.  Nothing in the file comes
from this project's arithmetic.  They pin tests/qrows_rules.py (tests/test_qrows_host.py) and, through it, the kernel.
Run from the repository root:  python tests/golden/gen_qrows.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import qrows_cases as C  # noqa: E402
from tests import qrows_rules as R  # noqa: E402

OUT = os.path.join(HERE, "qrows_cases.npz")


def main():
    out = {}
    idx, off, psw = C.request()
    out["indices"], out["offsets"], out["psw"] = idx, off, psw
    for bits in C.BITS:
        for dim in C.DIMS:
            out[f"q_{bits}_{dim}"] = C.torch_prepack(C.float_table(dim), bits)
        sp = R.special_rows(8, bits)                                 # (layout only: the bytes are data, the results below are torch's)
        si, so = C.special_request()
        out[f"special_q_{bits}"] = sp
        out[f"special_out_{bits}"] = C.torch_lookup(sp, bits, si, so)
    for bits, dim, it, weighted in C.case_names():
        dt = np.int32 if it == "i32" else np.int64
        out[C.key(bits, dim, it, weighted)] = C.torch_lookup(out[f"q_{bits}_{dim}"], bits, idx.astype(dt), off.astype(dt), psw if weighted else None)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; torch", torch.__version__)


if __name__ == "__main__":
    main()
