"""Properties of the COMPILED un-pooled kernel over row-quantised tables (embedding_gather_qrows.hip), read from the built library's gfx950
code (no GPU needed; skipped without llvm-objdump): the rows a lane group is meant to keep in flight really are -- the code issues at
least the plan's default unroll of code loads between two full ``s_waitcnt vmcnt(0)``.  The helpers are tests/test_isa_properties.py's.

A row is TWO loads in the code: its codes (``global_load_dwordx2``: two dwords per lane) and its tail (8 bits: scale and bias are another
``global_load_dwordx2``; 4 bits: one ``global_load_dword``).  For 8-bit tables the count of ``global_load_dwordx2`` is therefore halved."""
import ctypes
import re

import pytest

from param_amd import _lib
from tests.test_isa_properties import NS, _kernel_resources, _kernel_text, _row_loads_between_full_waits, bundles  # noqa: F401

D = 128                     # the benchmark's width: G = 16 lanes per row (8 bits), 8 (4 bits)


def default_plan(bits):
    op = _lib.pm_embbag_batch()
    op.num_tables, op.index_dtype, op.max_dim = 16, _lib.PM_I64, D
    op.batch = op.bag_count = 1
    op.num_indices = 1 << 20
    op.tables = op.rows = op.dims = op.out_offsets = op.indices = op.offsets = 64      # never dereferenced on the host
    op.out_stride = 16 * D
    _lib.set_tuning()
    return _lib.embedding_gather_qrows_plan(op, bits)


def symbol(bits, out, lanes, unroll):
    return f"{NS}29embedding_gather_qrows_kernelILi{bits}E{out}Li{lanes}ELi{unroll}EE"


@pytest.mark.parametrize("out", ["f", "NS_3fwd7OutBF16E", "NS_3fwd6OutF16E"], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("bits", [8, 4])
def test_default_instance_keeps_its_rows_in_flight(bundles, bits, out):  # noqa: F811
    p = default_plan(bits)
    assert p["group_lanes"] == (16 if bits == 8 else 8) and p["unroll"] in (1, 2, 4, 8)
    text = _kernel_text(bundles, symbol(bits, out, p["group_lanes"], p["unroll"]))
    x2 = _row_loads_between_full_waits(text, "global_load_dwordx2")
    rows = x2 // 2 if bits == 8 else x2
    print(f"bits {bits} out {out}: {x2} global_load_dwordx2 between two full waits = {rows} rows (plan: {p['unroll']})")
    assert rows >= p["unroll"]
    assert "global_load_dwordx4" not in text and "flat_load" not in text and "scratch_" not in text and "global_atomic" not in text
    assert len(re.findall(r"global_store_dwordx[24] .* nt", text)) > 0


def test_no_instance_spills(bundles):  # noqa: F811
    """every instantiation (bits x output x lane group x unroll): no scratch, the three LDS arrays only; the registers of the default
    instances are DESIGN.md's (section 3.13)"""
    res = {n: v for n, v in _kernel_resources(bundles).items() if "29embedding_gather_qrows_kernel" in n}
    assert len(res) == 2 * 3 * 4 * 4, len(res)
    for name, (_vgpr, _sgpr, scratch, lds) in res.items():
        assert scratch == 0 and lds == 256 * 8 + 256 * 8 + 256 * 4, (name, scratch, lds)
    for bits in (8, 4):
        p = default_plan(bits)
        regs = [next(v[0] for n, v in res.items() if n.startswith(symbol(bits, out, p["group_lanes"], p["unroll"])))
                for out in ("f", "NS_3fwd7OutBF16E", "NS_3fwd6OutF16E")]
        print(f"bits {bits}, D = {D}, unroll {p['unroll']}: registers fp32 / bf16 / fp16 output {regs}")
        assert max(regs) <= 256, regs                      # two waves per SIMD at least (accumulation registers count in)
    assert ctypes.sizeof(_lib.pm_embbag_batch) == 144
