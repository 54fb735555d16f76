"""Properties of the COMPILED element-wise Adagrad instances (``OPT == 2``) of the apply's main kernel and of the bag-major kernel,
read from the built library's gfx950 code (no GPU needed; skipped without the LLVM tools, like tests/test_isa_properties.py whose
helpers this file uses).

The note in embbag_bwd_sorted_kernels.inc says the Adagrad instances are the ones that spill when pushed, and the new instances carry
16 (fp32 tables) / 2 x 16 (16-bit tables) bytes of state per lane and row on top of the row-wise instance's registers.  Two things no
parity test would notice:
  * scratch: the code object's metadata shows a private segment of 0 bytes for every new instance;
  * loads in flight: the largest number of 16-byte loads issued between two full waits is not smaller than the same figure of the
    row-wise (``OPT == 1``) instance of the same kernel in the same library -- the existing instance is the yardstick, not a number.
"""
import re

import pytest

from tests.test_isa_properties import NS, _kernel_resources, _kernel_text, _row_loads_between_full_waits, bundles  # noqa: F401

# (kernel, template arguments with the optimizer left open): fp32 tables with G = 32 and bf16 tables, as the benchmark shapes launch them
MAIN = ["22bwd_sorted_main_kernelINS0_7SDstF32EjLi32ELb0ELi{opt}ELi1024E", "22bwd_sorted_main_kernelINS0_7SDstF32EjLi32ELb0ELi{opt}ELi512E",
        "22bwd_sorted_main_kernelINS0_8SDstBF16EjLi16ELb0ELi{opt}ELi1024E", "22bwd_sorted_main_kernelINS0_8SDstBF16EjLi16ELb0ELi{opt}ELi512E"]
UNIQUE = ["17bwd_unique_kernelINS0_7SDstF32ELi32ELi{opt}E", "17bwd_unique_kernelINS0_8SDstBF16ELi16ELi{opt}E"]


def test_no_element_wise_instance_uses_scratch(bundles):      # noqa: F811
    res = _kernel_resources(bundles)
    new = {}
    for n, v in res.items():
        m = re.search(r"(22bwd_sorted_main_kernel|23bwd_sorted_fixup_kernel)I\w+?Lb[01]ELi2ELi\d+EEE", n) or \
            re.search(r"(17bwd_unique_kernel|15hyb_rest_kernel)INS0_\w+?ELi\d+ELi2EEE", n)
        if m:
            new[n] = v
    # 3 dtypes x 2 key widths x 4 lane-group sizes x weighted x 3 tiles of main + fix-up, 3 x 4 of the bag-major and the left-over kernel
    assert len(new) == 2 * 144 + 2 * 12, len(new)
    spilled = {n: v[2] for n, v in new.items() if v[2] != 0}
    assert not spilled, spilled
    for pat in MAIN + UNIQUE:
        name = NS + pat.format(opt=2)
        hit = [v for n, v in new.items() if n.startswith(name)]
        assert len(hit) == 1 and hit[0][2] == 0, (name, hit)
        print(pat.format(opt=2), "vgpr / sgpr / scratch / lds", hit[0])


@pytest.mark.parametrize("pat", MAIN + UNIQUE)
def test_element_wise_instance_keeps_as_many_loads_in_flight_as_the_row_wise_one(bundles, pat):      # noqa: F811
    elem = _row_loads_between_full_waits(_kernel_text(bundles, NS + pat.format(opt=2)))
    rowwise = _row_loads_between_full_waits(_kernel_text(bundles, NS + pat.format(opt=1)))
    print(pat, "16-byte loads between two full waits: element-wise", elem, "row-wise", rowwise)
    assert rowwise >= 4
    assert elem >= rowwise, (pat, elem, rowwise)
