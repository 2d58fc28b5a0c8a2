"""Scratch budget of the paged kernels (CPU: the gfx950 code object's metadata, read the way
tests/test_kernel_budget.py does).  Every gather_paged_kernel instance keeps its pass -- four
16-byte units of K and of V per thread -- in registers, and every score_paged_kernel instance
for rows of up to 512 bytes its staged chunks and row pointers: no private segment, no spills."""
import re

from test_kernel_budget import _kernels


def test_paged_gather_kernels_do_not_spill(tmp_path):
    ks = _kernels(tmp_path)
    inst = {n: v for n, v in ks.items() if re.match(r"_ZN3kvc19gather_paged_kernelILi\dELi\d+E", n)}
    assert len(inst) == 21, sorted(inst)  # three storage dtypes x seven row widths
    for n, v in inst.items():
        assert v["private_segment_fixed_size"] == 0 and v.get("vgpr_spill_count", 0) == 0, (n, v)


def test_paged_score_kernels_do_not_spill(tmp_path):
    """NC <= 32 (the bound of score_kernel's own budget test: the 1 KiB-row instances hold a whole
    row per lane group)."""
    ks = _kernels(tmp_path)
    inst = {n: v for n, v in ks.items()
            if re.match(r"_ZN3kvc18score_paged_kernelILi\dELi(4|8|10|16|20|32)E", n)}
    assert len(inst) == 18, sorted(inst)
    for n, v in inst.items():
        assert v["private_segment_fixed_size"] == 0 and v.get("vgpr_spill_count", 0) == 0, (n, v)
