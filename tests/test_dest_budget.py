"""Scratch budget of the destination copy kernels (CPU: the gfx950 code object's metadata, read
the way tests/test_kernel_budget.py does).  Every gather_dest_kernel instance (every row width, NC = 4 .. 64
chunks of 16 B) keeps its pass -- four 16-byte units of K and of V per
thread -- in registers: no private segment, no spills."""
import re

from test_kernel_budget import _kernels


def test_dest_kernels_do_not_spill(tmp_path):
    ks = _kernels(tmp_path)
    inst = {n: v for n, v in ks.items() if re.match(r"_ZN3kvc18gather_dest_kernelILi\dELi\d+E", n)}
    # three storage dtypes x seven row widths (the issue's bound is NC <= 32; the 1 KiB rows,
    # NC = 64, hold no more per thread and are held to the same)
    assert len(inst) == 21, sorted(inst)
    for n, v in inst.items():
        assert v["private_segment_fixed_size"] == 0 and v.get("vgpr_spill_count", 0) == 0, (n, v)
