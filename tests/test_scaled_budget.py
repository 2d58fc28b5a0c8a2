"""Register / scratch / occupancy budgets of the scaled fp8 kernel instances (CPU: the gfx950
code object's metadata, in the manner of tests/test_fp8_budget.py).

The kernels that read or move dequantisation scales are kernels of their own names beside their
unscaled twins -- score_paged_scaled_kernel / score_ragged_scaled_kernel /
gather_paged_scaled_kernel / gather_ragged_scaled_kernel -- and exist for KVC_F8E4M3 (16) and
KVC_F8E5M2 (17) in the row widths NC = 4 / 8 / 16 and for nothing else.  None uses scratch, and
each keeps the occupancy (waves per SIMD by VGPRs and LDS) of its unscaled twin."""
import re

from test_fp8_budget import _all, waves_per_simd

TWINS = {  # scaled family -> (unscaled twin, threads per workgroup by NC)
    "25score_paged_scaled_kernel": ("18score_paged_kernel", {4: 256, 8: 512, 16: 512}),
    "26score_ragged_scaled_kernel": ("19score_ragged_kernel", {4: 256, 8: 512, 16: 512}),
    "26gather_paged_scaled_kernel": ("19gather_paged_kernel", {4: 256, 8: 256, 16: 256}),
    "27gather_ragged_scaled_kernel": ("20gather_ragged_kernel", {4: 256, 8: 256, 16: 256}),
}


def _family(ks, fam):
    inst = {}
    for n, v in ks.items():
        m = re.match(rf"_ZN3kvc{fam}ILi(\d+)ELi(\d+)EEE", n)
        if m:
            inst[(int(m.group(1)), int(m.group(2)))] = v
    return inst


def test_scaled_instances_exist_for_fp8_only_without_scratch_at_their_twins_occupancy(tmp_path):
    ks = _all(tmp_path)
    for fam, (twin, threads) in TWINS.items():
        inst, ref = _family(ks, fam), _family(ks, twin)
        want = [(dt, nc) for dt in (16, 17) for nc in (4, 8, 16)]
        assert sorted(inst) == want, (fam, sorted(inst))
        for (dt, nc), v in inst.items():
            r = ref[(dt, nc)]
            assert v["private_segment_fixed_size"] == 0, (fam, dt, nc, v)
            assert v.get("vgpr_spill_count", 0) == 0, (fam, dt, nc, v)
            assert waves_per_simd(v, threads[nc]) >= waves_per_simd(r, threads[nc]), \
                (fam, dt, nc, v, r)
            print(fam, dt, nc, "vgpr", v["vgpr_count"], "twin", r["vgpr_count"], "lds", v["lds"])


def test_no_other_kernel_carries_scales(tmp_path):
    """Every kernel whose name says `scaled` is one of the four families above."""
    ks = _all(tmp_path)
    named = [n for n in ks if "scaled" in n]
    assert len(named) == 4 * 6, named
    assert all(any(n.startswith(f"_ZN3kvc{fam}I") for fam in TWINS) for n in named), named
