"""Register / scratch / occupancy budgets of the paged-destination copy kernels (CPU: the gfx950
code object's metadata, in the manner of tests/test_scaled_budget.py).

gather_repage_kernel / gather_repage_ragged_kernel exist for exactly the (dtype, row width)
instances gather_paged_kernel has (21 of bf16 / fp16 / fp32 rows and 6 of fp8 rows); their
scale-carrying twins gather_repage_sc_kernel / gather_repage_ragged_sc_kernel for KVC_F8E4M3 (16) /
KVC_F8E5M2 (17) x NC 4 / 8 / 16 only.  None uses scratch or spills, and each keeps at least the
waves per SIMD of its in-place twin."""
from test_fp8_budget import _all, waves_per_simd
from test_scaled_budget import _family

THREADS = 256  # kGatherThreads
TWINS = {  # family -> in-place twin
    "20gather_repage_kernel": "19gather_paged_kernel",
    "27gather_repage_ragged_kernel": "20gather_ragged_kernel",
    "23gather_repage_sc_kernel": "26gather_paged_scaled_kernel",
    "30gather_repage_ragged_sc_kernel": "27gather_ragged_scaled_kernel",
}


def test_instances_scratch_and_occupancy(tmp_path):
    ks = _all(tmp_path)
    paged = _family(ks, "19gather_paged_kernel")
    assert len(paged) == 21 + 6 and len([k for k in paged if k[0] < 16]) == 21, sorted(paged)
    fp8 = [(dt, nc) for dt in (16, 17) for nc in (4, 8, 16)]
    for fam, twin in TWINS.items():
        inst, ref = _family(ks, fam), _family(ks, twin)
        assert sorted(inst) == (fp8 if "_sc_" in fam else sorted(paged)), (fam, sorted(inst))
        for key, v in inst.items():
            assert v["private_segment_fixed_size"] == 0, (fam, key, v)
            assert v.get("vgpr_spill_count", 0) == 0, (fam, key, v)
            assert waves_per_simd(v, THREADS) >= waves_per_simd(ref[key], THREADS), \
                (fam, key, v, ref[key])
            print(fam, key, "vgpr", v["vgpr_count"], "twin", ref[key]["vgpr_count"])


def test_no_other_kernel_is_a_repage_kernel(tmp_path):
    ks = _all(tmp_path)
    named = [n for n in ks if "repage" in n]
    assert len(named) == 2 * (21 + 6) + 2 * 6, named
    assert all(any(n.startswith(f"_ZN3kvc{fam}I") for fam in TWINS) for n in named), named
    assert not any("scaled" in n for n in named)
