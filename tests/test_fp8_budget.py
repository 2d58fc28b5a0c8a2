"""Register / scratch / occupancy budgets of the fp8 kernel instances (CPU: the gfx950 code
object's metadata, as tests/test_kernel_budget.py reads it).

Every kernel that takes the storage dtype exists for KVC_F8E4M3 (16) and KVC_F8E5M2 (17) in the
row widths NC = 4 / 8 / 16 (D = 64 / 128 / 256 bytes) and no other; none spills; each reaches the
occupancy of the bf16 instance of the same NC -- waves per SIMD as the VGPR count and the LDS claim
allow (512 VGPRs per SIMD lane in steps of 8, 160 KiB of LDS per CU, at most 8 waves per SIMD).
The fused select_gather instances for fp8 rows (last template argument true) stay within the 64
VGPRs of two 1 024-thread (four 512-thread) rows per CU."""
import re

from test_kernel_budget import _kernels

FAMILIES = {  # mangled prefix -> threads per workgroup by NC (score: score_waves(NC) * 64)
    "12score_kernel": {4: 256, 8: 512, 16: 512},
    "18score_paged_kernel": {4: 256, 8: 512, 16: 512},
    "19score_ragged_kernel": {4: 256, 8: 512, 16: 512},
    "13gather_kernel": {4: 256, 8: 256, 16: 256},
    "18gather_dest_kernel": {4: 256, 8: 256, 16: 256},
    "19gather_paged_kernel": {4: 256, 8: 256, 16: 256},
    "20gather_ragged_kernel": {4: 256, 8: 256, 16: 256},
}


def _all(tmp_path):
    import os
    import subprocess
    from test_kernel_budget import LLVM
    ks = _kernels(tmp_path)
    (co,) = [p for p in tmp_path.iterdir() if p.name.endswith("gfx950")]
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(co)], check=True,
                           capture_output=True, text=True, timeout=120).stdout
    lds = None  # (a kernel's keys are sorted: its LDS size comes before its name)
    for line in notes.splitlines():
        m = re.match(r"^    \.(name|group_segment_fixed_size):\s+(\S+)", line)
        if m and m.group(1) == "name":
            ks[m.group(2)]["lds"] = lds
            lds = None
        elif m:
            lds = int(m.group(2))
    assert all(v["lds"] is not None for v in ks.values())
    return ks


def waves_per_simd(v, threads):
    by_vgpr = 512 // (-(-v["vgpr_count"] // 8) * 8)
    waves = threads // 64
    by_lds = (163840 // v["lds"]) * waves // 4 if v.get("lds") else 8
    return min(8, by_vgpr, max(by_lds, 1))


def test_fp8_stream_kernels_exist_do_not_spill_and_keep_occupancy(tmp_path):
    ks = _all(tmp_path)
    for fam, threads in FAMILIES.items():
        inst = {}
        for n, v in ks.items():
            m = re.match(rf"_ZN3kvc{fam}ILi(\d+)ELi(\d+)EEE", n)
            if m:
                inst[(int(m.group(1)), int(m.group(2)))] = v
        for dt in (16, 17):
            assert sorted(nc for d, nc in inst if d == dt) == [4, 8, 16], (fam, dt)
            for nc in (4, 8, 16):
                v, ref = inst[(dt, nc)], inst[(1, nc)]
                assert v["private_segment_fixed_size"] == 0, (fam, dt, nc, v)
                assert v.get("vgpr_spill_count", 0) == 0, (fam, dt, nc, v)
                assert waves_per_simd(v, threads[nc]) >= waves_per_simd(ref, threads[nc]), \
                    (fam, dt, nc, v, ref)


def test_fp8_fused_select_gather_instances(tmp_path):
    ks = _all(tmp_path)
    pat = r"_ZN3kvc20select_gather_kernelILi1ELi(512|1024)ELi(\d+)ELb([01])ELb([01])ELb1EEE"
    inst = {}
    for n, v in ks.items():
        m = re.match(pat, n)
        if m:
            inst[tuple(int(g) for g in m.groups())] = v
    # 512-thread: reference and stable; 1 024-thread: reference with / without level-0 tables,
    # stable -- each for the three fp8 row widths
    want = {(512, nc, st, 1) for nc in (4, 8, 16) for st in (0, 1)} | \
        {(1024, nc, 0, l0) for nc in (4, 8, 16) for l0 in (0, 1)} | \
        {(1024, nc, 1, 0) for nc in (4, 8, 16)}
    assert set(inst) == want
    for key, v in inst.items():
        assert v["vgpr_count"] <= 64, (key, v)
        assert v["private_segment_fixed_size"] == 0 and v.get("vgpr_spill_count", 0) == 0, (key, v)
    # the fp8 flag exists for the 16-bit key class only
    assert not [n for n in ks if re.match(r"_ZN3kvc20select_gather_kernelILi0E.*Lb1EEEv", n)]
