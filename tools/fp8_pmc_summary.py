"""Hardware counters of the SCORE kernels, fp8 against bf16 ("fp8 caches";
profiles/r21_b_fp8_score_pmc.json).  Two steps on the GPU box, counters in a run of their own with
no tracing of any kind:

  rocprofv3 --pmc SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT \
      SQ_WAVE_CYCLES -d DIR --output-format csv -- python tools/fp8_bench.py --rounds 1 --reps 1
  python tools/fp8_pmc_summary.py DIR > profiles/<name>.json

The summary is the mean of each counter over the launches of every score_kernel<DT, NC> and
score_paged_kernel<DT, NC> instance in the csv files (DT 1 = bf16, 16 = e4m3, 17 = e5m2), with
the number of launches averaged.  Counter values are sums over the device as the profiler reports
them: compare instances, do not read them as cycles of one CU.
"""
import csv
import glob
import json
import re
import sys
from collections import defaultdict

COMMAND = ("rocprofv3 --pmc SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS "
           "SQ_LDS_BANK_CONFLICT SQ_WAVE_CYCLES -d DIR --output-format csv -- "
           "python tools/fp8_bench.py --rounds 1 --reps 1")
KERNEL = re.compile(r"(score_kernel|score_paged_kernel)<\(?(?:int\))?(\d+), *\(?(?:int\))?(\d+)>")


def summarise(directory):
    acc = defaultdict(list)
    for path in glob.glob(directory + "/**/*counter_collection.csv", recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                m = KERNEL.search(row["Kernel_Name"])
                if m:
                    key = (f"{m.group(1)}<{int(m.group(2))},{int(m.group(3))}>", row["Counter_Name"])
                    acc[key].append(float(row["Counter_Value"]))
    out = {"command": COMMAND}
    for (kernel, counter), v in sorted(acc.items()):
        out.setdefault(kernel, {})[counter] = dict(mean=sum(v) / len(v), n=len(v))
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    print(json.dumps(summarise(sys.argv[1]), indent=1))
