"""Hardware counters of the scaled fp8 SCORE / GATHER kernels against their unscaled twins
("fp8 caches", Scaled; profiles/r22_b_scaled_pmc.json).  On the GPU box, one counter
per profiler run (FETCH_SIZE and WRITE_SIZE do not fit one pass with an SQ counter: rocprofv3
answers error 38), each a run of its own with no tracing of any kind:

  for C in WRITE_SIZE FETCH_SIZE; do
    rocprofv3 --pmc $C -d DIR/$C --output-format csv -- \
        python tools/scaled_bench.py --rounds 1 --reps 1 --layers 4
  done
  python tools/scaled_pmc_summary.py DIR > profiles/<name>.json

The summary is the mean of each counter over the launches of every score_paged_kernel /
score_paged_scaled_kernel / gather_paged_kernel / gather_paged_scaled_kernel instance in the csv
files (DT 16 = e4m3, 17 = e5m2).  FETCH_SIZE / WRITE_SIZE are KiB summed over the device (on
gfx950 FETCH_SIZE sees half of wide coalesced read streams: compare instances,
tools/pmc_traffic.py).  The scaled instances' launches mix both scale-pool storages of the bench.
"""
import csv
import glob
import json
import re
import sys
from collections import defaultdict

COMMAND = ("for C in WRITE_SIZE FETCH_SIZE: rocprofv3 --pmc $C -d DIR/$C --output-format csv -- "
           "python tools/scaled_bench.py --rounds 1 --reps 1 --layers 4")
KERNEL = re.compile(r"((?:score|gather)_paged(?:_scaled)?_kernel)"
                    r"<\(?(?:int\))?(\d+), *\(?(?:int\))?(\d+)>")


def summarise(directory):
    acc = defaultdict(list)
    for path in glob.glob(directory + "/**/*counter_collection.csv", recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                m = KERNEL.search(row["Kernel_Name"])
                if m:
                    name = f"{m.group(1)}<{int(m.group(2))},{int(m.group(3))}>"
                    key = (name, row["Counter_Name"])
                    acc[key].append(float(row["Counter_Value"]))
    out = {"command": COMMAND}
    for (kernel, counter), v in sorted(acc.items()):
        out.setdefault(kernel, {})[counter] = dict(mean=sum(v) / len(v), n=len(v))
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    print(json.dumps(summarise(sys.argv[1]), indent=1))
