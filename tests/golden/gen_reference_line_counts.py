"""Records the line count of every .py file of the reference (tests/test_citations.py checks
this repo's `file.py:N[-M]` citations against them).  Usage:
    python tests/golden/gen_reference_line_counts.py REFERENCE_DIR
Only names and line counts are stored (reference_line_counts.json); nothing of the files' text.
"""
import json
import os
import sys

ref = sys.argv[1]
out = {}
for root, _, fs in os.walk(ref):
    for f in fs:
        if f.endswith(".py"):
            p = os.path.join(root, f)
            out[os.path.relpath(p, ref)] = sum(1 for _ in open(p, errors="ignore"))
dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_line_counts.json")
with open(dst, "w") as fh:
    json.dump(dict(sorted(out.items())), fh, indent=1)
    fh.write("\n")
print(f"{len(out)} files -> {dst}")
