"""Every `file.py:N[-M]` citation of a reference file in this repo lands inside that file.

Citations are how a reader checks parity against the reference, so a line range past the end
of the cited file is a defect.  The reference's file names and line counts are recorded in
tests/golden/reference_line_counts.json (tests/golden/gen_reference_line_counts.py), so the check
needs no copy of the reference.
"""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = os.path.join(ROOT, "tests", "golden", "reference_line_counts.json")
SKIP_DOCS = {"VERDICT.md", "ADVICE.md", "SURVEY.md", "BASELINE.md"}  # not authored here
PAT = re.compile(r"((?:[A-Za-z_][\w.-]*/)*[A-Za-z_][\w-]*\.py):(\d+)(?:-(\d+))?")


def _reference_files():
    with open(COUNTS) as f:
        return json.load(f)


def _resolve(cited, ref):
    """Line counts of the reference files a (possibly partial) path can name."""
    return [n for rel, n in ref.items() if rel == cited or rel.endswith("/" + cited)]


def test_reference_citations_in_range():
    ref = _reference_files()
    bad = []
    for root, dirs, fs in os.walk(ROOT):
        dirs[:] = [d for d in dirs if d not in (".git", "golden", "gpurun_out", "profiles")]
        for f in fs:
            if not f.endswith((".py", ".h", ".hip", ".cpp", ".md")) or f in SKIP_DOCS:
                continue
            p = os.path.join(root, f)
            for ln, line in enumerate(open(p, errors="ignore"), 1):
                for m in PAT.finditer(line):
                    counts = _resolve(m.group(1), ref)
                    if not counts:
                        continue  # one of this repo's own files
                    hi = int(m.group(3) or m.group(2))
                    if hi > max(counts):
                        bad.append(f"{os.path.relpath(p, ROOT)}:{ln}: {m.group(0)} "
                                   f"(file has {max(counts)} lines)")
    assert not bad, "\n".join(bad)


OWN = re.compile(r"\b((?:tests|tools|oracle|profiles|include|cs3602-llm-inference-acceleration_amd)"
                 r"/[\w./-]*\w\.(?:py|cpp|hip|h|c|sh|json|jsonl|csv|txt|md|npz))\b")


def test_repo_file_citations_exist():
    """Every path of this repo's own files named in its sources and docs (csrc comments
    included) exists -- a stale file reference is as misleading as a stale line number."""
    bad = []
    for root, dirs, fs in os.walk(ROOT):
        dirs[:] = [d for d in dirs if d not in (".git", "gpurun_out", "profiles", "__pycache__",
                                                "_build", "_lib")]
        for f in fs:
            if not f.endswith((".py", ".h", ".hip", ".cpp", ".c", ".sh", ".md")) or f in SKIP_DOCS:
                continue
            p = os.path.join(root, f)
            for ln, line in enumerate(open(p, errors="ignore"), 1):
                for m in OWN.finditer(line):
                    path = m.group(1)
                    if "*" in path or "<" in path:
                        continue
                    if not os.path.exists(os.path.join(ROOT, path)):
                        bad.append(f"{os.path.relpath(p, ROOT)}:{ln}: {path}")
    assert not bad, "\n".join(bad)
