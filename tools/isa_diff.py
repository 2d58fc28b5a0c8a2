#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 code of two builds of the engine (CPU; ROCm LLVM tools).

    python tools/isa_diff.py A.so B.so [regex]

Extracts the gfx950 code object of each library (as tests/test_kernel_budget.py does),
disassembles both with llvm-objdump -d, and prints one line per function symbol (kernels and the
device functions the compiler kept out of line) whose demangled name matches `regex`:

    n_A n_B  seq  mset  vgpr A/B  sgpr A/B  scratch A/B  lds A/B  waves A/B  name

n: instructions; seq: the instruction texts (mnemonic and operands) are equal in order; mset: the
multisets of mnemonics are equal (a pure reordering or register renaming keeps it); the resource
columns come from the code object's notes ('-' for a device function, which has none); waves: the
waves per SIMD the VGPR count allows (512 VGPRs, granule 8, at most 8).  A symbol in one build only
shows '-' on the other side.  The last line counts the symbols by outcome.
"""
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
NOTE_KEYS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def code_object(lib, tmp):
    """Path of the gfx950 code object extracted from `lib` into directory `tmp`."""
    os.makedirs(tmp)
    shutil.copy(lib, os.path.join(tmp, "lib.so"))
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp,
                   check=True, capture_output=True)
    (co,) = [f for f in os.listdir(tmp) if f.endswith("gfx950")]
    return os.path.join(tmp, co)


def functions(co):
    """{symbol: [(mnemonic, operands), ...]} of the code object's text."""
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True,
                          capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith(("\t", " ")):
            continue
        ins = line.split("//")[0].strip()
        if ins:
            mnem, _, ops = ins.partition(" ")
            cur.append((mnem, ops.strip()))
    return out


def notes(co):
    """{kernel symbol: {note key: int}} of the code object's AMDGPU metadata."""
    text = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True,
                          capture_output=True, text=True).stdout
    # a kernel's entry starts at "  - .key:" and its other keys sit at four spaces of indentation,
    # in alphabetical order: .name lies between the keys wanted, so collect each entry whole
    entries = []
    for line in text.splitlines():
        m = re.match(r"^  (- | {2})\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "- ":
            entries.append({})
        if entries:
            entries[-1][m.group(2)] = m.group(3)
    return {e["name"]: {k: int(e[k]) for k in NOTE_KEYS if k in e} for e in entries if "name" in e}


def waves(vgpr):
    return min(8, 512 // max(8, (vgpr + 7) // 8 * 8))


def demangle(names):
    """{symbol: readable name without the argument list}; the symbols themselves without c++filt."""
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), check=True,
                             capture_output=True, text=True).stdout.splitlines()
    except (OSError, subprocess.CalledProcessError):
        return dict(zip(names, names))
    return {n: re.sub(r"\(.*", "", d.replace("void ", "", 1)) for n, d in zip(names, out)}


def main(argv):
    if len(argv) not in (3, 4):
        sys.exit(__doc__)
    pat = re.compile(argv[3] if len(argv) == 4 else ".")
    with tempfile.TemporaryDirectory() as tmp:
        cos = [code_object(lib, os.path.join(tmp, side)) for lib, side in zip(argv[1:3], "ab")]
        fa, fb = (functions(co) for co in cos)
        na, nb = (notes(co) for co in cos)
    names = sorted(set(fa) | set(fb))
    pretty = demangle(names)
    tally = collections.Counter()
    print("n_A n_B seq mset vgpr sgpr scratch lds waves name   (A/B)")
    for n in names:
        if not pat.search(pretty[n]):
            continue
        a, b = fa.get(n), fb.get(n)
        if a is None or b is None:
            seq = mset = "-"
            tally["in one build only"] += 1
        else:
            seq = "eq" if a == b else "NE"
            mset = "eq" if collections.Counter(m for m, _ in a) == \
                collections.Counter(m for m, _ in b) else "NE"
            tally["identical" if seq == "eq" else
                  "reordered / renamed" if mset == "eq" else "different"] += 1
        cols = []
        for key in NOTE_KEYS:
            x, y = na.get(n, {}).get(key, "-"), nb.get(n, {}).get(key, "-")
            cols.append(f"{x}/{y}")
        va, vb = na.get(n, {}).get("vgpr_count"), nb.get(n, {}).get("vgpr_count")
        cols.append(f"{'-' if va is None else waves(va)}/{'-' if vb is None else waves(vb)}")
        print(len(a) if a is not None else "-", len(b) if b is not None else "-", seq, mset,
              *cols, pretty[n])
    print("# " + ", ".join(f"{v} {k}" for k, v in sorted(tally.items())))


if __name__ == "__main__":
    main(sys.argv)
