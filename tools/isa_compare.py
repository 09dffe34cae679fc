#!/usr/bin/env python3
"""tools/isa_compare.py PARENT_DIR NEW_DIR [--out FILE] -- the gfx950 code of two builds of the library's kernel objects, kernel by kernel.

The recipe of the profiles/*_isa_compare.txt records: for every *.o that both directories hold, take the gfx950 code object out of the
object's fat binary, disassemble it (llvm-objdump -d), cut the listing from label to label, drop addresses, encodings and the padding mark, and per kernel
print a hash of what is left and its instruction count, the two builds side by side:

    object kernel parent new verdict

verdict: "same (N instructions)", "DIFFER (A -> B instructions)", or "only in parent" / "only in new"; objects that only one directory
holds are named in the header.  The last header line is "# N kernels, M differ" (kernels of one build alone count as differing).
It hashes and counts; it does not look at what the instructions are.  Exit status 0 whatever the counts: the caller judges.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("W2XC_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
LABEL = re.compile(r"^[0-9a-f]+ <(\S+)>:$")


def disassemble(obj):
    """the llvm-objdump -d listing of the gfx950 code object in a hipcc object file ('' where it has none: host code only)"""
    with tempfile.TemporaryDirectory() as t:
        fat, co = os.path.join(t, "fat.bin"), os.path.join(t, "k.co")
        # (an explicit output: without one llvm-objcopy rewrites its input in place)
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(t, "copy.o")],
                       check=True, capture_output=True)
        if not os.path.exists(fat) or os.path.getsize(fat) == 0:
            return ""
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET,
                        "--output=" + co], check=True, capture_output=True)
        return subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout


def kernels(listing):
    """{label: (hash, instruction count)}: a label's lines up to the next label, each without its '// address: encoding' comment"""
    out, name, lines = {}, None, []

    def flush():
        if name is not None:
            out[name] = (hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16], len(lines))

    for line in listing.splitlines():
        m = LABEL.match(line)
        if m:
            flush()
            name, lines = m.group(1), []
        elif name is not None and line.startswith("\t") and line.strip() != "...":
            # ("...": llvm-objdump's mark for a run of zero bytes, the padding up to the next function's alignment -- no instruction, and whether a
            #  kernel has it depends on where the linker put its neighbour)
            lines.append(line.split("//")[0].strip())
    flush()
    return out


def has_fatbin(obj):
    r = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-S", obj], capture_output=True, text=True)
    return ".hip_fatbin" in r.stdout


def compare(parent_dir, new_dir):
    """(header lines, table rows, kernels, differing kernels)"""
    names = lambda d: {f for f in os.listdir(d) if f.endswith(".o") and has_fatbin(os.path.join(d, f))}
    po, no = names(parent_dir), names(new_dir)
    head = ["# objects only in the parent build: " + " ".join(sorted(po - no))] if po - no else []
    head += ["# objects only in the new build: " + " ".join(sorted(no - po))] if no - po else []
    rows, total, differ = [], 0, 0
    for obj in sorted(po & no):
        a, b = kernels(disassemble(os.path.join(parent_dir, obj))), kernels(disassemble(os.path.join(new_dir, obj)))
        for k in sorted(set(a) | set(b)):
            total += 1
            if k in a and k in b and a[k][0] == b[k][0]:
                verdict = "same (%d instructions)" % a[k][1]
            else:
                differ += 1
                verdict = "DIFFER (%d -> %d instructions)" % (a[k][1], b[k][1]) if k in a and k in b else "only in parent" if k in a else "only in new"
            rows.append("%s %s %s %s %s" % (obj, k, a[k][0] if k in a else "-", b[k][0] if k in b else "-", verdict))
    return head, rows, total, differ


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("parent_dir")
    ap.add_argument("new_dir")
    ap.add_argument("--out", help="write the table here as well")
    a = ap.parse_args(argv)
    head, rows, total, differ = compare(a.parent_dir, a.new_dir)
    text = "\n".join(head + ["# %d kernels, %d differ" % (total, differ), "# object kernel parent new verdict"] + rows) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
