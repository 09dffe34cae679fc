"""tools/isa_compare.py writes the profiles/*_isa_compare.txt records: per kernel of two builds of the library's objects, a hash of the gfx950
disassembly without addresses and encodings, and the instruction count.  Two builds of one source with the same flags must compare equal -- the
property every such record rests on -- and a build with another optimisation level must not.  No GPU: hipcc cross-compiles."""
import os
import re
import subprocess
import sys

from conftest import ROOT

CSRC = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PROBE_FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950"]   # the Makefile's rule for w2xc_probe.hip


def build_probe(d, flags):
    os.makedirs(d)
    subprocess.run([HIPCC] + flags + ["-c", os.path.join(CSRC, "w2xc_probe.hip"), "-o", os.path.join(d, "w2xc_probe.o")], check=True)
    return str(d)


def compare(a, b):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_compare.py"), a, b], capture_output=True, text=True, check=True)
    head = [l for l in r.stdout.splitlines() if l.startswith("#")]
    rows = [l.split(" ", 4) for l in r.stdout.splitlines() if not l.startswith("#")]
    m = re.fullmatch(r"# (\d+) kernels, (\d+) differ", head[-2])
    assert m and head[-1] == "# object kernel parent new verdict", r.stdout
    return int(m.group(1)), int(m.group(2)), rows


def test_same_flags_compare_equal_and_another_level_does_not(tmp_path):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(HIPCC) " + " ".join(PROBE_FLAGS).replace("gfx950", "$(ARCH)") + " -shared w2xc_probe.hip" in mk, "the flags here are the Makefile's"
    a, b = build_probe(tmp_path / "a", PROBE_FLAGS), build_probe(tmp_path / "b", PROBE_FLAGS)
    c = build_probe(tmp_path / "c", ["-O1"] + PROBE_FLAGS[1:])
    total, differ, rows = compare(a, b)
    assert total >= 1 and differ == 0 and len(rows) == total
    for obj, kernel, ha, hb, verdict in rows:
        assert obj == "w2xc_probe.o" and ha == hb and re.fullmatch(r"[0-9a-f]{16}", ha) and re.fullmatch(r"same \([1-9]\d* instructions\)", verdict), (kernel, verdict)
    total_c, differ_c, rows_c = compare(a, c)
    assert total_c == total and differ_c >= 1
    assert sum(1 for r in rows_c if r[2] != r[3] and r[4].startswith("DIFFER (")) == differ_c
