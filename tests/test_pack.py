"""The weight packers and shape predicates (waifu2x-converter-cpp_amd/csrc/w2xc_pack.cpp) are plain C++ loops over floats.  tests/cpp/pack_test.cpp is
built with g++ from that file alone -- which is the proof that the unit needs no HIP -- and checks what the kernels rely on: every weight at the
address the kernel's fragment addressing documents, zeros in every padding slot, the 16-bit terms of the split images as close to the weight as
bf16 / fp16 promise, both F(4x4,3x3) packers holding the same U, PROG's counters matching its job grid.  It needs no GPU and no library."""
import os
import subprocess

from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")


def test_packers_hold_their_properties():
    subprocess.run(["make", "-C", CPP, "_build/pack_test"], check=True)
    r = subprocess.run([os.path.join(CPP, "_build", "pack_test")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all packer properties hold" in r.stdout
