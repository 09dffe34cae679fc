"""The packers of upconv head models (w2xc_upconv_pack, w2xc_pad_layer, w2xc_pad_head in waifu2x-converter-cpp_amd/csrc/w2xc_pack.cpp):
tests/cpp/upconv_pack_test.cpp is built with g++ from that file alone, as tests/test_pack.py builds pack_test.cpp, and checks that every head weight sits
in the image once, at the lane its (plane, tap, output) says, and that zero-padded 16 -> 32 images hold exact zeros in the added planes.  No GPU, no library."""
import os
import subprocess

from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "csrc")


def test_upconv_packers_hold_their_properties():
    os.makedirs(os.path.join(CPP, "_build"), exist_ok=True)
    exe = os.path.join(CPP, "_build", "upconv_pack_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(CPP, "upconv_pack_test.cpp"),
                    os.path.join(CSRC, "w2xc_pack.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all upconv packer properties hold" in r.stdout
