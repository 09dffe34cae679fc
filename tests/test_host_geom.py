"""The integers of the engine's host side (waifu2x-converter-cpp_amd/csrc/w2xc_host_geom.hpp: a unit's rows and source view, the staging chunks and
their taper, the rows finished job rows cover, the job flags' epoch test, the sub-batches of a host batch, the image pipeline's planes) are plain
arithmetic.  tests/cpp/host_geom_test.cpp includes that same header and checks what the consumers of those numbers need over a sweep of sizes; it
needs no GPU and no library.  The second test keeps the engine's memory with one owner."""
import glob
import os
import re
import subprocess

from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "csrc")


def test_host_geometry_holds_its_properties():
    subprocess.run(["make", "-C", CPP, "_build/host_geom_test"], check=True)
    r = subprocess.run([os.path.join(CPP, "_build", "host_geom_test")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all host geometry properties hold" in r.stdout


def test_allocation_calls_have_one_owner():
    """hipMalloc / hipFree / hipHostMalloc / hipHostFree appear in the engine's host code only in w2xc_scratch.hpp (every grow-only buffer) and where
    the weights are uploaded (upload, w2xc_model.cpp) and freed (the weight loop of ~DevCtx, w2xc_engine.hpp)."""
    call = re.compile(r"\bhip(?:Host)?(?:Malloc|Free)\(")
    # file -> (start marker, end marker) of the one region that may hold such calls
    allowed = {"w2xc_model.cpp": ("int upload(", "\n}\n"), "w2xc_engine.hpp": ("for (auto &l : layers) {", "pipe.destroy();")}
    files = sorted(glob.glob(os.path.join(CSRC, "*.cpp")) + glob.glob(os.path.join(CSRC, "*.hpp")))
    assert len(files) > 10
    strays = []
    for path in files:
        name = os.path.basename(path)
        if name == "w2xc_scratch.hpp":
            continue
        text = open(path).read()
        lo = hi = -1
        if name in allowed:
            lo = text.index(allowed[name][0])
            hi = text.index(allowed[name][1], lo)
        for m in call.finditer(text):
            if not lo <= m.start() < hi:
                strays.append("%s:%d: %s" % (name, text.count("\n", 0, m.start()) + 1, m.group(0)))
    assert not strays, "allocation calls outside their owner:\n" + "\n".join(strays)
    assert call.search(open(os.path.join(CSRC, "w2xc_scratch.hpp")).read())
