"""Static checks on the gfx950 code objects the build produced (CPU-only: llvm-objdump / llvm-readelf on waifu2x-converter-cpp_amd/lib/*.o).

* the hazard "VALU writes an SGPR -> a VMEM instruction reads it: 5 wait states" for VMEM instructions inside asm statements, which the compiler's hazard
  recogniser does not look into (tools/check_sgpr_vmem_hazard.py; round 5's objects had 72 such places);
* no VGPR spill and no scratch in the kernels of the default fp32 frame -- a scratch reload inside a stage waits with vmcnt(0) for every transfer in flight.
"""
import glob
import os
import re
import subprocess
import sys

import pytest

from fp32_matrix import kernel_objects   # (tests/test_fp32_matrix.py checks the list itself)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "waifu2x-converter-cpp_amd", "lib")
KERNEL_OBJS = kernel_objects()   # csrc/Makefile's OBJ line: every object built from a .hip source, the batch forms, the head, TTA and the colour stages included
OBJS = [os.path.join(LIB, o) for o in KERNEL_OBJS if os.path.exists(os.path.join(LIB, o))]


def _built():
    if len(OBJS) < len(KERNEL_OBJS):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as graft
        graft.build()
    return [os.path.join(LIB, o) for o in KERNEL_OBJS]


@pytest.mark.parametrize("obj", KERNEL_OBJS)
def test_no_sgpr_vmem_hazard_inside_asm_statements(obj):
    _built()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_sgpr_vmem_hazard.py"), os.path.join(LIB, obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "hazards found: 0" in r.stdout


def _resources(obj):
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), os.path.join(LIB, obj)], capture_output=True, text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) vspill\s+(\d+) sspill\s+(\d+) scratch\s+(\d+)", line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), vspill=int(m.group(4)), scratch=int(m.group(6)))
    return rows


@pytest.mark.parametrize("obj,pattern,allow_scratch", [
    ("w2xc_wino4_p.o", r"conv3x3_wino4", False),
    ("w2xc_wino4_n.o", r"conv3x3_wino4", False),
    ("w2xc_first2_wino4.o", r"conv3x3_first2_wino4", False),
    # (the PROG instantiations -- ...ELb1ELb1EE -- call w4_prog_job, a real function: its frame is the only scratch in that object)
    ("w2xc_wino4_f.o", r"conv3x3_wino4I.*ELb1ELb0EEv", False),
    ("w2xc_kernels.o", r"conv3x3_(first|last|mfma2)", False),
    # the batch forms, the 128 -> 256 layer and the head of upconv models
    ("w2xc_wino4_b.o", r"conv3x3_wino4_batch", False),
    ("w2xc_wino4_bf.o", r"conv3x3_wino4_batch", False),
    ("w2xc_wino4_bi.o", r"conv3x3_wino4_batch_l", False),
    ("w2xc_wino4_bo.o", r"conv3x3_wino4_batch_l", False),
    ("w2xc_wino4_bw.o", r"conv3x3_wino4_batch_l", False),
    ("w2xc_wino4_w.o", r"conv3x3_wino4", False),
    ("w2xc_first2_wino4_b.o", r"conv3x3_first2_wino4_batch", False),
    ("w2xc_conv_batch.o", r"conv3x3_(first|last)_batch", False),
    ("w2xc_wino_b.o", r"conv3x3_wino_batch", False),
    ("w2xc_gather_batch.o", r"conv3x3_last_gather_x4_batch", False),
    ("w2xc_upconv.o", r"upconv4x4_head", False),
    ("w2xc_upconv_b.o", r"upconv4x4_head_batch", False),
])
def test_hot_kernels_do_not_spill_vector_registers(obj, pattern, allow_scratch):
    if not os.path.exists(os.path.join(LIB, obj)):
        _built()
    rows = {k: v for k, v in _resources(obj).items() if re.search(pattern, k)}
    assert rows, "no kernel matched %s in %s" % (pattern, obj)
    bad = {k: v for k, v in rows.items() if v["vspill"] != 0 or (v["scratch"] != 0 and not allow_scratch)}
    assert not bad, bad
