#!/usr/bin/env python3
"""tools/fp32_matrix_coverage.py <trace> > profiles/fp32_matrix_coverage.txt -- which fp32 convolution kernels a run of the GPU suite launched.
<trace> is the output directory of
    rocprofv3 --kernel-trace --stats -d <trace> -o old --output-format csv -- python -m pytest tests -m gpu --ignore=tests/test_gpu_fp32_matrix.py \\
        --deselect tests/test_gpu_rgba_tta.py::test_fused_ends_launch_no_colour_stage
(every *kernel_stats.csv below it is read: one per process of the run; that test's torch profiler and rocprofv3 want the same tracer), or a text file
of "<launches> <kernel name>" lines aggregated from such a directory.  Kernel names are read with tests/fp32_matrix.key_of_name and set against the
kernels of the built objects (fp32_matrix.built_keys) and the table of unreachable ones."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fp32_matrix as fm  # noqa: E402


def launches(trace):
    names = {}
    if os.path.isdir(trace):
        for f in glob.glob(os.path.join(trace, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                names[row["Name"]] = names.get(row["Name"], 0) + int(float(row.get("Calls") or 1))
    else:
        for line in open(trace):
            if line.strip():
                cnt, name = line.strip().split(" ", 1)
                names[name] = names.get(name, 0) + int(cnt)
    return names


def show(key):
    return "%s<%s>" % (key[0], ", ".join(str(a).lower() if isinstance(a, bool) else str(a) for a in key[1])) if key[1] else key[0]


def main():
    seen = {}
    for name, cnt in launches(sys.argv[1]).items():
        if fm.is_fp32_conv(name):
            key = fm.key_of_name(name)
            assert key is not None, name
            seen[key] = seen.get(key, 0) + cnt
    built = fm.built_keys()
    assert set(seen) <= built, sorted(set(seen) - built)
    verdict = {k: "unreachable" if k in fm.UNREACHABLE else "launched" if k in seen else "never" for k in built}
    count = lambda v: sum(1 for x in verdict.values() if x == v)
    print("# Which fp32 convolution kernels (symbols matching conv3x3_ or upconv4x4_head, the 16-bit split kernels aside) the GPU suite launched WITHOUT")
    print("# tests/test_gpu_fp32_matrix.py, on one MI355X: tools/fp32_matrix_coverage.py on a rocprofv3 kernel trace of that run (its docstring has the command).")
    print("# %d kernels built: %d launched, %d never launched (each is a key of a case of tests/fp32_matrix.py), %d that no public call reaches"
          % (len(built), count("launched"), count("never"), count("unreachable")))
    print("# (UNREACHABLE there; %d of them seen here)." % sum(1 for k in seen if k in fm.UNREACHABLE))
    print("# verdict launches kernel")
    for k in sorted(built):
        print("%-11s %8d %s" % (verdict[k], seen.get(k, 0), show(k)))


if __name__ == "__main__":
    main()
