#!/usr/bin/env python
"""Host cost of selection, this tree against a checkout of another commit (the parent) built beside it: one fresh process per side and round, the sides
alternating, the order swapped every round; with --aa the other tree is measured twice per round, which gives the A/A margin of the session.

    python tools/chain_ab.py --other DIR [--rounds 5] [--out FILE]          w2xc_plan_rows of the scale model on three planes (no device)
    python tools/chain_ab.py --other DIR --gpu [--aa] [--rounds 5] ...      the smallest whole calls on one MI355X: convert_device and the uint8 RGB image
                                                                           call at 64 x 64, one image -- where host work is the largest share of a call

Per measurement and side: the per-call time of every round, their median and their spread (max - min).  One JSON object."""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(root, gpu):
    sys.path.insert(0, root)
    spec = importlib.util.spec_from_file_location("graft_entry_ab", os.path.join(root, "__graft_entry__.py"))
    graft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(graft)
    from tools import gen_model
    w2xc = graft.load_package()
    ms = w2xc._ModelSet.from_layers(gen_model.synth_layers(seed=gen_model.SEEDS["scale2.0x"]))
    res = {}

    def per_call(f, calls, sync=lambda: None):
        f(); sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        sync()
        return (time.perf_counter() - t0) / calls * 1e6

    if not gpu:
        banded = w2xc.make_opts(workspace_mb=64)
        res["plan_3840x2160_us"] = per_call(lambda: ms.plan_rows(3840, 2160), 5000)
        res["plan_3000x4000_64MiB_us"] = per_call(lambda: ms.plan_rows(3000, 4000, opts=banded), 5000)
        res["plan_64x64_us"] = per_call(lambda: ms.plan_rows(64, 64), 5000)
    else:
        import numpy as np
        import torch
        torch.cuda.set_device(0)
        st = torch.cuda.current_stream()
        o = w2xc.make_opts(device=0)
        d_in = torch.from_numpy(np.random.default_rng(1).random((64, 64), dtype=np.float32)).cuda()
        d_out = torch.empty_like(d_in)
        res["convert_device_64x64_us"] = per_call(lambda: ms.convert_device(d_in.data_ptr(), 256, 64, 64, d_out.data_ptr(), 256, stream=st.cuda_stream, opts=o),
                                                  2000, torch.cuda.synchronize)
        rgb = w2xc._ModelSet.from_layers(gen_model.synth_layers([3, 32, 32, 64, 64, 128, 128, 3], 7))
        img = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (64, 64, 3), dtype=np.uint8)).cuda()
        out = torch.empty((128, 128, 3), dtype=torch.uint8, device="cuda")
        res["image_rgb_u8_64x64_us"] = per_call(lambda: w2xc.process_image_rgb_u8_device(img.data_ptr(), 192, 64, 64, out.data_ptr(), 384, scale=rgb, iterations=1,
                                                                                         stream=st.cuda_stream, opts=o), 1000, torch.cuda.synchronize)
    print("CHAIN_AB " + json.dumps(res))


def run_side(root, gpu):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", root] + (["--gpu"] if gpu else [])
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("CHAIN_AB ")][-1][len("CHAIN_AB "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other"); ap.add_argument("--child"); ap.add_argument("--gpu", action="store_true"); ap.add_argument("--aa", action="store_true")
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.gpu)
    sides = {"other": os.path.abspath(a.other), "this": HERE}
    if a.aa:
        sides["other_again"] = sides["other"]
    runs = {s: {} for s in sides}
    for rnd in range(a.rounds):
        order = list(sides) if rnd % 2 == 0 else list(sides)[::-1]
        for s in order:
            for k, v in run_side(sides[s], a.gpu).items():
                runs[s].setdefault(k, []).append(round(v, 3))
    rep = {"rounds": a.rounds, "order": "alternating, reversed every round; one process per side and round", "sides": {}}
    for s, d in runs.items():
        rep["sides"][s] = {k: {"per_round": v, "median": statistics.median(v), "spread": round(max(v) - min(v), 3)} for k, v in d.items()}
    text = json.dumps(rep, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
