#!/usr/bin/env python
"""tools/rgb_image_bench.py -- one uint8 image through an RGB model, x2, resident in HBM on both ends: w2xc_process_image_rgb_u8_ex_device against
the only route the library offered for such a model before it -- torch ops for uint8 -> float planes and the nearest-neighbour 2x, then
w2xc_convert_planes_device, then torch ops back to uint8 -- in ONE process on ONE device, the two routes alternating call by call.

    python tools/rgb_image_bench.py [--sizes 64x64,256x256,1080x1920] [--rounds 9] [--out profiles/rgb_image_bench.json]

Model: tools/gen_model.py's synthetic 3 -> 32 -> 32 -> 64 -> 64 -> 128 -> 128 -> 3 (seed 301), fp32, default options.  A timed window is `reps` calls
enqueued back to back on one stream and one synchronisation (reps chosen so that a window is >= ~50 ms); a round times one window of each route.
Reported per size (h x w of the SOURCE image): the median over rounds of ms per image for both routes, the spread (max - min over rounds) of each,
the ratio, and `ok` = the new entry point's median is not above the old route's by more than the old route's spread.  The two routes' bytes are
compared once per size (<= 1 LSB: the torch route multiplies by a rounded 1/255 and rounds like the library, but composes its own operations)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64x64,256x256,1080x1920")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgb_image_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as graft
    from tools import gen_model
    w2xc = graft.load_package()
    if not torch.cuda.is_available() or w2xc.device_count() < 1:
        raise SystemExit("rgb_image_bench needs a HIP device (there is no CPU fallback to time)")
    torch.cuda.set_device(0)
    planes = [3, 32, 32, 64, 64, 128, 128, 3]
    ms = w2xc._ModelSet.from_layers(gen_model.synth_layers(planes, 301))
    ms_old = w2xc._ModelSet.from_layers(gen_model.synth_layers(planes, 301))   # (a context of its own: each route keeps its workspaces)
    o = w2xc.make_opts(device=0)
    st = torch.cuda.current_stream()
    rows = []
    for size in a.sizes.split(","):
        h, w = [int(v) for v in size.split("x")]
        H, W = 2 * h, 2 * w
        img = torch.from_numpy(np.random.default_rng(h + w).integers(0, 256, (h, w, 3)).astype(np.uint8)).cuda()
        out_new = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        planes_out = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
        scale = torch.tensor(np.float32(1 / 255), device="cuda")
        old = {}

        def new_route():
            w2xc.process_image_rgb_u8_device(img.data_ptr(), w * 3, w, h, out_new.data_ptr(), W * 3, None, ms, 1, 0.0, stream=st.cuda_stream, opts=o)

        def old_route():
            x = img.permute(2, 0, 1).to(torch.float32) * scale                                     # uint8 -> three float planes
            up = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous()           # the 4x larger nearest-neighbour planes
            ms_old.convert_planes_device(3, up.data_ptr(), H * W * 4, W * 4, W, H, planes_out.data_ptr(), H * W * 4, W * 4, stream=st.cuda_stream, opts=o)
            old["out"] = (planes_out * 255.0).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()

        def window(f, reps):
            st.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            st.synchronize()
            return (time.perf_counter() - t0) * 1e3 / reps

        new_route(), old_route()   # warm-up: workspace growth, weight packing, torch's kernels
        st.synchronize()
        diff = (out_new.to(torch.int16) - old["out"].to(torch.int16)).abs()
        reps = max(3, min(200, int(50.0 / max(window(new_route, 3), 1e-3))))
        tn, to = [], []
        for _ in range(a.rounds):
            tn.append(window(new_route, reps))
            to.append(window(old_route, reps))
        m_new, m_old = statistics.median(tn), statistics.median(to)
        row = dict(size="%dx%d" % (h, w), out_mpix=round(H * W / 1e6, 4), reps=reps, new_ms=round(m_new, 4), new_spread_ms=round(max(tn) - min(tn), 4),
                   old_ms=round(m_old, 4), old_spread_ms=round(max(to) - min(to), 4), speedup=round(m_old / m_new, 3),
                   ok=bool(m_new <= m_old + (max(to) - min(to))), max_byte_diff=int(diff.max()), bytes_differing=float((diff != 0).float().mean()))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del img, out_new, planes_out
        old.clear()
        ms.trim(), ms_old.trim()
    res = dict(tool="tools/rgb_image_bench.py", device=torch.cuda.get_device_name(0), rounds=a.rounds,
               model="3-32-32-64-64-128-128-3, tools/gen_model.py seed 301, fp32, default options", iterations=1,
               new="w2xc_process_image_rgb_u8_ex_device", old="torch uint8 <-> float planes and nearest 2x around w2xc_convert_planes_device",
               unit="ms per image (a window of `reps` calls on one stream + one synchronisation, / reps); median over rounds",
               all_ok=all(r["ok"] for r in rows), rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
