#!/usr/bin/env python
"""tools/rgba_image_bench.py -- one uint8 RGBA image through a scale model, x2, resident in HBM on both ends: w2xc_process_image_rgba_u8_ex_device against
what a caller who wanted to keep alpha had before it -- a torch split, the 3-channel call on the colour, w2xc_convert_plane_nn2x_device on alpha / 255 (Y
models) or the RGB call on the grey image (A, A, A) (RGB models), then a torch round and merge -- in ONE process on ONE device, the two routes alternating
call by call, for both model kinds.

    python tools/rgba_image_bench.py [--sizes 64x64,256x256,1080x1920] [--kinds y,rgb] [--rounds 9] [--out profiles/rgba_image_bench.json]

Models: tools/gen_model.py's synthetic 1 -> 32 -> 32 -> 64 -> 64 -> 128 -> 128 -> 1 (the scale2.0x seed) and 3 -> ... -> 3 (seed 301), fp32, default options,
bleed_passes = -1 (7 passes).  The image's alpha bytes are random in 1..255: the bleed runs all its passes (no step depends on the data) and changes nothing,
so that the two routes' bytes can be compared -- `identical` per row.  A timed window is `reps` calls enqueued back to back on one stream and one
synchronisation (reps chosen so that a window is >= ~50 ms); a round times one window of each route.  Reported per kind and size (h x w of the SOURCE image):
the median over rounds of ms per image for both routes, the spread (max - min over rounds) of each, the ratio, and `ok` = the new entry point's median is not
above the composed route's by more than the composed route's spread."""
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
    ap.add_argument("--kinds", default="y,rgb")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgba_image_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as graft
    from tools import gen_model
    w2xc = graft.load_package()
    if not torch.cuda.is_available() or w2xc.device_count() < 1:
        raise SystemExit("rgba_image_bench needs a HIP device (there is no CPU fallback to time)")
    torch.cuda.set_device(0)
    topo = {"y": ([1, 32, 32, 64, 64, 128, 128, 1], gen_model.SEEDS["scale2.0x"]), "rgb": ([3, 32, 32, 64, 64, 128, 128, 3], 301)}
    o = w2xc.make_opts(device=0)
    st = torch.cuda.current_stream()
    rows = []
    for kind in a.kinds.split(","):
        ms = w2xc._ModelSet.from_layers(gen_model.synth_layers(*topo[kind]))
        ms_old = w2xc._ModelSet.from_layers(gen_model.synth_layers(*topo[kind]))   # (a context of its own: each route keeps its workspaces)
        for size in a.sizes.split(","):
            h, w = [int(v) for v in size.split("x")]
            H, W = 2 * h, 2 * w
            host = np.random.default_rng(h + w).integers(0, 256, (h, w, 4)).astype(np.uint8)
            host[:, :, 3] = np.maximum(host[:, :, 3], 1)
            img = torch.from_numpy(host).cuda()
            out_new = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
            out3 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            grey_out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            plane_out = torch.empty((H, W), dtype=torch.float32, device="cuda")
            scale = torch.tensor(np.float32(1 / 255), device="cuda")
            old = {}

            def new_route():
                w2xc.process_image_rgba_u8_device(img.data_ptr(), w * 4, w, h, out_new.data_ptr(), W * 4, None, ms, 1, 0.0, -1, stream=st.cuda_stream, opts=o)

            def old_route():
                rgb = img[:, :, :3].contiguous()                                                        # the split
                if kind == "y":
                    ms_old.scale2x_image_u8_device(rgb.data_ptr(), w * 3, w, h, out3.data_ptr(), W * 3, 1, stream=st.cuda_stream, opts=o)
                    al = img[:, :, 3].to(torch.float32) * scale
                    ms_old.convert_nn2x_device(al.data_ptr(), w * 4, w, h, plane_out.data_ptr(), W * 4, stream=st.cuda_stream, opts=o)
                    a8 = (plane_out * 255.0).round().clamp(0, 255).to(torch.uint8).unsqueeze(2)       # the round
                else:
                    w2xc.process_image_rgb_u8_device(rgb.data_ptr(), w * 3, w, h, out3.data_ptr(), W * 3, None, ms_old, 1, 0.0, stream=st.cuda_stream, opts=o)
                    grey = img[:, :, 3:].expand(h, w, 3).contiguous()
                    w2xc.process_image_rgb_u8_device(grey.data_ptr(), w * 3, w, h, grey_out.data_ptr(), W * 3, None, ms_old, 1, 0.0, stream=st.cuda_stream, opts=o)
                    a8 = grey_out[:, :, 1:2]
                old["out"] = torch.cat([out3, a8], dim=2)                                               # the merge

            def window(f, reps):
                st.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    f()
                st.synchronize()
                return (time.perf_counter() - t0) * 1e3 / reps

            new_route(), old_route()   # warm-up: workspace growth, weight packing, torch's kernels
            st.synchronize()
            identical = bool(torch.equal(out_new, old["out"]))
            reps = max(3, min(200, int(50.0 / max(window(new_route, 3), 1e-3))))
            tn, to = [], []
            for _ in range(a.rounds):
                tn.append(window(new_route, reps))
                to.append(window(old_route, reps))
            m_new, m_old = statistics.median(tn), statistics.median(to)
            row = dict(kind=kind, size="%dx%d" % (h, w), out_mpix=round(H * W / 1e6, 4), reps=reps, new_ms=round(m_new, 4),
                       new_spread_ms=round(max(tn) - min(tn), 4), old_ms=round(m_old, 4), old_spread_ms=round(max(to) - min(to), 4),
                       speedup=round(m_old / m_new, 3), ok=bool(m_new <= m_old + (max(to) - min(to))), identical=identical)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del img, out_new, out3, grey_out, plane_out
            old.clear()
            ms.trim(), ms_old.trim()
    res = dict(tool="tools/rgba_image_bench.py", device=torch.cuda.get_device_name(0), rounds=a.rounds,
               models="y: 1-32-32-64-64-128-128-1 (tools/gen_model.py, the scale2.0x seed); rgb: 3-32-32-64-64-128-128-3 (seed 301); fp32, default options",
               iterations=1, bleed_passes=-1, new="w2xc_process_image_rgba_u8_ex_device",
               old="torch split, the 3-channel call, w2xc_convert_plane_nn2x_device on alpha (y) / the RGB call on (A, A, A) (rgb), torch round and merge",
               unit="ms per image (a window of `reps` calls on one stream + one synchronisation, / reps); median over rounds",
               all_ok=all(r["ok"] for r in rows), all_identical=all(r["identical"] for r in rows), rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
