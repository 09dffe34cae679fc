#!/usr/bin/env python
"""tools/upconv_bench.py -- one uint8 image through an upconv head model (upstream's upconv_7 topology, 3-16-32-64-128-128-256 and a 4x4 stride-2
transposed-convolution head 256 -> 3), x2, resident in HBM on both ends, in ONE process on ONE device, the routes alternating call by call:

  (a) new      w2xc_process_image_rgb_u8_ex_device with the head model as scale model
  (b) composed the route a caller can put together without head models: torch uint8 -> float planes and replicate pad by 1, w2xc_convert_planes_device on
               the six 3x3 layers as a model of their own (its 16- and 256-plane layers have no fast kernel there: conv3x3_direct), torch conv_transpose2d
               on the device, torch uint8 conversion
  (c) vgg7     for context: w2xc_process_image_rgb_u8_ex_device with the RGB vgg_7 scale model 3-32-32-64-64-128-128-3 at the same sizes

    python tools/upconv_bench.py [--sizes 64x64,256x256,1080x1920] [--rounds 7] [--out profiles/upconv_bench.json]

A timed window is `reps` calls enqueued back to back on one stream and one synchronisation (reps chosen so that a window of (a) is >= ~50 ms); a round
times one window of each route.  Reported per size (h x w of the SOURCE image): the median over rounds of ms per image for every route and each route's
spread (max - min over rounds), `ok` = (a)'s median is not above (b)'s by more than (b)'s spread, the largest difference of (a)'s bytes from (b)'s in
uint8 steps (not expected to be 0: (b)'s narrow and wide layers run another kernel), the per-layer ms of (a)'s model from the profile hooks
(w2xc_opts.profile, one call) and the head's achieved GB/s against the 4 C bytes per z pixel it has to read."""
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upconv_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    import __graft_entry__ as graft
    from tools import gen_model
    w2xc = graft.load_package()
    if not torch.cuda.is_available() or w2xc.device_count() < 1:
        raise SystemExit("upconv_bench needs a HIP device (there is no CPU fallback to time)")
    torch.cuda.set_device(0)
    seed = gen_model.SEEDS["upconv7"]
    layers = gen_model.synth_layers(gen_model.TOPOLOGY_UPCONV7, seed)
    hw, hb = gen_model.synth_head(gen_model.TOPOLOGY_UPCONV7[-1], 3, seed)
    ms = w2xc._ModelSet.from_layers(layers, head=(hw, hb))
    ms_prof = w2xc._ModelSet.from_layers(layers, head=(hw, hb))   # (the profiled call: a context of its own)
    ms_chain = w2xc._ModelSet.from_layers(layers)                 # route (b): the 3x3 layers alone
    ms_vgg = w2xc._ModelSet.from_layers(gen_model.synth_layers([3, 32, 32, 64, 64, 128, 128, 3], 301))
    d_hw = torch.from_numpy(hw).cuda()
    d_hb = torch.from_numpy(hb.astype(np.float32)).cuda()
    o = w2xc.make_opts(device=0)
    st = torch.cuda.current_stream()
    names = [ms.kernel_name(l) for l in range(ms.n_layers)]
    rows = []
    for size in a.sizes.split(","):
        h, w = [int(v) for v in size.split("x")]
        H, W = 2 * h, 2 * w
        img = torch.from_numpy(np.random.default_rng(h + w).integers(0, 256, (h, w, 3)).astype(np.uint8)).cuda()
        out_new = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        out_vgg = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        z = torch.empty((256, h + 2, w + 2), dtype=torch.float32, device="cuda")
        scale = torch.tensor(np.float32(1 / 255), device="cuda")
        old = {}

        def new_route():
            w2xc.process_image_rgb_u8_device(img.data_ptr(), w * 3, w, h, out_new.data_ptr(), W * 3, None, ms, 1, 0.0, stream=st.cuda_stream, opts=o)

        def composed_route():
            x = F.pad((img.permute(2, 0, 1).to(torch.float32) * scale)[None], (1, 1, 1, 1), mode="replicate")[0].contiguous()
            ms_chain.convert_planes_device(3, x.data_ptr(), (h + 2) * (w + 2) * 4, (w + 2) * 4, w + 2, h + 2, z.data_ptr(), (h + 2) * (w + 2) * 4, (w + 2) * 4,
                                           stream=st.cuda_stream, opts=o)
            y = F.conv_transpose2d(z[None], d_hw, d_hb, stride=2, padding=3)[0]
            old["out"] = (y * 255.0).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()

        def vgg_route():
            w2xc.process_image_rgb_u8_device(img.data_ptr(), w * 3, w, h, out_vgg.data_ptr(), W * 3, None, ms_vgg, 1, 0.0, stream=st.cuda_stream, opts=o)

        def window(f, reps):
            st.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            st.synchronize()
            return (time.perf_counter() - t0) * 1e3 / reps

        new_route(), composed_route(), vgg_route()   # warm-up: workspace growth, weight packing, torch's kernels
        st.synchronize()
        assert tuple(old["out"].shape) == (H, W, 3)
        diff = (out_new.to(torch.int16) - old["out"].to(torch.int16)).abs()
        reps = max(3, min(200, int(50.0 / max(window(new_route, 3), 1e-3))))
        reps_old = max(2, min(reps, int(100.0 / max(window(composed_route, 2), 1e-3))))   # (the composed route is slow at the large size)
        tn, to, tv = [], [], []
        for _ in range(a.rounds):
            tn.append(window(new_route, reps))
            to.append(window(composed_route, reps_old))
            tv.append(window(vgg_route, reps))
        # per-layer ms of one profiled plane call (float planes in and out: the head kernel's float form)
        po = w2xc.make_opts(device=0, profile=1)
        x = (img.permute(2, 0, 1).to(torch.float32) * scale).contiguous()
        y = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
        layer_ms = None
        for k in range(3):   # (the last of three: warm)
            ms_prof.profile_reset(0)
            ms_prof.convert_planes_up2x_device(3, x.data_ptr(), h * w * 4, w * 4, w, h, y.data_ptr(), H * W * 4, W * 4, stream=st.cuda_stream, opts=po)
            st.synchronize()
            layer_ms = ms_prof.profile_read(0)[0]
        head_ms = layer_ms[-1]
        m_new, m_old, m_vgg = statistics.median(tn), statistics.median(to), statistics.median(tv)
        row = dict(size="%dx%d" % (h, w), out_mpix=round(H * W / 1e6, 4), reps=reps, reps_composed=reps_old,
                   new_ms=round(m_new, 4), new_spread_ms=round(max(tn) - min(tn), 4),
                   composed_ms=round(m_old, 4), composed_spread_ms=round(max(to) - min(to), 4),
                   vgg7_ms=round(m_vgg, 4), vgg7_spread_ms=round(max(tv) - min(tv), 4),
                   speedup_over_composed=round(m_old / m_new, 3), ok=bool(m_new <= m_old + (max(to) - min(to))),
                   max_byte_diff_vs_composed=int(diff.max()), bytes_differing=float((diff != 0).float().mean()),
                   layer_ms=[round(v, 4) for v in layer_ms],
                   head_gbs=round(4.0 * 256 * (h + 2) * (w + 2) / (head_ms * 1e-3) / 1e9, 1) if head_ms > 0 else None)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del img, out_new, out_vgg, z, x, y
        old.clear()
        for m in (ms, ms_prof, ms_chain, ms_vgg):
            m.trim()
        torch.cuda.empty_cache()
    res = dict(tool="tools/upconv_bench.py", device=torch.cuda.get_device_name(0), rounds=a.rounds,
               model="3-16-32-64-128-128-256 + head 256->3, tools/gen_model.py seed %d, fp32, default options" % seed, kernels=names, iterations=1,
               new="w2xc_process_image_rgb_u8_ex_device, the head model as scale model",
               composed="torch uint8 -> float planes + replicate pad 1, w2xc_convert_planes_device on the six 3x3 layers, torch conv_transpose2d, torch -> uint8",
               vgg7="w2xc_process_image_rgb_u8_ex_device, RGB vgg_7 scale model 3-32-32-64-64-128-128-3 (seed 301)",
               unit="ms per image (a window of `reps` calls on one stream + one synchronisation, / reps); median over rounds; layer_ms: one profiled "
                    "w2xc_convert_planes_up2x_device call (event pairs around every launch), head_gbs = 4 * 256 * (h + 2) * (w + 2) bytes / the head's ms",
               all_ok=all(r["ok"] for r in rows), rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
