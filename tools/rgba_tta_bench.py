#!/usr/bin/env python
"""tools/rgba_tta_bench.py -- TTA for the RGBA image calls (w2xc_process_image_rgba_u8_batch_tta_device, w2xc_process_image_rgba_u8_up2x_batch_tta_device),
timed in ONE process on ONE device, the two sides of every comparison alternating window by window.  Three model kinds: Y models 1-32-32-64-64-128-128-1,
RGB models 3-32-32-64-64-128-128-3, the published upconv_7 topology 3-16-32-64-128-128-256-(head 3); fp32, default options, scale only, one x2 iteration,
the default bleed.  Inputs are resident RGBA images.

    python tools/rgba_tta_bench.py [--n 16] [--rounds 7] [--out profiles/rgba_tta_bench.json]

(a) the new call at n = 1 against the route it is defined by (include/w2xc_hip.h, the RGBA TTA calls), composed from calls that existed before:
    w2xc_bleed_rgba_u8_device, the 3-channel TTA call of the route on the bled image, and for alpha -- Y route -- torch for u8 / 255,
    w2xc_convert_batch_tta_device with the nearest-2x fold, torch for the rounding, -- RGB and head routes -- torch for the grey image (A, A, A) and the
    3-channel TTA call on it; torch for the merge.
(b) at 64^2 and 256^2: the new call at n images against n calls of it at n = 1.
Sizes 64^2, 256^2 and 1080 x 1920 source pixels.  The bytes of the two sides must be equal.  `ok` = the new side's median is not above the baseline's by more
than the baseline's spread (max - min over rounds).  A timed window is `reps` calls enqueued back to back and one synchronisation, reps chosen so that a
window is >= ~30 ms.  Reported: the median over rounds of ms per image, each side's spread, the ratio."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
Y_TOPO = [1, 32, 32, 64, 64, 128, 128, 1]
RGB_TOPO = [3, 32, 32, 64, 64, 128, 128, 3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="64x64,256x256,1080x1920")
    ap.add_argument("--kinds", default="y,rgb,head")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgba_tta_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as graft
    from tools import gen_model
    w2xc = graft.load_package()
    if not torch.cuda.is_available() or w2xc.device_count() < 1:
        raise SystemExit("rgba_tta_bench needs a HIP device (there is no CPU fallback to time)")
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream()
    s = st.cuda_stream
    o = w2xc.make_opts(device=0)
    n = a.n

    def window(f, reps):
        st.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        st.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    def compare(new, old, per):
        """alternating windows; ms per `per` units: (median new, spread new, median old, spread old, reps)"""
        new(), old()
        st.synchronize()
        reps = max(1, min(5000, int(30.0 / max(window(new, 3), 1e-4))))
        tn, to = [], []
        for _ in range(a.rounds):
            tn.append(window(new, reps) / per)
            to.append(window(old, reps) / per)
        return statistics.median(tn), max(tn) - min(tn), statistics.median(to), max(to) - min(to), reps

    head_layers = gen_model.synth_layers(gen_model.TOPOLOGY_UPCONV7, gen_model.SEEDS["upconv7"])
    head = gen_model.synth_head(gen_model.TOPOLOGY_UPCONV7[-1], 3, gen_model.SEEDS["upconv7"], True)
    make = {"y": lambda: w2xc._ModelSet.from_layers(gen_model.synth_layers(Y_TOPO, gen_model.SEEDS["scale2.0x"])),
            "rgb": lambda: w2xc._ModelSet.from_layers(gen_model.synth_layers(RGB_TOPO, 301)),
            "head": lambda: w2xc._ModelSet.from_layers(head_layers, head=head)}
    rows = []
    for kind in filter(None, a.kinds.split(",")):
        mb, ms = make[kind](), make[kind]()          # (a context each: each side keeps its own workspaces)
        rgba = w2xc.process_image_rgba_u8_up2x_batch_device if kind == "head" else w2xc.process_image_rgba_u8_batch_device
        for size in filter(None, a.sizes.split(",")):
            h, w = [int(v) for v in size.split("x")]
            H, W = 2 * h, 2 * w
            batch_too = h * w <= 256 * 256
            cnt = n if batch_too else 1
            host = np.random.default_rng(1000 * h + w).integers(0, 256, (cnt, h, w, 4)).astype(np.uint8)
            host[:, h // 4:h // 2, w // 4:w // 2, 3] = 0          # a transparent block, an opaque one, partial values elsewhere
            host[:, h // 2:, : w // 3, 3] = 255
            d_in = torch.from_numpy(host).cuda()
            d_b, d_s = (torch.zeros((cnt, H, W, 4), dtype=torch.uint8, device="cuda") for _ in range(2))
            bled = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
            colour, ares = (torch.empty((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
            a2 = torch.empty((H, W), dtype=torch.float32, device="cuda")
            P = ms.n_layers

            def call(dst, i0, k, m):
                rgba(k, d_in[i0].data_ptr(), h * w * 4, w * 4, w, h, dst[i0].data_ptr(), H * W * 4, W * 4, None, m, 1, 0.0, -1, stream=s, opts=o, tta=True)

            def new_one():
                call(d_b, 0, 1, mb)

            def composed_one():
                w2xc.bleed_rgba_u8_device(d_in[0].data_ptr(), w * 4, w, h, P, bled.data_ptr(), w * 3, stream=s)
                if kind == "y":
                    w2xc.process_image_u8_device(bled.data_ptr(), w * 3, w, h, colour.data_ptr(), W * 3, None, ms, 1, 0.0, stream=s, opts=o, tta=True)
                    a1 = (d_in[0, :, :, 3].to(torch.float32) * np.float32(1.0 / 255.0)).contiguous()
                    ms.convert_batch_tta_device(1, a1.data_ptr(), w * h * 4, w * 4, w, h, a2.data_ptr(), W * H * 4, W * 4, nn2x=True, stream=s, opts=o)
                    d_s[0, :, :, 3] = torch.clamp(torch.round(a2 * np.float32(255.0)), 0, 255).to(torch.uint8)
                else:
                    grey = d_in[0, :, :, 3:4].expand(h, w, 3).contiguous()
                    if kind == "head":
                        w2xc.process_image_rgb_u8_up2x_batch_device(1, bled.data_ptr(), 0, w * 3, w, h, colour.data_ptr(), 0, W * 3, None, ms, 1, 0.0, stream=s,
                                                                    opts=o, tta=True)
                        w2xc.process_image_rgb_u8_up2x_batch_device(1, grey.data_ptr(), 0, w * 3, w, h, ares.data_ptr(), 0, W * 3, None, ms, 1, 0.0, stream=s,
                                                                    opts=o, tta=True)
                    else:
                        w2xc.process_image_rgb_u8_device(bled.data_ptr(), w * 3, w, h, colour.data_ptr(), W * 3, None, ms, 1, 0.0, stream=s, opts=o, tta=True)
                        w2xc.process_image_rgb_u8_device(grey.data_ptr(), w * 3, w, h, ares.data_ptr(), W * 3, None, ms, 1, 0.0, stream=s, opts=o, tta=True)
                    d_s[0, :, :, 3] = ares[:, :, 1]
                d_s[0, :, :, :3] = colour

            def batch():
                call(d_b, 0, n, mb)

            def singles():
                for i in range(n):
                    call(d_s, i, 1, ms)

            parts = [("a", 1, new_one, composed_one, lambda: bool(torch.equal(d_b[0], d_s[0])))]
            if batch_too:
                parts.append(("b", n, batch, singles, lambda: bool(torch.equal(d_b, d_s))))
            for part, per, new, old, eq in parts:
                m_n, s_n, m_o, s_o, reps = compare(new, old, per)
                row = dict(part=part, kind=kind, size="%dx%d" % (h, w), n=per, reps=reps, new_ms=round(m_n, 4), new_spread_ms=round(s_n, 4),
                           baseline="composed route" if part == "a" else "%d calls at n = 1" % n, baseline_ms=round(m_o, 4), baseline_spread_ms=round(s_o, 4),
                           speedup=round(m_o / m_n, 3), equal=eq(), ok=bool(m_n <= m_o + s_o))
                rows.append(row)
                print(json.dumps(row), flush=True)
            del d_in, d_b, d_s, bled, colour, ares, a2
            for m in (mb, ms):
                m.trim()
    res = dict(tool="tools/rgba_tta_bench.py", device=torch.cuda.get_device_name(0), rounds=a.rounds, n=n,
               models="y: 1-32-32-64-64-128-128-1, seed %d; rgb: 3-32-32-64-64-128-128-3, seed 301; head: 3-16-32-64-128-128-256-(head 3), seed %d"
                      % (gen_model.SEEDS["scale2.0x"], gen_model.SEEDS["upconv7"]),
               options="fp32, default options, scale only, 1 iteration, default bleed passes, resident RGBA images, tta = 1",
               unit="ms per image: a window of `reps` calls + one synchronisation, / reps (/ n); median over rounds; spread = max - min",
               all_equal=all(r["equal"] for r in rows), all_ok=all(r["ok"] for r in rows), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
