#!/usr/bin/env python
"""tools/tta_bench.py -- test-time augmentation of one uint8 image, x2, resident in HBM on both ends, for a Y model and for an RGB model: the TTA call
(w2xc_process_image_u8_tta_device / w2xc_process_image_rgb_u8_tta_device, tta = 1) against
  (a) the route a caller composed before it: the colour building blocks, torch flips / transposes of the float planes, 8 calls of
      w2xc_convert_plane_nn2x_device (Y) / w2xc_convert_planes_nn2x_device (RGB), torch flips back, the torch fp32 sum in the order of the header, the
      building blocks back to uint8 -- its bytes must equal the TTA call's;
  (b) 8 calls of the image call without TTA (what TTA costs in CNN work, without the variants' traffic),
in ONE process on ONE device, the three routes alternating window by window.

    python tools/tta_bench.py [--sizes 64x64,256x256,1080x1920] [--rounds 7] [--out profiles/tta_bench.json]

Models: tools/gen_model.py's synthetic scale2.0x Y model (1 -> 32 -> 32 -> 64 -> 64 -> 128 -> 128 -> 1) and the RGB model of rgb_image_bench.py
(3 -> ... -> 3, seed 301), fp32, default options.  A timed window is `reps` calls enqueued back to back on one stream and one synchronisation (reps chosen
so that a window is >= ~50 ms); a round times one window of each route.  Reported per model and size (h x w of the SOURCE image): the median over rounds
of ms per image, the spread (max - min over rounds) of each route, the ratios, `equal` = the bytes of (a) are those of the TTA call, and `ok` = the TTA
call's median is not above (a)'s by more than (a)'s spread."""
import argparse
import ctypes as C
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as graft
    from tools import gen_model
    w2xc = graft.load_package()
    if not torch.cuda.is_available() or w2xc.device_count() < 1:
        raise SystemExit("tta_bench needs a HIP device (there is no CPU fallback to time)")
    torch.cuda.set_device(0)
    lib = w2xc.lib()
    kinds = {"y": gen_model.synth_layers(seed=gen_model.SEEDS["scale2.0x"]), "rgb": gen_model.synth_layers([3, 32, 32, 64, 64, 128, 128, 3], 301)}
    o = w2xc.make_opts(device=0)
    st = torch.cuda.current_stream()
    s = st.cuda_stream
    eighth = torch.tensor(np.float32(0.125), device="cuda")

    def T(k, x):      # on (..., h, w) tensors; contiguous results
        if k & 1:
            x = x.flip(-1)
        if k & 2:
            x = x.flip(-2)
        if k & 4:
            x = x.transpose(-1, -2)
        return x.contiguous()

    def Tinv(k, x):
        if k & 4:
            x = x.transpose(-1, -2)
        if k & 2:
            x = x.flip(-2)
        if k & 1:
            x = x.flip(-1)
        return x

    def mean8(vs):
        acc = vs[0] + vs[1]
        for v in vs[2:]:
            acc = acc + v
        return (acc * eighth).contiguous()

    rows = []
    for kind, layers in kinds.items():
        rgb = kind == "rgb"
        ms, ms_a, ms_b = (w2xc._ModelSet.from_layers(layers) for _ in range(3))   # (a context each: every route keeps its own workspaces)
        call = w2xc.process_image_rgb_u8_device if rgb else w2xc.process_image_u8_device
        for size in a.sizes.split(","):
            h, w = [int(v) for v in size.split("x")]
            H, W = 2 * h, 2 * w
            img = torch.from_numpy(np.random.default_rng(h + w).integers(0, 256, (h, w, 3)).astype(np.uint8)).cuda()
            out_tta, out_a, out_b = (torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(3))
            pl = torch.empty((3, h, w), dtype=torch.float32, device="cuda")
            uv2 = torch.empty((2, H, W), dtype=torch.float32, device="cuda")

            def tta_route():
                call(img.data_ptr(), w * 3, w, h, out_tta.data_ptr(), W * 3, None, ms, 1, 0.0, stream=s, opts=o, tta=True)

            def composed_route():
                if rgb:
                    w2xc.u8_to_rgb_device(img.data_ptr(), w * 3, w, h, pl.data_ptr(), stream=s)
                    vs = []
                    for k in range(8):
                        x = T(k, pl)
                        r = torch.empty((3, 2 * x.shape[1], 2 * x.shape[2]), dtype=torch.float32, device="cuda")
                        ms_a.convert_planes_nn2x_device(3, x.data_ptr(), h * w * 4, x.shape[2] * 4, x.shape[2], x.shape[1], r.data_ptr(), H * W * 4,
                                                        2 * x.shape[2] * 4, stream=s, opts=o)
                        vs.append(Tinv(k, r))
                    res = mean8(vs)
                    w2xc.rgb_to_u8_device(res.data_ptr(), W, H, out_a.data_ptr(), W * 3, stream=s)
                else:
                    lib.w2xc_u8_to_yuv_device(C.c_void_p(img.data_ptr()), w * 3, w, h, C.c_void_p(pl[0].data_ptr()), C.c_void_p(pl[1].data_ptr()),
                                              C.c_void_p(pl[2].data_ptr()), C.c_void_p(s))
                    vs = []
                    for k in range(8):
                        x = T(k, pl[0])
                        r = torch.empty((2 * x.shape[0], 2 * x.shape[1]), dtype=torch.float32, device="cuda")
                        ms_a.convert_nn2x_device(x.data_ptr(), x.shape[1] * 4, x.shape[1], x.shape[0], r.data_ptr(), 2 * x.shape[1] * 4, stream=s, opts=o)
                        vs.append(Tinv(k, r))
                    y2 = mean8(vs)
                    for c in (0, 1):
                        lib.w2xc_resize2x_cubic_device(C.c_void_p(pl[1 + c].data_ptr()), w, h, C.c_void_p(uv2[c].data_ptr()), C.c_void_p(s))
                    lib.w2xc_yuv_to_u8_device(C.c_void_p(y2.data_ptr()), C.c_void_p(uv2[0].data_ptr()), C.c_void_p(uv2[1].data_ptr()), W, H,
                                              C.c_void_p(out_a.data_ptr()), W * 3, C.c_void_p(s))

            def eight_plain_route():
                for _ in range(8):
                    call(img.data_ptr(), w * 3, w, h, out_b.data_ptr(), W * 3, None, ms_b, 1, 0.0, stream=s, opts=o)

            def window(f, reps):
                st.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    f()
                st.synchronize()
                return (time.perf_counter() - t0) * 1e3 / reps

            tta_route(), composed_route(), eight_plain_route()   # warm-up: workspace growth, weight packing, torch's kernels
            st.synchronize()
            equal = bool(torch.equal(out_tta, out_a))
            reps = max(2, min(200, int(50.0 / max(window(tta_route, 2), 1e-3))))
            tt, ta, tb = [], [], []
            for _ in range(a.rounds):
                tt.append(window(tta_route, reps))
                ta.append(window(composed_route, reps))
                tb.append(window(eight_plain_route, reps))
            m_t, m_a, m_b = statistics.median(tt), statistics.median(ta), statistics.median(tb)
            row = dict(model=kind, size="%dx%d" % (h, w), out_mpix=round(H * W / 1e6, 4), reps=reps, tta_ms=round(m_t, 4),
                       tta_spread_ms=round(max(tt) - min(tt), 4), composed_ms=round(m_a, 4), composed_spread_ms=round(max(ta) - min(ta), 4),
                       eight_plain_ms=round(m_b, 4), eight_plain_spread_ms=round(max(tb) - min(tb), 4), speedup_vs_composed=round(m_a / m_t, 3),
                       ratio_to_eight_plain=round(m_t / m_b, 3), equal=equal, ok=bool(m_t <= m_a + (max(ta) - min(ta))))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del img, out_tta, out_a, out_b, pl, uv2
            ms.trim(), ms_a.trim(), ms_b.trim()
    res = dict(tool="tools/tta_bench.py", device=torch.cuda.get_device_name(0), rounds=a.rounds,
               models=dict(y="1-32-32-64-64-128-128-1, tools/gen_model.py scale2.0x seed", rgb="3-32-32-64-64-128-128-3, seed 301"),
               options="fp32, default options", iterations=1,
               tta="w2xc_process_image_[rgb_]u8_tta_device, tta = 1",
               composed="building blocks + torch flips + 8 x w2xc_convert_plane[s]_nn2x_device + torch fp32 sum",
               eight_plain="8 x w2xc_process_image_[rgb_]u8_ex_device",
               unit="ms per image (a window of `reps` calls on one stream + one synchronisation, / reps); median over rounds",
               all_equal=all(r["equal"] for r in rows), all_ok=all(r["ok"] for r in rows), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
