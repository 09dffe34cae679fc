#!/usr/bin/env python
"""tools/yuv_frames_bench.py -- the YUV frame call (w2xc_process_frames_yuv_u8_device), timed in ONE process on ONE device, the two sides of every
comparison alternating window by window.  7-layer Y models 1-32-32-64-64-128-128-1, fp32, default options; resident 4:2:0 frames, planar, full range.

    python tools/yuv_frames_bench.py [--rounds 7] [--sizes 64x64,256x256,1080x1920] [--ns 1,8] [--out profiles/yuv_frames_bench.json]

(a) the new call on n frames against the route it is defined by, composed from public calls: w2xc_y8_to_plane_device, w2xc_convert_batch_device (nn2x = 0 for
    the noise pass, 1 for the scale pass), w2xc_plane_to_y8_device; for chroma torch u8 * (1 / 255), w2xc_resize2x_cubic_device per plane, torch
    clamp(round(255 v)) and the copy into the output planes.  Modes scale and noise_scale.  The bytes of the two sides must be equal.  `ok` = the new side's
    median is not above the composed route's by more than that route's spread (max - min over rounds).
(b) for context, no threshold: what a caller does today -- w2xc_process_image_u8_ex_device on an RGB image of the frame's size, per frame (the colour matrix
    both ways, chroma enlarged at luma resolution); building the RGB image from 4:2:0 planes and subsampling the result again are not in the figure.
(c) the chroma kernel alone (w2xc_chroma2x_u8_device on the U and V planes of one 1080 x 1920 4:2:0 frame): ms, and GB/s over the bytes it has to move --
    cw ch in, 4 cw ch out, two planes -- beside the 6.29 TB/s SURVEY.md measured for HBM.  (--chroma-launches N launches only that kernel, for a
    kernel trace: the window's figure holds the launch cost of a kernel of a few microseconds.)
A timed window is `reps` calls enqueued back to back and one synchronisation, reps chosen so that a window is >= ~30 ms.  Reported: the median over rounds
of ms per frame, each side's spread, the ratio."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
Y_TOPO = [1, 32, 32, 64, 64, 128, 128, 1]
HBM_TBPS = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="64x64,256x256,1080x1920")
    ap.add_argument("--ns", default="1,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_frames_bench.json"))
    ap.add_argument("--chroma-launches", type=int, default=0, help="only launch the chroma kernel of (c) this many times: the program of a kernel trace")
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as graft
    from tools import gen_model
    w2xc = graft.load_package()
    if not torch.cuda.is_available() or w2xc.device_count() < 1:
        raise SystemExit("yuv_frames_bench needs a HIP device (there is no CPU fallback to time)")
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream()
    s = st.cuda_stream
    o = w2xc.make_opts(device=0)
    lib = w2xc.lib()

    if a.chroma_launches:   # rocprofv3 --kernel-trace --stats -- python tools/yuv_frames_bench.py --chroma-launches 200: the kernel's own time
        cw, ch = w2xc.yuv_chroma_size(1920, 1080, w2xc.YUV_420)
        src = torch.randint(0, 256, (2, ch, cw), dtype=torch.uint8, device="cuda")
        dst = torch.zeros((2, 2 * ch, 2 * cw), dtype=torch.uint8, device="cuda")
        for _ in range(a.chroma_launches):
            w2xc.chroma2x_u8_device(src.data_ptr(), 2, cw * ch, cw, 1, cw, ch, dst.data_ptr(), 4 * cw * ch, 2 * cw, 1, 2 * cw, 2 * ch, stream=s)
        st.synchronize()
        return

    def window(f, reps):
        st.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        st.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    def reps_for(f):
        f()
        st.synchronize()
        return max(1, min(5000, int(30.0 / max(window(f, 3), 1e-4))))

    def compare(new, old, per):
        """alternating windows; ms per `per` units: (median new, spread new, median old, spread old, reps)"""
        old()
        reps = reps_for(new)
        tn, to = [], []
        for _ in range(a.rounds):
            tn.append(window(new, reps) / per)
            to.append(window(old, reps) / per)
        return statistics.median(tn), max(tn) - min(tn), statistics.median(to), max(to) - min(to), reps

    def one(f, per):
        reps = reps_for(f)
        t = [window(f, reps) / per for _ in range(a.rounds)]
        return statistics.median(t), max(t) - min(t), reps

    def planes(d_y, d_u, d_v, w, h, cw, ch):
        p = w2xc.YuvPlanes()
        p.y, p.y_stride, p.y_frame_stride = d_y.data_ptr(), w, w * h
        p.u, p.v, p.c_stride, p.c_frame_stride, p.c_px = d_u.data_ptr(), d_v.data_ptr(), cw, cw * ch, 1
        return p

    mk = lambda seed: w2xc._ModelSet.from_layers(gen_model.synth_layers(Y_TOPO, seed))
    # (a context per side: each side keeps its own workspaces)
    new_m = {"noise": mk(gen_model.SEEDS["noise1"]), "scale": mk(gen_model.SEEDS["scale2.0x"])}
    old_m = {"noise": mk(gen_model.SEEDS["noise1"]), "scale": mk(gen_model.SEEDS["scale2.0x"])}
    rgb_m = {"noise": mk(gen_model.SEEDS["noise1"]), "scale": mk(gen_model.SEEDS["scale2.0x"])}
    rows, detour = [], []
    for size in filter(None, a.sizes.split(",")):
        h, w = [int(v) for v in size.split("x")]
        H, W = 2 * h, 2 * w
        cw, ch = w2xc.yuv_chroma_size(w, h, w2xc.YUV_420)
        ocw, och = w2xc.yuv_chroma_size(W, H, w2xc.YUV_420)
        for n in [int(v) for v in a.ns.split(",")]:
            rng = np.random.default_rng(1000 * h + w + n)
            d_y = torch.from_numpy(rng.integers(0, 256, (n, h, w), dtype=np.uint8)).cuda()
            d_u, d_v = (torch.from_numpy(rng.integers(0, 256, (n, ch, cw), dtype=np.uint8)).cuda() for _ in range(2))
            out_new = [torch.zeros((n, H, W), dtype=torch.uint8, device="cuda")] + [torch.zeros((n, och, ocw), dtype=torch.uint8, device="cuda") for _ in range(2)]
            out_old = [torch.zeros_like(t) for t in out_new]
            pi, po = planes(d_y, d_u, d_v, w, h, cw, ch), planes(*out_new, W, H, ocw, och)
            f0, f1 = (torch.empty((n, h, w), dtype=torch.float32, device="cuda") for _ in range(2))
            f2 = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
            up = torch.empty((2 * ch, 2 * cw), dtype=torch.float32, device="cuda")
            for mode in ("scale", "noise_scale"):
                noise_n, noise_o = (new_m["noise"], old_m["noise"]) if mode == "noise_scale" else (None, None)

                def new():
                    w2xc.process_frames_yuv_u8_device(n, w, h, w2xc.YUV_420, pi, po, noise_n, new_m["scale"], 1, w2xc.RANGE_FULL, stream=s, opts=o)

                def old():
                    w2xc.y8_to_plane_device(d_y.data_ptr(), n, w * h, w, w, h, w2xc.RANGE_FULL, f0.data_ptr(), 4 * w * h, stream=s)
                    src = f0
                    if noise_o is not None:
                        noise_o.convert_batch_device(n, f0.data_ptr(), 4 * w * h, 4 * w, w, h, f1.data_ptr(), 4 * w * h, 4 * w, nn2x=False, stream=s, opts=o)
                        src = f1
                    old_m["scale"].convert_batch_device(n, src.data_ptr(), 4 * w * h, 4 * w, w, h, f2.data_ptr(), 4 * W * H, 4 * W, nn2x=True, stream=s, opts=o)
                    w2xc.plane_to_y8_device(f2.data_ptr(), n, 4 * W * H, W, H, w2xc.RANGE_FULL, out_old[0].data_ptr(), W * H, W, stream=s)
                    for d_c, d_o in ((d_u, out_old[1]), (d_v, out_old[2])):
                        c = d_c.to(torch.float32) * float(np.float32(1.0 / 255.0))
                        for i in range(n):
                            lib.w2xc_resize2x_cubic_device(c[i].data_ptr(), cw, ch, up.data_ptr(), s)
                            d_o[i].copy_(torch.clamp(torch.round(up * 255.0), 0, 255)[:och, :ocw])

                new(), old()
                st.synchronize()
                equal = all(torch.equal(x, y) for x, y in zip(out_new, out_old))
                if not equal:
                    raise SystemExit("%s %s n=%d: the new call and the composed route differ" % (size, mode, n))
                tn, sn, to, so, reps = compare(new, old, n)
                rows.append({"size": size, "mode": mode, "n": n, "new_ms_per_frame": round(tn, 5), "new_spread": round(sn, 5), "composed_ms_per_frame": round(to, 5),
                             "composed_spread": round(so, 5), "ratio_composed_over_new": round(to / tn, 3), "reps": reps, "bytes_equal": equal,
                             "ok": bool(tn <= to + so)})
                print(json.dumps(rows[-1]), flush=True)
            # (b) the detour through an RGB image, per frame, for context
            rgb = torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
            rgb_out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            if n == 1:
                for mode in ("scale", "noise_scale"):
                    def rgb_call():
                        w2xc.process_image_u8_device(rgb.data_ptr(), 3 * w, w, h, rgb_out.data_ptr(), 3 * W, noise=rgb_m["noise"] if mode == "noise_scale" else None,
                                                     scale=rgb_m["scale"], iterations=1, stream=s, opts=o)
                    t, sp, reps = one(rgb_call, 1)
                    detour.append({"size": size, "mode": mode, "rgb_image_call_ms_per_frame": round(t, 5), "spread": round(sp, 5), "reps": reps})
                    print(json.dumps(detour[-1]), flush=True)
    # (c) the chroma kernel alone: U and V of one 1080 x 1920 4:2:0 frame, as two planes of one launch
    h, w = 1080, 1920
    cw, ch = w2xc.yuv_chroma_size(w, h, w2xc.YUV_420)
    src = torch.randint(0, 256, (2, ch, cw), dtype=torch.uint8, device="cuda")
    dst = torch.zeros((2, 2 * ch, 2 * cw), dtype=torch.uint8, device="cuda")
    chroma = lambda: w2xc.chroma2x_u8_device(src.data_ptr(), 2, cw * ch, cw, 1, cw, ch, dst.data_ptr(), 4 * cw * ch, 2 * cw, 1, 2 * cw, 2 * ch, stream=s)
    t, sp, reps = one(chroma, 1)
    moved = 2 * (cw * ch + 4 * cw * ch)
    kernel = {"planes": "2 x %dx%d -> 2 x %dx%d" % (cw, ch, 2 * cw, 2 * ch), "ms": round(t, 5), "spread": round(sp, 5), "reps": reps, "bytes_moved": moved,
              "GBps": round(moved / (t * 1e-3) / 1e9, 1), "hbm_measured_GBps_SURVEY": HBM_TBPS * 1e3,
              "note": "a window is back-to-back launches: the figure holds the launch cost of a %.0f us kernel" % (t * 1e3)}
    print(json.dumps(kernel), flush=True)
    res = {"tool": "tools/yuv_frames_bench.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "frames_vs_composed": rows, "rgb_detour_context": detour,
           "chroma_kernel_1080p": kernel, "all_ok": all(r["ok"] for r in rows)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("all_ok", res["all_ok"])


if __name__ == "__main__":
    main()
