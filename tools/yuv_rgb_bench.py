#!/usr/bin/env python
"""tools/yuv_rgb_bench.py -- YUV frames through RGB models (w2xc_process_frames_yuv_u8_rgb_device), timed in ONE process on ONE device, the two sides of every
comparison alternating window by window.  fp32, default options; resident planar 4:2:0 frames, limited range, BT.709.  Models: the 7-layer three-plane chain
3-32-32-64-64-128-128-3 (scale mode) and the published upconv_7 topology with random weights (its own 2x).

    python tools/yuv_rgb_bench.py [--rounds 7] [--sizes 64x64,256x256,1080x1920] [--ns 1,8] [--out profiles/yuv_rgb_bench.json]

(a) the new call on n frames against the route it is defined by, composed from public calls: w2xc_yuv8_to_rgb_device, w2xc_convert_planes_batch_device with
    nn2x = 1 (or w2xc_convert_planes_up2x_batch_device for the head model), w2xc_rgb_to_yuv8_device.  The bytes of the two sides must be equal.  `ok` = the new
    side's median is not above the composed route's by more than that route's spread (max - min over rounds).
(b) for context, no threshold: w2xc_process_image_rgb_u8_ex_device on an RGB image of the frame's size, per frame (uint8-fused first and last layers, no colour
    matrix; building the RGB image from 4:2:0 planes and subsampling the result again are not in the figure).
(c) the two new kernels alone on 1080 x 1920 4:2:0 frames: us, and GB/s over the bytes they have to move -- 1.5 w h bytes and 12 w h bytes of floats -- in two
    forms: "rotating", every launch on the next of ROTATE sets of buffers, 336 MB in all and so more than the 256 MiB of Infinity Cache, beside the 6.29 TB/s
    SURVEY.md measured for HBM; and "resident", every launch on the same 28 MB, which stay in that cache: not an HBM rate.  (A window is back-to-back launches:
    both figures hold the launch cost.)
A timed window is `reps` calls enqueued back to back and one synchronisation, reps chosen so that a window is >= ~100 ms.  Reported: the median over rounds
of ms per frame, each side's spread, the ratio."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RGB_TOPO = [3, 32, 32, 64, 64, 128, 128, 3]
HBM_TBPS = 6.29
ROTATE = 12   # buffer sets of the kernels-alone figure: 12 x 28 MB is more than the 256 MiB Infinity Cache


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="64x64,256x256,1080x1920")
    ap.add_argument("--ns", default="1,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_rgb_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as graft
    from tools import gen_model
    w2xc = graft.load_package()
    if not torch.cuda.is_available() or w2xc.device_count() < 1:
        raise SystemExit("yuv_rgb_bench needs a HIP device (there is no CPU fallback to time)")
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream()
    s = st.cuda_stream
    o = w2xc.make_opts(device=0)
    LAY, RNG, MAT = w2xc.YUV_420, w2xc.RANGE_LIMITED, w2xc.MATRIX_BT709

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
        return max(1, min(20000, int(100.0 / max(window(f, 3), 1e-4))))

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

    def rgb7():
        return w2xc._ModelSet.from_layers(gen_model.synth_layers(RGB_TOPO, 301))

    def upconv7():
        return w2xc._ModelSet.from_layers(gen_model.synth_layers(gen_model.TOPOLOGY_UPCONV7, gen_model.SEEDS["upconv7"]),
                                          head=gen_model.synth_head(gen_model.TOPOLOGY_UPCONV7[-1], 3, gen_model.SEEDS["upconv7"], True))
    # (a context per side: each side keeps its own workspaces)
    models = {"rgb7": [rgb7() for _ in range(3)], "upconv7": [upconv7() for _ in range(3)]}
    rows, context = [], []
    for size in filter(None, a.sizes.split(",")):
        h, w = [int(v) for v in size.split("x")]
        H, W = 2 * h, 2 * w
        cw, ch = w2xc.yuv_chroma_size(w, h, LAY)
        ocw, och = w2xc.yuv_chroma_size(W, H, LAY)
        for n in [int(v) for v in a.ns.split(",")]:
            rng = np.random.default_rng(1000 * h + w + n)
            d_y = torch.from_numpy(rng.integers(16, 236, (n, h, w), dtype=np.uint8)).cuda()
            d_u, d_v = (torch.from_numpy(rng.integers(16, 241, (n, ch, cw), dtype=np.uint8)).cuda() for _ in range(2))
            out_new = [torch.zeros((n, H, W), dtype=torch.uint8, device="cuda")] + [torch.zeros((n, och, ocw), dtype=torch.uint8, device="cuda") for _ in range(2)]
            out_old = [torch.zeros_like(t) for t in out_new]
            pi, po, pc = planes(d_y, d_u, d_v, w, h, cw, ch), planes(*out_new, W, H, ocw, och), planes(*out_old, W, H, ocw, och)
            f0 = torch.empty((n, 3, h, w), dtype=torch.float32, device="cuda")
            f1 = torch.empty((n, 3, H, W), dtype=torch.float32, device="cuda")
            for name in ("rgb7", "upconv7"):
                m_new, m_old, m_img = models[name]

                def new():
                    w2xc.process_frames_yuv_u8_rgb_device(n, w, h, LAY, pi, po, None, m_new, 1, RNG, MAT, stream=s, opts=o)

                def old():
                    w2xc.yuv8_to_rgb_device(pi, n, w, h, LAY, RNG, MAT, f0.data_ptr(), 12 * w * h, 4 * w * h, stream=s)
                    if m_old.has_head:
                        m_old.convert_planes_up2x_batch_device(n, 3, f0.data_ptr(), 12 * w * h, 4 * w * h, 4 * w, w, h, f1.data_ptr(), 12 * W * H, 4 * W * H, 4 * W, stream=s,
                                                               opts=o)
                    else:
                        m_old.convert_planes_batch_device(n, 3, f0.data_ptr(), 12 * w * h, 4 * w * h, 4 * w, w, h, f1.data_ptr(), 12 * W * H, 4 * W * H, 4 * W, nn2x=True,
                                                          stream=s, opts=o)
                    w2xc.rgb_to_yuv8_device(f1.data_ptr(), 12 * W * H, 4 * W * H, n, W, H, LAY, RNG, MAT, pc, stream=s)

                new(), old()
                st.synchronize()
                equal = all(torch.equal(x, y) for x, y in zip(out_new, out_old))
                if not equal:
                    raise SystemExit("%s %s n=%d: the new call and the composed route differ" % (size, name, n))
                tn, sn, to, so, reps = compare(new, old, n)
                rows.append({"size": size, "model": name, "n": n, "new_ms_per_frame": round(tn, 5), "new_spread": round(sn, 5), "composed_ms_per_frame": round(to, 5),
                             "composed_spread": round(so, 5), "ratio_composed_over_new": round(to / tn, 3), "reps": reps, "bytes_equal": equal,
                             "ok": bool(tn <= to + so)})
                print(json.dumps(rows[-1]), flush=True)
                # (b) the RGB-image call on an image of the frame's size, per frame, for context
                if n == 1:
                    rgb = torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
                    rgb_out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
                    t, sp, reps = one(lambda: w2xc.process_image_rgb_u8_device(rgb.data_ptr(), 3 * w, w, h, rgb_out.data_ptr(), 3 * W, None, m_img, 1, 0.0, stream=s, opts=o), 1)
                    context.append({"size": size, "model": name, "rgb_image_call_ms_per_frame": round(t, 5), "spread": round(sp, 5), "reps": reps})
                    print(json.dumps(context[-1]), flush=True)
    # (c) the two kernels alone on 1080 x 1920 frames: rotating over ROTATE buffer sets (past the Infinity Cache), and resident on one set
    h, w = 1080, 1920
    cw, ch = w2xc.yuv_chroma_size(w, h, LAY)
    sets = []
    for _ in range(ROTATE):
        d_y = torch.randint(0, 256, (1, h, w), dtype=torch.uint8, device="cuda")
        d_u, d_v = (torch.randint(0, 256, (1, ch, cw), dtype=torch.uint8, device="cuda") for _ in range(2))
        sets.append((planes(d_y, d_u, d_v, w, h, cw, ch), torch.rand((1, 3, h, w), dtype=torch.float32, device="cuda"), (d_y, d_u, d_v)))
    moved = w * h + 2 * cw * ch + 12 * w * h
    turn = [0]

    def to_rgb(rotate):
        p, f, _ = sets[turn[0] % ROTATE if rotate else 0]
        turn[0] += 1
        w2xc.yuv8_to_rgb_device(p, 1, w, h, LAY, RNG, MAT, f.data_ptr(), 12 * w * h, 4 * w * h, stream=s)

    def from_rgb(rotate):
        p, f, _ = sets[turn[0] % ROTATE if rotate else 0]
        turn[0] += 1
        w2xc.rgb_to_yuv8_device(f.data_ptr(), 12 * w * h, 4 * w * h, 1, w, h, LAY, RNG, MAT, p, stream=s)

    kernels = {}
    for name, fn in (("k_yuv8_to_rgb", to_rgb), ("k_rgb_to_yuv8", from_rgb)):
        kernels[name] = {"frame": "1080x1920 4:2:0", "bytes_moved": moved, "hbm_measured_GBps_SURVEY": HBM_TBPS * 1e3}
        for form, rotate in (("rotating", True), ("resident", False)):
            t, sp, reps = one(lambda: fn(rotate), 1)
            kernels[name][form] = {"us": round(t * 1e3, 2), "spread_us": round(sp * 1e3, 2), "reps": reps, "GBps": round(moved / (t * 1e-3) / 1e9, 1),
                                   "working_set_MB": round((ROTATE if rotate else 1) * moved / 1e6, 1)}
        print(json.dumps({name: kernels[name]}), flush=True)
    res = {"tool": "tools/yuv_rgb_bench.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "frames_vs_composed": rows, "rgb_image_call_context": context,
           "kernels_1080p": kernels, "all_ok": all(r["ok"] for r in rows)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f_:
        json.dump(res, f_, indent=1)
        f_.write("\n")
    print("all_ok", res["all_ok"])


if __name__ == "__main__":
    main()
