#!/usr/bin/env python
"""tools/yuv16_bench.py -- the 16-bit YUV frame calls (w2xc_process_frames_yuv_u16_device, w2xc_process_frames_yuv_u16_rgb_device), timed in ONE process on ONE
device, the two sides of every comparison alternating window by window.  fp32, default options; resident 4:2:0 frames of 10-bit samples, limited range, scale
mode; two frame formats: planar low-packed words (yuv420p10le) and P010 (high-packed, U and V interleaved).  Models: the 7-layer Y chain for the Y route, the
7-layer three-plane chain 3-32-32-64-64-128-128-3 by BT.2020 for the RGB route.

    python tools/yuv16_bench.py [--rounds 7] [--sizes 64x64,256x256,1080x1920] [--ns 1,8] [--out profiles/yuv16_bench.json]

(a) each new call on n frames against the route it is defined by, composed from public calls (w2xc_y16_to_plane_device, w2xc_convert_batch_device,
    w2xc_plane_to_y16_device and w2xc_chroma2x_u16_device per chroma plane; w2xc_yuv16_to_rgb_device, w2xc_convert_planes_batch_device,
    w2xc_rgb_to_yuv16_device).  The words of the two sides must be equal.  `ok` = the new side's median is not above the composed route's by more than the
    larger of that route's spread (max - min over rounds) and 1 % of its median: at n >= 2 both sides launch the same kernels with the same arguments.
(b) the ends alone on 1080 x 1920 4:2:0 frames, every launch on the next of ROTATE sets of buffers (more than the 256 MiB Infinity Cache in all): us and GB/s
    over the bytes they have to move, k_yuv16_to_rgb and k_rgb_to_yuv16 planar and P010 beside k_yuv8_to_rgb / k_rgb_to_yuv8, and k_chroma2x_u16 beside
    k_chroma2x_u8, all measured in this run.  `expectation`: the 16-bit kernel's GB/s is not below the 8-bit kernel's by more than the two kernels' spreads.
A timed window is `reps` calls enqueued back to back and one synchronisation, reps chosen so that a window is >= ~100 ms."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RGB_TOPO = [3, 32, 32, 64, 64, 128, 128, 3]
ROTATE = 12      # buffer sets of the RGB ends: 12 x 28 MB (8-bit) / 31 MB (16-bit) is more than the 256 MiB Infinity Cache
ROTATE_C = 64    # ... of the chroma kernels: 64 x 5.2 MB (8-bit) / 10.4 MB (16-bit)
DEPTH = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="64x64,256x256,1080x1920")
    ap.add_argument("--ns", default="1,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv16_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as graft
    from tools import gen_model
    w2xc = graft.load_package()
    if not torch.cuda.is_available() or w2xc.device_count() < 1:
        raise SystemExit("yuv16_bench needs a HIP device (there is no CPU fallback to time)")
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream()
    s = st.cuda_stream
    o = w2xc.make_opts(device=0)
    LAY, RNG, MAT = w2xc.YUV_420, w2xc.RANGE_LIMITED, w2xc.MATRIX_BT2020
    LOW, HIGH = w2xc.PACK_LOW, w2xc.PACK_HIGH

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

    def words(shape, lo, hi, shift, rng):
        """words of 10-bit values in [lo, hi) on the device (int16 tensors: the bits are what counts)"""
        v = (rng.integers(lo, hi, shape).astype(np.uint16) << shift).astype(np.uint16)
        return torch.from_numpy(v.view(np.int16)).cuda()

    def side(fmt, n, w, h, cw, ch, rng=None):
        """(Yuv16Planes, tensors) of n frames: fmt 'planar_low' or 'p010'; rng: filled with video-range values, else zeros"""
        p010 = fmt == "p010"
        shift = 16 - DEPTH if p010 else 0
        mk = (lambda shape, lo, hi: words(shape, lo, hi, shift, rng)) if rng is not None else (lambda shape, lo, hi: torch.zeros(shape, dtype=torch.int16, device="cuda"))
        t_y = mk((n, h, w), 64, 941)
        p = w2xc.Yuv16Planes()
        p.pack = HIGH if p010 else LOW
        p.y, p.y_stride, p.y_frame_stride = t_y.data_ptr(), 2 * w, 2 * w * h
        if p010:
            t_c = [mk((n, ch, cw, 2), 64, 961)]
            p.u, p.v, p.c_stride, p.c_frame_stride, p.c_px = t_c[0].data_ptr(), t_c[0].data_ptr() + 2, 4 * cw, 4 * cw * ch, 2
        else:
            t_c = [mk((n, ch, cw), 64, 961) for _ in range(2)]
            p.u, p.v, p.c_stride, p.c_frame_stride, p.c_px = t_c[0].data_ptr(), t_c[1].data_ptr(), 2 * cw, 2 * cw * ch, 1
        return p, [t_y] + t_c

    y7 = lambda: w2xc._ModelSet.from_layers(gen_model.synth_layers(seed=gen_model.SEEDS["scale2.0x"]))
    rgb7 = lambda: w2xc._ModelSet.from_layers(gen_model.synth_layers(RGB_TOPO, 301))
    models = {"y": [y7(), y7()], "rgb": [rgb7(), rgb7()]}      # (a context per side: each side keeps its own workspaces)
    rows = []
    for size in filter(None, a.sizes.split(",")):
        h, w = [int(v) for v in size.split("x")]
        H, W = 2 * h, 2 * w
        cw, ch = w2xc.yuv_chroma_size(w, h, LAY)
        ocw, och = w2xc.yuv_chroma_size(W, H, LAY)
        for n in [int(v) for v in a.ns.split(",")]:
            y0 = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
            y1 = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
            f0 = torch.empty((n, 3, h, w), dtype=torch.float32, device="cuda")
            f1 = torch.empty((n, 3, H, W), dtype=torch.float32, device="cuda")
            for fmt in ("planar_low", "p010"):
                pi, keep_i = side(fmt, n, w, h, cw, ch, np.random.default_rng(1000 * h + w + n))
                po, out_new = side(fmt, n, W, H, ocw, och)
                pc, out_old = side(fmt, n, W, H, ocw, och)
                for route in ("y", "rgb"):
                    m_new, m_old = models[route]

                    if route == "y":
                        def new():
                            w2xc.process_frames_yuv_u16_device(n, w, h, LAY, pi, po, None, m_new, 1, RNG, stream=s, opts=o, depth=DEPTH)

                        def old():
                            w2xc.y16_to_plane_device(pi.y, n, pi.y_frame_stride, pi.y_stride, w, h, RNG, DEPTH, pi.pack, y0.data_ptr(), 4 * w * h, stream=s)
                            m_old.convert_batch_device(n, y0.data_ptr(), 4 * w * h, 4 * w, w, h, y1.data_ptr(), 4 * W * H, 4 * W, nn2x=True, stream=s, opts=o)
                            w2xc.plane_to_y16_device(y1.data_ptr(), n, 4 * W * H, W, H, RNG, DEPTH, pc.pack, pc.y, pc.y_frame_stride, pc.y_stride, stream=s)
                            for src, dst in ((pi.u, pc.u), (pi.v, pc.v)):
                                w2xc.chroma2x_u16_device(src, n, pi.c_frame_stride, pi.c_stride, pi.c_px, pi.pack, cw, ch, DEPTH, dst, pc.c_frame_stride, pc.c_stride,
                                                         pc.c_px, pc.pack, ocw, och, stream=s)
                    else:
                        def new():
                            w2xc.process_frames_yuv_u16_rgb_device(n, w, h, LAY, pi, po, None, m_new, 1, RNG, MAT, stream=s, opts=o, depth=DEPTH)

                        def old():
                            w2xc.yuv16_to_rgb_device(pi, n, w, h, LAY, RNG, DEPTH, MAT, f0.data_ptr(), 12 * w * h, 4 * w * h, stream=s)
                            m_old.convert_planes_batch_device(n, 3, f0.data_ptr(), 12 * w * h, 4 * w * h, 4 * w, w, h, f1.data_ptr(), 12 * W * H, 4 * W * H, 4 * W, nn2x=True,
                                                              stream=s, opts=o)
                            w2xc.rgb_to_yuv16_device(f1.data_ptr(), 12 * W * H, 4 * W * H, n, W, H, LAY, RNG, DEPTH, MAT, pc, stream=s)

                    for t in out_new + out_old:
                        t.zero_()
                    new(), old()
                    st.synchronize()
                    equal = all(torch.equal(x, y) for x, y in zip(out_new, out_old))
                    if not equal:
                        raise SystemExit("%s %s %s n=%d: the new call and the composed route differ" % (size, fmt, route, n))
                    tn, sn, to, so, reps = compare(new, old, n)
                    margin = max(so, 0.01 * to)
                    rows.append({"size": size, "format": fmt, "route": route, "n": n, "new_ms_per_frame": round(tn, 5), "new_spread": round(sn, 5),
                                 "composed_ms_per_frame": round(to, 5), "composed_spread": round(so, 5), "margin": round(margin, 5),
                                 "ratio_composed_over_new": round(to / tn, 3), "reps": reps, "words_equal": equal, "ok": bool(tn <= to + margin)})
                    print(json.dumps(rows[-1]), flush=True)
                del keep_i
    # (b) the ends alone on 1080 x 1920 frames, rotating over buffer sets past the Infinity Cache
    h, w = 1080, 1920
    cw, ch = w2xc.yuv_chroma_size(w, h, LAY)
    rng = np.random.default_rng(7)

    def side8(n, w_, h_, cw_, ch_):
        d_y = torch.randint(0, 256, (n, h_, w_), dtype=torch.uint8, device="cuda")
        d_u, d_v = (torch.randint(0, 256, (n, ch_, cw_), dtype=torch.uint8, device="cuda") for _ in range(2))
        p = w2xc.YuvPlanes()
        p.y, p.y_stride, p.y_frame_stride = d_y.data_ptr(), w_, w_ * h_
        p.u, p.v, p.c_stride, p.c_frame_stride, p.c_px = d_u.data_ptr(), d_v.data_ptr(), cw_, cw_ * ch_, 1
        return p, (d_y, d_u, d_v)

    floats = [torch.rand((1, 3, h, w), dtype=torch.float32, device="cuda") for _ in range(ROTATE)]
    sets = {"u8": [side8(1, w, h, cw, ch) for _ in range(ROTATE)], "planar_low": [side("planar_low", 1, w, h, cw, ch, rng) for _ in range(ROTATE)],
            "p010": [side("p010", 1, w, h, cw, ch, rng) for _ in range(ROTATE)]}
    turn = [0]

    def rgb_end(kind, to_rgb):
        k = turn[0] % ROTATE
        turn[0] += 1
        p, f = sets[kind][k][0], floats[k]
        if kind == "u8":
            if to_rgb:
                w2xc.yuv8_to_rgb_device(p, 1, w, h, LAY, RNG, MAT, f.data_ptr(), 12 * w * h, 4 * w * h, stream=s)
            else:
                w2xc.rgb_to_yuv8_device(f.data_ptr(), 12 * w * h, 4 * w * h, 1, w, h, LAY, RNG, MAT, p, stream=s)
        elif to_rgb:
            w2xc.yuv16_to_rgb_device(p, 1, w, h, LAY, RNG, DEPTH, MAT, f.data_ptr(), 12 * w * h, 4 * w * h, stream=s)
        else:
            w2xc.rgb_to_yuv16_device(f.data_ptr(), 12 * w * h, 4 * w * h, 1, w, h, LAY, RNG, DEPTH, MAT, p, stream=s)

    def figure(f, moved, rotate):
        t, sp, reps = one(f, 1)
        return {"us": round(t * 1e3, 2), "spread_us": round(sp * 1e3, 2), "reps": reps, "bytes_moved": moved, "GBps": round(moved / (t * 1e-3) / 1e9, 1),
                "GBps_low": round(moved / ((t + sp) * 1e-3) / 1e9, 1), "working_set_MB": round(rotate * moved / 1e6, 1)}

    def expect(new, ref):
        """the 16-bit kernel's GB/s is not below the 8-bit kernel's, the kernels' own spreads as margin: its median against the 8-bit kernel's slowest round"""
        margin = ref["GBps"] - ref["GBps_low"] + new["GBps"] - new["GBps_low"]
        return "met" if new["GBps"] >= ref["GBps"] - margin else "missed"

    kernels = {}
    samples = w * h + 2 * cw * ch
    for to_rgb, name8, name16 in ((True, "k_yuv8_to_rgb", "k_yuv16_to_rgb"), (False, "k_rgb_to_yuv8", "k_rgb_to_yuv16")):
        kernels[name8] = figure(lambda: rgb_end("u8", to_rgb), samples + 12 * w * h, ROTATE)
        for fmt in ("planar_low", "p010"):
            r = figure(lambda: rgb_end(fmt, to_rgb), 2 * samples + 12 * w * h, ROTATE)
            r["expectation_GBps_not_below_8bit"] = expect(r, kernels[name8])
            kernels["%s %s" % (name16, fmt)] = r
        print(json.dumps({k: v for k, v in kernels.items() if name8 in k or name16 in k}), flush=True)
    del sets, floats
    # the chroma kernels: both planes of a 960 x 540 chroma frame -> 1920 x 1080, one launch
    ocw, och = 2 * cw, 2 * ch
    c8 = [(side8(1, w, h, cw, ch), side8(1, 2 * w, 2 * h, ocw, och)) for _ in range(ROTATE_C)]
    c16 = {fmt: [(side(fmt, 1, w, h, cw, ch, rng), side(fmt, 1, 2 * w, 2 * h, ocw, och)) for _ in range(ROTATE_C)] for fmt in ("planar_low", "p010")}
    # (the chroma kernel alone: a noise-free frame call is not it; the block takes one plane, so a frame's two planes are two launches of it on planar planes)
    def chroma8():
        k = turn[0] % ROTATE_C
        turn[0] += 1
        (pi, _), (po, _) = c8[k]
        for src, dst in ((pi.u, po.u), (pi.v, po.v)):
            w2xc.chroma2x_u8_device(src, 1, 0, cw, 1, cw, ch, dst, 0, ocw, 1, ocw, och, stream=s)

    def chroma16(fmt):
        k = turn[0] % ROTATE_C
        turn[0] += 1
        (pi, _), (po, _) = c16[fmt][k]
        for src, dst in ((pi.u, po.u), (pi.v, po.v)):
            w2xc.chroma2x_u16_device(src, 1, 0, pi.c_stride, pi.c_px, pi.pack, cw, ch, DEPTH, dst, 0, po.c_stride, po.c_px, po.pack, ocw, och, stream=s)

    kernels["k_chroma2x_u8 (two launches: U, V)"] = figure(chroma8, 2 * (cw * ch + ocw * och), ROTATE_C)
    for fmt in ("planar_low", "p010"):
        r = figure(lambda: chroma16(fmt), 4 * (cw * ch + ocw * och), ROTATE_C)
        r["expectation_GBps_not_below_8bit"] = expect(r, kernels["k_chroma2x_u8 (two launches: U, V)"])
        kernels["k_chroma2x_u16 %s (two launches: U, V)" % fmt] = r
    print(json.dumps({k: v for k, v in kernels.items() if "chroma" in k}), flush=True)
    res = {"tool": "tools/yuv16_bench.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "depth": DEPTH, "frames_vs_composed": rows,
           "kernels_1080p_rotating": kernels, "all_ok": all(r["ok"] for r in rows)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f_:
        json.dump(res, f_, indent=1)
        f_.write("\n")
    print("all_ok", res["all_ok"])


if __name__ == "__main__":
    main()
