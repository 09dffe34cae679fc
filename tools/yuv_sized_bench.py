#!/usr/bin/env python
"""tools/yuv_sized_bench.py -- the sized YUV frame calls (include/w2xc_hip.h, "Sized YUV frames") against the composed routes of public calls the header defines
them as, timed in ONE process on ONE device, the two sides alternating window by window.  fp32, default options; resident 4:2:0 frames (left-sited), limited
range, scale mode; two frame formats: 8-bit planar and 10-bit P010; the 7-layer Y chain for the Y route, the 7-layer three-plane chain 3-32-32-64-64-128-128-3 by
BT.709 for the RGB route.

    python tools/yuv_sized_bench.py [--rounds 7] [--shapes 64x64:96x96,256x256:384x384,720x1280:1080x1920,540x960:2160x3840] [--ns 1,8]
                                    [--bench-parent a.json,b.json,c.json --bench-new d.json,e.json,f.json] [--out profiles/yuv_sized_bench.json]

(a) per shape (HxW:OUT_HxOUT_W; iterations = ITERATIONS_AUTO's), n, format and route: ms per frame (median of the rounds, and the spread max - min) of the composed
    route -- every buffer allocated beforehand, its calls enqueued back to back: the luma blocks or the RGB ends, one convert call per 2x step,
    w2xc_resize_linear_device per plane, w2xc_chroma_resize_* per chroma plane -- and of the sized call; the two sides' bytes are compared first.  `ok` = the
    sized call's median is not above the composed route's by more than the larger of that route's spread and 1 % of its median.  A row that misses is recorded
    as missed.
(b) the resize kernels alone on the chroma of a 1080 x 1920 frame at exactly 2x (960 x 540 -> 1920 x 1080 per plane), every launch on the next of ROTATE sets of
    buffers (more than the 256 MiB Infinity Cache in all), beside k_chroma2x_u8_sited / _u16_sited measured in the same run: us and GB/s over the bytes they have
    to move.  Expectation, reported and not gated: within the 2x kernel's own spread plus the cost of per-thread coefficients.
(c) --bench-parent / --bench-new: the JSON lines of `bench.py --gpus 1 --steps 10 --warmup 3` runs of the parent commit's build and of this tree (fresh
    processes, alternating): medians and spreads of ms_per_step, and the gate that the difference of the medians lies inside the parent's spread.
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
ROTATE_C = 64    # buffer sets of the chroma kernels: 64 x 5.2 MB (8-bit) / 10.4 MB (16-bit) is more than the 256 MiB Infinity Cache
DEPTH = 10


def bench_py_part(parent_files, new_files):
    """medians and spreads of ms_per_step over the runs' JSON lines, and the gate"""
    def read(path):
        with open(path) as f:
            lines = [ln for ln in f.read().splitlines() if ln.startswith("{") and "ms_per_step" in ln]
        return json.loads(lines[-1])["ms_per_step"]
    p, n = [read(f) for f in parent_files], [read(f) for f in new_files]
    pm, nm = statistics.median(p), statistics.median(n)
    return {"command": "python bench.py --gpus 1 --steps 10 --warmup 3, fresh processes, the parent's build and this tree alternating", "parent_ms_per_step": p,
            "new_ms_per_step": n, "parent_median": pm, "new_median": nm, "parent_spread": round(max(p) - min(p), 4), "new_spread": round(max(n) - min(n), 4),
            "gate": "new_median - parent_median <= parent_spread", "ok": bool(nm - pm <= max(p) - min(p))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="64x64:96x96,256x256:384x384,720x1280:1080x1920,540x960:2160x3840")
    ap.add_argument("--ns", default="1,8")
    ap.add_argument("--bench-parent", default="")
    ap.add_argument("--bench-new", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_sized_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as graft
    from tools import gen_model
    w2xc = graft.load_package()
    if not torch.cuda.is_available() or w2xc.device_count() < 1:
        raise SystemExit("yuv_sized_bench needs a HIP device (there is no CPU fallback to time)")
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream()
    s = st.cuda_stream
    RNG, MAT, CHROMA = w2xc.RANGE_LIMITED, w2xc.MATRIX_BT709, w2xc.YUV_420_LEFT
    COS = CHROMA & 0x30

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

    def alternate(sides, per):
        for f in sides.values():
            f()
        reps = reps_for(next(iter(sides.values())))
        t = {k: [] for k in sides}
        for _ in range(a.rounds):
            for k, f in sides.items():
                t[k].append(window(f, reps) / per)
        return {k: (statistics.median(v), max(v) - min(v)) for k, v in t.items()}, reps

    def side(fmt, n, w, h, cw, ch, rng=None):
        """(planes struct, tensors) of n frames: fmt 'u8' (planar bytes) or 'p010' (high-packed words, U and V interleaved); rng: video-range values"""
        if fmt == "u8":
            mk = (lambda shape: torch.from_numpy(rng.integers(16, 236, shape, dtype=np.uint8)).cuda()) if rng is not None else \
                (lambda shape: torch.zeros(shape, dtype=torch.uint8, device="cuda"))
            t = [mk((n, h, w)), mk((n, ch, cw)), mk((n, ch, cw))]
            p = w2xc.YuvPlanes()
            p.y, p.y_stride, p.y_frame_stride = t[0].data_ptr(), w, w * h
            p.u, p.v, p.c_stride, p.c_frame_stride, p.c_px = t[1].data_ptr(), t[2].data_ptr(), cw, cw * ch, 1
            return p, t
        mk = (lambda shape: torch.from_numpy(((rng.integers(64, 941, shape).astype(np.uint16) << (16 - DEPTH)).astype(np.uint16)).view(np.int16)).cuda()) \
            if rng is not None else (lambda shape: torch.zeros(shape, dtype=torch.int16, device="cuda"))
        t = [mk((n, h, w)), mk((n, ch, cw, 2))]
        p = w2xc.Yuv16Planes()
        p.pack = w2xc.PACK_HIGH
        p.y, p.y_stride, p.y_frame_stride = t[0].data_ptr(), 2 * w, 2 * w * h
        p.u, p.v, p.c_stride, p.c_frame_stride, p.c_px = t[1].data_ptr(), t[1].data_ptr() + 2, 4 * cw, 4 * cw * ch, 2
        return p, t

    def sized_call(fmt, route, model, n, w, h, pi, ow, oh, po, o):
        if fmt == "u8" and route == "y":
            return lambda: w2xc.process_frames_yuv_u8_sized_device(n, w, h, CHROMA, pi, ow, oh, po, None, model, w2xc.ITERATIONS_AUTO, RNG, stream=s, opts=o)
        if fmt == "u8":
            return lambda: w2xc.process_frames_yuv_u8_rgb_sized_device(n, w, h, CHROMA, pi, ow, oh, po, None, model, w2xc.ITERATIONS_AUTO, RNG, MAT, stream=s, opts=o)
        if route == "y":
            return lambda: w2xc.process_frames_yuv_u16_sized_device(n, w, h, CHROMA, pi, ow, oh, po, None, model, w2xc.ITERATIONS_AUTO, RNG, stream=s, opts=o, depth=DEPTH)
        return lambda: w2xc.process_frames_yuv_u16_rgb_sized_device(n, w, h, CHROMA, pi, ow, oh, po, None, model, w2xc.ITERATIONS_AUTO, RNG, MAT, stream=s, opts=o,
                                                                    depth=DEPTH)

    def composed_call(fmt, route, model, n, w, h, pi, ow, oh, po, o, it):
        """the route of the header from public calls, every plane allocated here; -> the callable that enqueues it"""
        planes = 3 if route == "rgb" else 1
        levels = [torch.empty((n, planes, h << i, w << i), dtype=torch.float32, device="cuda") for i in range(it + 1)]
        W, H = w << it, h << it
        shrunk = torch.empty((n, planes, oh, ow), dtype=torch.float32, device="cuda") if (ow, oh) != (W, H) else levels[-1]
        cw, ch = w2xc.yuv_chroma_size(w, h, CHROMA)
        ocw, och = w2xc.yuv_chroma_size(ow, oh, CHROMA)

        def run():
            d = levels[0]
            if route == "y" and fmt == "u8":
                w2xc.y8_to_plane_device(pi.y, n, pi.y_frame_stride, pi.y_stride, w, h, RNG, d.data_ptr(), 4 * w * h, stream=s)
            elif route == "y":
                w2xc.y16_to_plane_device(pi.y, n, pi.y_frame_stride, pi.y_stride, w, h, RNG, DEPTH, pi.pack, d.data_ptr(), 4 * w * h, stream=s)
            elif fmt == "u8":
                w2xc.yuv8_to_rgb_device(pi, n, w, h, CHROMA, RNG, MAT, d.data_ptr(), 12 * w * h, 4 * w * h, stream=s)
            else:
                w2xc.yuv16_to_rgb_device(pi, n, w, h, CHROMA, RNG, DEPTH, MAT, d.data_ptr(), 12 * w * h, 4 * w * h, stream=s)
            lw, lh = w, h
            for i in range(it):
                nx = levels[i + 1]
                if route == "y":
                    model.convert_batch_device(n, d.data_ptr(), 4 * lw * lh, 4 * lw, lw, lh, nx.data_ptr(), 16 * lw * lh, 8 * lw, nn2x=True, stream=s, opts=o)
                else:
                    model.convert_planes_batch_device(n, 3, d.data_ptr(), 12 * lw * lh, 4 * lw * lh, 4 * lw, lw, lh, nx.data_ptr(), 48 * lw * lh, 16 * lw * lh, 8 * lw,
                                                      nn2x=True, stream=s, opts=o)
                d, lw, lh = nx, 2 * lw, 2 * lh
            if shrunk is not d:
                for p in range(n * planes):
                    w2xc.resize_linear_device(d.data_ptr() + 4 * p * lw * lh, lw, lh, shrunk.data_ptr() + 4 * p * ow * oh, ow, oh, stream=s)
                d = shrunk
            if route == "rgb" and fmt == "u8":
                w2xc.rgb_to_yuv8_device(d.data_ptr(), 12 * ow * oh, 4 * ow * oh, n, ow, oh, CHROMA, RNG, MAT, po, stream=s)
            elif route == "rgb":
                w2xc.rgb_to_yuv16_device(d.data_ptr(), 12 * ow * oh, 4 * ow * oh, n, ow, oh, CHROMA, RNG, DEPTH, MAT, po, stream=s)
            elif fmt == "u8":
                w2xc.plane_to_y8_device(d.data_ptr(), n, 4 * ow * oh, ow, oh, RNG, po.y, po.y_frame_stride, po.y_stride, stream=s)
                for src, dst in ((pi.u, po.u), (pi.v, po.v)):
                    w2xc.chroma_resize_u8_device(src, n, pi.c_frame_stride, pi.c_stride, pi.c_px, cw, ch, dst, po.c_frame_stride, po.c_stride, po.c_px, ocw, och, w, h,
                                                 ow, oh, 1, 1, COS, stream=s)
            else:
                w2xc.plane_to_y16_device(d.data_ptr(), n, 4 * ow * oh, ow, oh, RNG, DEPTH, po.pack, po.y, po.y_frame_stride, po.y_stride, stream=s)
                for src, dst in ((pi.u, po.u), (pi.v, po.v)):
                    w2xc.chroma_resize_u16_device(src, n, pi.c_frame_stride, pi.c_stride, pi.c_px, pi.pack, cw, ch, DEPTH, dst, po.c_frame_stride, po.c_stride, po.c_px,
                                                  po.pack, ocw, och, w, h, ow, oh, 1, 1, COS, stream=s)
        return run

    models = {"y": w2xc._ModelSet.from_layers(gen_model.synth_layers(seed=gen_model.SEEDS["scale2.0x"])),
              "rgb": w2xc._ModelSet.from_layers(gen_model.synth_layers(RGB_TOPO, 301))}
    opts = w2xc.make_opts(device=0)
    rows = []
    for shape in filter(None, a.shapes.split(",")):
        (h, w), (oh, ow) = ([int(v) for v in part.split("x")] for part in shape.split(":"))
        it = w2xc.sized_iterations(w, h, ow, oh)
        cw, ch = w2xc.yuv_chroma_size(w, h, CHROMA)
        ocw, och = w2xc.yuv_chroma_size(ow, oh, CHROMA)
        for n in [int(v) for v in a.ns.split(",")]:
            for fmt in ("u8", "p010"):
                pi, t_i = side(fmt, n, w, h, cw, ch, np.random.default_rng(1000 * h + w + n))
                (po_s, t_s), (po_c, t_c) = side(fmt, n, ow, oh, ocw, och), side(fmt, n, ow, oh, ocw, och)
                for route in ("y", "rgb"):
                    sides = {"composed": composed_call(fmt, route, models[route], n, w, h, pi, ow, oh, po_c, opts, it),
                             "sized": sized_call(fmt, route, models[route], n, w, h, pi, ow, oh, po_s, opts)}
                    for f in sides.values():
                        f()
                    st.synchronize()
                    equal = all(torch.equal(x, y) for x, y in zip(t_s, t_c))
                    assert equal, "%s %s %s n=%d: the sized call and its composed route differ" % (shape, fmt, route, n)
                    t, reps = alternate(sides, n)
                    ref_t, ref_s = t["composed"]
                    margin = max(ref_s, 0.01 * ref_t)
                    row = {"shape": shape, "iterations": it, "format": fmt, "route": route, "n": n, "reps": reps, "bytes_equal": equal, "margin": round(margin, 5)}
                    for k, (m, sp) in t.items():
                        row[k + "_ms_per_frame"], row[k + "_spread"] = round(m, 5), round(sp, 5)
                    row["ok"] = bool(t["sized"][0] <= ref_t + margin)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    for x in t_s + t_c:
                        x.zero_()
                del pi, t_i, po_s, t_s, po_c, t_c
    # (b) the kernels alone: both planes of a 960 x 540 chroma frame -> 1920 x 1080, rotating over buffer sets past the Infinity Cache
    h, w = 1080, 1920
    cw, ch = w2xc.yuv_chroma_size(w, h, CHROMA)
    ocw, och = 2 * cw, 2 * ch
    rng = np.random.default_rng(7)
    turn = [0]

    def figure(f, moved, rotate):
        reps = reps_for(f)
        t = [window(f, reps) for _ in range(a.rounds)]
        m, sp = statistics.median(t), max(t) - min(t)
        return {"us": round(m * 1e3, 2), "spread_us": round(sp * 1e3, 2), "reps": reps, "bytes_moved": moved, "GBps": round(moved / (m * 1e-3) / 1e9, 1),
                "GBps_low": round(moved / ((m + sp) * 1e-3) / 1e9, 1), "working_set_MB": round(rotate * moved / 1e6, 1)}

    csets = {fmt: [(side(fmt, 1, w, h, cw, ch, rng), side(fmt, 1, 2 * w, 2 * h, ocw, och)) for _ in range(ROTATE_C)] for fmt in ("u8", "p010")}

    def chroma(fmt, resize):
        k = turn[0] % ROTATE_C
        turn[0] += 1
        (pi, _), (po, _) = csets[fmt][k]
        for src, dst in ((pi.u, po.u), (pi.v, po.v)):
            if fmt == "u8" and resize:
                w2xc.chroma_resize_u8_device(src, 1, 0, cw, 1, cw, ch, dst, 0, ocw, 1, ocw, och, w, h, 2 * w, 2 * h, 1, 1, COS, stream=s)
            elif fmt == "u8":
                w2xc.chroma2x_u8_sited_device(src, 1, 0, cw, 1, cw, ch, dst, 0, ocw, 1, ocw, och, COS, stream=s)
            elif resize:
                w2xc.chroma_resize_u16_device(src, 1, 0, pi.c_stride, pi.c_px, pi.pack, cw, ch, DEPTH, dst, 0, po.c_stride, po.c_px, po.pack, ocw, och, w, h, 2 * w, 2 * h,
                                              1, 1, COS, stream=s)
            else:
                w2xc.chroma2x_u16_sited_device(src, 1, 0, pi.c_stride, pi.c_px, pi.pack, cw, ch, DEPTH, dst, 0, po.c_stride, po.c_px, po.pack, ocw, och, COS, stream=s)

    kernels = {}
    for fmt, bps, tag in (("u8", 1, "8"), ("p010", 2, "16")):
        moved = 2 * bps * (cw * ch + ocw * och)
        # the same bytes from both, first
        chroma(fmt, False)
        st.synchronize()
        k0 = (turn[0] - 1) % ROTATE_C
        want = [x.clone() for x in csets[fmt][k0][1][1]]
        for x in csets[fmt][k0][1][1]:
            x.zero_()
        turn[0] -= 1
        chroma(fmt, True)
        st.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(want, csets[fmt][k0][1][1])), "the resize kernel at exactly 2x is not the 2x kernel's output"
        ref = figure(lambda: chroma(fmt, False), moved, ROTATE_C)
        new = figure(lambda: chroma(fmt, True), moved, ROTATE_C)
        again = figure(lambda: chroma(fmt, False), moved, ROTATE_C)
        new["against_2x_us"] = round(new["us"] - ref["us"], 2)
        new["within_2x_spread"] = bool(new["us"] <= max(ref["us"], again["us"]) + max(ref["spread_us"], again["spread_us"]))
        kernels["k_chroma2x_u%s_sited %s left (two launches: U, V)" % (tag, fmt)] = ref
        kernels["k_chroma_resize_u%s %s left at exactly 2x (two launches: U, V)" % (tag, fmt)] = new
        kernels["k_chroma2x_u%s_sited %s left, measured again" % (tag, fmt)] = again
    print(json.dumps(kernels), flush=True)
    res = {"tool": "tools/yuv_sized_bench.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "depth": DEPTH, "chroma": "W2XC_YUV_420_LEFT",
           "reference": "the composed route of public calls, in the same process", "frames": rows, "kernels_1080p_chroma_2x_rotating": kernels,
           "all_ok": all(r["ok"] for r in rows), "missed": [r for r in rows if not r["ok"]]}
    if a.bench_parent and a.bench_new:
        res["bench_py"] = bench_py_part(a.bench_parent.split(","), a.bench_new.split(","))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f_:
        json.dump(res, f_, indent=1)
        f_.write("\n")
    print("all_ok", res["all_ok"])


if __name__ == "__main__":
    main()
