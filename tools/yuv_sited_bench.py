#!/usr/bin/env python
"""tools/yuv_sited_bench.py -- the YUV frame calls with chroma siting flags (include/w2xc_hip.h, "Chroma siting") against the centred calls of ANOTHER build of the
library (the parent commit, built beside this tree), timed in ONE process on ONE device, the sides alternating window by window.  fp32, default options; resident
4:2:0 frames, limited range, scale mode; two frame formats: 8-bit planar and 10-bit P010; the 7-layer Y chain for the Y route, the 7-layer three-plane chain
3-32-32-64-64-128-128-3 by BT.709 for the RGB route.

    python tools/yuv_sited_bench.py --other DIR [--rounds 7] [--sizes 64x64,256x256,1080x1920] [--ns 1,8] [--out profiles/yuv_sited_bench.json]

(a) per size, n, format and route: ms per frame (median of the rounds, and the spread max - min) of the OTHER build's centred call (W2XC_YUV_420), of this build's
    centred call, and of this build's calls with W2XC_YUV_420_LEFT and W2XC_YUV_420_TOPLEFT.  `ok` = a sited call's median is not above the other build's centred
    median by more than the larger of that side's spread and 1 % of its median.  Without --other the reference is this build's centred call.
(b) the six sited kernels alone on 1080 x 1920 4:2:0 frames, every launch on the next of ROTATE sets of buffers (more than the 256 MiB Infinity Cache in all): us and
    GB/s over the bytes they have to move, beside their centred forms measured in this run.  Expectations, reported and not gated: to-RGB and the 2x are not below
    their centred forms beyond the two spreads; from-RGB is within its spread plus the share of halo samples a tile converts again (a left column of 32 and a top
    row of 64 + 1 luma samples of a 64 x 32 tile: 1 / 64 for a co-sited x, 1 / 32 more for a co-sited y).
A timed window is `reps` calls enqueued back to back and one synchronisation, reps chosen so that a window is >= ~100 ms."""
import argparse
import importlib.util
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


def load_other(root):
    """the package of another tree under a name of its own: its library beside this tree's in one process"""
    pkg = os.path.join(root, "waifu2x-converter-cpp_amd")
    spec = importlib.util.spec_from_file_location("w2xc_amd_other", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["w2xc_amd_other"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", default=None, help="a checkout of the commit to compare against, built (its lib/libw2xc_hip.so exists)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="64x64,256x256,1080x1920")
    ap.add_argument("--ns", default="1,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_sited_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as graft
    from tools import gen_model
    w2xc = graft.load_package()
    if not torch.cuda.is_available() or w2xc.device_count() < 1:
        raise SystemExit("yuv_sited_bench needs a HIP device (there is no CPU fallback to time)")
    other = load_other(a.other) if a.other else w2xc
    assert other is w2xc or os.path.realpath(other.LIB_PATH) != os.path.realpath(w2xc.LIB_PATH)
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream()
    s = st.cuda_stream
    RNG, MAT = w2xc.RANGE_LIMITED, w2xc.MATRIX_BT709
    C420, LEFT, TOPLEFT = w2xc.YUV_420, w2xc.YUV_420_LEFT, w2xc.YUV_420_TOPLEFT

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
        """{name: (median, spread)} of the sides, one window each per round, in turn"""
        for f in sides.values():
            f()
        reps = reps_for(next(iter(sides.values())))
        t = {k: [] for k in sides}
        for _ in range(a.rounds):
            for k, f in sides.items():
                t[k].append(window(f, reps) / per)
        return {k: (statistics.median(v), max(v) - min(v)) for k, v in t.items()}, reps

    def side(lib, fmt, n, w, h, cw, ch, rng=None):
        """(planes struct of `lib`, tensors) of n frames: fmt 'u8' (planar bytes) or 'p010' (high-packed words, U and V interleaved); rng: video-range values"""
        if fmt == "u8":
            mk = (lambda shape: torch.from_numpy(rng.integers(16, 236, shape, dtype=np.uint8)).cuda()) if rng is not None else \
                (lambda shape: torch.zeros(shape, dtype=torch.uint8, device="cuda"))
            t = [mk((n, h, w)), mk((n, ch, cw)), mk((n, ch, cw))]
            p = lib.YuvPlanes()
            p.y, p.y_stride, p.y_frame_stride = t[0].data_ptr(), w, w * h
            p.u, p.v, p.c_stride, p.c_frame_stride, p.c_px = t[1].data_ptr(), t[2].data_ptr(), cw, cw * ch, 1
            return p, t
        mk = (lambda shape: torch.from_numpy(((rng.integers(64, 941, shape).astype(np.uint16) << (16 - DEPTH)).astype(np.uint16)).view(np.int16)).cuda()) \
            if rng is not None else (lambda shape: torch.zeros(shape, dtype=torch.int16, device="cuda"))
        t = [mk((n, h, w)), mk((n, ch, cw, 2))]
        p = lib.Yuv16Planes()
        p.pack = lib.PACK_HIGH
        p.y, p.y_stride, p.y_frame_stride = t[0].data_ptr(), 2 * w, 2 * w * h
        p.u, p.v, p.c_stride, p.c_frame_stride, p.c_px = t[1].data_ptr(), t[1].data_ptr() + 2, 4 * cw, 4 * cw * ch, 2
        return p, t

    def frame_call(lib, fmt, route, model, n, w, h, chroma, pi, po, o):
        if fmt == "u8" and route == "y":
            return lambda: lib.process_frames_yuv_u8_device(n, w, h, chroma, pi, po, None, model, 1, RNG, stream=s, opts=o)
        if fmt == "u8":
            return lambda: lib.process_frames_yuv_u8_rgb_device(n, w, h, chroma, pi, po, None, model, 1, RNG, MAT, stream=s, opts=o)
        if route == "y":
            return lambda: lib.process_frames_yuv_u16_device(n, w, h, chroma, pi, po, None, model, 1, RNG, stream=s, opts=o, depth=DEPTH)
        return lambda: lib.process_frames_yuv_u16_rgb_device(n, w, h, chroma, pi, po, None, model, 1, RNG, MAT, stream=s, opts=o, depth=DEPTH)

    def models_of(lib):
        return {"y": lib._ModelSet.from_layers(gen_model.synth_layers(seed=gen_model.SEEDS["scale2.0x"])), "rgb": lib._ModelSet.from_layers(gen_model.synth_layers(RGB_TOPO, 301))}

    libs = {"other_centred": (other, C420), "centred": (w2xc, C420), "left": (w2xc, LEFT), "topleft": (w2xc, TOPLEFT)}
    models = {k: models_of(lib) for k, (lib, _) in libs.items()}      # (a context per side: each side keeps its own workspaces)
    opts = {k: lib.make_opts(device=0) for k, (lib, _) in libs.items()}
    rows = []
    for size in filter(None, a.sizes.split(",")):
        h, w = [int(v) for v in size.split("x")]
        H, W = 2 * h, 2 * w
        cw, ch = w2xc.yuv_chroma_size(w, h, C420)
        ocw, och = w2xc.yuv_chroma_size(W, H, C420)
        for n in [int(v) for v in a.ns.split(",")]:
            for fmt in ("u8", "p010"):
                keep, ins, outs = [], {}, {}
                for k, (lib, _) in libs.items():
                    ins[k], t_i = side(lib, fmt, n, w, h, cw, ch, np.random.default_rng(1000 * h + w + n))
                    outs[k], t_o = side(lib, fmt, n, W, H, ocw, och)
                    keep.append((t_i, t_o))
                for route in ("y", "rgb"):
                    sides = {k: frame_call(lib, fmt, route, models[k][route], n, w, h, chroma, ins[k], outs[k], opts[k]) for k, (lib, chroma) in libs.items()}
                    for f in sides.values():
                        f()
                    st.synchronize()
                    # the two centred sides give the same samples, and luma of the Y route does not depend on the siting
                    assert all(torch.equal(x, y) for x, y in zip(keep[0][1], keep[1][1])), "%s %s %s n=%d: the two builds' centred calls differ" % (size, fmt, route, n)
                    if route == "y":
                        assert torch.equal(keep[1][1][0], keep[2][1][0]) and not torch.equal(keep[1][1][1], keep[2][1][1])
                    t, reps = alternate(sides, n)
                    ref_t, ref_s = t["other_centred"]
                    margin = max(ref_s, 0.01 * ref_t)
                    row = {"size": size, "format": fmt, "route": route, "n": n, "reps": reps, "margin": round(margin, 5)}
                    for k, (m, sp) in t.items():
                        row[k + "_ms_per_frame"], row[k + "_spread"] = round(m, 5), round(sp, 5)
                    row["ok"] = bool(t["left"][0] <= ref_t + margin and t["topleft"][0] <= ref_t + margin)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                del keep, ins, outs
    # (b) the kernels alone on 1080 x 1920 frames, rotating over buffer sets past the Infinity Cache
    h, w = 1080, 1920
    cw, ch = w2xc.yuv_chroma_size(w, h, C420)
    rng = np.random.default_rng(7)
    turn = [0]

    def one(f):
        reps = reps_for(f)
        t = [window(f, reps) for _ in range(a.rounds)]
        return statistics.median(t), max(t) - min(t), reps

    def figure(f, moved, rotate):
        t, sp, reps = one(f)
        return {"us": round(t * 1e3, 2), "spread_us": round(sp * 1e3, 2), "reps": reps, "bytes_moved": moved, "GBps": round(moved / (t * 1e-3) / 1e9, 1),
                "GBps_low": round(moved / ((t + sp) * 1e-3) / 1e9, 1), "working_set_MB": round(rotate * moved / 1e6, 1)}

    def expect(new, ref, halo=0.0):
        margin = ref["GBps"] - ref["GBps_low"] + new["GBps"] - new["GBps_low"]
        return "met" if new["GBps"] >= ref["GBps"] * (1.0 - halo) - margin else "missed"

    kernels = {}
    floats = [torch.rand((1, 3, h, w), dtype=torch.float32, device="cuda") for _ in range(ROTATE)]
    sets = {fmt: [side(w2xc, fmt, 1, w, h, cw, ch, rng) for _ in range(ROTATE)] for fmt in ("u8", "p010")}
    samples = w * h + 2 * cw * ch

    def rgb_end(fmt, to_rgb, chroma):
        k = turn[0] % ROTATE
        turn[0] += 1
        p, f = sets[fmt][k][0], floats[k]
        if fmt == "u8" and to_rgb:
            w2xc.yuv8_to_rgb_device(p, 1, w, h, chroma, RNG, MAT, f.data_ptr(), 12 * w * h, 4 * w * h, stream=s)
        elif fmt == "u8":
            w2xc.rgb_to_yuv8_device(f.data_ptr(), 12 * w * h, 4 * w * h, 1, w, h, chroma, RNG, MAT, p, stream=s)
        elif to_rgb:
            w2xc.yuv16_to_rgb_device(p, 1, w, h, chroma, RNG, DEPTH, MAT, f.data_ptr(), 12 * w * h, 4 * w * h, stream=s)
        else:
            w2xc.rgb_to_yuv16_device(f.data_ptr(), 12 * w * h, 4 * w * h, 1, w, h, chroma, RNG, DEPTH, MAT, p, stream=s)

    for fmt, bps, tag in (("u8", 1, "8"), ("p010", 2, "16")):
        for to_rgb in (True, False):
            name = ("k_yuv%s_to_rgb" if to_rgb else "k_rgb_to_yuv%s") % tag
            moved = bps * samples + 12 * w * h
            ref = figure(lambda: rgb_end(fmt, to_rgb, C420), moved, ROTATE)
            kernels["%s %s centred" % (name, fmt)] = ref
            for label, chroma, halo in (("left", LEFT, 1.0 / 64), ("topleft", TOPLEFT, 1.0 / 64 + 1.0 / 32)):
                r = figure(lambda: rgb_end(fmt, to_rgb, chroma), moved, ROTATE)
                r["expectation"] = expect(r, ref, 0.0 if to_rgb else halo)
                kernels["%s_sited %s %s" % (name, fmt, label)] = r
            print(json.dumps({k: v for k, v in kernels.items() if k.startswith(name)}), flush=True)
    del sets, floats
    # the chroma kernels: both planes of a 960 x 540 chroma frame -> 1920 x 1080, one launch per plane on planar bytes, one launch for the P010 pair
    ocw, och = 2 * cw, 2 * ch
    csets = {fmt: [(side(w2xc, fmt, 1, w, h, cw, ch, rng), side(w2xc, fmt, 1, 2 * w, 2 * h, ocw, och)) for _ in range(ROTATE_C)] for fmt in ("u8", "p010")}

    def chroma(fmt, cosited):
        k = turn[0] % ROTATE_C
        turn[0] += 1
        (pi, _), (po, _) = csets[fmt][k]
        for src, dst in ((pi.u, po.u), (pi.v, po.v)):
            if fmt == "u8":
                w2xc.chroma2x_u8_sited_device(src, 1, 0, cw, 1, cw, ch, dst, 0, ocw, 1, ocw, och, cosited, stream=s)
            else:
                w2xc.chroma2x_u16_sited_device(src, 1, 0, pi.c_stride, pi.c_px, pi.pack, cw, ch, DEPTH, dst, 0, po.c_stride, po.c_px, po.pack, ocw, och, cosited, stream=s)

    for fmt, bps, tag in (("u8", 1, "8"), ("p010", 2, "16")):
        moved = 2 * bps * (cw * ch + ocw * och)
        ref = figure(lambda: chroma(fmt, 0), moved, ROTATE_C)
        kernels["k_chroma2x_u%s %s centred (two launches: U, V)" % (tag, fmt)] = ref
        for label, cosited in (("left", w2xc.CHROMA_COSITED_X), ("topleft", w2xc.CHROMA_COSITED_X | w2xc.CHROMA_COSITED_Y)):
            r = figure(lambda: chroma(fmt, cosited), moved, ROTATE_C)
            r["expectation"] = expect(r, ref)
            kernels["k_chroma2x_u%s_sited %s %s (two launches: U, V)" % (tag, fmt, label)] = r
    print(json.dumps({k: v for k, v in kernels.items() if "chroma" in k}), flush=True)
    res = {"tool": "tools/yuv_sited_bench.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "depth": DEPTH,
           "reference": "the other build's centred call" if a.other else "this build's centred call (no --other)", "frames": rows,
           "kernels_1080p_rotating": kernels, "all_ok": all(r["ok"] for r in rows)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f_:
        json.dump(res, f_, indent=1)
        f_.write("\n")
    print("all_ok", res["all_ok"])


if __name__ == "__main__":
    main()
