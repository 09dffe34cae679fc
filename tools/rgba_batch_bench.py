#!/usr/bin/env python
"""tools/rgba_batch_bench.py -- the batch forms of the RGBA call and the one-launch tiled colour bleed, timed in ONE process on ONE device, the two sides of
every comparison alternating window by window.

    python tools/rgba_batch_bench.py [--parent-lib PATH] [--n 16] [--rounds 7] [--out profiles/rgba_batch_bench.json]

(a) w2xc_process_image_rgba_u8_batch[_device] on n images against n calls of w2xc_process_image_rgba_u8_ex[_device], resident in HBM on both ends (device
    forms, one stream) and from pageable host memory (host forms), at 64^2, 128^2, 256^2 and 512^2 source pixels, for a Y model pair and an RGB model pair,
    modes scale (x2) and noise_scale (x2), fp32, default options, automatic bleed passes.  The bytes must be equal.  `ok` = the batch's median is not above the
    singles' by more than the singles' spread (max - min over rounds).
(b) w2xc_bleed_rgba_u8_device of this tree against the same symbol of the parent commit's library (--parent-lib, loaded with ctypes beside the tree's; without
    it (b) is skipped), P in {1, 7, 14} passes at 64^2, 128^2, 256^2, 512^2 and 1080 x 1920.  The bytes must be equal.  `ok` = this tree's median is not above the parent's
    by more than the parent's spread.

Images: random colour bytes; alpha 255 inside a centred ellipse that covers about half the image, a 9-pixel ramp of partial alpha around it, 0 outside -- a
sprite on a transparent ground.  A timed window is `reps` calls (of the batch, or of the n singles) enqueued back to back and one synchronisation, reps
chosen so that a window is >= ~30 ms.  Reported: the median over rounds of ms per image (a) / ms per call (b), each side's spread, the ratio."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sprite(np, h, w, seed):
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 4)).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    r = np.hypot((yy - h / 2 + 0.5) / (0.4 * h), (xx - w / 2 + 0.5) / (0.4 * w))      # 1 on the ellipse: pi * 0.16 = half the area
    edge = 9.0 / (0.4 * min(h, w))
    img[:, :, 3] = np.clip(np.rint(255 * (1 + (1 - r) / edge)), 0, 255).astype(np.uint8)
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libw2xc_hip.so of the parent commit, for (b)")
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="64x64,128x128,256x256,512x512")
    ap.add_argument("--bleed-sizes", default="64x64,128x128,256x256,512x512,1080x1920")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgba_batch_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as graft
    from tools import gen_model
    w2xc = graft.load_package()
    if not torch.cuda.is_available() or w2xc.device_count() < 1:
        raise SystemExit("rgba_batch_bench needs a HIP device (there is no CPU fallback to time)")
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

    # ---- (a) the batch against n single calls ----
    y7 = [1, 32, 32, 64, 64, 128, 128, 1]
    kinds = {"y": (gen_model.synth_layers(y7, gen_model.SEEDS["noise1"]), gen_model.synth_layers(y7, gen_model.SEEDS["scale2.0x"])),
             "rgb": (gen_model.synth_layers([3, 32, 32, 64, 64, 128, 128, 3], 301), gen_model.synth_layers([3, 32, 32, 64, 64, 128, 128, 3], 302))}
    rows = []
    for kind, (ln, ls) in kinds.items():
        # (a context each for the batch and for the singles: each side keeps its own workspaces)
        sets = [(w2xc._ModelSet.from_layers(ln), w2xc._ModelSet.from_layers(ls)) for _ in range(2)]
        for size in filter(None, a.sizes.split(",")):   # (--sizes "": part (b) alone)
            h, w = [int(v) for v in size.split("x")]
            H, W = 2 * h, 2 * w
            host = np.stack([sprite(np, h, w, 1000 * h + i) for i in range(n)])
            d_in = torch.from_numpy(host).cuda()
            d_b, d_s = (torch.zeros((n, H, W, 4), dtype=torch.uint8, device="cuda") for _ in range(2))
            h_b, h_s = (np.zeros((n, H, W, 4), np.uint8) for _ in range(2))
            for mode in ("scale", "noise_scale"):
                (nb, sb), (ns, ss) = [(m[0] if mode == "noise_scale" else None, m[1]) for m in sets]

                def batch_dev():
                    w2xc.process_image_rgba_u8_batch_device(n, d_in.data_ptr(), h * w * 4, w * 4, w, h, d_b.data_ptr(), H * W * 4, W * 4, nb, sb, 1, 0.0, -1,
                                                            stream=s, opts=o)

                def singles_dev():
                    for i in range(n):
                        w2xc.process_image_rgba_u8_device(d_in[i].data_ptr(), w * 4, w, h, d_s[i].data_ptr(), W * 4, ns, ss, 1, 0.0, -1, stream=s, opts=o)

                def batch_host():
                    w2xc.process_image_rgba_u8_batch(host, nb, sb, 1, o, 0.0, -1, out=h_b)

                def singles_host():
                    for i in range(n):
                        h_s[i] = w2xc.process_image_rgba_u8(host[i], ns, ss, 1, o, 0.0, -1)

                for where, new, old, eq in (("resident", batch_dev, singles_dev, lambda: bool(torch.equal(d_b, d_s))),
                                            ("host", batch_host, singles_host, lambda: bool(np.array_equal(h_b, h_s)))):
                    m_n, s_n, m_o, s_o, reps = compare(new, old, n)
                    row = dict(part="a", model=kind, mode=mode, size="%dx%d" % (h, w), where=where, n=n, reps=reps, batch_ms=round(m_n, 4),
                               batch_spread_ms=round(s_n, 4), singles_ms=round(m_o, 4), singles_spread_ms=round(s_o, 4), speedup=round(m_o / m_n, 3),
                               equal=eq(), ok=bool(m_n <= m_o + s_o))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
            del d_in, d_b, d_s
            for pair in sets:
                for ms in pair:
                    ms.trim()

    # ---- (b) the bleed against the parent commit's library ----
    if a.parent_lib:
        sig = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        libs = {"tree": w2xc.lib().w2xc_bleed_rgba_u8_device, "parent": C.CDLL(os.path.abspath(a.parent_lib)).w2xc_bleed_rgba_u8_device}
        for f in libs.values():
            f.restype, f.argtypes = C.c_int, sig
        for size in a.bleed_sizes.split(","):
            h, w = [int(v) for v in size.split("x")]
            d_in = torch.from_numpy(sprite(np, h, w, 7 * h + w)).cuda()
            outs = {k: torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for k in libs}
            for P in (1, 7, 14):
                def run(k):
                    rc = libs[k](d_in.data_ptr(), w * 4, w, h, P, outs[k].data_ptr(), w * 3, s)
                    assert rc == 0, (k, rc)
                m_n, s_n, m_o, s_o, reps = compare(lambda: run("tree"), lambda: run("parent"), 1)
                row = dict(part="b", size="%dx%d" % (h, w), passes=P, reps=reps, tree_ms=round(m_n, 5), tree_spread_ms=round(s_n, 5), parent_ms=round(m_o, 5),
                           parent_spread_ms=round(s_o, 5), speedup=round(m_o / m_n, 3), equal=bool(torch.equal(outs["tree"], outs["parent"])),
                           ok=bool(m_n <= m_o + s_o))
                rows.append(row)
                print(json.dumps(row), flush=True)
    res = dict(tool="tools/rgba_batch_bench.py", device=torch.cuda.get_device_name(0), rounds=a.rounds, n=n,
               models=dict(y="1-32-32-64-64-128-128-1 noise1 / scale2.0x seeds of tools/gen_model.py", rgb="3-32-32-64-64-128-128-3, seeds 301 / 302"),
               options="fp32, default options, 1 iteration, bleed_passes = -1 (7 for scale, 14 for noise_scale)",
               unit="(a) ms per image, (b) ms per call: a window of `reps` calls + one synchronisation, / reps; median over rounds; spread = max - min",
               all_equal=all(r["equal"] for r in rows), all_ok=all(r["ok"] for r in rows), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
