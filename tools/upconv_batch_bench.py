#!/usr/bin/env python
"""tools/upconv_batch_bench.py -- the batch and TTA forms of upconv head models, timed in ONE process on ONE device, the two sides of every comparison
alternating window by window.  Scale model: the published upconv_7 topology 3-16-32-64-128-128-256-(head 3); noise model: 3-32-32-64-64-128-128-3; fp32,
default options, one x2 iteration.

    python tools/upconv_batch_bench.py [--n 16] [--rounds 7] [--out profiles/upconv_batch_bench.json]

(a) w2xc_process_image_rgb_u8_up2x_batch[_device] on n images against n calls of w2xc_process_image_rgb_u8_ex[_device], resident in HBM on both ends
    (device forms, one stream) and from pageable host memory (host forms), at 64^2, 128^2, 256^2 and 512^2 source pixels, modes scale and noise_scale.
(b) the TTA form (w2xc_process_image_rgb_u8_up2x_batch_device, n = 1, tta = 1) on one resident 64^2 and one 256^2 image against the route a caller could
    compose before: w2xc_u8_to_rgb_device, w2xc_tta_spread_device, w2xc_convert_planes_up2x_device on each of the 8 variants, w2xc_tta_gather_device,
    w2xc_rgb_to_u8_device.
The bytes of the two sides must be equal.  `ok` = the new call's median is not above the baseline's by more than the baseline's spread (max - min over
rounds).  A timed window is `reps` calls (of the batch, or of the n singles) enqueued back to back and one synchronisation, reps chosen so that a window
is >= ~30 ms.  Reported: the median over rounds of ms per image, each side's spread, the ratio; and w2xc_batch_plan's answer for every size."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NOISE_TOPO = [3, 32, 32, 64, 64, 128, 128, 3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="64x64,128x128,256x256,512x512")
    ap.add_argument("--tta-sizes", default="64x64,256x256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upconv_batch_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as graft
    from tools import gen_model
    w2xc = graft.load_package()
    if not torch.cuda.is_available() or w2xc.device_count() < 1:
        raise SystemExit("upconv_batch_bench needs a HIP device (there is no CPU fallback to time)")
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

    noise_layers = gen_model.synth_layers(NOISE_TOPO, 301)
    head_layers = gen_model.synth_layers(gen_model.TOPOLOGY_UPCONV7, gen_model.SEEDS["upconv7"])
    head = gen_model.synth_head(gen_model.TOPOLOGY_UPCONV7[-1], 3, gen_model.SEEDS["upconv7"], True)
    # (a context each: each side keeps its own workspaces)
    sets = [(w2xc._ModelSet.from_layers(noise_layers), w2xc._ModelSet.from_layers(head_layers, head=head)) for _ in range(2)]
    rows = []
    # ---- (a) the batch against n single calls ----
    for size in filter(None, a.sizes.split(",")):   # (--sizes "": part (b) alone)
        h, w = [int(v) for v in size.split("x")]
        H, W = 2 * h, 2 * w
        host = np.random.default_rng(1000 * h + w).integers(0, 256, (n, h, w, 3)).astype(np.uint8)
        d_in = torch.from_numpy(host).cuda()
        d_b, d_s = (torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
        h_b, h_s = (np.zeros((n, H, W, 3), np.uint8) for _ in range(2))
        plan = dict(noise=sets[0][0].batch_plan(3, w, h, False, o), scale=sets[0][1].batch_plan(3, w, h, opts=o, up2x=True))
        for mode in ("scale", "noise_scale"):
            (nb, sb), (ns, ss) = [(m[0] if mode == "noise_scale" else None, m[1]) for m in sets]

            def batch_dev():
                w2xc.process_image_rgb_u8_up2x_batch_device(n, d_in.data_ptr(), h * w * 3, w * 3, w, h, d_b.data_ptr(), H * W * 3, W * 3, nb, sb, 1, 0.0, stream=s, opts=o)

            def singles_dev():
                for i in range(n):
                    w2xc.process_image_rgb_u8_device(d_in[i].data_ptr(), w * 3, w, h, d_s[i].data_ptr(), W * 3, ns, ss, 1, 0.0, stream=s, opts=o)

            def batch_host():
                w2xc.process_image_rgb_u8_up2x_batch(host, nb, sb, 1, o, 0.0, out=h_b)

            def singles_host():
                for i in range(n):
                    h_s[i] = w2xc.process_image_rgb_u8(host[i], ns, ss, 1, o, 0.0)

            for where, new, old, eq in (("resident", batch_dev, singles_dev, lambda: bool(torch.equal(d_b, d_s))),
                                        ("host", batch_host, singles_host, lambda: bool(np.array_equal(h_b, h_s)))):
                m_n, s_n, m_o, s_o, reps = compare(new, old, n)
                row = dict(part="a", mode=mode, size="%dx%d" % (h, w), where=where, n=n, reps=reps, batch_ms=round(m_n, 4), batch_spread_ms=round(s_n, 4),
                           singles_ms=round(m_o, 4), singles_spread_ms=round(s_o, 4), speedup=round(m_o / m_n, 3), equal=eq(), ok=bool(m_n <= m_o + s_o),
                           batch_plan=plan)
                rows.append(row)
                print(json.dumps(row), flush=True)
        del d_in, d_b, d_s
        for pair in sets:
            for ms in pair:
                ms.trim()

    # ---- (b) the TTA form against the composed route ----
    for size in filter(None, a.tta_sizes.split(",")):
        h, w = [int(v) for v in size.split("x")]
        ps, PS = h * w, 4 * h * w
        d_img = torch.from_numpy(np.random.default_rng(7 * h + w).integers(0, 256, (h, w, 3)).astype(np.uint8)).cuda()
        d_new, d_old = (torch.zeros((2 * h, 2 * w, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
        d_x = torch.empty((3, h, w), dtype=torch.float32, device="cuda")
        v_in = torch.empty((2, 12 * ps), dtype=torch.float32, device="cuda")     # the upright group, the transposed group
        v_out = torch.empty((2, 12 * PS), dtype=torch.float32, device="cuda")
        d_y = torch.empty((3, 2 * h, 2 * w), dtype=torch.float32, device="cuda")
        new_ms, old_ms = sets[0][1], sets[1][1]

        def tta_new():
            w2xc.process_image_rgb_u8_up2x_batch_device(1, d_img.data_ptr(), h * w * 3, w * 3, w, h, d_new.data_ptr(), 12 * h * w, 2 * w * 3, None, new_ms, 1, 0.0,
                                                        stream=s, opts=o, tta=True)

        def tta_composed():
            w2xc.u8_to_rgb_device(d_img.data_ptr(), w * 3, w, h, d_x.data_ptr(), s)
            w2xc.tta_spread_device(d_x.data_ptr(), 3, ps * 4, w * 4, w, h, v_in[0].data_ptr(), v_in[1].data_ptr(), ps * 4, s)
            for k in range(8):
                g, vw, vh = k >> 2, (h if k & 4 else w), (w if k & 4 else h)
                old_ms.convert_planes_up2x_device(3, v_in[g].data_ptr() + (k & 3) * 3 * ps * 4, ps * 4, vw * 4, vw, vh, v_out[g].data_ptr() + (k & 3) * 3 * PS * 4,
                                                  PS * 4, 2 * vw * 4, stream=s, opts=o)
            w2xc.tta_gather_device(v_out[0].data_ptr(), v_out[1].data_ptr(), PS * 4, 3, 2 * w, 2 * h, d_y.data_ptr(), PS * 4, 2 * w * 4, s)
            w2xc.rgb_to_u8_device(d_y.data_ptr(), 2 * w, 2 * h, d_old.data_ptr(), 2 * w * 3, s)

        m_n, s_n, m_o, s_o, reps = compare(tta_new, tta_composed, 1)
        row = dict(part="b", size="%dx%d" % (h, w), reps=reps, tta_ms=round(m_n, 4), tta_spread_ms=round(s_n, 4), composed_ms=round(m_o, 4),
                   composed_spread_ms=round(s_o, 4), speedup=round(m_o / m_n, 3), equal=bool(torch.equal(d_new, d_old)), ok=bool(m_n <= m_o + s_o),
                   batch_plan=new_ms.batch_plan(3, w, h, opts=o, up2x=True))
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = dict(tool="tools/upconv_batch_bench.py", device=torch.cuda.get_device_name(0), rounds=a.rounds, n=n,
               model="scale 3-16-32-64-128-128-256-(head 3), seed %d; noise 3-32-32-64-64-128-128-3, seed 301" % gen_model.SEEDS["upconv7"],
               options="fp32, default options, 1 iteration",
               unit="(a) ms per image, (b) ms per call: a window of `reps` calls + one synchronisation, / reps; median over rounds; spread = max - min",
               all_equal=all(r["equal"] for r in rows), all_ok=all(r["ok"] for r in rows), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
