#!/usr/bin/env python
"""tools/upconv_rgba_bench.py -- the RGBA call for upconv head models (w2xc_process_image_rgba_u8_up2x_batch_device), timed in ONE process on ONE device, the
two sides of every comparison alternating window by window.  Scale model: the published upconv_7 topology 3-16-32-64-128-128-256-(head 3); noise model:
3-32-32-64-64-128-128-3; fp32, default options, one x2 iteration, the default bleed.  Inputs are resident RGBA images.

    python tools/upconv_rgba_bench.py [--n 16] [--rounds 7] [--out profiles/upconv_rgba_bench.json]

(a) the new call at n = 1 against the route a caller could compose before (include/w2xc_hip.h, "upconv head models", RGBA): w2xc_bleed_rgba_u8_device,
    w2xc_process_image_rgb_u8_ex_device on the bled image, torch for the grey image (A, A, A), w2xc_process_image_rgb_u8_ex_device on it without the noise
    model, torch for the merge of the colour bytes with channel 1 of that result.
(b) the new call at n images against n calls of it at n = 1.
Sizes 64^2, 256^2 and 1080 x 1920 source pixels, modes scale and noise_scale.  The bytes of the two sides must be equal.  `ok` = the new side's median is
not above the baseline's by more than the baseline's spread (max - min over rounds).  A timed window is `reps` calls enqueued back to back and one
synchronisation, reps chosen so that a window is >= ~30 ms.  Reported: the median over rounds of ms per image, each side's spread, the ratio."""
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
    ap.add_argument("--sizes", default="64x64,256x256,1080x1920")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upconv_rgba_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as graft
    from tools import gen_model
    w2xc = graft.load_package()
    if not torch.cuda.is_available() or w2xc.device_count() < 1:
        raise SystemExit("upconv_rgba_bench needs a HIP device (there is no CPU fallback to time)")
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
    for size in filter(None, a.sizes.split(",")):
        h, w = [int(v) for v in size.split("x")]
        H, W = 2 * h, 2 * w
        host = np.random.default_rng(1000 * h + w).integers(0, 256, (n, h, w, 4)).astype(np.uint8)
        host[:, h // 4:h // 2, w // 4:w // 2, 3] = 0          # a transparent block, an opaque one, partial values elsewhere
        host[:, h // 2:, : w // 3, 3] = 255
        d_in = torch.from_numpy(host).cuda()
        d_b, d_s = (torch.zeros((n, H, W, 4), dtype=torch.uint8, device="cuda") for _ in range(2))
        bled = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
        colour, ares = (torch.empty((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
        for mode in ("scale", "noise_scale"):
            (nb, sb), (ns, ss) = [(m[0] if mode == "noise_scale" else None, m[1]) for m in sets]
            P = ss.n_layers + (ns.n_layers if ns else 0)

            def call(dst, i0, cnt, mn=nb, ms=sb):
                w2xc.process_image_rgba_u8_up2x_batch_device(cnt, d_in[i0].data_ptr(), h * w * 4, w * 4, w, h, dst[i0].data_ptr(), H * W * 4, W * 4, mn, ms, 1, 0.0,
                                                             -1, stream=s, opts=o)

            def new_one():
                call(d_b, 0, 1)

            def composed_one():
                w2xc.bleed_rgba_u8_device(d_in[0].data_ptr(), w * 4, w, h, P, bled.data_ptr(), w * 3, stream=s)
                w2xc.process_image_rgb_u8_device(bled.data_ptr(), w * 3, w, h, colour.data_ptr(), W * 3, ns, ss, 1, 0.0, stream=s, opts=o)
                grey = d_in[0, :, :, 3:4].expand(h, w, 3).contiguous()
                w2xc.process_image_rgb_u8_device(grey.data_ptr(), w * 3, w, h, ares.data_ptr(), W * 3, None, ss, 1, 0.0, stream=s, opts=o)
                d_s[0, :, :, :3] = colour
                d_s[0, :, :, 3] = ares[:, :, 1]

            def batch():
                call(d_b, 0, n)

            def singles():
                for i in range(n):
                    call(d_s, i, 1, ns, ss)

            for part, per, new, old, eq in (("a", 1, new_one, composed_one, lambda: bool(torch.equal(d_b[0], d_s[0]))),
                                            ("b", n, batch, singles, lambda: bool(torch.equal(d_b, d_s)))):
                m_n, s_n, m_o, s_o, reps = compare(new, old, per)
                row = dict(part=part, mode=mode, size="%dx%d" % (h, w), n=per, reps=reps, new_ms=round(m_n, 4), new_spread_ms=round(s_n, 4),
                           baseline="composed route" if part == "a" else "%d calls at n = 1" % n, baseline_ms=round(m_o, 4), baseline_spread_ms=round(s_o, 4),
                           speedup=round(m_o / m_n, 3), equal=eq(), ok=bool(m_n <= m_o + s_o))
                rows.append(row)
                print(json.dumps(row), flush=True)
        del d_in, d_b, d_s, bled, colour, ares
        for pair in sets:
            for ms in pair:
                ms.trim()
    res = dict(tool="tools/upconv_rgba_bench.py", device=torch.cuda.get_device_name(0), rounds=a.rounds, n=n,
               model="scale 3-16-32-64-128-128-256-(head 3), seed %d; noise 3-32-32-64-64-128-128-3, seed 301" % gen_model.SEEDS["upconv7"],
               options="fp32, default options, 1 iteration, default bleed passes, resident RGBA images",
               unit="ms per image: a window of `reps` calls + one synchronisation, / reps (/ n); median over rounds; spread = max - min",
               all_equal=all(r["equal"] for r in rows), all_ok=all(r["ok"] for r in rows), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
