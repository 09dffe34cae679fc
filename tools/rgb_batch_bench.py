#!/usr/bin/env python
"""tools/rgb_batch_bench.py -- the batched chain of RGB models, timed in ONE process on ONE device, the two sides of every comparison alternating window by
window.  Model: 3-32-32-64-64-128-128-3, fp32, default options, one x2 iteration.

    python tools/rgb_batch_bench.py [--parent-lib PATH] [--n 16] [--rounds 7] [--out profiles/rgb_batch_bench.json]

(a) w2xc_process_image_rgb_u8_batch[_device] on n images against n calls of w2xc_process_image_rgb_u8_ex[_device], resident in HBM on both ends (device
    forms, one stream) and from pageable host memory (host forms), at 64^2, 128^2, 256^2 and 512^2 source pixels, modes scale and noise_scale.  The bytes
    must be equal.  `ok` = the batch's median is not above the singles' by more than the singles' spread (max - min over rounds).
(b) the TTA call (w2xc_process_image_rgb_u8_tta_device) on one resident 64^2 and one 256^2 image, this tree's library against the parent commit's
    (--parent-lib, loaded with ctypes beside the tree's; without it (b) is skipped).  The bytes must be equal.  `ok` = this tree's median is not above the
    parent's by more than the parent's spread.

A timed window is `reps` calls (of the batch, or of the n singles) enqueued back to back and one synchronisation, reps chosen so that a window is >= ~30 ms.
Reported: the median over rounds of ms per image, each side's spread, the ratio; and w2xc_batch_plan's answer for every size."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOPO = [3, 32, 32, 64, 64, 128, 128, 3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libw2xc_hip.so of the parent commit, for (b)")
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="64x64,128x128,256x256,512x512")
    ap.add_argument("--tta-sizes", default="64x64,256x256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgb_batch_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as graft
    from tools import gen_model
    w2xc = graft.load_package()
    if not torch.cuda.is_available() or w2xc.device_count() < 1:
        raise SystemExit("rgb_batch_bench needs a HIP device (there is no CPU fallback to time)")
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

    layers = (gen_model.synth_layers(TOPO, 301), gen_model.synth_layers(TOPO, 302))
    rows = []
    # ---- (a) the batch against n single calls (a context each: each side keeps its own workspaces) ----
    sets = [(w2xc._ModelSet.from_layers(layers[0]), w2xc._ModelSet.from_layers(layers[1])) for _ in range(2)]
    for size in filter(None, a.sizes.split(",")):   # (--sizes "": part (b) alone)
        h, w = [int(v) for v in size.split("x")]
        H, W = 2 * h, 2 * w
        host = np.random.default_rng(1000 * h + w).integers(0, 256, (n, h, w, 3)).astype(np.uint8)
        d_in = torch.from_numpy(host).cuda()
        d_b, d_s = (torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
        h_b, h_s = (np.zeros((n, H, W, 3), np.uint8) for _ in range(2))
        plan = dict(noise=sets[0][0].batch_plan(3, w, h, False, o), scale=sets[0][1].batch_plan(3, w, h, True, o))
        for mode in ("scale", "noise_scale"):
            (nb, sb), (ns, ss) = [(m[0] if mode == "noise_scale" else None, m[1]) for m in sets]

            def batch_dev():
                w2xc.process_image_rgb_u8_batch_device(n, d_in.data_ptr(), h * w * 3, w * 3, w, h, d_b.data_ptr(), H * W * 3, W * 3, nb, sb, 1, 0.0, stream=s, opts=o)

            def singles_dev():
                for i in range(n):
                    w2xc.process_image_rgb_u8_device(d_in[i].data_ptr(), w * 3, w, h, d_s[i].data_ptr(), W * 3, ns, ss, 1, 0.0, stream=s, opts=o)

            def batch_host():
                w2xc.process_image_rgb_u8_batch(host, nb, sb, 1, o, 0.0, out=h_b)

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

    # ---- (b) the TTA call against the parent commit's library ----
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        vp, ci, cs = C.c_void_p, C.c_int, C.c_size_t
        parent.w2xc_model_from_arrays.restype = ci
        parent.w2xc_model_from_arrays.argtypes = [ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        sig = [vp, vp, vp, cs, ci, ci, vp, cs, ci, C.c_double, vp, C.POINTER(w2xc.Opts), ci]
        funcs = {"tree": w2xc.lib().w2xc_process_image_rgb_u8_tta_device, "parent": parent.w2xc_process_image_rgb_u8_tta_device}
        for f in funcs.values():
            f.restype, f.argtypes = ci, sig
        nl = len(layers[1])
        keep = [np.ascontiguousarray(l[2], dtype=np.float32) for l in layers[1]], [np.ascontiguousarray(l[3], dtype=np.float64) for l in layers[1]]
        ph = vp()
        rc = parent.w2xc_model_from_arrays(nl, (ci * nl)(*[l[0] for l in layers[1]]), (ci * nl)(*[l[1] for l in layers[1]]),
                                           (vp * nl)(*[x.ctypes.data for x in keep[0]]), (vp * nl)(*[x.ctypes.data for x in keep[1]]), C.byref(ph))
        assert rc == 0, rc
        handles = {"tree": sets[0][1].handle, "parent": ph}
        for size in a.tta_sizes.split(","):
            h, w = [int(v) for v in size.split("x")]
            d_in = torch.from_numpy(np.random.default_rng(7 * h + w).integers(0, 256, (h, w, 3)).astype(np.uint8)).cuda()
            outs = {k: torch.zeros((2 * h, 2 * w, 3), dtype=torch.uint8, device="cuda") for k in funcs}

            def run(k):
                rc = funcs[k](None, handles[k], d_in.data_ptr(), w * 3, w, h, outs[k].data_ptr(), 2 * w * 3, 1, 0.0, s, C.byref(o), 1)
                assert rc == 0, (k, rc)
            m_n, s_n, m_o, s_o, reps = compare(lambda: run("tree"), lambda: run("parent"), 1)
            row = dict(part="b", size="%dx%d" % (h, w), reps=reps, tree_ms=round(m_n, 4), tree_spread_ms=round(s_n, 4), parent_ms=round(m_o, 4),
                       parent_spread_ms=round(s_o, 4), speedup=round(m_o / m_n, 3), equal=bool(torch.equal(outs["tree"], outs["parent"])), ok=bool(m_n <= m_o + s_o),
                       batch_plan=sets[0][1].batch_plan(3, w, h, True, o))
            rows.append(row)
            print(json.dumps(row), flush=True)
    res = dict(tool="tools/rgb_batch_bench.py", device=torch.cuda.get_device_name(0), rounds=a.rounds, n=n, model="3-32-32-64-64-128-128-3, seeds 301 / 302",
               options="fp32, default options, 1 iteration",
               unit="(a) ms per image, (b) ms per call: a window of `reps` calls + one synchronisation, / reps; median over rounds; spread = max - min",
               all_equal=all(r["equal"] for r in rows), all_ok=all(r["ok"] for r in rows), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
