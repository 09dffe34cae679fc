#!/usr/bin/env python
"""tools/image_batch_bench.py -- per-image time of the image batch entry points against N single-image calls, in ONE process on ONE device, the two
forms alternating round by round (so both see the same clocks and the same box).

    python tools/image_batch_bench.py [--sizes 64,128,256,512,1024] [--ns 1,4,16,64] [--rounds 5] [--out profiles/image_batch_bench.json]

resident     uint8 images in HBM: N w2xc_process_image_u8_ex_device calls enqueued back to back on one stream, then one synchronisation, against
             one w2xc_process_image_u8_batch_device call + synchronisation
host         pageable numpy images, outputs preallocated: N w2xc_process_image_u8_ex calls against one w2xc_process_image_u8_batch call
modes        scale (one 2x iteration) and noise_scale (a noise pass, then one 2x iteration); the models are tools/gen_model.py's noise1 and scale2.0x
             (the default 7-layer fp32 chain)
Reported per source size, mode and N: the median over rounds of (wall time / N) in ms for both forms, the spread (max - min over rounds) of the
single-call figure, and `ok` = the batch median is not above the single-call median by more than that spread.  Every batch result is checked
byte-identical against the single calls once per configuration."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,256,512,1024")
    ap.add_argument("--ns", default="1,4,16,64")
    ap.add_argument("--modes", default="scale,noise_scale")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_batch_bench.json"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as graft
    from tools import gen_model
    w2xc = graft.load_package()
    lib = w2xc.lib()
    torch.cuda.set_device(0)
    mn = w2xc._ModelSet.from_layers(gen_model.synth_layers(seed=gen_model.SEEDS["noise1"]))
    msc = w2xc._ModelSet.from_layers(gen_model.synth_layers(seed=gen_model.SEEDS["scale2.0x"]))
    o = w2xc.make_opts(device=0)
    st = torch.cuda.current_stream()
    rows = []
    for s in [int(v) for v in a.sizes.split(",")]:
        S = 2 * s
        for mode in a.modes.split(","):
            noise = mn if "noise" in mode else None
            hn = noise.handle if noise else None
            for n in [int(v) for v in a.ns.split(",")]:
                x = np.random.default_rng(s + n).integers(0, 256, (n, s, s, 3), dtype=np.uint8)
                d_in = torch.from_numpy(x).cuda()
                d_single = torch.zeros((n, S, S, 3), dtype=torch.uint8, device="cuda")
                d_batch = torch.zeros_like(d_single)

                def singles():
                    for i in range(n):
                        rc = lib.w2xc_process_image_u8_ex_device(hn, msc.handle, C.c_void_p(d_in[i].data_ptr()), s * 3, s, s,
                                                                 C.c_void_p(d_single[i].data_ptr()), S * 3, 1, 0.0, C.c_void_p(st.cuda_stream), C.byref(o))
                        assert rc == 0, w2xc.last_error()
                    st.synchronize()

                def batched():
                    w2xc.process_image_u8_batch_device(n, d_in.data_ptr(), s * s * 3, s * 3, s, s, d_batch.data_ptr(), S * S * 3, S * 3, noise, msc, 1,
                                                       0.0, stream=st.cuda_stream, opts=o)
                    st.synchronize()

                # the host forms on the C entry points, outputs allocated and touched beforehand on both sides: what is timed is the library
                h_single = np.zeros((n, S, S, 3), np.uint8)
                h_batch = np.zeros_like(h_single)
                ip = (C.c_void_p * n)(*[x[i].ctypes.data for i in range(n)])
                op = (C.c_void_p * n)(*[h_batch[i].ctypes.data for i in range(n)])

                def host_singles():
                    for i in range(n):
                        rc = lib.w2xc_process_image_u8_ex(hn, msc.handle, ip[i], s * 3, s, s, h_single[i].ctypes.data, S * 3, 1, 0.0, None)
                        assert rc == 0, w2xc.last_error()

                def host_batch():
                    rc = lib.w2xc_process_image_u8_batch(hn, msc.handle, n, ip, s * 3, s, s, op, S * 3, 1, 0.0, None)
                    assert rc == 0, w2xc.last_error()

                def timed(f):
                    t0 = time.perf_counter()
                    f()
                    return (time.perf_counter() - t0) * 1e3 / n

                def ab(f_single, f_batch, rounds, key, row):
                    ts, tb = [], []
                    for _ in range(rounds):
                        ts.append(timed(f_single))
                        tb.append(timed(f_batch))
                    ms_s, ms_b, spread = statistics.median(ts), statistics.median(tb), max(ts) - min(ts)
                    row[key + "_single_ms"] = round(ms_s, 4)
                    row[key + "_single_spread_ms"] = round(spread, 4)
                    row[key + "_batch_ms"] = round(ms_b, 4)
                    row[key + "_speedup"] = round(ms_s / ms_b, 3)
                    row[key + "_ok"] = bool(ms_b <= ms_s + spread)
                singles(), batched()   # warm-up (workspace growth, weight packing)
                row = dict(size=s, mode=mode, n=n, out_mpix=S * S / 1e6, identical=bool(torch.equal(d_single, d_batch)))
                ab(singles, batched, a.rounds, "resident", row)
                if not a.no_host:
                    host_singles(), host_batch()
                    row["host_identical"] = bool(np.array_equal(h_single, h_batch) and np.array_equal(h_batch, d_batch.cpu().numpy()))
                    ab(host_singles, host_batch, max(3, a.rounds // 2 + 1), "host", row)
                rows.append(row)
                print(json.dumps(row), flush=True)
                del d_in, d_single, d_batch
        mn.trim(), msc.trim()   # (the next size starts from the memory a fresh process would have)
    res = dict(tool="tools/image_batch_bench.py", device=torch.cuda.get_device_name(0), rounds=a.rounds,
               models="noise1 / scale2.0x (tools/gen_model.py, 7 layers, fp32)", iterations=1,
               unit="ms per image (wall time of the whole call sequence / N)",
               all_identical=all(r["identical"] and r.get("host_identical", True) for r in rows),
               all_ok=all(r["resident_ok"] and r.get("host_ok", True) for r in rows), rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
