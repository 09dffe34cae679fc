#!/usr/bin/env python
"""tools/batch_bench.py -- per-plane time of the batch entry points against N single-plane calls, in ONE process on ONE device, the two forms
alternating round by round (so both see the same clocks and the same box).

    python tools/batch_bench.py [--sizes 128,256,512] [--ns 1,4,16,64] [--rounds 5] [--out profiles/batch_bench.json]

resident     planes in HBM: N w2xc_convert_plane[_nn2x]_device calls enqueued back to back on one stream, then one synchronisation, against one
             w2xc_convert_batch_device call + synchronisation
host         pageable numpy planes: N w2xc_convert_plane[_nn2x] calls against one w2xc_convert_batch call
Reported: the median over rounds of (wall time / N) in ms, per source size, nn2x and N; the model is tools/gen_model.py's noise1 (the default 7-layer
fp32 chain).  Every batch result is checked bit-identical against the single calls once per configuration."""
import argparse
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
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--ns", default="1,4,16,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_bench.json"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as graft
    from tools import gen_model
    w2xc = graft.load_package()
    torch.cuda.set_device(0)
    ms = w2xc._ModelSet.from_layers(gen_model.synth_layers(seed=gen_model.SEEDS["noise1"]))
    o = w2xc.make_opts(device=0)
    st = torch.cuda.current_stream()
    rows = []
    for s in [int(v) for v in a.sizes.split(",")]:
        for up in (0, 1):
            S = s << up
            for n in [int(v) for v in a.ns.split(",")]:
                x = np.random.default_rng(s + n + up).random((n, s, s), dtype=np.float32)
                d_in = torch.from_numpy(x).cuda()
                d_single = torch.empty((n, S, S), dtype=torch.float32, device="cuda")
                d_batch = torch.empty_like(d_single)
                conv = ms.convert_nn2x_device if up else ms.convert_device

                def singles():
                    for i in range(n):
                        conv(d_in[i].data_ptr(), s * 4, s, s, d_single[i].data_ptr(), S * 4, stream=st.cuda_stream, opts=o)
                    st.synchronize()

                def batched():
                    ms.convert_batch_device(n, d_in.data_ptr(), s * s * 4, s * 4, s, s, d_batch.data_ptr(), S * S * 4, S * 4, nn2x=bool(up),
                                            stream=st.cuda_stream, opts=o)
                    st.synchronize()

                def host_singles():
                    f = ms.convert_nn2x if up else ms.convert
                    return [f(x[i]) for i in range(n)]

                def host_batch():
                    return ms.convert_batch(x, nn2x=bool(up))

                def timed(f):
                    t0 = time.perf_counter()
                    f()
                    return (time.perf_counter() - t0) * 1e3 / n
                singles(), batched()   # warm-up (workspace growth, weight packing)
                identical = bool(torch.equal(d_single, d_batch))
                ts, tb = [], []
                for _ in range(a.rounds):
                    ts.append(timed(singles))
                    tb.append(timed(batched))
                row = dict(size=s, nn2x=up, n=n, out_mpix=S * S / 1e6, identical=identical,
                           resident_single_ms=round(statistics.median(ts), 4), resident_batch_ms=round(statistics.median(tb), 4))
                row["resident_speedup"] = round(row["resident_single_ms"] / row["resident_batch_ms"], 3)
                row["resident_batch_mpix_s"] = round(S * S / 1e3 / row["resident_batch_ms"], 1)
                if not a.no_host:
                    hs, hb = host_singles(), host_batch()
                    row["host_identical"] = bool(all(np.array_equal(hs[i], hb[i]) for i in range(n)))
                    ths, thb = [], []
                    for _ in range(max(2, a.rounds // 2)):
                        ths.append(timed(host_singles))
                        thb.append(timed(host_batch))
                    row["host_single_ms"] = round(statistics.median(ths), 4)
                    row["host_batch_ms"] = round(statistics.median(thb), 4)
                    row["host_speedup"] = round(row["host_single_ms"] / row["host_batch_ms"], 3)
                rows.append(row)
                print(json.dumps(row), flush=True)
                del d_in, d_single, d_batch
    res = dict(tool="tools/batch_bench.py", device=torch.cuda.get_device_name(0), rounds=a.rounds, model="noise1 (tools/gen_model.py, 7 layers, fp32)",
               unit="ms per plane (wall time of the whole call sequence / N)", rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
