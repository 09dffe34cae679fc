"""The failure paths: calls that fail AFTER they have touched the device, by w2xc_debug_fail_nth (include/w2xc_hip.h) -- an allocation, a weight upload or a
layer launch fails on the host, in place of the runtime call; nothing faulty reaches the device, nothing is exhausted.  tests/test_gpu_fail_paths.py runs
the resident cases in its own process and the host-route groups below in children (`python tests/fail_cases.py <group>`: one line per k, exit status 0 only
if every k passed), so that a feeder or drainer that does not join fails the test at its time limit and does not stall the suite.

ONE loop serves every case, fail_loop:
  1. the expected result: the call on an untouched set of models built from the same arrays, and the scratch bytes that set holds afterwards;
  2. the models under test go cold for the kind in hand -- scratch growth: a warm call, then w2xc_model_trim; weight events: new models --
  3. and the call's events E are counted between two calls with nth = 0;
  4. for every k in 1 .. E: cold again, arm k, call.  The call returns the documented code (W2XC_ERR_NOMEM for ALLOC, W2XC_ERR_HIP for COPY and LAUNCH), the
     message is there (ALLOC: it names the buffer), the seam has seen its k-th event and so disarmed itself, nothing outside the outputs was written (their
     interior is unspecified), THE SAME CALL MADE AGAIN RETURNS OK WITH THE EXPECTED BITS, and the scratch bytes are those of the untouched models: no buffer
     was lost or doubled;
  5. E >= 1 (or the case's own minimum), else the loop would have tested nothing.
A case is a function that makes a Run: the models of one call and the call itself."""
import ctypes as C
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import stream_cases as sc  # noqa: E402
from tools import gen_model  # noqa: E402

ALLOC, COPY, LAUNCH = 1, 2, 3
KIND = {ALLOC: "ALLOC", COPY: "COPY", LAUNCH: "LAUNCH"}
# every `what` of a Scratch::reserve (waifu2x-converter-cpp_amd/csrc) and upload's
BUFFERS = ("the activation workspace", "the gather-job counters", "the input rows", "the output rows", "the input staging ring", "the output staging ring",
           "the band buffer", "the job flags", "Model::filter planes", "the Model::filter bounce ring", "the image planes", "the RGBA images and their planes",
           "the bleed's pass stamps", "the frames", "the image", "a weight image")
NAMED = re.compile(r"memory for (.+) failed")

PRODUCT = lambda: gen_model.synth_layers(seed=gen_model.SEEDS["noise1"])        # noqa: E731  [1, 32, 32, 64, 64, 128, 128, 1]: the shipped topology
SCALE = lambda: gen_model.synth_layers(seed=gen_model.SEEDS["scale2.0x"])       # noqa: E731


def rand_plane(h, w, seed):
    return np.random.default_rng(seed).random((h, w), dtype=np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want):
    return len(got) == len(want) and all(g.shape == w_.shape and g.dtype == w_.dtype and np.array_equal(bits(g), bits(w_)) for g, w_ in zip(got, want))


class Run:
    """the models of one call and the call: call() -> the outputs (numpy arrays, rims checked; raises W2xcError), rims() -> after a failed call: nothing
    outside the outputs was written, no input either"""
    models = ()

    def call(self):
        raise NotImplementedError

    def rims(self):
        pass

    def scratch_bytes(self):
        return [m.fill_scratch(0, 0) for m in self.models]

    def trim(self):
        for m in self.models:
            m.trim()


class StreamRun(Run):
    """a row of tests/stream_cases.py at its own shape, on the null stream with a device sync on either side; new models with every instance"""

    def __init__(self, w, torch, row):
        self.torch = torch
        ctx = sc.Ctx(w, torch)
        self.case = row.build(ctx, 0)
        self.models = [ctx._models[k] for k in sorted(ctx._models)]

    def call(self):
        for buf, real, _ in self.case.ins:
            buf.copy_(real)
        for buf, fill, _ in self.case.outs:
            buf.copy_(fill)
        self.torch.cuda.synchronize()
        try:
            self.case.call(0)
        finally:
            self.torch.cuda.synchronize()
        return [check(buf.cpu().numpy()) if check else buf.cpu().numpy() for buf, _, check in self.case.outs]

    def rims(self):
        for buf, _, check in self.case.outs:
            if check:
                check(buf.cpu().numpy())
        for buf, real, _ in self.case.ins:
            assert self.torch.equal(buf.view(self.torch.uint8), real.view(self.torch.uint8)), "an input buffer was written"


class PlaneRun(Run):
    """w2xc_convert_plane_device (n = None) or w2xc_convert_batch_device on planes resident in a NaN buffer with rims (stream_cases.FLay)"""

    def __init__(self, w, torch, layers, x, **okw):
        self.w, self.torch = w, torch
        self.models = [w._ModelSet.from_layers(layers())]
        self.x = np.ascontiguousarray(x, np.float32)
        self.lay = sc.FLay(self.x.shape)
        self.d_in = torch.from_numpy(self.lay.scatter(self.x)).cuda()
        self.fill = torch.full((self.lay.total,), float("nan"), dtype=torch.float32, device="cuda")
        self.d_out = self.fill.clone()
        self.o = w.make_opts(device=0, **okw)

    def call(self):
        ms, lay, torch = self.models[0], self.lay, self.torch
        self.d_out.copy_(self.fill)
        torch.cuda.synchronize()
        pi, po = self.d_in.data_ptr() + 4 * sc.RIM_F, self.d_out.data_ptr() + 4 * sc.RIM_F
        try:
            if self.x.ndim == 2:
                h, w_ = self.x.shape
                ms.convert_device(pi, lay.bytes(0), w_, h, po, lay.bytes(0), stream=0, opts=self.o)
            else:
                n, h, w_ = self.x.shape
                ms.convert_batch_device(n, pi, lay.bytes(0), lay.bytes(1), w_, h, po, lay.bytes(0), lay.bytes(1), stream=0, opts=self.o)
        finally:
            torch.cuda.synchronize()
        return [lay.gather(self.d_out.cpu().numpy())]

    def rims(self):
        self.lay.gather(self.d_out.cpu().numpy())
        assert np.array_equal(bits(self.lay.gather(self.d_in.cpu().numpy())), bits(self.x)), "the input planes were written"


RIM_ROWS, RIM_COLS = 2, 8


class HostRun(Run):
    """w2xc_convert_plane / _nn2x on a host plane: the builder of tests/test_gpu_scratch_poison.py section c (profile = 1), the output a view into a NaN
    array with RIM_ROWS rows above and below and RIM_COLS floats left and right of every row; pinned: both planes page-locked (torch)"""

    def __init__(self, w, torch, layers, x, nn2x=False, pinned=False, **okw):
        self.w, self.up = w, 1 if nn2x else 0
        self.models = [w._ModelSet.from_layers(layers())]
        h, w_ = x.shape
        H, W = h << self.up, w_ << self.up
        shape = (H + 2 * RIM_ROWS, W + 2 * RIM_COLS)
        if pinned:
            self.keep = (torch.from_numpy(np.ascontiguousarray(x)).pin_memory(), torch.empty(shape, dtype=torch.float32).pin_memory())
            self.x, self.big = self.keep[0].numpy(), self.keep[1].numpy()
        else:
            self.x, self.big = np.ascontiguousarray(x, np.float32), np.empty(shape, np.float32)
        self.x0 = self.x.copy()
        self.out = self.big[RIM_ROWS:RIM_ROWS + H, RIM_COLS:RIM_COLS + W]
        self.o = w.make_opts(profile=1, **okw)

    def call(self):
        w, ms, x = self.w, self.models[0], self.x
        self.big[...] = np.nan
        h, w_ = x.shape
        lib = w.lib()
        if self.up:
            rc = lib.w2xc_convert_plane_nn2x(ms.handle, x.ctypes.data, x.strides[0], w_, h, self.out.ctypes.data, self.big.strides[0], C.byref(self.o))
        else:
            rc = lib.w2xc_convert_plane(ms.handle, x.ctypes.data, x.strides[0], w_, h, self.out.ctypes.data, self.big.strides[0], 1, C.byref(self.o))
        if rc != w.OK:
            raise w.W2xcError(rc, w.last_error())
        self.rims()
        return [self.out.copy()]

    def rims(self):
        rest = np.ones(self.big.shape, bool)
        rest[RIM_ROWS:-RIM_ROWS, RIM_COLS:-RIM_COLS] = False
        assert np.isnan(self.big[rest]).all(), "floats around the output plane were written"
        assert np.array_equal(bits(self.x), bits(self.x0)), "the input plane was written"


class HostBatchRun(Run):
    """w2xc_convert_batch on n host planes, the outputs views into one NaN array with rims around every plane"""

    def __init__(self, w, torch, layers, x, **okw):
        self.w = w
        self.models = [w._ModelSet.from_layers(layers())]
        self.x = np.ascontiguousarray(x, np.float32)
        n, h, w_ = self.x.shape
        self.big = np.empty((n, h + 2 * RIM_ROWS, w_ + 2 * RIM_COLS), np.float32)
        self.out = self.big[:, RIM_ROWS:-RIM_ROWS, RIM_COLS:-RIM_COLS]
        self.o = w.make_opts(**okw)

    def call(self):
        self.big[...] = np.nan
        self.models[0].convert_batch(self.x, opts=self.o, out=self.out)
        self.rims()
        return [self.out.copy()]

    def rims(self):
        rest = np.ones(self.big.shape, bool)
        rest[:, RIM_ROWS:-RIM_ROWS, RIM_COLS:-RIM_COLS] = False
        assert np.isnan(self.big[rest]).all(), "floats around the output planes were written"


class FilterChainRun(Run):
    """Model::filter chained by hand on host planes with filter_resident = 1 (tests/test_gpu_scratch_poison.py: test_filter_chains).  A call that failed at
    layer l is made AGAIN by call(): the same layer on the same planes -- the pointers of the previous layer's result, which filter_resident would find on the
    device -- and then the rest of the chain; it must upload them (res_valid is withdrawn by the failed call), not use what the failed call left"""

    def __init__(self, w, torch, layers, x):
        self.w = w
        self.models = [w._ModelSet.from_layers(layers())]
        self.x = np.ascontiguousarray(x, np.float32)
        self.o = w.make_opts(filter_resident=1)
        self.at, self.t = 0, None

    def call(self):
        m = self.models[0]
        if self.t is None:
            self.at, self.t = 0, self.x
        while self.at < m.n_layers:
            nxt = m.filter(self.at, list(self.t), opts=self.o)     # (raises with at / t kept: the next call() resumes here)
            self.at, self.t = self.at + 1, nxt
        out, self.t = self.t, None
        return [out]

    def trim(self):
        Run.trim(self)
        self.t = None        # (a cold model starts its chain over)


class ImageHostRun(Run):
    """w2xc_scale2x_image_u8 on a host image: the device copies of the image (img_io) around the device sequence"""

    def __init__(self, w, torch, layers, img):
        self.models = [w._ModelSet.from_layers(layers())]
        self.img = img

    def call(self):
        return [self.models[0].scale2x_image_u8(self.img, 1)]


def fail_loop(w, make, kind, weights=False, exact=True, min_events=1, must_name=(), log=print, what=""):
    """the loop of the module's docstring; make() -> a Run on new models.  exact = False: the call's events are not the same from run to run (units on threads
    of their own) -- a k the run did not reach leaves the seam armed and the call OK, with the expected bits, and at least one k must have failed.
    -> (E, the buffers the ALLOC messages named)"""
    code = w.ERR_NOMEM if kind == ALLOC else w.ERR_HIP
    untouched = make()
    want = untouched.call()
    want_bytes = untouched.scratch_bytes()
    assert all(np.isfinite(o.astype(np.float64)).all() for o in want), "the expected result is finite"

    def cold(run):
        if weights or run is None:
            run = make()
            if not weights:
                assert same(run.call(), want), "the warm call of the models under test"
        if not weights:
            run.trim()
            assert run.scratch_bytes() == [0] * len(run.models)
        return run

    run = cold(None)
    w.debug_fail_nth(kind, 0)
    got = run.call()
    E = w.debug_fail_nth(kind, 0)
    assert same(got, want), "the counted call"
    assert run.scratch_bytes() == want_bytes, (run.scratch_bytes(), want_bytes)
    log("%s %s: E = %d" % (what, KIND[kind], E))
    assert E >= min_events, "%s %s: %d events, the case wants at least %d" % (what, KIND[kind], E, min_events)
    named, failed_ks = set(), 0
    for k in range(1, E + 1):
        run = cold(run)
        assert w.debug_fail_nth(kind, 0) >= 0
        w.debug_fail_nth(kind, k)
        err = None
        try:
            got = run.call()
        except w.W2xcError as e:
            err = e
        seen = w.debug_fail_nth(kind, 0)
        tag = "%s %s k = %d of %d" % (what, KIND[kind], k, E)
        if err is None and not exact and seen < k:      # this run had fewer events than the counted one: nothing failed, nothing may differ
            assert same(got, want), tag
            log("%s: only %d events this time, OK" % (tag, seen))
            continue
        assert err is not None, "%s: the call returned OK (%d events seen)" % (tag, seen)
        failed_ks += 1
        assert err.code == code, "%s: code %d, not %d (%s)" % (tag, err.code, code, err)
        msg = str(err).split(": ", 1)[1]
        assert msg.strip(), "%s: w2xc_last_error() is empty" % tag
        if kind == ALLOC:
            m = NAMED.search(msg)
            assert m and m.group(1) in BUFFERS, "%s: the message does not name its buffer: %r" % (tag, msg)
            named.add(m.group(1))
        assert seen == k if exact else seen >= k, "%s: %d events seen: the k-th event did not end the call" % (tag, seen)   # (it fired: the seam is disarmed)
        run.rims()
        again = run.call()
        assert same(again, want), "%s: the same call made again differs from the untouched models' result" % tag
        assert run.scratch_bytes() == want_bytes, "%s: scratch bytes %s, untouched %s" % (tag, run.scratch_bytes(), want_bytes)
        log("%s: %d, %s -> recovered" % (tag, err.code, msg[:90]))
    assert failed_ks >= 1
    if kind == ALLOC:
        assert set(must_name) <= named, "%s: no failure named %s" % (what, sorted(set(must_name) - named))
    return E, named


# ---- the host routes: groups of cases, one child process each ----
def host_groups(w, torch):
    P, S = PRODUCT, SCALE
    big = rand_plane(301, 423, 5) - 0.5          # the smallest plane at which prog / tail32 / tail16 / first_chunks engage (test_gpu_scratch_poison.py, section c)
    bands = rand_plane(333, 260, 12) - 0.5       # band_rows = 100: four bands; host_units = 3: three units
    both = (ALLOC, LAUNCH)
    pipe = ("the input rows", "the output rows", "the input staging ring", "the output staging ring", "the activation workspace")
    prog = ("the band buffer", "the job flags", "the gather-job counters")

    def host(layers, x, **kw):
        return lambda: HostRun(w, torch, layers, x, **kw)

    def batch_331():
        """n = 7 at 33 x 47 under a workspace budget of three images: sub-batches of 3 + 3 + 1 (test_batch_sub_batches_3_3_1's rule at section d's smallest size)"""
        ms = w._ModelSet.from_layers(P())
        p = ms.plan_rows(47, 33, opts=w.make_opts(device=0))
        per = sum(((int(b) + 3) // 4 + 63) // 64 * 64 * 4 for b in p.workspace_bytes)
        mb = (3 * per + (1 << 20) - 1) >> 20
        assert 3 * per <= mb << 20 < 4 * per and ms.batch_plan(1, 47, 33, False, w.make_opts(device=0, workspace_mb=mb)) == (1, 3)
        x = np.stack([rand_plane(33, 47, 200 + i) - 0.5 for i in range(7)])
        return lambda: HostBatchRun(w, torch, P, x, workspace_mb=mb)

    filt = lambda: FilterChainRun(w, torch, lambda: gen_model.synth_layers([3, 32, 64, 64, 3], 91),      # noqa: E731
                                  np.random.default_rng(3).standard_normal((3, 45, 70)).astype(np.float32))
    img = lambda: ImageHostRun(w, torch, S, np.random.default_rng(5).integers(0, 256, (23, 37, 3), dtype=np.uint8))    # noqa: E731
    # name -> [(case, make, kinds, keywords of fail_loop)]
    return {
        "prog": [("prog-pageable", host(P, big), both, dict(must_name=pipe + prog)),
                 ("prog-pinned", host(P, big, pinned=True), both, dict(must_name=pipe[:2] + pipe[4:]))],
        "tails": [("tail32", host(P, big, fusion=w.FUSION_GATHER_LAUNCH), both, dict(must_name=pipe)),
                  ("tail16", host(S, big + 0.5, precision=w.PRECISION_FP16X2), both, dict(must_name=pipe)),
                  ("first-chunks", host(P, big, host_chunk_kb=16), both, dict(must_name=pipe + prog))],
        # four bands: pin_band[1] and its flags grow in band 2, while band 1 is being drained; the launches of band 3 are the failed launch mid-band
        "bands": [("four-bands", host(P, bands, band_rows=100), both, dict(must_name=pipe + prog)),
                  ("three-units", host(P, bands, host_units=3), both, dict(exact=False, must_name=("the input rows",)))],
        "routes": [("batch-3+3+1", batch_331(), both, dict(must_name=pipe)),
                   ("filter-chain", filt, both, dict(must_name=("Model::filter planes", "the Model::filter bounce ring"))),
                   ("image-host", img, both, dict(must_name=("the image", "the image planes")))],
    }


GROUPS = ("prog", "tails", "bands", "routes")


def main(argv):
    """python tests/fail_cases.py <group> [count]: the group's cases through fail_loop (count: the counting step alone, nothing armed -- what the time limit of
    the group's child is ten times of); one line per k; exit status 0 only if every k passed"""
    import torch
    import __graft_entry__ as graft
    w = graft.load_package()
    assert w.device_count() >= 1 and torch.cuda.is_available(), "no HIP device"
    torch.cuda.set_device(0)
    group, count_only = argv[1], len(argv) > 2 and argv[2] == "count"
    t0 = time.perf_counter()
    for name, make, kinds, kw in host_groups(w, torch)[group]:
        for kind in kinds:
            if count_only:
                run = make()
                run.call()
                run.trim()
                w.debug_fail_nth(kind, 0)
                run.call()
                print("%s %s: E = %d" % (name, KIND[kind], w.debug_fail_nth(kind, 0)), flush=True)
            else:
                fail_loop(w, make, kind, what=name, log=lambda s: print(s, flush=True), **kw)
    print("group %s: %s in %.2f s" % (group, "counted" if count_only else "every k passed", time.perf_counter() - t0), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
