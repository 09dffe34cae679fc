"""Every device entry point (the rows of tests/stream_cases.py) on a caller's NON-BLOCKING stream, between work of the caller's on that stream and with no
host synchronisation in between: include/w2xc_hip.h promises "enqueued on `hip_stream` and NOT synchronised on return".

A row's reference is the same call on the null stream with device syncs around it -- the form every other GPU test verifies -- and every comparison is
equality of bits.  A measured run starts with the call once on the null stream on STALE inputs, synced: every grow-only scratch buffer then has its size (the
measured call allocates nothing) and holds the intermediates of another result.  Then, on a stream `s`: a sleep kernel, device-to-device copies of the real
inputs into the input buffers (which hold the stale data), the event `arrived`, the library call, copies of the outputs (which held a sentinel), an overwrite
of the inputs with stale data.  A launch or copy of the call that is not on `s` runs while the sleep still holds `s` up: it reads the stale inputs or what
the stale run left in scratch, or its result is overwritten, or it is not in the copy -- the bits differ.  (A memset that leaves `s` clears early; in the
back-to-back test the first call's work lies between it and the second call's kernels.)  `arrived` is still pending when the call returns, or the case is
inconclusive and fails.  Two positive controls make the mistake on purpose and must see the stale inputs' result: the whole call on stream 0, on three rows,
and only the LATE stage of a two-stage sequence of block calls on stream 0 -- which also shows why the warm-up runs on the stale inputs: behind a warm-up on
the real ones that late stage finds the right planes and cannot be seen.

The sleep is 5 x the slowest row's warm enqueue time on the host and at least 30 ms (host jitter on a shared machine is a few times the mean); with
W2XC_STREAM_ORDER_REPORT=<path> the per-row enqueue times and the delay are written there (profiles/stream_order_enqueue.txt)."""
import ctypes as C
import os
import time

import pytest

import stream_cases as sc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HIP_STREAM_NON_BLOCKING = 0x01
MIN_DELAY_MS = 30.0
MODEL_AND_FRAME = [r.id for r in sc.ROWS if r.family in ("model", "frame")]


@pytest.fixture(scope="module")
def ctx(w2xc):
    assert w2xc.device_count() >= 1, "no HIP device visible: libw2xc_hip has no CPU fallback, -m gpu tests need an MI355X"
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return sc.Ctx(w2xc, torch)


def hip_runtime():
    """the HIP runtime this process has loaded (torch's, which libw2xc_hip.so binds to as well)"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, "one HIP runtime in the process: %s" % sorted(paths)
    return C.CDLL(paths.pop())


@pytest.fixture(scope="module")
def side_stream(ctx):
    """the caller's stream: torch's side streams do not synchronise with the null stream -- read back from the runtime, once"""
    s = torch.cuda.Stream()
    flags = C.c_uint(0xFFFF)
    get = hip_runtime().hipStreamGetFlags
    get.argtypes, get.restype = [C.c_void_p, C.POINTER(C.c_uint)], C.c_int
    assert get(C.c_void_p(s.cuda_stream), C.byref(flags)) == 0
    assert flags.value & HIP_STREAM_NON_BLOCKING, "torch.cuda.Stream() is a blocking stream here (flags %#x): the null stream would wait for it" % flags.value
    assert s.cuda_stream != 0
    return s


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def prepare(case):
    """stale inputs, sentinel outputs"""
    for buf, _, stale in case.ins:
        buf.copy_(stale)
    for buf, fill, _ in case.outs:
        buf.copy_(fill)


def reference(case, stale=False):
    """the call on the null stream with a device sync on either side -> the output buffers, rims checked"""
    prepare(case)
    if not stale:
        for buf, real, _ in case.ins:
            buf.copy_(real)
    torch.cuda.synchronize()
    case.call(0)
    torch.cuda.synchronize()
    outs = [buf.clone() for buf, _, _ in case.outs]
    for o, (_, fill, check) in zip(outs, case.outs):
        assert not same_bits(o, fill), "the call wrote nothing"
        if check is not None:
            check(o.cpu().numpy())
    for (buf, real, stale_data) in case.ins:
        assert same_bits(buf, stale_data if stale else real), "an input buffer was written"
    return outs


class Spy:
    """the library, noting the symbols looked up on it"""

    def __init__(self, lib):
        self.lib, self.seen = lib, []

    def __getattr__(self, name):
        self.seen.append(name)
        return getattr(self.lib, name)


def cycles_per_ms():
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000000)
    n = 10000000
    e0.record()
    torch.cuda._sleep(n)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    assert ms > 0.5, "the sleep kernel's %d cycles took %g ms: too short to scale from" % (n, ms)
    return n / ms


@pytest.fixture(scope="module")
def table(ctx, side_stream):
    """every row built, run once for its reference and once more, warm, under time.perf_counter; -> the cases, the references, the enqueue times and the delay"""
    t = {"cases": {}, "refs": {}, "enqueue_ms": {}, "errors": {}}
    for row in sc.ROWS:
        try:
            case = row.build(ctx, 0)
            spy = Spy(ctx.w._lib)      # (the wrappers look their entry points up on the package's private `_lib` at call time, as `lib()` returns it)
            ctx.w._lib = spy
            try:
                ref = reference(case)
            finally:
                ctx.w._lib = spy.lib
            assert row.symbol in spy.seen, "%s reaches %s, not %s" % (row.id, spy.seen, row.symbol)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            case.call(0)
            t["enqueue_ms"][row.id] = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
            t["cases"][row.id], t["refs"][row.id] = case, ref
        except Exception as e:      # (reported by the row's own test; an error of the HIP runtime ends the module: nothing more is started on the device)
            if isinstance(e, RuntimeError) and not (isinstance(e, ctx.w.W2xcError) and e.code != ctx.w.ERR_HIP):
                raise
            t["errors"][row.id] = e
    assert t["enqueue_ms"], "no row could be built: %r" % t["errors"]
    slowest = max(t["enqueue_ms"], key=t["enqueue_ms"].get)
    t["delay_ms"] = max(MIN_DELAY_MS, 5.0 * t["enqueue_ms"][slowest])
    t["cycles_per_ms"] = cycles_per_ms()
    t["cycles"] = int(t["delay_ms"] * t["cycles_per_ms"])
    # the sleep really lasts that long (within a fifth: the scale comes from one 4 ms sleep; what a case relies on is `arrived`, asserted per case)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side_stream):
        e0.record()
        torch.cuda._sleep(t["cycles"])
        e1.record()
    side_stream.synchronize()
    t["slept_ms"] = e0.elapsed_time(e1)
    assert t["slept_ms"] >= 0.8 * t["delay_ms"], "a sleep of %d cycles lasted %.1f ms, not %.1f" % (t["cycles"], t["slept_ms"], t["delay_ms"])
    path = os.environ.get("W2XC_STREAM_ORDER_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("# host time of one warm call on the null stream per row of tests/stream_cases.py (time.perf_counter), and the delay the stream-order\n"
                    "# tests sleep for on the caller's stream: max(%g ms, 5 x the slowest row)\n" % MIN_DELAY_MS)
            f.write("device: %s\n" % torch.cuda.get_device_name(0))
            f.write("sleep kernel: %.0f cycles per ms; delay %.1f ms = %d cycles, measured %.1f ms; slowest row: %s\n"
                    % (t["cycles_per_ms"], t["delay_ms"], t["cycles"], t["slept_ms"], slowest))
            for rid in sorted(t["enqueue_ms"], key=t["enqueue_ms"].get, reverse=True):
                f.write("%-44s %8.3f ms\n" % (rid, t["enqueue_ms"][rid]))
    return t


def enqueue(cases, s, cycles, lib_stream, warm_on_stale=True):
    """the measured sequence for one call, or for several back to back, on `s` with no host sync inside; lib_stream: what the library is given (s, or -- the
    positive control -- 0), or a function of the case that makes the call.  First every case runs once on the null stream on its stale inputs (warm_on_stale;
    else, for the control that shows the difference, on its real ones): scratch has its size and holds another call's intermediates.
    -> (the copies of the outputs per case, whether `arrived` had completed when each call returned)"""
    call = lib_stream if callable(lib_stream) else (lambda c: c.call(lib_stream))
    copies = [[torch.empty_like(buf) for buf, _, _ in c.outs] for c in cases]
    events = [torch.cuda.Event() for _ in cases]
    for c in cases:
        prepare(c)
        if not warm_on_stale:
            for buf, real, _ in c.ins:
                buf.copy_(real)
        torch.cuda.synchronize()
        c.call(0)
        torch.cuda.synchronize()
    for c in cases:
        prepare(c)
    torch.cuda.synchronize()
    early = []
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        for c, cp, arrived in zip(cases, copies, events):
            for buf, real, _ in c.ins:
                buf.copy_(real, non_blocking=True)
            arrived.record(s)
            call(c)
            early.append(arrived.query())
            for (buf, _, _), keep in zip(c.outs, cp):
                keep.copy_(buf, non_blocking=True)
            for buf, _, stale in c.ins:
                buf.copy_(stale, non_blocking=True)
    s.synchronize()
    torch.cuda.synchronize()
    return copies, early


def built(table, rid):
    if rid in table["errors"]:
        raise table["errors"][rid]
    return table["cases"][rid], table["refs"][rid]


def differing(got, want):
    return [k for k, (g, w_) in enumerate(zip(got, want)) if not same_bits(g, w_)]


@pytest.mark.parametrize("rid", [r.id for r in sc.ROWS])
def test_call_is_ordered_on_the_callers_stream(ctx, side_stream, table, rid):
    case, ref = built(table, rid)
    assert not differing(reference(case), ref), "two runs on the null stream differ"
    got, early = enqueue([case], side_stream, table["cycles"], side_stream.cuda_stream)
    assert early == [False], ("inconclusive: the inputs had arrived when the call returned -- it waited for the device, or took longer than the %.0f ms sleep"
                              % table["delay_ms"])
    bad = differing(got[0], ref)
    assert not bad, "output buffers %s differ from the null-stream run: work of the call left the caller's stream" % bad


@pytest.mark.parametrize("rid", sc.CONTROL)
def test_positive_control_a_call_on_stream_0_is_seen(ctx, side_stream, table, rid):
    """the library call on stream 0 while the caller's stream sleeps: it runs at once, on the stale inputs (valid memory), and the copies that the caller's
    stream takes later hold the stale inputs' result"""
    case, ref = built(table, rid)
    stale_ref = reference(case, stale=True)
    assert len(differing(stale_ref, ref)) == len(ref), "the stale inputs give another result in every output buffer"
    got, early = enqueue([case], side_stream, table["cycles"], 0)
    assert early == [False]
    assert len(differing(got[0], ref)) == len(ref), "the harness did not see a call that left the caller's stream"
    assert not differing(got[0], stale_ref), "the misplaced call ran before the inputs arrived: on the stale data"


def two_stage(ctx):
    """luma bytes -> float planes -> luma bytes as two block calls, the planes in a buffer that is neither input nor output: what scratch is to one call.
    call(stream, late=None): `late` is the stream of the second stage"""
    n, h, w = 3, 37, 53
    c = sc.Case(ctx)
    pi, li = c.bytes_in(n, h, w, 5000)
    po, lo = c.bytes_out(n, h, w)
    mid = torch.full((n * h * w,), float("nan"), dtype=torch.float32, device="cuda")

    def call(stream, late=None):
        ctx.w.y8_to_plane_device(pi, n, li.frame, li.row, w, h, sc.LIMITED, mid.data_ptr(), 4 * h * w, stream=stream)
        ctx.w.plane_to_y8_device(mid.data_ptr(), n, 4 * h * w, w, h, sc.LIMITED, po, lo.frame, lo.row, stream=stream if late is None else late)
    c.call = call
    c.keep.append(mid)
    return c


def test_positive_control_a_late_stage_on_stream_0_is_seen(ctx, side_stream, table):
    """only the second of two stages leaves the caller's stream: it runs at once on the planes the warm-up left, and is seen because those are the stale
    inputs' planes.  Behind a warm-up on the real inputs the same mistake gives the right bytes -- the reason for the stale warm-up"""
    case = two_stage(ctx)
    ref, stale_ref = reference(case), reference(case, stale=True)
    assert len(differing(stale_ref, ref)) == len(ref)
    s, cycles = side_stream, table["cycles"]
    got, early = enqueue([case], s, cycles, s.cuda_stream)
    assert early == [False] and not differing(got[0], ref), "both stages on the caller's stream"
    got, early = enqueue([case], s, cycles, lambda c: c.call(s.cuda_stream, late=0))
    assert early == [False]
    assert len(differing(got[0], ref)) == len(ref), "the harness did not see a late stage that left the caller's stream"
    assert not differing(got[0], stale_ref), "the late stage read the planes of the stale warm-up"
    got, early = enqueue([case], s, cycles, lambda c: c.call(s.cuda_stream, late=0), warm_on_stale=False)
    assert early == [False] and not differing(got[0], ref), "behind a warm-up on the real inputs the misplaced stage finds the right planes"


@pytest.mark.parametrize("rid", MODEL_AND_FRAME)
def test_two_calls_back_to_back(ctx, side_stream, table, rid):
    """two calls on the caller's stream with no sync between them: the second with other data and a smaller size (no scratch grows), each equal to its own
    null-stream run -- the second must not start on scratch the first still uses, nor the first see the second's.  (Both are warmed on their stale inputs, the
    second last: neither finds its own intermediates in scratch.)"""
    first, ref1 = built(table, rid)
    second = sc.BY_ID[rid].build(ctx, 1)
    ref2 = reference(second)
    assert not differing(reference(first), ref1)
    got, early = enqueue([first, second], side_stream, table["cycles"], side_stream.cuda_stream)
    assert early == [False, False], "inconclusive: %s" % early
    assert not differing(got[0], ref1), "the first call"
    assert not differing(got[1], ref2), "the second call"
