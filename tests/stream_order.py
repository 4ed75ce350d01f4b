"""Stream-order harness (tests only).

The C ABI takes the stream of every launch, memset and copy from the caller (include/lidf_hip.h: the trailing
`lidf_stream_t`), and the Python layer passes torch's current stream (`_lib.current_stream`). Run on the default
stream with a device-wide synchronise after it, an entry that queued a launch on another stream, waited on the wrong
one, forked a side stream too early, consumed it too soon or handed a temporary back to the allocator while a side
stream still used it gives the right answer all the same. This harness runs an entry (an `entry_cases.Entry`) twice:

  baseline()     on the default stream, the device synchronised before and after.
  late_inputs()  on a fresh stream `s`, with no host synchronisation issued here between the first queued delay and
                 the final s.synchronize(). The live tensors the entry reads hold DECOYS; queued on `s` are, in this
                 order, a bounded delay, the device-to-device copies of the staged real values into the live tensors
                 (module parameters through p.data.copy_), the entry, and clones of its results. Whatever ran on, or
                 waited on, another queue saw the decoy.
  slow_side()    for an entry that owns a second stream: the same delay queued on THAT stream just before the call,
                 `s` left free, so the side work lags the caller's stream; results cloned on `s` right after the call
                 are right only if the join holds.

`s` is chosen so that it shares no hardware queue with the null stream or the entry's side stream (fresh_stream()):
two streams on one queue run in submission order, and a launch on the wrong one of them would wait out the delay like
a right one. What remains unseen is a launch on some third pool stream that happens to share s's queue — nothing in
the library creates one.

Decoys are valid inputs, so that even a failing run never hands a kernel an out-of-range index: NaN for every float
array, zero for masks, and for an integer array either its own values or — only where the entry's builder names it in
`zero`, having checked in the entry's code that zero is in range — all zero.

After the call, still on `s` and before any synchronisation, churn() allocates tensors of the sizes the call took
from _lib.workspace (recorded by a wrapper installed the way ws_poison.Poisoner is) and of its results and fills them
with 0xFF bytes: under correct lifetimes that cannot change a result cloned earlier in stream order.

The delay is a fixed-length spin (torch.cuda._sleep), calibrated once per process with events; nothing waits for a
host flag. Its length is max(20 ms, 3 x the host time one enqueue of the entry takes on a fresh stream), capped at
250 ms: a case at the cap is too large. The host time is a sizing input, never a pass criterion. An event recorded on
the delayed stream right behind the delay must still be pending when the entry returns to the host, or the run is
inconclusive and fails; entries that read a size back wait for their stream themselves and are exempt (`reads_back`).
"""
import time

import torch

MIN_MS, CAP_MS = 20.0, 250.0
DELAYS = {}      # case name -> (mode, milliseconds): what the runs of this process used (printed by the tests)
_CAL = {}


def cycles_per_ms(dev):
    """torch.cuda._sleep cycles per millisecond on `dev`: one 50 M-cycle spin timed with events, after a warm-up."""
    if dev.index not in _CAL:
        with torch.cuda.device(dev):
            torch.cuda._sleep(1000000)
            torch.cuda.synchronize(dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            n = 50000000
            a.record()
            torch.cuda._sleep(n)
            b.record()
            b.synchronize()
            _CAL[dev.index] = n / a.elapsed_time(b)
    return _CAL[dev.index]


def spin(ms, dev):
    """Queue a spin of `ms` milliseconds on the current stream of `dev`."""
    with torch.cuda.device(dev):
        torch.cuda._sleep(int(ms * cycles_per_ms(dev)))


def independent(a, b, dev, ms=5.0):
    """Whether work queued on stream `b` runs while stream `a` spins. Streams are multiplexed onto a few hardware
    queues (GPU_MAX_HW_QUEUES; HIP's default is 4) and two streams that share one run in submission order — a false
    ordering that would hide exactly what this harness looks for. A bounded probe: a spin of `ms` on `a`, a memset on
    `b`, and whether the spin is still running when the memset has finished (at the latest when the spin ends)."""
    if a.cuda_stream == b.cuda_stream:
        return False
    word = torch.zeros((1,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    end_a, end_b = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(a):
        spin(ms, dev)
        end_a.record(a)
    with torch.cuda.stream(b):
        word.fill_(1)
        end_b.record(b)
    end_b.synchronize()
    apart = not end_a.query()
    torch.cuda.synchronize(dev)
    return apart


def fresh_stream(dev, apart_from=()):
    """A pool stream that runs beside every stream of `apart_from` (see independent()); the null stream is always one
    of them. Fails when 32 candidates — torch's whole pool — all share a queue with one of them."""
    others = [torch.cuda.default_stream(dev)] + [o for o in apart_from if o is not None]
    for _ in range(32):
        s = torch.cuda.Stream(dev)
        if all(independent(o, s, dev) for o in others):
            return s
    raise AssertionError("no pool stream runs beside %s: too few hardware queues for this harness" % (others,))


def tree_map(fn, obj):
    if torch.is_tensor(obj):
        return fn(obj)
    if isinstance(obj, dict):
        return {k: tree_map(fn, v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(tree_map(fn, v) for v in obj)
    return obj


def tree_tensors(obj):
    out = []
    tree_map(lambda t: out.append(t) or t, obj)
    return out


def decoy(name, t, zero):
    """The decoy of input `name` (see the module docstring)."""
    if name in zero or t.dtype in (torch.bool, torch.uint8):
        return torch.zeros_like(t)
    if t.is_floating_point():
        return torch.full_like(t, float("nan"))
    return t.clone()


class Recorder:
    """Wraps _lib.workspace for the duration of a test: the sizes every call took."""

    def __init__(self):
        self.sizes = []

    def install(self, monkeypatch):
        from implicit_depth_amd import _lib
        real = _lib.workspace

        def workspace(nbytes, device):
            self.sizes.append(max(int(nbytes), 1))
            return real(nbytes, device)

        monkeypatch.setattr(_lib, "workspace", workspace)
        return self

    def begin(self):
        self.sizes = []
        return self


def churn(sizes, results, dev):
    """On the current stream: fresh allocations of the call's workspace sizes and of its results' sizes, each
    filled with 0xFF bytes (NaN floats, -1 ints); released again at once, so that later ones can land on the same
    blocks. Returns how many were made."""
    todo = list(sizes) + [t.numel() * t.element_size() for t in tree_tensors(results)]
    for n in todo:
        if n:
            torch.empty((n,), dtype=torch.uint8, device=dev).fill_(0xFF)
    return len(todo)


def _params(entry):
    return [p for m in entry.modules for p in list(m.parameters()) + list(m.buffers())]


def _stage(entry, dev):
    return {k: v.to(dev).contiguous() for k, v in entry.inputs.items()}


def baseline(entry, dev):
    """The entry on the default stream, the device synchronised before and after."""
    live = _stage(entry, dev)
    torch.cuda.synchronize(dev)
    out = tree_map(lambda t: t.detach().clone(), entry.call(live))
    torch.cuda.synchronize(dev)
    return entry.finish(out) if entry.finish is not None else out


def enqueue_ms(entry, dev):
    """(host milliseconds one enqueue of the (warmed-up) entry takes on a FRESH stream — its allocator pool empty and
    its packed weight entries absent, as the stressed run will find them —, the results of that run).
    Entries that read a size back include their wait; a sizing input only."""
    live = _stage(entry, dev)
    torch.cuda.synchronize(dev)
    w = torch.cuda.Stream(dev)
    with torch.cuda.stream(w):
        t0 = time.perf_counter()
        out = entry.call(live)
        dt = time.perf_counter() - t0
        out = tree_map(lambda t: t.detach().clone(), out)
    w.synchronize()
    torch.cuda.synchronize(dev)
    return 1e3 * dt, (entry.finish(out) if entry.finish is not None else out)


def delay_ms(host_ms, name=None, mode=None):
    ms = max(MIN_MS, 3.0 * host_ms)
    assert ms < CAP_MS, ("the delay of %s reached the %g ms cap (enqueue %.1f ms): the case is too large"
                         % (name, CAP_MS, host_ms))
    if name is not None:
        DELAYS[(name, mode)] = ms
        print("stream_order: %s [%s] enqueue %.2f ms -> delay %.1f ms" % (name, mode, host_ms, ms))
    return ms


class LateRun:
    """One "late inputs" run in three steps, so that several can be enqueued back to back: __init__ stages the real
    values, builds the decoys and fills the modules' parameters with NaN (the caller synchronises the device once
    after every run is prepared); enqueue() queues delay, copies, entry, clones and churn on the stream; finish()
    waits for the stream and returns (results, whether the delay was still running when the entry returned)."""

    def __init__(self, entry, dev):
        self.entry, self.dev = entry, dev
        self.staged = _stage(entry, dev)
        self.params = _params(entry)
        self.pstaged = [p.detach().clone() for p in self.params]
        self.live = {k: decoy(k, v, entry.zero) for k, v in self.staged.items()}
        for p in self.params:
            if p.is_floating_point():
                p.data.fill_(float("nan"))
        self.stream, self.got, self.running = None, None, None

    def enqueue(self, ms, stream, recorder=None):
        dev, entry = self.dev, self.entry
        s = self.stream = stream
        behind = torch.cuda.Event()
        if recorder is not None:
            recorder.begin()
        try:
            with torch.cuda.stream(s):
                spin(ms, dev)
                behind.record(s)
                for k in self.live:
                    self.live[k].copy_(self.staged[k])
                for p, q in zip(self.params, self.pstaged):
                    p.data.copy_(q)
                out = entry.call(self.live)
                self.running = not behind.query()
                self.got = tree_map(lambda t: t.detach().clone(), out)
                churn(recorder.sizes if recorder is not None else (), self.got, dev)
        except BaseException:
            self.restore()
            raise
        return self

    def restore(self):
        """The modules' real parameters back in place (after a failed enqueue)."""
        torch.cuda.synchronize(self.dev)
        for p, q in zip(self.params, self.pstaged):
            p.data.copy_(q)
        torch.cuda.synchronize(self.dev)

    def finish(self):
        self.stream.synchronize()
        got = self.entry.finish(self.got) if self.entry.finish is not None else self.got
        return got, self.running


def side_of(entry):
    return entry.side() if entry.side is not None else None


def late_inputs(entry, dev, ms, recorder=None, apart_from=()):
    """The "late inputs" run on a fresh stream that shares no hardware queue with the null stream, the entry's own
    side stream or `apart_from`: (results, delay still running at the return)."""
    s = fresh_stream(dev, (side_of(entry),) + tuple(apart_from))
    run = LateRun(entry, dev)
    torch.cuda.synchronize(dev)
    return run.enqueue(ms, s, recorder).finish()


def slow_side(entry, dev, ms, side, recorder=None):
    """The "slow side" run: real inputs, the delay on the entry's own second stream `side`. Returns (results cloned
    on the caller's stream, whether the delay was still running when the entry returned to the host)."""
    live = _stage(entry, dev)
    s = fresh_stream(dev, (side,))
    torch.cuda.synchronize(dev)
    behind = torch.cuda.Event()
    if recorder is not None:
        recorder.begin()
    with torch.cuda.stream(side):
        spin(ms, dev)
        behind.record(side)
    with torch.cuda.stream(s):
        out = entry.call(live)
        running = not behind.query()
        got = tree_map(lambda t: t.detach().clone(), out)
        churn(recorder.sizes if recorder is not None else (), got, dev)
    s.synchronize()
    side.synchronize()
    return (entry.finish(got) if entry.finish is not None else got), running


def compare(got, base, entry, what):
    """Bit for bit with the baseline, except the entry's `loose` results, each held by its own function."""
    from entry_cases import same
    got, base = (dict(got), dict(base)) if isinstance(base, dict) else (got, base)
    for k, fn in entry.loose.items():
        fn(got.pop(k), base.pop(k))
    same(got, base, what, ref="the default-stream run")
