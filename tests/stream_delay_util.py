"""Is the work of one HIP stream ordered after the work of another where it has to be?  (TEST-ONLY.)

On an idle GPU a producer finishes microseconds before an unordered consumer starts, so a missing `wait_event`, a wait on an
EARLIER event than the right one, or a side-stream reader whose buffer the main stream overwrites too soon all pass a bit-equality
test.  Two tools make them fail deterministically:

  poison(models)   fills everything a pass should rewrite -- every floating-point tensor reachable from `plan._bufs` -- with
                   `retire_util.SENTINEL`.  A consumer that runs before its producer then reads the sentinel, not the (equal)
                   numbers the previous pass left there.
  stall(stream, ms) queues a bounded spin on one stream.  Whatever that stream was going to produce is late by `ms`; everybody
                   who is properly ordered behind it waits, everybody who is not runs ahead and reads poison.

Delay points (`delay_points`, installed on `nlt_amd.capi` for the length of a `with` block):
  (i)   right AFTER every `record_event(ev, stream)`, on the recording stream.  One stall per interval between two records tells
        "waited on the right event" from "waited on an earlier one": the work the right event covers and the earlier one does
        not is what the stall holds back.  (A stall BEFORE the producer would delay its own event too and prove nothing.)
  (ii)  at the start of a named stream before the pass: plain `stall(stream, ms)` by the caller.
  (iii) right BEFORE the n-th `_call` of a pass, on the stream that launch goes to.  `_capi._call` is the one launch helper of
        the adapters, so counting its invocations enumerates a pass that is issued eagerly (a tape replay calls neither hook).

Not poisoned, and why (each is an INPUT or STATE of a pass, not a result of it):
  'tapes' entries            recorded launches: host objects (`retire_util._walk` skips them)
  grads['zero_bias']         zeros read by every backward-data launch, written once when the gradient buffers are made
  _capi._ws_cache            split-K scratch keeps ticket counters that must stay zero between launches
  plan._front_blob, packs    folded / packed weights: inputs, rewritten only when a weight changes
"""
import contextlib
import statistics

import torch

from nlt_amd import capi as C
from retire_util import SENTINEL, _walk

MIN_STALL_MS, MAX_STALL_MS, STALL_FACTOR = 5.0, 200.0, 10.0
# buffers under plan._bufs that are state, not per-pass results: path suffix -> reason (every one costs coverage: keep it short)
NOT_POISONED = {"['grads']['zero_bias']": "zeros every backward-data launch reads as its bias; written once, never again"}


# ------------------------------------------------------------------------------------------------------------ poison
def poison_targets(models, exclude=()):
    """[(container path, tensor)] of what `poison` fills: the floating-point tensors reachable from each model's `plan._bufs`
    (dicts, lists, tuples; 'tapes' skipped), minus NOT_POISONED and `exclude` (path suffixes)."""
    models = list(models) if isinstance(models, (list, tuple)) else [models]
    found = {}
    for i, m in enumerate(models):
        _walk(m.plan._bufs, 'plan._bufs' if len(models) == 1 else 'models[%d].plan._bufs' % i, found)
    skip = tuple(NOT_POISONED) + tuple(exclude)
    return [(p, t) for p, t in found.values() if t.dtype.is_floating_point and not p.endswith(skip)]


def poison(models, exclude=()):
    """Fills every target with SENTINEL (on the current stream: a pass issued afterwards from this stream is behind the fills,
    and the plans' side streams only ever start behind an event of the stream the pass is issued on).  Returns the paths."""
    targets = poison_targets(models, exclude)
    for _, t in targets:
        t.fill_(SENTINEL)
    return [p for p, _ in targets]


def blame(models, run, same, exclude=()):
    """For a failing self-check: poisons ONE buffer at a time in front of run() and returns the paths for which
    same(run()) is False -- the buffers that are state rather than a per-pass result (or that a pass reads before writing)."""
    bad = []
    for path, t in poison_targets(models, exclude):
        run()                                               # a clean pass in between: what a pass rewrites is whole again
        t.fill_(SENTINEL)
        if not same(run()):
            bad.append(path)
    return bad


# ------------------------------------------------------------------------------------------------------------- stall
class _Spin:
    """How to keep a stream busy for a given time, found out once per process by timing with events."""

    def __init__(self):
        self.kind, self.per_ms, self.ballast, self.note = None, None, None, ''

    def _time(self, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def calibrate(self):
        if self.kind is not None:
            return self
        sleep = getattr(torch.cuda, '_sleep', None)
        if sleep is not None:
            # what one "cycle" of the spin kernel is on this GPU is not assumed: two lengths, a ratio of ~4 or it does not scale
            n = 2_000_000
            sleep(n)                                        # (first launch: module load)
            t1 = statistics.median(self._time(lambda: sleep(n)) for _ in range(3))
            t4 = statistics.median(self._time(lambda: sleep(4 * n)) for _ in range(3))
            if t1 > 0.05 and 3.0 <= t4 / t1 <= 5.0:
                self.kind, self.per_ms = 'sleep', 3 * n / (t4 - t1)
                self.note = "torch.cuda._sleep: %.0f cycles per ms (%.3f ms / %.3f ms for %d / %d cycles)" % (self.per_ms, t1, t4, n, 4 * n)
                return self
            self.note = "torch.cuda._sleep does not scale here (%.3f ms / %.3f ms for %d / %d cycles); " % (t1, t4, n, 4 * n)
        # in-stream ballast: repeated passes over a buffer far larger than the caches
        self.ballast = torch.zeros(64 << 20, device='cuda')           # 256 MB
        self.ballast.add_(1.0)
        t = statistics.median(self._time(lambda: [self.ballast.add_(1.0) for _ in range(8)]) for _ in range(3))
        self.kind, self.per_ms = 'ballast', 8 / t
        self.note += "ballast: %.2f passes over 256 MB per ms" % self.per_ms
        return self

    def enqueue(self, ms):
        if self.kind == 'sleep':
            torch.cuda._sleep(int(ms * self.per_ms))
        else:
            for _ in range(max(1, int(round(ms * self.per_ms)))):
                self.ballast.add_(1.0)


_spin = _Spin()


def calibration():
    """One line on how `stall` spins on this machine."""
    return _spin.calibrate().note


def stall(stream, ms):
    """Queues a spin of about `ms` milliseconds (at most MAX_STALL_MS) on `stream`; returns at once."""
    _spin.calibrate()
    with torch.cuda.stream(stream):
        _spin.enqueue(min(float(ms), MAX_STALL_MS))


def measured_stall(run, what, repeats=3):
    """(pass time, stall) in ms for a scenario: the median wall time of `run()` on the GPU by events on the current stream (run()
    must leave the current stream behind its results), and a stall of at least STALL_FACTOR times that and MIN_STALL_MS -- the
    host's enqueue jitter of a fraction of a millisecond cannot close such a gap -- capped at MAX_STALL_MS.  Prints both."""
    _spin.calibrate()
    t = statistics.median(_spin._time(run) for _ in range(repeats))
    ms = min(max(STALL_FACTOR * t, MIN_STALL_MS), MAX_STALL_MS)
    print("stream-order %s: pass %.3f ms, stall %.1f ms (%s)" % (what, t, ms, _spin.kind))
    return t, ms


# ------------------------------------------------------------------------------------------- streams a stall can tell apart
# A process has a handful of hardware queues (4 by default) and the runtime binds every stream to one of them.  Two streams on
# ONE queue are executed in the order of submission: a stall on the first also holds the second back, a consumer without its
# event edge still runs after its producer, and a test between the two proves nothing.  In a long process (the whole suite)
# dozens of streams exist and a freshly made one lands on the caller's queue one time in four.  So the tests do not take whatever
# stream a plan or a pipeline makes: they hand it streams that were PROBED to run beside each other.
PROBE_MS = 4.0
_independent = []


def holds_back(a, b, ms=PROBE_MS):
    """Does a stall queued on stream `a` hold back work queued on stream `b` afterwards?  (Wall clock on the host: a launch and
    an event on an idle queue are through in well under 0.1 ms.)"""
    import time
    _spin.calibrate()
    with torch.cuda.stream(b):
        x = torch.zeros(16, device='cuda')
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    stall(a, ms)
    t0 = time.perf_counter()
    with torch.cuda.stream(b):
        x.add_(1.0)
        done.record(b)
    done.synchronize()
    waited = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return waited > 0.5 * ms


def independent_streams(n, tries=48):
    """n streams no one of which is held back by a stall on another: the current stream first, the rest drawn from torch's
    stream pool and probed against every one already chosen.  Found once per process (a stream keeps its queue) and printed.
    Raises if the machine does not have that many -- a test must not run on streams it cannot tell apart."""
    if not _independent:
        _independent.append(torch.cuda.current_stream())
    drawn = 0
    while len(_independent) < n and drawn < tries:
        s = torch.cuda.Stream(priority=0 if drawn < 32 else -1)     # (the pool hands out 32 streams per priority in turn)
        drawn += 1
        if any(s.cuda_stream == c.cuda_stream for c in _independent):
            continue
        if not any(holds_back(c, s) or holds_back(s, c) for c in _independent):
            _independent.append(s)
            print("stream-order: stream %#x runs beside %s (candidate %d)"
                  % (s.cuda_stream, ['%#x' % c.cuda_stream for c in _independent[:-1]], drawn))
    if len(_independent) < n:
        raise AssertionError("only %d of %d streams that a stall can tell apart were found among %d candidates: the others share a "
                             "hardware queue with one of them, and a stream-ordering test on them would be vacuous"
                             % (len(_independent), n, drawn))
    if _independent[0].cuda_stream != torch.cuda.current_stream().cuda_stream:
        raise AssertionError("independent_streams() was first asked on another current stream")
    return list(_independent[:n])


# ------------------------------------------------------------------------------------------------------ delay points
class DelayPoints:
    """What a pass issued while the hooks were in: `records` = [recording stream] per record_event, `calls` = [(entry point,
    stream handle it was launched on)] per `_call`, `marks` = [(label, records so far, calls so far)] for `mark(label)`."""

    def __init__(self):
        self.records, self.calls, self.marks = [], [], []

    def mark(self, label):
        self.marks.append((label, len(self.records), len(self.calls)))


@contextlib.contextmanager
def delay_points(monkeypatch, after_record=None, before_call=None):
    """Hooks `capi.record_event` and `capi._call` for the block and restores both on the way out.
    after_record(k, stream): called right after the k-th record of the block (k from 0), with the recording stream.
    before_call(n, name): called right before the n-th launch of the block, with its entry point's name; the current stream is
    the one the launch goes to."""
    dp = DelayPoints()
    real_record, real_call = C.record_event, C._call

    def record_event(ev, stream):
        real_record(ev, stream)
        k = len(dp.records)
        dp.records.append(stream)
        if after_record is not None:
            after_record(k, stream)

    def _call(name, *args):
        n = len(dp.calls)
        dp.calls.append((name, C._stream()))
        if before_call is not None:
            before_call(n, name)
        real_call(name, *args)

    with monkeypatch.context() as mp:
        mp.setattr(C, 'record_event', record_event)
        mp.setattr(C, '_call', _call)
        yield dp


def stall_after_record(k, ms):
    """after_record hook: stall the recording stream right behind the k-th record."""
    return lambda i, stream: stall(stream, ms) if i == k else None


def stall_before_call(n, ms):
    """before_call hook: stall the stream of the n-th launch right in front of it."""
    return lambda i, name: stall(torch.cuda.current_stream(), ms) if i == n else None
