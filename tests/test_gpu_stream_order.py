"""-m gpu: is the work ordered BETWEEN the HIP streams of every hot path -- the fused forward's side stream, the backward's
weight-gradient streams and its mid-backward gradient hook, launch-tape replays of both, the lanes of a RenderPipeline and the
`obs_override` state they share?  tests/stream_delay_util.py: everything a pass should rewrite is filled with a sentinel
(`poison`) and one stream is held back at a chosen point (`stall`); a consumer that lacks an edge then reads the sentinel or the
previous stage's data and the result differs in its bits from the REFERENCE -- the same call, undelayed and unpoisoned, on the
same model.  Every comparison is `torch.equal`.

Common shapes: depth 256, 64 x 64 UV (level 6 is 1 x 1), camera 32 x 32, 2 frames.  Training legs run `deterministic = true`
(atomic-free adjoints: a train step repeats bit for bit); inference is deterministic as it is.  Sweeps issue eagerly
(`use_tape = False`: the delay points hook the launch helper and the event record, which a tape replay bypasses).

The stall of a scenario is measured, not fixed: 10 x the undelayed pass (median of 3, by events), at least 5 ms, at most
200 ms; every test prints both (DESIGN.md section 3 lists them).  hipGraphs are out of scope: a graph has no stream to stall."""
import copy
import itertools

import pytest
import torch

import nlt_amd
import stream_delay_util as SD
from nlt_amd import capi as C
from nlt_amd import nlt_test
from nlt_amd.datasets import get_dataset_class
from nlt_amd.datasets.nlt import ResidentTexels
from nlt_amd.datasets.synth import synthetic_store
from nlt_amd.models import get_model_class
from nlt_amd.pipeline import RenderPipeline
from oracle import nlt_oracle as O
from gpu_util import make_pair, to_device_batch

pytestmark = pytest.mark.gpu
UV, CAM, N = 64, 32, 2
KEYS = ('pred', 'pred_camspc', 'base_camspc')


def _batch(k, seed):
    return to_device_batch(*O.synth_batch(N, UV, UV, CAM, CAM, CAM, CAM, k=k, seed=seed))


def _render(pm, batch, **kw):
    """Model.call's rendered maps as tensors of this call's own (clones on the caller's stream)."""
    with torch.no_grad():
        out = pm.call(batch, 'test', **kw)
    return _own(out)


def _own(out):
    return {'cam': out[0].clone(), **{k: out[3][k].clone() for k in KEYS}}


def _diff(ref, got):
    """'' if every map is bit-equal, else which ones differ and in how many elements."""
    bad = []
    for k in ref:
        if not torch.equal(ref[k], got[k]):
            ne = ref[k] != got[k]
            bad.append("%s: %d of %d elements differ%s" % (k, int(ne.sum()), ne.numel(),
                                                           ", sentinel in the result" if bool((got[k] == SD.SENTINEL).any()) else ""))
    return '; '.join(bad)


def _self_check(models, run, ref, what, diff=_diff):
    """A poisoned pass without a stall must give the reference bits: a buffer for which it does not is state, not a result."""
    SD.poison(models)
    d = diff(ref, run())
    if d:
        torch.cuda.synchronize()
        culprits = SD.blame(models, run, lambda got: not diff(ref, got))
        pytest.fail("%s: a poisoned, unstalled pass differs from the reference (%s); buffers a pass reads before writing: %s"
                    % (what, d, culprits))


def _sweep(monkeypatch, models, run, ref, ms, streams, what, diff=_diff):
    """Delay points (i), after every event record of the pass, and (ii), at the start of each named stream: the poisoned pass
    must give the reference bits under each.  Returns the number of points."""
    with SD.delay_points(monkeypatch) as dp:
        d = diff(ref, run())
    assert not d, "%s: the undelayed pass under the hooks differs (%s)" % (what, d)
    nrec = len(dp.records)
    _self_check(models, run, ref, what, diff)
    for k in range(nrec):
        SD.poison(models)
        with SD.delay_points(monkeypatch, after_record=SD.stall_after_record(k, ms)) as dp2:
            got = run()
        assert len(dp2.records) == nrec, "%s: %d records, %d in the counting pass" % (what, len(dp2.records), nrec)
        d = diff(ref, got)
        assert not d, "%s: stall of %.1f ms behind event record %d of %d: %s" % (what, ms, k, nrec, d)
    for name, s in streams:
        SD.poison(models)
        SD.stall(s, ms)
        d = diff(ref, run())
        assert not d, "%s: stall of %.1f ms at the start of %s: %s" % (what, ms, name, d)
    torch.cuda.synchronize()
    print("stream-order %s: %d event records + %d streams swept" % (what, nrec, len(streams)))
    return nrec + len(streams)


def _own_streams(plan, bwd_streams=None):
    """Gives the plan side streams that were probed to run beside the caller's stream and beside each other
    (stream_delay_util.independent_streams) instead of whatever the stream pool would hand it: on two streams that share a
    hardware queue a stall delays both and no test between them can fail.  Before the plan's first pass."""
    s = SD.independent_streams(2 + (bwd_streams or 0))
    assert plan._side is None and plan._bside is None
    plan._side = (s[1], [C.new_event() for _ in range(plan.n_down + 3)])
    if bwd_streams:
        plan._bside = [s[2], [], None, s[3] if bwd_streams > 1 else None]


# ------------------------------------------------------------------------------------------------------ forward plans
def _infer_model(precision='fp32', k=2, seed=21, tape=False):
    _, pm = make_pair(depth=256, uv=UV, im=CAM, seed=seed, **({} if precision == 'fp32' else {'precision': precision}))
    pm.build('cuda')
    pm.plan.use_tape = tape
    _own_streams(pm.plan)
    batch = _batch(k, 30 + k)
    for _ in range(2):                                          # plan-time trials, then a pass on the chosen kernels
        _render(pm, batch)
    torch.cuda.synchronize()
    return pm, batch


def test_a_removed_wait_is_detected():
    """Vacuity guard.  The forward's final join (main waits for ev[D + 1] of the side stream) taken out and the side stream
    stalled at its start: the decoder reads the sentinel in the query halves of fm[l] -- memory the plan owns, wrong numbers,
    nothing else -- and the result MUST differ.  If it does not, the stall does not stall here and nothing below proves anything."""
    print("stream-order: " + SD.calibration())
    pm, batch = _infer_model()
    ref = _render(pm, batch)
    _, ms = SD.measured_stall(lambda: _render(pm, batch), 'forward fp32 k=2 (vacuity guard)')
    side, events = pm.plan._side
    join = events[pm.plan.n_down + 1]
    real = C.wait_event
    skipped = []

    def wait_event(stream, ev):
        if ev is join:
            skipped.append(stream)
            return
        real(stream, ev)
    try:
        C.wait_event = wait_event
        SD.poison(pm)
        SD.stall(side, ms)
        got = _render(pm, batch)
    finally:
        C.wait_event = real
        torch.cuda.synchronize()                                 # the side stream's late launches are through before anything else runs
    assert len(skipped) == 1
    d = _diff(ref, got)
    assert d, "the forward without its final join and with a %.1f ms stall on the side stream still gives the reference bits: " \
              "the stall does not hold a stream back on this machine, every stream-ordering test is vacuous" % ms
    print("stream-order vacuity guard: without the join -> " + d)
    assert not _diff(ref, _render(pm, batch))                    # whole again


@pytest.mark.parametrize('k', [2, 1])
@pytest.mark.parametrize('precision', ['fp32', 'f32x3_9', 'bf16'])
def test_forward_two_streams_under_every_delay_point(monkeypatch, precision, k):
    """k = 2: observation mean in the conv epilogue; k = 1: `alias_obs`, observation features written straight into fm[l];
    bf16: the observation means are launches of their own."""
    pm, batch = _infer_model(precision, k)
    assert pm.plan.two_streams and not pm.plan.use_tape
    what = 'forward %s k=%d' % (precision, k)
    ref = _render(pm, batch)
    _, ms = SD.measured_stall(lambda: _render(pm, batch), what)
    run = lambda: _render(pm, batch)
    cur = torch.cuda.current_stream()
    n = _sweep(monkeypatch, pm, run, ref, ms, [('the caller\'s stream', cur), ('plan._side[0]', pm.plan._side[0])], what)
    assert n == pm.plan.n_down + 1 + 2                           # ev[0], ev[2..D], ev[D + 1]; two streams
    # write-after-read between passes: the next pass's front kernel (and the poison in front of it) on main against the previous
    # pass's side-stream readers -- two passes back to back, the side stream held back at the start of each
    other = _batch(k, 40 + k)
    ref2 = _render(pm, other)
    torch.cuda.synchronize()
    SD.poison(pm)
    a = _render(pm, batch)
    SD.poison(pm)
    SD.stall(pm.plan._side[0], ms)
    b = _render(pm, other)
    assert not _diff(ref, a) and not _diff(ref2, b), (what, _diff(ref, a), _diff(ref2, b))
    SD.poison(pm)
    SD.stall(pm.plan._side[0], ms)
    a = _render(pm, batch)
    SD.poison(pm)
    SD.stall(pm.plan._side[0], ms)
    b = _render(pm, other)
    assert not _diff(ref, a) and not _diff(ref2, b), (what, _diff(ref, a), _diff(ref2, b))
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------- train step
def _train_model(fused, bwd_streams, k, tape=False):
    _, pm = make_pair(depth=256, uv=UV, im=CAM, loss='l2', seed=23, deterministic=True)
    assert pm.deterministic and not pm.plan.autotune
    pm.plan.use_tape, pm.plan.fuse_train, pm.plan.bwd_streams = tape, fused, bwd_streams
    pm.build('cuda')
    _own_streams(pm.plan, bwd_streams)
    batch = _batch(k, 50 + k)
    snap = {}
    r = pm.bucket_ranges
    # the snapshot an all-reduce of range i would take, made on the stream the hook runs on
    pm.plan.grad_hook = lambda i: snap.__setitem__(i, pm.flat_grads[r[i]:r[i + 1]].clone())

    def run():
        snap.clear()
        loss, _ = pm.train_forward_backward(batch, N)
        return {'loss': loss.clone(), 'grads': pm.flat_grads.clone(), **{'snap%d' % i: t for i, t in sorted(snap.items())}}
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    return pm, run


def _train_diff(pm):
    r = pm.bucket_ranges

    def diff(ref, got):
        bad = []
        if ref['loss'].cpu().numpy().tobytes() != got['loss'].cpu().numpy().tobytes():
            bad.append("loss %r != %r" % (float(got['loss']), float(ref['loss'])))
        if not torch.equal(ref['grads'], got['grads']):
            ne = ref['grads'] != got['grads']
            bad.append("flat_grads: %d of %d elements differ, first at %d" % (int(ne.sum()), ne.numel(), int(ne.nonzero()[0])))
        for i in (0, 1):                                         # the hook's snapshots against the FINAL bucket ranges of the reference
            key = 'snap%d' % i
            if key not in got:
                bad.append("the gradient hook did not fire for range %d" % i)
            elif not torch.equal(got[key], ref['grads'][r[i]:r[i + 1]]):
                ne = got[key] != ref['grads'][r[i]:r[i + 1]]
                bad.append("range %d as the hook saw it: %d of %d elements are not final" % (i, int(ne.sum()), ne.numel()))
        return '; '.join(bad)
    return diff


@pytest.mark.parametrize('bwd_streams', [0, 1, 2])
@pytest.mark.parametrize('fused', [True, False])
def test_train_step_and_the_overlap_hook_under_every_delay_point(monkeypatch, fused, bwd_streams):
    """Loss, flat gradient bucket and what the mid-backward hook sees of ranges 0 and 1 (the snapshot a collective would send),
    under a stall behind every event record of forward and backward, at the start of the main and both weight-gradient
    streams, in front of the fused end's backward launch (its gradients belong to range 0) and in front of the last weight
    gradient of each range on each side stream.  Stalls on the weight-gradient streams: a dgrad on main that overwrites a
    gradient buffer a queued wgrad still has to read; stalls on main: a wgrad that starts before its dpre is complete."""
    k = 1 if fused else 2                                        # fused: the training configs' one observation (split folded
    pm, run = _train_model(fused, bwd_streams, k)                # into the backward-data launches); unfused: `level_split` launches
    what = 'train step fused=%s bwd_streams=%d k=%d' % (fused, bwd_streams, k)
    diff = _train_diff(pm)
    ref = run()
    torch.cuda.synchronize()
    assert float(ref['grads'].abs().sum()) > 0 and not diff(ref, ref)
    _, ms = SD.measured_stall(run, what)
    bs = pm.plan._bside
    sides = [] if not bwd_streams else [('plan._bside[0]', bs[0])] + ([('plan._bside[3]', bs[3])] if bwd_streams > 1 else [])
    assert (bs is None) == (bwd_streams == 0) and len(sides) == bwd_streams
    fwd_side = [('plan._side[0]', pm.plan._side[0])] if fused else []      # (the layer-by-layer train forward is one stream)
    streams = [('the caller\'s stream', torch.cuda.current_stream())] + fwd_side + sides
    n = _sweep(monkeypatch, pm, run, ref, ms, streams, what, diff) - len(streams)
    # the fused forward's D + 1 records; one per dealt weight gradient (>= 2 per expanding block and 3 per level) + the joins
    assert n >= (pm.plan.n_down + 1 if fused else 0) + ((2 * (pm.plan.n_up - 2) + 3 * pm.plan.n_down + bwd_streams) if bwd_streams else 0)
    # (iii) named launches: a counting pass tells where they are
    hook = pm.plan.grad_hook
    with SD.delay_points(monkeypatch) as dp:
        pm.plan.grad_hook = lambda i: (dp.mark(i), hook(i))
        try:
            assert not diff(ref, run())
        finally:
            pm.plan.grad_hook = hook
    ends = {i: c for i, _, c in dp.marks}
    assert sorted(ends) == [0, 1]
    points = []
    if fused:
        (at,) = [i for i, (name, _) in enumerate(dp.calls) if name == 'nlt_back_backward']
        assert at < ends[0]
        points.append(('F.back.bwd on main', at))
    for i, lo in ((0, 0), (1, ends[0])):
        for name, s in sides:
            wg = [j for j in range(lo, ends[i]) if 'backward_weights' in dp.calls[j][0] and dp.calls[j][1] == s.cuda_stream]
            assert wg, (what, 'no weight gradient of range %d on %s' % (i, name))
            points.append(('the last weight gradient of range %d on %s' % (i, name), wg[-1]))
    for name, at in points:
        SD.poison(pm)
        with SD.delay_points(monkeypatch, before_call=SD.stall_before_call(at, ms)) as dp3:
            got = run()
        assert dp3.calls == dp.calls
        d = diff(ref, got)
        assert not d, "%s: stall of %.1f ms in front of %s (launch %d, %s): %s" % (what, ms, name, at, dp.calls[at][0], d)
    torch.cuda.synchronize()
    print("stream-order %s: %d named launches: %s" % (what, len(points), [p for p, _ in points]))


# -------------------------------------------------------------------------------------------------------- tape replays
def _store_setup(k=1, frames=12):
    store = synthetic_store(frames, UV, CAM, seed=5, k=k)
    cfg = nlt_amd.make_config(depth=256, uvh=UV, uvw=UV, imh=CAM, imw=CAM, bs=N)
    pm = get_model_class('nlt')(cfg).build('cuda')
    pm.register_trainable()
    _own_streams(pm.plan)
    g = torch.Generator(device='cuda').manual_seed(9)
    with torch.no_grad():
        for c in pm._conv_layers():
            c.bias.uniform_(-0.1, 0.1, generator=g)
    ds = get_dataset_class('nlt')(cfg, 'train', store, k=k, ring=0)
    id_lists = [store['ids'][i * N:(i + 1) * N] for i in range(frames // N)]
    return pm, ds, id_lists


@pytest.mark.parametrize('native', [False, True])
def test_forward_tape_replays_with_a_stalled_stream(native):
    """Float and store-resident batches: once the tape is recorded (third sight), poison, stall each stream at its start in
    turn, replay.  native: the replay walks the recorded calls in C (`set_thread_native_replay`)."""
    pm, ds, id_lists = _store_setup(k=2, frames=4)
    assert pm.plan.use_tape
    for resident in (False, True):
        batch = ds.load_batch(id_lists[1], resident=resident)
        what = 'forward tape replay %s%s' % ('resident' if resident else 'float', ' native' if native else '')
        for _ in range(3):
            ref = _render(pm, batch)
        _, ms = SD.measured_stall(lambda: _render(pm, batch), what)
        run = lambda: _render(pm, batch)
        _self_check(pm, run, ref, what)
        C.set_thread_native_replay(native)
        try:
            for name, s in (('the caller\'s stream', torch.cuda.current_stream()), ('plan._side[0]', pm.plan._side[0])):
                before = pm.plan.tape_replays
                SD.poison(pm)
                SD.stall(s, ms)
                d = _diff(ref, run())
                assert not d, "%s: stall of %.1f ms at the start of %s: %s" % (what, ms, name, d)
                assert pm.plan.tape_replays == before + 1
        finally:
            C.set_thread_native_replay(False)
        torch.cuda.synchronize()


@pytest.mark.parametrize('native', [False, True])
def test_train_step_tape_replays_with_a_stalled_stream(native):
    pm, run = _train_model(True, 2, 1, tape=True)
    what = 'train step tape replay' + (' native' if native else '')
    diff = _train_diff(pm)
    for _ in range(2):                                           # (two passes were made: this is sight 3, a replay, and sight 4)
        ref = run()
    torch.cuda.synchronize()
    assert pm.plan.tape_replays >= 2
    _, ms = SD.measured_stall(run, what)
    _self_check(pm, run, ref, what, diff)
    bs = pm.plan._bside
    C.set_thread_native_replay(native)
    try:
        for name, s in (('the caller\'s stream', torch.cuda.current_stream()), ('plan._side[0]', pm.plan._side[0]),
                        ('plan._bside[0]', bs[0]), ('plan._bside[3]', bs[3])):
            before = pm.plan.tape_replays
            SD.poison(pm)
            SD.stall(s, ms)
            d = diff(ref, run())
            assert not d, "%s: stall of %.1f ms at the start of %s: %s" % (what, ms, name, d)
            assert pm.plan.tape_replays == before + 2            # forward and backward tape
    finally:
        C.set_thread_native_replay(False)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------- pipeline
class _Ctx:
    """One model, one dataset and the sequential references of every pipeline test (computed once, never changed)."""

    def __init__(self):
        self.pm, ds, id_lists = _store_setup(k=1, frames=12)
        self.batches = {r: [ds.load_batch(ids, resident=r) for ids in id_lists] for r in (False, True)}
        self.agg = [a.clone() for a in nlt_test.extract_feat(self.pm, self.batches[False][:2])]
        self.keep = []              # every override state a reference was made with stays allocated: a later build cannot be
        self.serial = itertools.count()    # handed memory that already holds the right maps
        self.maps()                 # plan-time trials of the override plan ...
        self.plain = {r: [_render(self.pm, b) for b in self.batches[r]] for r in (False, True)}
        # ... and of the ordinary forward are over; the plan keeps ONE buffer set, so every switch between the two kinds of
        # pass would run them again (and choose by the clock again)
        self.pm.plan.autotune = False
        self.plain = {r: [_render(self.pm, b) for b in self.batches[r]] for r in (False, True)}
        torch.cuda.synchronize()

    def maps(self, scale=None):
        """A fresh set of override maps and the sequential renders with (a copy of) them.  scale None: `agg` itself; else
        a * scale + 0.01 -- 0.5 first (agg2 = a * 0.5 + 0.01); every later set gets a scale of its own, so that no memory a build is handed
        can hold the right maps by coincidence."""
        vals = [a.clone() if scale is None else a * scale + 0.01 for a in self.agg]
        twin = [v.clone() for v in vals]
        ref = {r: [_render(self.pm, b, obs_override=twin) for b in self.batches[r][:4]] for r in (False, True)}
        self.keep.append((twin, self.pm.plan.q._ovr_state))
        torch.cuda.synchronize()
        return vals, ref

    def throwaway(self):
        """Maps nobody renders a reference for: what a timed round switches to (a state build + first-sight passes per round)."""
        return [a * self.new_scale() + 0.01 for a in self.agg]

    def new_scale(self):
        return 0.5 + next(self.serial) / 64.0                    # 0.5 first: agg2 = a * 0.5 + 0.01


@pytest.fixture(scope='module')
def ctx():
    c = _Ctx()
    yield c
    torch.cuda.synchronize()


COMBOS = [(lanes, threads, resident) for lanes in (2, 3) for threads in (False, True) for resident in (False, True)]


def _warm_pipeline(ctx, lanes, threads, resident, **kw):
    """One pipeline object for the whole test, two rounds through it before anything is measured."""
    pipe = RenderPipeline(ctx.pm, lanes, threads=threads)
    pipe._streams = SD.independent_streams(lanes + 1)[1:]        # lanes that a stall can tell apart from each other and the caller
    batches = ctx.batches[resident][:lanes]
    for _ in range(2):
        for t in [pipe.submit(b, 'test', **kw) for b in batches]:
            t.result()
    torch.cuda.synchronize()
    return pipe, batches


def _round(pipe, batches, **kw):
    """Every batch through the pipeline; results as clones on the caller's stream behind `ticket.result()`."""
    tickets = []
    for b in batches:
        tickets.append(pipe.submit(b, 'test', **kw))
        if pipe._threads:
            pipe.drain()                                         # (host: that lane has issued its batch -- who builds a shared
    return [_own(t.result()) for t in tickets]                   #  state is then the submission order, not a race of threads)


def _late_twin(batch):
    """A batch at new addresses whose contents arrive LATE: zeros now (in-bounds frame ids and warp coordinates -- a lane that
    does not wait renders frame 0 from the wrong place, it does not leave the stores), the real contents by `fill()`."""
    pairs = []

    def twin(t):
        z = torch.zeros_like(t)
        pairs.append((z, t))
        return z
    out = []
    for x in batch:
        if torch.is_tensor(x) and x.is_cuda:
            out.append(twin(x))
        elif isinstance(x, ResidentTexels):
            y = copy.copy(x)
            y.ids, y.nn_ids = twin(x.ids), twin(x.nn_ids)
            y._float = y._base = y._warp = None
            out.append(y)
        else:
            out.append(x)
    return tuple(out), lambda: [z.copy_(t) for z, t in pairs]


@pytest.mark.parametrize('lanes,threads,resident', COMBOS)
def test_warm_pipeline_waits_for_its_inputs_and_the_caller_for_its_lanes(ctx, lanes, threads, resident):
    pipe, batches = _warm_pipeline(ctx, lanes, threads, resident)
    what = 'pipeline %d lanes%s %s' % (lanes, ' threads' if threads else '', 'resident' if resident else 'float')
    ref = ctx.plain[resident][:lanes]
    try:
        models = list(pipe._lanes)
        _, ms = SD.measured_stall(lambda: _round(pipe, batches), what)
        SD.poison(models)                                        # self-check
        for i, (r, g) in enumerate(zip(ref, _round(pipe, batches))):
            assert not _diff(r, g), "%s: poisoned, unstalled round, batch %d: %s" % (what, i, _diff(r, g))
        # (a) the batch tensors are produced on the caller's stream behind a stall: the lanes must wait for their inputs
        cur = torch.cuda.current_stream()
        twins = [_late_twin(b) for b in batches]
        torch.cuda.synchronize()
        SD.poison(models)
        SD.stall(cur, ms)
        for _, fill in twins:
            fill()
        for i, (r, g) in enumerate(zip(ref, _round(pipe, [b for b, _ in twins]))):
            assert not _diff(r, g), "%s: (a) inputs late by %.1f ms on the caller's stream, batch %d: %s" % (what, ms, i, _diff(r, g))
        # (b) a lane's stream is held back: result() + a clone on the caller's stream must still see the finished batch
        for lane in range(lanes):
            SD.poison(models)
            SD.stall(pipe._streams[lane], ms)
            for i, (r, g) in enumerate(zip(ref, _round(pipe, batches))):
                assert not _diff(r, g), "%s: (b) lane %d held back by %.1f ms, batch %d: %s" % (what, lane, ms, i, _diff(r, g))
        torch.cuda.synchronize()
    finally:
        pipe.close()


def _align(pipe, lane, batch, **kw):
    """Submits (and collects) until `lane` is the next one to be given a batch."""
    while pipe._next % pipe.n != lane:
        pipe.submit(batch, 'test', **kw).result()
    pipe.drain()
    torch.cuda.synchronize()


@pytest.mark.parametrize('lanes,threads,resident', COMBOS)
def test_override_state_hand_off_between_lanes_of_a_warm_pipeline(ctx, lanes, threads, resident):
    """(c) Rendering with `agg`, then -- no weight change, so `submit` synchronises nothing -- batches with a NEW feat_agg:
    lane i builds the override state on its stream, every other lane is handed the cached state.  With lane i's stream held
    back, a lane that does not wait for the build reads maps that have not been written yet."""
    cases = ((0, 0, False), (1, 1, False), (1, (1 + 1) % lanes, False), (lanes - 1, lanes - 1, True))
    # every sequential reference first: a reference pass builds (and leaves behind) an override state of its own
    agg, ref_agg = ctx.maps()
    sets = [ctx.maps(ctx.new_scale()) for _ in cases]
    pipe, batches = _warm_pipeline(ctx, lanes, threads, resident, obs_override=agg)
    what = 'override hand-off %d lanes%s %s' % (lanes, ' threads' if threads else '', 'resident' if resident else 'float')
    try:
        models = list(pipe._lanes)
        # the undelayed pass of THIS scenario: a round that switches to new maps (state build, first-sight passes)
        _, ms = SD.measured_stall(lambda: _round(pipe, batches, obs_override=ctx.throwaway()), what)
        for i, (r, g) in enumerate(zip(ref_agg[resident], _round(pipe, batches, obs_override=agg))):
            assert not _diff(r, g), "%s: warm round with agg, batch %d: %s" % (what, i, _diff(r, g))
        # builder lane, stalled lane, a round without override in between (the sequence ADVICE.md names)
        for (builder, stalled, between), (new, ref_new) in zip(cases, sets):
            if between:
                for i, (r, g) in enumerate(zip(ctx.plain[resident], _round(pipe, batches))):
                    assert not _diff(r, g), "%s: round without override, batch %d: %s" % (what, i, _diff(r, g))
            _align(pipe, builder, batches[0], **({} if between else {'obs_override': agg}))
            serial = ctx.pm.plan.q._ovr_state['serial']
            SD.poison(models)
            SD.stall(pipe._streams[stalled], ms)
            order = [batches[(builder + j) % lanes] for j in range(lanes)]          # lane `builder` first, then its consumers
            want = [ref_new[resident][(builder + j) % lanes] for j in range(lanes)]
            got = _round(pipe, order, obs_override=new)
            assert ctx.pm.plan.q._ovr_state['serial'] != serial                      # a new state was built inside the pipeline
            for j, (r, g) in enumerate(zip(want, got)):
                assert not _diff(r, g), ("%s: lane %d builds the state for the new maps, lane %d is held back by %.1f ms%s: the batch of "
                                         "lane %d differs from pm.call(batch, 'test', obs_override=agg2): %s"
                                         % (what, builder, stalled, ms, ', a round without override before' if between else '',
                                            (builder + j) % lanes, _diff(r, g)))
            torch.cuda.synchronize()
            agg = new
    finally:
        pipe.close()


def _state_memory(st):
    """[(address, bytes, dtype)] of every device tensor the override state made: its maps, derived kernels and fragments."""
    found = []

    def walk(x):
        if torch.is_tensor(x):
            if x.is_cuda and x.numel():
                found.append((x.data_ptr(), x.numel() * x.element_size(), x.dtype))
        elif isinstance(x, dict):
            for v in x.values():
                walk(v)
        elif isinstance(x, (list, tuple)):
            for v in x:
                walk(v)
        elif hasattr(x, '_packed'):
            walk((x.kernel, x.bias, x._packed, getattr(x, '_packed_bf', None)))
    walk({k: v for k, v in st.items() if k not in ('stamp', 'serial', 'ovr', 'ready', 'streams')})
    return found


@pytest.mark.parametrize('lanes,threads,resident', COMBOS)
def test_replaced_override_state_outlives_the_lanes_that_still_read_it(ctx, lanes, threads, resident):
    """(d) A batch with `agg` is queued on lane j behind a stall; every lane (j last, behind its own stall) then switches to new
    maps, which lets the old state go, and nothing the test holds refers to it any more.  Tensors of the old maps' sizes are
    then allocated and sentinel-filled on every lane's stream -- what a later `torch.empty` and a kernel would do.  Lane j's
    delayed batch must still come out with its sequential bits."""
    old, ref_old = ctx.maps(ctx.new_scale())
    new, ref_new = ctx.maps(ctx.new_scale())
    first = ctx.throwaway()
    pipe, batches = _warm_pipeline(ctx, lanes, threads, resident, obs_override=first)
    what = 'replaced override state %d lanes%s %s' % (lanes, ' threads' if threads else '', 'resident' if resident else 'float')
    try:
        models = list(pipe._lanes)
        j = 1
        # the undelayed pass of THIS scenario: a round that switches to new maps (state build, first-sight passes)
        _, ms = SD.measured_stall(lambda: _round(pipe, batches, obs_override=ctx.throwaway()), what)
        _align(pipe, 0, batches[0], obs_override=first)
        got = _round(pipe, batches, obs_override=old)             # lane 0 builds the old state, the others are handed it
        for i, (r, g) in enumerate(zip(ref_old[resident], got)):
            assert not _diff(r, g), "%s: round with the old maps, batch %d: %s" % (what, i, _diff(r, g))
        _align(pipe, j, batches[0], obs_override=old)
        st = ctx.pm.plan.q._ovr_state
        memory = _state_memory(st)
        assert len(memory) >= 10
        del st
        SD.poison(models)
        SD.stall(pipe._streams[j], ms)
        delayed = _round_submit(pipe, [batches[j]], obs_override=old)
        del old
        order = [(j + 1 + i) % lanes for i in range(lanes)]       # every lane switches; lane j last, behind its stall
        tickets = _round_submit(pipe, [batches[i] for i in order], obs_override=new)
        hits, fills = 0, []
        for s in pipe._streams:
            with torch.cuda.stream(s):
                for _, nbytes, dtype in memory:
                    t = torch.empty(nbytes // torch.empty(0, dtype=dtype).element_size(), device='cuda', dtype=dtype)
                    t.fill_(SD.SENTINEL)
                    fills.append(t)
        addresses = {a for a, _, _ in memory}
        hits = sum(1 for t in fills if t.data_ptr() in addresses)
        print("stream-order %s: %d of %d sentinel tensors were handed the address of a tensor of the replaced state"
              % (what, hits, len(fills)))
        d = _diff(ref_old[resident][j], _own(delayed[0].result()))
        assert not d, ("%s: lane %d's batch, queued with the old maps behind a %.1f ms stall, was rendered after the old state's memory "
                       "was handed out again (%d of %d sentinel tensors got an old address): %s" % (what, j, ms, hits, len(fills), d))
        for i, t in zip(order, tickets):
            d = _diff(ref_new[resident][i], _own(t.result()))
            assert not d, "%s: batch of lane %d with the new maps: %s" % (what, i, d)
        torch.cuda.synchronize()
    finally:
        pipe.close()


def _round_submit(pipe, batches, **kw):
    tickets = []
    for b in batches:
        tickets.append(pipe.submit(b, 'test', **kw))
        if pipe._threads:
            pipe.drain()
    return tickets
