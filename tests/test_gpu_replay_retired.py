"""-m gpu: replays after the buffers they baked in were let go.

Three mechanisms bake device addresses into something that outlives the call: the launch tapes of RenderPlan (`_run_taped`), the
inference hipGraphs of Model (`use_graphs`; the lanes of RenderPipeline(graphs=True) use the same) and trainvali.GraphedTrainStep.
The project lets such memory go in two places: `RenderPlan._buffers` keeps ONE shape resident (a call at any other (n, k, h, w)
drops the whole activation set), and `_capi._workspace` replaces a cached scratch tensor when a larger one is needed -- the
per-device families (front_bwd, back_bwd, wgrad_*) by ANY model of the process.  A replay that still points at the old memory
returns the right result (it reads what it wrote) and overwrites whoever owns that memory now.

Every scenario: bring the mechanism into its replay state, let `retire_util.Retired` watch a disturbing action, then
  (i)   something must really have been retired,
  (ii)  arm the retired tensors with a sentinel, run the replay path again, and none of them may have been written,
  (iii) the results equal the undisturbed reference,
and the mechanism must be replaying again after one or two further calls (re-recording / re-capturing is fine, staying eager
is not).  `plan.autotune = False` everywhere: the kernels are the heuristics', a forward repeats bit for bit.

What each replay can reach (read off the code, confirmed by the mutations named in DESIGN.md section 3): a forward bakes in the
plan's buffer set and, only where a split-K choice is stored, scratch keyed by (stream, plan) that no other model can grow -- so
in (b) and (e) the grown scratch is memory the forward never pointed into, and the scenarios pin that the guard costs no
correctness.  The backward (c) and the train graph (i) do point into the shared families."""
import numpy as np
import pytest
import torch

import nlt_amd
from nlt_amd import capi as C
from nlt_amd import trainvali
from nlt_amd.pipeline import RenderPipeline
from oracle import nlt_oracle as O
from gpu_util import make_pair, to_device_batch
from retire_util import Retired
from test_gpu_pipeline import _setup, _same

pytestmark = pytest.mark.gpu

UV, CAM = 64, 32


def _fresh_scratch():
    """The scratch cache is the process's: a family an earlier test (or an earlier leg of this one) grew would never grow
    again.  Every test and every leg starts from an empty cache; the epoch moves, so whatever tape or graph is still alive
    knows."""
    C._ws_cache.clear()
    C._alloc_epoch[0] += 1


@pytest.fixture(autouse=True)
def fresh_scratch():
    _fresh_scratch()
    yield


def _model(seed=9, uv=UV, cam=CAM, **kw):
    _, pm = make_pair(depth=256, uv=uv, im=cam, loss='l2', seed=seed, **kw)
    pm.build('cuda')
    pm.plan.autotune = False
    return pm


def _batch(n, seed, uv=UV, cam=CAM, k=2):
    return to_device_batch(*O.synth_batch(n, uv, uv, cam, cam, cam, cam, k=k, seed=seed))


def _ab():
    """Batch A (n = 2, k = 2) and batch B (n = 1, k = 2): made once per test, so A keeps its addresses throughout."""
    return _batch(2, 60), _batch(1, 61)


class _Big:
    """A second, larger model in the same process (depth 256, UV 128^2, camera 64^2, n = 2 unless told otherwise): one
    forward and one train step of it grow the scratch families every model of the process shares."""

    def __init__(self, uv=128, cam=64, n=2, k=2):
        self.model = _model(seed=17, uv=uv, cam=cam)
        self.batch = _batch(n, 18, uv, cam, k)
        self.opt = nlt_amd.optim.AdamAMSGrad(self.model, 1e-3)
        self.n = n

    def run(self, side_of=None):
        """side_of = a plan whose weight-gradient side stream this model's plan shall get too: torch deals side streams round
        robin from a small pool, so a process with enough plans sees two of them on one stream -- and their per-stream
        weight-gradient scratch is then one buffer.  The pool is turned until the next stream it deals is that one."""
        e0 = C._alloc_epoch[0]
        with torch.no_grad():
            self.model.call(self.batch, 'test')
        if side_of is not None:
            want = side_of._bside[0].cuda_stream
            seen = []
            while seen.count(want) < 2:                                  # dealt twice: the distance is the pool's period
                assert len(seen) < 256, "the stream pool never dealt the side stream again"
                seen.append(torch.cuda.Stream().cuda_stream)
            period = len(seen) - 1 - seen.index(want)
            for _ in range(period - 1):
                torch.cuda.Stream()
        trainvali.distributed_train_step(self.model, self.batch, self.opt, self.n)
        torch.cuda.synchronize()
        if side_of is not None:
            assert self.model.plan._bside[0].cuda_stream == side_of._bside[0].cuda_stream
        assert C._alloc_epoch[0] > e0, "the big model allocated no scratch"


def _own_scratch(pm, batch):
    """One train step of the model itself, so that it owns scratch of the shared families at ITS size (an ordinary history:
    train, then evaluate) -- what a larger model then replaces."""
    trainvali.distributed_train_step(pm, batch, nlt_amd.optim.AdamAMSGrad(pm, 1e-3), batch[1].shape[0])
    torch.cuda.synchronize()


def _test_call(pm, batch):
    with torch.no_grad():
        out = pm.call(batch, 'test')
    torch.cuda.synchronize()
    return out[3]['pred'], out[0]


# ---------------------------------------------------------------- (a), (b): the forward launch tape
@pytest.mark.parametrize('disturbance', ['other_shape', 'big_model'])
def test_forward_tape_after_its_buffers_or_the_scratch_were_let_go(disturbance):
    """(a) call(B) at another batch size drops A's buffer set -- the tapes hang under it and go with it.  (b) a bigger model grows
    the shared scratch: `_alloc_epoch` moves and `tape_valid` refuses every older tape."""
    pm = _model()
    A, B = _ab()
    big = _Big() if disturbance == 'big_model' else None
    if big is not None:
        _own_scratch(pm, A)
    ref_pred, ref_cam = (t.clone() for t in _test_call(pm, A))              # the first, eager call
    for _ in range(2):
        _test_call(pm, A)
    assert pm.plan.tape_replays >= 1                                         # eager, recorded, replayed
    e0 = C._alloc_epoch[0]
    with Retired(pm) as r:
        if big is None:
            _test_call(pm, B)
        else:
            big.run()
            assert C._alloc_epoch[0] > e0
    assert r.retired, "the disturbance retired nothing"
    r.arm()
    replays = pm.plan.tape_replays
    outs = [_test_call(pm, A) for _ in range(3)]
    r.check()
    for pred, cam in outs:
        assert torch.equal(pred, ref_pred) and torch.equal(cam, ref_cam)
    assert pm.plan.tape_replays > replays                                    # ... and it is replaying again


# ---------------------------------------------------------------- (c): the backward launch tape
@pytest.mark.parametrize('n', [2, 1])
def test_backward_tape_after_a_bigger_model_grew_every_scratch_family_it_uses(n):
    """The loop of test_backward_plan_is_bit_reproducible_given_the_texel_gradient at UV 256 (k = 1, three passes): its backward
    tape points into front_bwd, back_bwd and the weight-gradient families.  A model at UV 512^2 (n = 2) replaces them.
    n = 2 is that test's batch; there front_bwd is already as large as it ever gets (its size query caps the workgroups at 1536,
    reached at 6144 groups of 8 texels: n = 2 at 256^2 has 8192), so no model can retire it -- the test asserts exactly that
    and holds every other family to "replaced".  n = 1 (4096 groups) is below the cap: there EVERY family the backward used,
    front_bwd included, must have been replaced."""
    uv = 256
    pm = _model(seed=31, uv=uv, cam=uv // 2)
    batch = _batch(n, 32, uv, uv // 2, k=1)
    base, cvis, lvis, nn_base, nn_rgb = batch[1], batch[2], batch[3], batch[8], batch[9]
    g = torch.Generator(device='cuda').manual_seed(5)
    dpred = (torch.rand((n, uv, uv, 3), device='cuda', generator=g) - 0.5).contiguous()

    def one_pass():
        with torch.no_grad():
            pm._render(base, cvis, lvis, batch[4], nn_rgb, nn_base, None, None, False, inference=False)
            pm.flat_grads.zero_()
            pm.plan.backward(dpred, base, cvis, lvis, nn_rgb, nn_base, None, generation=pm.plan.generation)
        torch.cuda.synchronize()
        return pm.flat_grads.clone()

    big = _Big(uv=512, cam=256, n=2, k=1)
    runs = [one_pass() for _ in range(3)]
    assert float(runs[0].abs().max()) > 0 and pm.plan.tape_replays >= 1
    assert all(torch.equal(x, runs[0]) for x in runs[1:])
    fam = lambda key: key[1].split('.')[0] if isinstance(key[1], str) else 'splitk'
    used = {key: t for key, t in C._ws_cache.items() if fam(key) in ('front_bwd', 'back_bwd') or fam(key).startswith('wgrad')}
    assert {'front_bwd', 'back_bwd'} <= {fam(k) for k in used} and any(fam(k).startswith('wgrad') for k in used), sorted(used)
    front = lambda *shape: C._size('nlt_front_backward_workspace_floats', *shape)
    capped = {k for k in used if fam(k) == 'front_bwd' and front(n, uv, uv) == front(2, 512, 512)}
    assert bool(capped) == (n == 2)
    with Retired(pm) as r:
        big.run(side_of=pm.plan)
    stayed = {key for key, t in used.items() if C._ws_cache[key] is t}
    assert stayed == capped, "scratch the backward used was not replaced: %r" % (sorted(stayed - capped),)
    assert r.retired and set(r.paths()) >= {'_ws_cache[%r]' % (k,) for k in used if k not in capped}
    r.arm()
    replays = pm.plan.tape_replays
    after = [one_pass() for _ in range(3)]
    r.check()
    assert all(torch.equal(x, runs[0]) for x in after)
    assert pm.plan.tape_replays > replays


# ---------------------------------------------------------------- (d), (e): the inference hipGraphs
@pytest.mark.parametrize('disturbance', ['other_shape', 'big_model'])
def test_inference_graph_after_its_buffers_or_the_scratch_were_let_go(disturbance):
    """(d) use_graphs: call(A) x 4, call(B), call(A) x 3 -- an evaluation loop whose last batch is short, then repeated.  (e) the
    big model in between instead.  The graph of A must not be replayed over the buffer set call(B) dropped."""
    pm = _model()
    A, B = _ab()
    big = _Big() if disturbance == 'big_model' else None
    if big is not None:
        _own_scratch(pm, A)
    ref_pred, ref_cam = (t.clone() for t in _test_call(pm, A))              # eager
    pm.use_graphs = True
    for i in range(4):
        pred, cam = _test_call(pm, A)
        assert torch.equal(pred, ref_pred) and torch.equal(cam, ref_cam), i
    assert pm._graph['graph'] is not None and pm._graph['hits'] >= 1
    with Retired(pm) as r:
        if big is None:
            _test_call(pm, B)
        else:
            big.run()
    assert r.retired, "the disturbance retired nothing"
    r.arm()
    outs = [tuple(t.clone() for t in _test_call(pm, A)) for _ in range(3)]
    r.check()
    for pred, cam in outs:
        assert torch.equal(pred, ref_pred) and torch.equal(cam, ref_cam)
    assert pm._graph['graph'] is not None and pm._graph['hits'] >= 1         # captured (again) and replayed
    hits = pm._graph['hits']
    A[1].mul_(0.5)                                                           # base changes in place: the replay follows it
    pred, cam = (t.clone() for t in _test_call(pm, A))
    assert pm._graph['hits'] == hits + 1
    pm.use_graphs = False
    e_pred, e_cam = _test_call(pm, A)
    assert torch.equal(pred, e_pred) and torch.equal(cam, e_cam) and not torch.equal(pred, ref_pred)
    r.check()


# ---------------------------------------------------------------- (f), (g): pipeline lanes over batches of 2, 2, 1, 2, 2 frames
@pytest.mark.parametrize('kind,lanes', [('graphs', 2), ('threads', 3)])
def test_pipeline_lanes_over_a_store_whose_middle_batch_is_short(kind, lanes):
    """The same five batch objects round after round; the short one changes the shape on whichever lane it lands.  (f) graphs:
    every lane replays one hipGraph per set of input addresses.  (g) threads: launch tapes, one host thread per lane."""
    pm, ds, id_lists = _setup(uv=64, cam=32, k=2, frames=10)
    pm.plan.autotune = False
    id_lists[2] = id_lists[2][:1]
    batches = [ds.load_batch(ids) for ids in id_lists]
    assert [b[1].shape[0] for b in batches] == [2, 2, 1, 2, 2]
    with torch.no_grad():
        ref = [pm.call(b, 'test') for b in batches]
    torch.cuda.synchronize()
    pipe = RenderPipeline(pm, lanes, threads=kind == 'threads', graphs=kind == 'graphs')

    def one_round():
        outs = [t.result() for t in [pipe.submit(b, 'test') for b in batches]]
        torch.cuda.synchronize()
        for a, b in zip(ref, outs):
            _same(a, b)

    one_round()
    assert all(l is not None for l in pipe._lanes)
    with Retired(list(pipe._lanes)) as r:
        one_round()
        one_round()
    assert r.retired, "no lane let a buffer set go"
    r.arm()
    for _ in range(3):                                  # (5 batches over 2 lanes: a lane meets the same batch every other round)
        one_round()
    r.check()
    # ... and a lane that sees one shape only is in its replay state after three sights
    for _ in range(3):
        outs = [t.result() for t in [pipe.submit(b, 'test') for b in batches[:lanes]]]
        torch.cuda.synchronize()
        for a, b in zip(ref, outs):
            _same(a, b)
    r.check()
    if kind == 'graphs':
        assert all(l._graph['graph'] is not None and l._graph['hits'] >= 1 for l in pipe._lanes), [l._graph['hits'] for l in pipe._lanes]
    else:
        assert all(l.plan.tape_replays >= 1 for l in pipe._lanes)
    pipe.close()


# ---------------------------------------------------------------- (h), (i), (j): the graphed train step
def _train_leg(graphed, disturbance, deterministic, watch):
    """3 steps on A, the disturbance, 3 more steps on A, from the same seed and the same plan choices; `watch`: Retired around
    the disturbance, armed before and checked after the last three steps."""
    _fresh_scratch()
    pm = _model(seed=9)
    if deterministic:
        pm.deterministic = True
    A, B = _ab()
    big = _Big() if disturbance == 'big_model' else None
    opt = nlt_amd.optim.AdamAMSGrad(pm, 1e-3)
    step = trainvali.GraphedTrainStep(pm, opt, 2, warmup=1) if graphed else (lambda b: trainvali.distributed_train_step(pm, b, opt, 2))
    losses = [float(step(A)[0]) for _ in range(3)]
    if graphed:
        assert step.failed is None and step.graph is not None
    extra = {}

    def disturb():
        if big is not None:
            big.run()
            return
        lv, _ = trainvali.distributed_vali_step(pm, B, 1)
        extra['vali'] = float(lv)
        extra['pred'] = _test_call(pm, B)[0].clone()

    r = None
    if watch:
        with Retired(pm) as r:
            disturb()
        assert r.retired, "the disturbance retired nothing"
        r.arm()
    else:
        disturb()
    losses += [float(step(A)[0]) for _ in range(3)]
    torch.cuda.synchronize()
    if r is not None:
        r.check()
    if graphed:
        assert step.failed is None and step.graph is not None               # captured again, not eager for good
    return losses, pm.flat_params.detach().clone(), extra


def _within_bars(got, want):
    """The bars of test_graphed_train_step_replays_the_same_step_as_the_eager_one: losses rtol 1e-4, weights max-abs 1e-4 (the
    validation loss under the losses' bar, the rendered texels under the weights')."""
    np.testing.assert_allclose(got[0], want[0], rtol=1e-4)
    assert float((got[1] - want[1]).abs().max()) < 1e-4
    if want[2]:
        np.testing.assert_allclose(got[2]['vali'], want[2]['vali'], rtol=1e-4)
        assert float((got[2]['pred'] - want[2]['pred']).abs().max()) < 1e-4


@pytest.mark.parametrize('disturbance', ['other_shape', 'big_model'])
def test_graphed_train_step_after_its_buffers_or_the_scratch_were_let_go(disturbance):
    """(h) a validation step and a test call at another batch size between graphed train steps; (i) a bigger model's train step.
    Against a second model run eagerly through the identical sequence."""
    eager = _train_leg(False, disturbance, False, watch=False)
    graphed = _train_leg(True, disturbance, False, watch=True)
    _within_bars(graphed, eager)


def test_deterministic_graphed_train_step_after_its_buffers_were_let_go():
    """(j) `model.deterministic = True`: two eager legs through the sequence of (h) measure the eager step against itself; where they
    are bit-equal the graphed leg must be bit-equal to them too, else the bars of (h) hold.  Outcome on MI355X: see DESIGN.md
    section 3."""
    e1 = _train_leg(False, 'other_shape', True, watch=False)
    e2 = _train_leg(False, 'other_shape', True, watch=False)
    graphed = _train_leg(True, 'other_shape', True, watch=True)
    bit_equal = (e1[0] == e2[0] and torch.equal(e1[1], e2[1]) and e1[2]['vali'] == e2[2]['vali']
                 and torch.equal(e1[2]['pred'], e2[2]['pred']))
    print("deterministic eager legs bit-equal: %s; graphed vs eager max |dw| %.3e, losses %r vs %r"
          % (bit_equal, float((graphed[1] - e1[1]).abs().max()), graphed[0], e1[0]))
    if bit_equal:
        assert graphed[0] == e1[0] and torch.equal(graphed[1], e1[1])
        assert graphed[2]['vali'] == e1[2]['vali'] and torch.equal(graphed[2]['pred'], e1[2]['pred'])
    else:
        _within_bars(graphed, e1)
