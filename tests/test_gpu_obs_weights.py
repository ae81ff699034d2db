"""-m gpu: `obs_weights` -- the per-frame, per-observation factor of the aggregate (nlt/models/nlt.py:141-164) -- through every
plan, forward and train step, against the oracle.

The argument selects a route of its own: the fused ends refuse it, so every forward is the layer-by-layer plan (`L0.stem` with
weights, every `L*.o.s1` on `_conv` + a separate weighted `*.mean` launch); the backward drops the level-split fold and the fused
`level_split_backward` for `*.q.s1.act` + `*.o.mean` per level and ends in `nlt_stem_backward` with weights; no launch tape, no
hipGraph, no bf16.  Each case spies the adapters and asserts that this route is what ran.

Inputs (tests/obs_weights_util.py): n != k, weights with an exact 0, negative values and values > 1, and -- asserted on the oracle
in every case's setup -- a weighted result >= 1000 x the case's bar away from the unweighted one and from the ones under the
weights flipped along the frame / observation axis.  A swapped index, a weight applied to the features handed to the next level, a
stale tape or graph replayed for a weighted call or a missing 1 / k cannot pass.

Bars are the suite's own (tests/test_gpu_nonsquare.py, test_gpu_fused.py, test_gpu_tape.py): `pred`, `pred_camspc` <= 1e-4 rel-L2,
`base_camspc` / `gt_camspc` <= 1e-6, UV gather indices bit-exact, feature maps <= 1e-5; train step against float64: loss <= 1e-5
relative, flat bucket and every kernel / bias <= 1e-5 (mask-conditioned at slope 0.3, unconditioned at slope 1); three Adam steps'
losses within rtol 1e-4 of the fp32 oracle's.

Measured on the MI355X, 2026-10-20: see DESIGN.md section 3."""
import inspect
import os

import numpy as np
import pytest
import torch

import nlt_amd
from nlt_amd import capi as C
from nlt_amd import trainvali
from nlt_amd.models import get_model_class
from oracle import nlt_oracle as O
from oracle import tf_ops as T
from gpu_util import rel_l2, make_pair, to_device_batch, hip_activation_masks, _dump, _set_alpha, _per_tensor
import obs_weights_util as U

pytestmark = pytest.mark.gpu
TOL, EXACT_TOL, FEAT_TOL = 1e-4, 1e-6, 1e-5
LOSS_TOL, GRAD_TOL_FLAT, GRAD_TOL_TENSOR = 1e-5, 1e-5, 1e-5


def _threads():
    torch.set_num_threads(min(os.cpu_count() or 1, 16))


# ---------------------------------------------------------------------------------------------------------------- references
_FWD = {}


def _oracle(c):
    """{'kw', 'batch', 'nn', 'w', 'ref', 'dist'} of a forward case, computed once: the fp32 oracle's weighted result (mode vali:
    gt_camspc included) after the sensitivity conditions held."""
    if c not in _FWD:
        _threads()
        kw, batch, nn, w = U.forward_inputs(c)
        om = O.OracleModel(**kw)
        ref, dist = U.assert_sensitive(lambda wv: U.oracle_forward(om, batch, nn, wv, 'vali'), w, U.FORWARD_BARS, U.case_id(c))
        _FWD[c] = dict(kw=kw, batch=batch, nn=nn, w=w, ref=ref, dist=dist)
    return _FWD[c]


def _levels(pm):
    """Stride-2 levels of the encoder (the contracting layers after L0)."""
    return sum(pm.net['query'].is_contracting) - 1


def _product(kw, **product_only):
    _, pm = make_pair(**kw, **product_only)
    pm.build('cuda')
    return pm


# ---------------------------------------------------------------------------------------------------------------------- spies
def _is_fused_or_folding(name):
    """Adapters of launches that could carry an observation mean in their epilogue: the fused ends and the encoder conv families."""
    return ((name.startswith('front') and 'forward' in name) or name.startswith('back_forward')
            or name in ('conv_c32_forward', 'conv_wino_forward') or (name.startswith('conv_tile') and name.endswith('_forward')))


def _spy(monkeypatch, names, keep):
    """Every call of the adapters `names` (the engine looks `C.<fn>` up at call time), plan-time trials included, as
    (name, {argument: value} for the arguments in `keep`)."""
    calls = []
    for name in names:
        real = getattr(C, name)
        sig = inspect.signature(real)

        def spy(*a, _name=name, _real=real, _sig=sig, **kw):
            args = _sig.bind(*a, **kw)
            args.apply_defaults()
            calls.append((_name, {x: args.arguments[x] for x in keep if x in args.arguments}))
            return _real(*a, **kw)
        monkeypatch.setattr(C, name, spy)
    return calls


def _spy_forward(monkeypatch):
    names = ['stem_forward', 'obs_mean_forward'] + [x for x in dir(C) if _is_fused_or_folding(x) and callable(getattr(C, x))]
    assert {'front4_forward', 'back_forward', 'conv_c32_forward', 'conv_wino_forward', 'conv_tile_forward', 'conv_tile3_forward',
            'conv_tile3w_s2_forward'} <= set(names)
    return _spy(monkeypatch, names, ('obs_weights', 'mean_out'))


def _carries(call, wd):
    w = call[1].get('obs_weights')
    return w is not None and w.is_contiguous() and tuple(w.shape) == tuple(wd.shape) and torch.equal(w, wd)


def _assert_forward_route(calls, wd, n_means, stem=True):
    """The weighted layer-by-layer forward is what ran: the stem and every observation mean got the weights, and no fused end or
    mean-folding conv launch carried an observation mean."""
    stems = [c for c in calls if c[0] == 'stem_forward']
    means = [c for c in calls if c[0] == 'obs_mean_forward']
    assert (len(stems) >= 1) == stem and all(_carries(c, wd) for c in stems), stems
    assert len(means) >= n_means and all(_carries(c, wd) for c in means), (len(means), n_means)
    rest = [c for c in calls if c[0] not in ('stem_forward', 'obs_mean_forward')]
    assert not [c[0] for c in rest if c[0].startswith(('front', 'back_forward'))], sorted({c[0] for c in rest})
    assert all(c[1]['mean_out'] is None for c in rest), sorted({c[0] for c in rest if c[1]['mean_out'] is not None})


BACKWARD_SPIED = ('obs_mean_backward', 'stem_backward', 'level_split_backward', 'front_backward', 'back_backward',
                  'conv_backward_data', 'lrelu_backward')


def _assert_backward_route(calls, wd, levels):
    """... and the weighted backward: `obs_mean_backward` with the weights on every level, `stem_backward` with them, none of the
    fused / folded forms."""
    means = [c for c in calls if c[0] == 'obs_mean_backward']
    stems = [c for c in calls if c[0] == 'stem_backward']
    assert len(means) >= levels and len(means) % levels == 0 and all(_carries(c, wd) for c in means), len(means)
    assert stems and all(_carries(c, wd) for c in stems)
    ran = {c[0] for c in calls}
    assert not ran & {'level_split_backward', 'front_backward', 'back_backward'}, ran
    dgrads = [c for c in calls if c[0] == 'conv_backward_data']
    assert dgrads and all(c[1]['split'] is None for c in dgrads)
    assert 'lrelu_backward' in ran


# ---------------------------------------------------------------------------------------------------------------- comparisons
def _bufs(pm, n, k):
    (b,) = [b for b in pm.plan._bufs.values() if tuple(b['obs'][0].shape[:2]) == (n, k)]
    return b


def _errors(pm, out, ref, mode, n, k, uvh, uvw, maps=True):
    pred_c, gt_c, _, vis = out
    torch.cuda.synchronize()
    rec = {'rel_l2_pred_uv': rel_l2(vis['pred'].cpu(), ref['pred']), 'rel_l2_pred_camspc': rel_l2(pred_c.cpu(), ref['pred_camspc']),
           'rel_l2_base_camspc': rel_l2(vis['base_camspc'].cpu(), ref['base_camspc'])}
    if mode == 'test':
        assert gt_c is None
    else:
        rec['rel_l2_gt_camspc'] = rel_l2(gt_c.cpu(), ref['gt_camspc'])
    fx, fy, inside = T.resampler_indices(ref['warp_px'], uvh, uvw)
    idx = vis['uv_indices'].cpu().numpy()
    np.testing.assert_array_equal(idx[..., 0], fx)
    np.testing.assert_array_equal(idx[..., 1], fy)
    np.testing.assert_array_equal(idx[..., 2], inside.astype(np.int32))
    if maps:
        b = _bufs(pm, n, k)
        cl = b['C']
        assert len(cl) == len(ref['feats']) == len(ref['obs'])
        # the observation half of fm[l] is the WEIGHTED aggregate; obs[l], handed to level l + 1, the UNweighted features (:162-166)
        rec['rel_l2_fm_obs_half'] = [rel_l2(b['fm'][l][..., cl[l]:].cpu(), ref['feats'][l]) for l in range(len(cl))]
        rec['rel_l2_obs_unweighted'] = [rel_l2(b['obs'][l].cpu(), np.stack(ref['obs'][l], 1)) for l in range(len(cl))]
    return rec


def _check_forward(rec, what):
    print(what, {k: ('%.2e' % v if isinstance(v, float) else ' '.join('%.1e' % x for x in v)) for k, v in rec.items()})
    assert rec['rel_l2_pred_uv'] <= TOL and rec['rel_l2_pred_camspc'] <= TOL, (what, rec)
    assert rec['rel_l2_base_camspc'] <= EXACT_TOL and rec.get('rel_l2_gt_camspc', 0.0) <= EXACT_TOL, (what, rec)
    assert max(rec.get('rel_l2_fm_obs_half', [0.0])) <= FEAT_TOL and max(rec.get('rel_l2_obs_unweighted', [0.0])) <= FEAT_TOL, (what, rec)


# -------------------------------------------------------------------------------------------------------- forward, every route
@pytest.mark.parametrize('c', U.FORWARD, ids=U.case_id)
def test_forward_in_every_mode_vs_oracle(c, monkeypatch):
    """Model.call(db, mode, obs_weights=w, want_indices=True) for test, vali and train under no_grad on one autotuned model (the
    first call runs the layer-by-layer plan's trials with the weights in place)."""
    uvh, uvw, hc, wc, imh, imw, n, k = c
    o = _oracle(c)
    pm = _product(o['kw'])
    db, wd = to_device_batch(o['batch'], o['nn']), o['w'].cuda()
    calls = _spy_forward(monkeypatch)
    for mode in ('test', 'vali', 'train'):
        with torch.no_grad():
            out = pm.call(db, mode, obs_weights=wd, want_indices=True)
        rec = _errors(pm, out, o['ref'], mode, n, k, uvh, uvw)
        _dump('obs_weights_forward_%s_%s' % (U.case_id(c), mode), dict(rec, oracle_distances=o['dist']))
        _check_forward(rec, 'forward %s %s' % (U.case_id(c), mode))
    _assert_forward_route(calls, wd, 3 * _levels(pm))
    assert pm.plan.tape_replays == 0


VARIANTS = ['layerwise_call', 'f32x3_9', 'f32x3', 'fuse_ends_off', 'algo_direct']


@pytest.mark.parametrize('variant', VARIANTS)
def test_forward_variants_vs_oracle(variant, monkeypatch):
    """Model._call(x, y_obs, obs_weights=w) (the reference's layer-by-layer structure), the two split precisions,
    plan.fuse_ends = False and conv_algo = ALGO_DIRECT: the same comparison (64 x 192 (2, 3) for the first and the last, 64 x 64
    (3, 2) for the others)."""
    c = U.FORWARD[2] if variant in ('layerwise_call', 'algo_direct') else U.FORWARD[1]
    uvh, uvw, hc, wc, imh, imw, n, k = c
    o = _oracle(c)
    pm = _product(o['kw'], **({'precision': variant} if variant.startswith('f32x3') else {}))
    if variant == 'fuse_ends_off':
        pm.plan.fuse_ends = False
    if variant == 'algo_direct':
        pm.conv_algo = C.ALGO_DIRECT
    db, wd = to_device_batch(o['batch'], o['nn']), o['w'].cuda()
    calls = _spy_forward(monkeypatch)
    if variant == 'layerwise_call':
        x = torch.cat((db[1], db[2], db[3]), 3)
        y_obs = [(db[9][:, i] - db[8][:, i]).contiguous() for i in range(k)]
        with torch.no_grad():
            got = pm._call(x, y_obs, obs_weights=wd)
        torch.cuda.synchronize()
        rec = {'rel_l2_layerwise': rel_l2(got.cpu(), o['ref']['call_out'])}
        print('forward', variant, U.case_id(c), rec)
        _dump('obs_weights_forward_%s' % variant, rec)
        assert rec['rel_l2_layerwise'] <= TOL, rec
        _assert_forward_route(calls, wd, _levels(pm) + 1, stem=False)
        return
    with torch.no_grad():
        out = pm.call(db, 'vali', obs_weights=wd, want_indices=True)
    rec = _errors(pm, out, o['ref'], 'vali', n, k, uvh, uvw)
    _dump('obs_weights_forward_%s' % variant, rec)
    _check_forward(rec, 'forward %s %s' % (variant, U.case_id(c)))
    _assert_forward_route(calls, wd, _levels(pm))


def _generic_pair(monkeypatch, c, loss='l2', **branch):
    """(oracle, product) of a config branch that runs layer by layer through generic.py, depth 256, with the case's sizes."""
    uvh, uvw, hc, wc, imh, imw, n, k = c[:8]
    if branch.get('kernel') == 3:
        import conv_k3_ref as R
        monkeypatch.setattr(T, 'conv2d_transpose_same', R.conv2d_transpose_same)
    dims = dict(depth=256, uvh=uvh, uvw=uvw, imh=imh, imw=imw, loss=loss, **branch)
    om = O.OracleModel(seed=U.seeds(c)[0], **dims)
    pm = get_model_class('nlt')(nlt_amd.make_config(**dims))
    pm.load_weights(om.numpy_weights())
    pm.register_trainable()
    assert pm.generic
    return om, pm.build('cuda')


@pytest.mark.parametrize('branch', [dict(kernel=3), dict(norm='layer')], ids=['kernel3', 'norm_layer'])
def test_generic_models_forward_vs_oracle(branch, monkeypatch):
    """`Model.generic` (kernel = 3; norm = layer): generic.forward's weighted obs_mean, forward only."""
    _threads()
    c = U.FORWARD[1]
    uvh, uvw, hc, wc, imh, imw, n, k = c
    _, batch, nn, w = U.forward_inputs(c)
    om, pm = _generic_pair(monkeypatch, c, **branch)
    ref, dist = U.assert_sensitive(lambda wv: U.oracle_forward(om, batch, nn, wv, 'vali'), w, {'pred': TOL, 'pred_camspc': TOL}, str(branch))
    db, wd = to_device_batch(batch, nn), w.cuda()
    calls = _spy_forward(monkeypatch)
    with torch.no_grad():
        out = pm.call(db, 'vali', obs_weights=wd, want_indices=True)
    rec = _errors(pm, out, ref, 'vali', n, k, uvh, uvw, maps=False)
    _dump('obs_weights_forward_generic_%s' % '_'.join('%s%s' % x for x in branch.items()), dict(rec, oracle_distances=dist))
    _check_forward(rec, 'forward generic %s' % branch)
    _assert_forward_route(calls, wd, _levels(pm) + 1, stem=False)


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_bf16_refuses_the_weights_and_serves_the_next_calls():
    """precision = bf16 is an inference mode of the fused plans: with weights the NLTError that names `obs_weights` -- as the
    model's first call ever and between replays -- and the unweighted calls around it meet the bf16-operand oracle (<= 1e-4,
    tests/test_gpu_bf16.py's bar on the texels), the later ones bit for bit what the earlier ones returned."""
    _threads()
    c = U.FORWARD[1]
    uvh, uvw, hc, wc, imh, imw, n, k = c
    kw, batch, nn, w = U.forward_inputs(c)
    om = O.OracleModel(**kw)
    pb = get_model_class('nlt')(nlt_amd.make_config(precision='bf16', **{x: kw[x] for x in ('depth', 'uvh', 'uvw', 'imh', 'imw')}))
    pb.load_weights(om.numpy_weights())
    pb.register_trainable()
    pb.build('cuda')
    om.set_precision('bf16')
    with torch.no_grad():
        o_c, _, _, o_vis = om.call(batch, 'test', nn_list=nn)
    db, wd = to_device_batch(batch, nn), w.cuda()
    with pytest.raises(C.NLTError, match='obs_weights'):
        pb.call(db, 'test', obs_weights=wd)
    outs = [pb.call(db, 'test') for _ in range(3)]
    keep = (outs[2][0].clone(), outs[2][3]['pred'].clone())
    torch.cuda.synchronize()
    rec = {'rel_l2_pred_uv': rel_l2(keep[1].cpu(), o_vis['pred']), 'rel_l2_pred_camspc': rel_l2(keep[0].cpu(), o_c)}
    print('bf16 after the refused call', rec)
    assert rec['rel_l2_pred_uv'] <= TOL and rec['rel_l2_pred_camspc'] <= TOL, rec
    replays = pb.plan.tape_replays
    assert replays >= 1
    with pytest.raises(C.NLTError, match='obs_weights'):
        pb.call(db, 'test', obs_weights=wd)
    assert pb.plan.tape_replays == replays
    for _ in range(3):              # (the census of packed fragments that follows the trials may end here: one re-record at most)
        again = pb.call(db, 'test')
        torch.cuda.synchronize()
        assert torch.equal(again[0], keep[0]) and torch.equal(again[3]['pred'], keep[1])
    assert pb.plan.tape_replays > replays


def test_generic_training_through_the_weights_is_refused_and_the_next_step_is_clean(monkeypatch):
    """The layer-by-layer branch models take the weights forward only: the backward raises NotImplementedError("training through
    obs_weights").  The flat gradient bucket it had begun to fill is not read by the next step: an unweighted step right after
    meets the oracle at tests/test_gpu_conv_k3.py's bars (loss 1e-5, every kernel / bias 5e-3 against the fp32 oracle)."""
    _threads()
    c = U.FORWARD[1]
    uvh, uvw, hc, wc, imh, imw, n, k = c
    _, batch, nn, w = U.forward_inputs(c)
    om, pm = _generic_pair(monkeypatch, c, kernel=3)
    db, wd = to_device_batch(batch, nn), w.cuda()
    with torch.no_grad():
        ref_w = om.call(batch, 'train', nn_list=nn, obs_weights=w)[0]
    pred, gt, _, _ = pm(db, mode='train', obs_weights=wd)
    assert rel_l2(pred.detach().cpu(), ref_w) <= TOL
    lp = pm.compute_loss(pred, gt, keep_batch=True).sum() / n
    pm.flat_params.grad = None
    with pytest.raises(NotImplementedError, match='training through obs_weights'):
        lp.backward()
    torch.cuda.synchronize()
    po, go, _, _ = om.call(batch, 'train', nn_list=nn)
    lo = om.compute_loss(po, go, keep_batch=True).sum() / n
    grads = torch.autograd.grad(lo, om.parameters())
    pred, gt, _, vis = pm(db, mode='train')
    lp = pm.compute_loss(pred, gt, keep_batch=True).sum() / n
    pm.flat_params.grad = None
    lp.backward()
    torch.cuda.synchronize()
    assert rel_l2(pred.detach().cpu(), po.detach()) <= TOL
    assert abs(float(lp.detach()) - float(lo.detach())) <= LOSS_TOL * abs(float(lo.detach()))
    it = iter(grads)
    worst = max(float((getattr(cv, nm).cpu() - g).norm() / (g.norm() + 1e-30)) for cv in pm._conv_layers()
                for nm, g in ((nm, next(it)) for nm in ('dkernel', 'dbias')))
    print('generic step after the refused backward: worst per-tensor gradient rel-L2 %.3e (bound 5e-3)' % worst)
    assert worst <= 5e-3, worst


# ------------------------------------------------------------------------------------ plan state across weighted / unweighted
@pytest.mark.parametrize('graphs', [False, True], ids=['tapes', 'hipgraph'])
def test_weighted_calls_between_replays_of_the_unweighted_plan(graphs):
    """One model: three unweighted `test` calls (trials, record, replay), a weighted call, unweighted, a weighted call after the
    weights changed IN PLACE at the same address, unweighted.  Every weighted result meets the oracle for ITS weights (nothing
    keyed on the address is replayed), every unweighted one is bit-equal to the first replayed one, and the replay counters
    (plan.tape_replays; with use_graphs the captured graph's hits) stand still over the weighted calls and move on the unweighted
    ones.  The FIRST weighted call runs the layer-by-layer plan's plan-time trials, which drop every recorded tape by design
    (`_autotune` -> `_drop_tapes`) and start the census of packed fragments whose end, four passes later, invalidates the tapes
    once more: each unweighted step is three calls (at worst eager, record, replay), all three held to the same bits."""
    c = U.FORWARD[1]
    uvh, uvw, hc, wc, imh, imw, n, k = c
    o = _oracle(c)
    om = O.OracleModel(**o['kw'])
    w2 = U.variants(o['w'])['frames_flipped']                    # (>= 1000 x the bar away from w's result: _oracle asserted it)
    ref2 = U.oracle_forward(om, o['batch'], o['nn'], w2, 'test')
    with torch.no_grad():
        plain = om.call(o['batch'], 'test', nn_list=o['nn'])
    pm = _product(o['kw'])
    pm.use_graphs = graphs
    db, wd = to_device_batch(o['batch'], o['nn']), o['w'].cuda()
    count = (lambda: pm._graph['hits']) if graphs else (lambda: pm.plan.tape_replays)

    def unweighted():
        out = pm.call(db, 'test', want_indices=True)
        torch.cuda.synchronize()
        return out[0].clone(), out[3]['pred'].clone(), out[3]['uv_indices'].clone()

    def weighted(ref, what):
        before = count()
        out = pm.call(db, 'test', obs_weights=wd, want_indices=True)
        rec = _errors(pm, out, ref, 'test', n, k, uvh, uvw)
        _dump('obs_weights_state_%s_%s' % ('hipgraph' if graphs else 'tapes', what), rec)
        _check_forward(rec, 'state %s %s' % ('hipgraph' if graphs else 'tapes', what))
        assert count() == before, what

    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))
    first = [unweighted() for _ in range(3)]
    keep = first[2]
    assert count() >= 1
    assert rel_l2(keep[1].cpu(), plain[3]['pred']) <= TOL and rel_l2(keep[0].cpu(), plain[0]) <= TOL
    weighted(o['ref'], 'first_weighted_call')
    before = count()
    for _ in range(3):
        assert same(unweighted(), keep)
    assert count() > before
    data_ptr = wd.data_ptr()
    wd.copy_(w2)
    assert wd.data_ptr() == data_ptr
    weighted(ref2, 'weights_changed_in_place')
    before = count()
    for _ in range(3):
        assert same(unweighted(), keep)
    assert count() > before


def test_a_model_whose_first_call_is_weighted_then_serves_unweighted_calls():
    """The layer-by-layer plan's trials run with the weights in place; whatever they chose, the unweighted calls after (their own
    trials, record, replay) are within 1e-4 of the oracle."""
    c = U.FORWARD[3]
    uvh, uvw, hc, wc, imh, imw, n, k = c
    o = _oracle(c)
    om = O.OracleModel(**o['kw'])
    with torch.no_grad():
        plain = om.call(o['batch'], 'test', nn_list=o['nn'])
    pm = _product(o['kw'])
    db, wd = to_device_batch(o['batch'], o['nn']), o['w'].cuda()
    out = pm.call(db, 'test', obs_weights=wd, want_indices=True)
    _check_forward(_errors(pm, out, o['ref'], 'test', n, k, uvh, uvw), 'first call ever, weighted')
    for i in range(3):
        out = pm.call(db, 'test')
        torch.cuda.synchronize()
        rec = {'rel_l2_pred_uv': rel_l2(out[3]['pred'].cpu(), plain[3]['pred']), 'rel_l2_pred_camspc': rel_l2(out[0].cpu(), plain[0])}
        print('unweighted call %d after a weighted first call' % i, rec)
        assert rec['rel_l2_pred_uv'] <= TOL and rec['rel_l2_pred_camspc'] <= TOL, rec
    assert pm.plan.tape_replays >= 1
    pm.plan.fuse_ends = False                                    # ... and the layer-by-layer plan those trials tuned, unweighted
    out = pm.call(db, 'test')
    torch.cuda.synchronize()
    assert rel_l2(out[3]['pred'].cpu(), plain[3]['pred']) <= TOL and rel_l2(out[0].cpu(), plain[0]) <= TOL


# ------------------------------------------------------------------------------------------------- train step against float64
_TRAIN = {}


def _oracle_train(c):
    """(loss, gradients) of the float64 oracle's weighted step, after the sensitivity conditions on the flat bucket and on the
    observation path's L0 kernel held; once per case."""
    if c not in _TRAIN:
        _threads()
        w = U.forward_inputs(c)[3]
        full = {}

        def evaluate(wv):
            lo, grads, q = U.oracle_train(c, wv)
            if wv is w:
                full['lo'], full['grads'] = lo, grads
            return q
        _, dist = U.assert_sensitive(evaluate, w, U.TRAIN_BARS, U.case_id(c))
        _TRAIN[c] = (full['lo'], full['grads'], dist)
    return _TRAIN[c]


def _train_pair(c, deterministic=False):
    uvh, uvw, hc, wc, imh, imw, n, k, loss, alpha = c
    kw, batch, nn, w = U.forward_inputs(c)
    om, pm = make_pair(loss=loss, **kw)
    _set_alpha(om, pm, alpha)
    if deterministic:
        pm.deterministic = True
    pm.build('cuda')
    return om, pm, batch, nn, w


def _step_record(pm, c, lp, lo, grads, cond):
    """The measured distances of the step `pm` just made from the float64 oracle's (and, at a slope with a kink, from the
    float64 oracle's on the branches the HIP forward took); cond: the cache of that second oracle run."""
    uvh, uvw, hc, wc, imh, imw, n, k, loss, alpha = c
    flat, worst = _per_tensor(pm, grads)
    rec = {'loss_hip': lp, 'loss_oracle_f64': lo, 'flat_rel': flat, 'worst_unconditioned': worst}
    if alpha != 1.0:
        masks = hip_activation_masks(pm)
        if not cond or any(not all(torch.equal(a, b) for a, b in zip(masks[key], cond[0][key])) for key in masks):
            cond[:] = (masks,) + U.oracle_train(c, U.forward_inputs(c)[3], masks=masks)[:2]
        flat_m, worst_m = _per_tensor(pm, cond[2])
        rec.update({'loss_oracle_f64_hip_masks': cond[1], 'flat_rel_hip_masks': flat_m, 'worst_hip_masks': worst_m})
    return rec


def _check_step(r, alpha, what):
    lo = r['loss_oracle_f64']
    print(what, {k: (v if not isinstance(v, list) else v[:2]) for k, v in r.items()})
    assert abs(r['loss_hip'] - lo) <= LOSS_TOL * abs(lo), (what, r['loss_hip'], lo)
    if alpha == 1.0:
        assert r['flat_rel'] <= GRAD_TOL_FLAT, (what, r['flat_rel'])
        assert r['worst_unconditioned'][0][0] <= GRAD_TOL_TENSOR, (what, r['worst_unconditioned'][:4])
    else:
        assert abs(r['loss_hip'] - r['loss_oracle_f64_hip_masks']) <= LOSS_TOL * abs(lo), what
        assert r['flat_rel_hip_masks'] <= GRAD_TOL_FLAT, (what, r['flat_rel_hip_masks'])
        assert r['worst_hip_masks'][0][0] <= GRAD_TOL_TENSOR, (what, r['worst_hip_masks'][:4])


@pytest.mark.parametrize('c', U.TRAIN, ids=U.case_id)
def test_train_step_vs_float64(c, monkeypatch):
    """pm.call(db, 'train', obs_weights=w), compute_loss(...).sum() / n, .backward() against the float64 oracle's step under
    the same weights, twice (the first pass runs the plan-time trials of both directions), with the route spied in both
    directions."""
    uvh, uvw, hc, wc, imh, imw, n, k, loss, alpha = c
    lo, grads, dist = _oracle_train(c)
    _, pm, batch, nn, w = _train_pair(c)
    db, wd = to_device_batch(batch, nn), w.cuda()
    fwd = _spy_forward(monkeypatch)
    bwd = _spy(monkeypatch, BACKWARD_SPIED, ('obs_weights', 'split'))
    recs, cond = [], []
    for rep in range(2):
        pred, gt, _, _ = pm(db, mode='train', obs_weights=wd)
        lp = pm.compute_loss(pred, gt, keep_batch=True).sum() / n
        pm.flat_params.grad = None
        lp.backward()
        torch.cuda.synchronize()
        recs.append(dict(_step_record(pm, c, float(lp.detach()), lo, grads, cond), oracle_distances=dist))
    _dump('obs_weights_train_%s' % U.case_id(c), recs)
    for rep, r in enumerate(recs):
        _check_step(r, alpha, 'train %s pass %d' % (U.case_id(c), rep))
    _assert_forward_route(fwd, wd, 2 * _levels(pm))
    _assert_backward_route(bwd, wd, _levels(pm))
    assert pm.plan.tape_replays == 0


def test_three_adam_steps_follow_the_oracle(monkeypatch):
    """Three steps of trainvali.distributed_train_step(..., obs_weights=w) (its keyword; the graph-free train_forward_backward
    route) against three steps of the fp32 oracle with KerasAdamAMSGrad: losses within rtol 1e-4 (tests/test_gpu_tape.py's bar)."""
    c = U.TRAIN[3]
    uvh, uvw, hc, wc, imh, imw, n, k, loss, alpha = c
    om, pm, batch, nn, w = _train_pair(c)
    _oracle_train(c)                                             # (the case's sensitivity conditions)
    db, wd = to_device_batch(batch, nn), w.cuda()
    bwd = _spy(monkeypatch, BACKWARD_SPIED, ('obs_weights', 'split'))
    opt_o = O.KerasAdamAMSGrad(om.parameters(), 1e-3)
    opt_p = nlt_amd.optim.AdamAMSGrad(pm, 1e-3)
    lo, lp = [], []
    for step in range(3):
        lo.append(float(O.train_step(om, opt_o, batch, global_bs=n, nn_list=nn, obs_weights=w)[0]))
        lp.append(float(trainvali.distributed_train_step(pm, db, opt_p, global_bs=n, obs_weights=wd)[0]))
    torch.cuda.synchronize()
    print('three weighted Adam steps: HIP', lp, 'oracle', lo)
    _dump('obs_weights_three_adam_steps', {'loss_hip': lp, 'loss_oracle_f32': lo})
    np.testing.assert_allclose(lp, lo, rtol=1e-4)
    assert lo[2] < lo[0]
    _assert_backward_route(bwd, wd, _levels(pm))
    assert pm.plan.tape_replays == 0


# -------------------------------------------------------------------------------------------------------- deterministic mode
def test_deterministic_mode_repeats_bit_for_bit_and_meets_float64():
    """model.deterministic = True before the first step; two fresh models, same seed, same weighted batch, three steps each:
    losses, flat gradient bucket and parameters bit-identical, step 1 at the float64 bars.  The whole-model run of
    nlt_stem_backward_det with weights and of the `_det` weight-gradient siblings on the narrow levels of 64 x 64."""
    c = U.TRAIN[3]
    uvh, uvw, hc, wc, imh, imw, n, k, loss, alpha = c
    lo, grads, dist = _oracle_train(c)
    runs = []
    for leg in range(2):
        _, pm, batch, nn, w = _train_pair(c, deterministic=True)
        assert pm.deterministic and not pm.plan.autotune
        db, wd = to_device_batch(batch, nn), w.cuda()
        opt = nlt_amd.optim.AdamAMSGrad(pm, 1e-3)
        out = []
        for step in range(3):
            loss_, _ = trainvali.distributed_train_step(pm, db, opt, n, obs_weights=wd)
            torch.cuda.synchronize()
            out.append((loss_.clone(), pm.flat_grads.clone(), pm.flat_params.detach().clone()))
            if leg == 0 and step == 0:
                rec = _step_record(pm, c, float(loss_), lo, grads, [])
                _dump('obs_weights_deterministic_step1', dict(rec, oracle_distances=dist))
                _check_step(rec, alpha, 'deterministic step 1')
        runs.append(out)
    for (la, ga, pa), (lb, gb, pb) in zip(*runs):
        assert la.cpu().numpy().tobytes() == lb.cpu().numpy().tobytes(), (float(la), float(lb))
        assert torch.equal(ga, gb) and torch.equal(pa, pb)
        assert torch.isfinite(ga).all() and float(ga.abs().sum()) > 0


# ------------------------------------------------------------------------------------------------------- the argument's guard
def test_views_give_the_bits_of_their_dense_copy_and_bad_arguments_launch_nothing(monkeypatch):
    """A `w_wide[:, :k]` view and a transposed-storage view are read as their dense copy (bit-equal `pred`, `pred_camspc`, feature
    maps); float64, int32, CPU, [k], [N, k + 1] and [N * k + 1] raise ValueError naming what they got, and the plan's `pred`
    buffer and `generation` are untouched by the refused call."""
    c = U.FORWARD[1]
    uvh, uvw, hc, wc, imh, imw, n, k = c
    o = _oracle(c)
    pm = _product(o['kw'])
    db, wd = to_device_batch(o['batch'], o['nn']), o['w'].cuda()

    def run(wv):
        with torch.no_grad():
            out = pm.call(db, 'test', obs_weights=wv, want_indices=True)
        b = _bufs(pm, n, k)
        torch.cuda.synchronize()
        return out, [out[0].clone(), out[3]['pred'].clone()] + [t.clone() for t in b['fm']]
    out, dense = run(wd)
    _check_forward(_errors(pm, out, o['ref'], 'test', n, k, uvh, uvw), 'dense weights')
    wide = O.synth_obs_weights(n, 4).cuda()
    strided = o['w'].t().contiguous().cuda().t()                 # [n, k] with strides (1, n)
    assert not wide[:, :k].is_contiguous() and not strided.is_contiguous() and torch.equal(strided, wd)
    for name, view in (('slice of a wider tensor', wide[:, :k]), ('transposed storage', strided),
                       ('the reference\'s (N, 1, 1, 1, k)', wd.reshape(n, 1, 1, 1, k))):
        got = run(view)[1]
        assert all(torch.equal(a, b) for a, b in zip(got, dense)), name
    b = _bufs(pm, n, k)
    pred_before, gen = b['pred'].clone(), pm.plan.generation
    launches = []
    real = pm.plan._launch
    monkeypatch.setattr(pm.plan, '_launch', lambda *a, **kw: (launches.append(a[0]), real(*a, **kw))[1])
    x = torch.cat((db[1], db[2], db[3]), 3)
    y_obs = [(db[9][:, i] - db[8][:, i]).contiguous() for i in range(k)]
    bad = {'float64': wd.double(), 'int32': wd.to(torch.int32), 'cpu': o['w'], '[k]': wd[0].contiguous(),
           '[N, k + 1]': O.synth_obs_weights(n, k + 1).cuda(), '[N * k + 1]': torch.zeros(n * k + 1, device='cuda')}
    for name, arg in bad.items():
        for call in (lambda: pm.call(db, 'test', obs_weights=arg), lambda: pm.call(db, 'train', obs_weights=arg),
                     lambda: pm._call(x, y_obs, obs_weights=arg),
                     lambda: pm.plan.forward(db[1], db[2], db[3], db[9], db[8], obs_weights=arg),
                     lambda: pm.plan.backward(torch.zeros_like(db[1]), db[1], db[2], db[3], db[9], db[8], obs_weights=arg)):
            with pytest.raises(ValueError, match='obs_weights') as e:
                call()
            assert str(tuple(arg.shape)) in str(e.value) and str(arg.dtype) in str(e.value) and str(arg.device) in str(e.value), name
    torch.cuda.synchronize()
    assert not launches and pm.plan.generation == gen and torch.equal(b['pred'], pred_before)


def test_forward_and_backward_of_a_step_read_the_same_weights():
    """The autograd function keeps the dense copy made at the call, not the caller's view: a step whose weights came as a view of
    a wider tensor that is overwritten between the forward and the backward leaves the gradients of the same step with dense
    weights, bit for bit (deterministic mode, so that the bits can be compared)."""
    c = U.TRAIN[3]
    uvh, uvw, hc, wc, imh, imw, n, k, loss, alpha = c
    _, pm, batch, nn, w = _train_pair(c, deterministic=True)
    db, wd = to_device_batch(batch, nn), w.cuda()
    wide = torch.cat((w, w.flip(0)), 1).cuda()
    assert torch.equal(wide[:, :k], wd) and not wide[:, :k].is_contiguous()
    got = []
    for leg in range(2):
        pred, gt, _, _ = pm(db, mode='train', obs_weights=wd if leg == 0 else wide[:, :k])
        lp = pm.compute_loss(pred, gt, keep_batch=True).sum() / n
        if leg == 1:
            wide.zero_()
        pm.flat_params.grad = None
        lp.backward()
        torch.cuda.synchronize()
        got.append((lp.detach().clone(), pm.flat_grads.clone()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert float(got[0][1].abs().sum()) > 0
