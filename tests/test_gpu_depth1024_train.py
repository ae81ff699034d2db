"""-m gpu: the depth-1024 network (the released dragon_sss.ini: 53.8 M parameters, eight stride-2 levels) through the train step,
against the oracle's float64 autograd.

Depth 1024 is the only network whose backward reaches
  - the first-generation weight gradient (csrc/wgrad.hip) at 1024 channels: a level narrower than 4 texels per grid row (the
    tiled and narrow kernels need gw >= 4) is 1 x 1 / 2 x 2 texels at 256^2 and 2 x 2 / 4 x 4 at 512^2;
  - the widest GEMMs: the bottleneck deconv over its self-concatenated [fm[D] | fm[D]] input (4 x 1024 channels), 1024 -> 1024
    stride-1 convs, 2048 -> 1024 stride-2 convs;
  - the backward-data launches with a handful of GEMM rows and K = 4096 where the plan-time trials pick split-K.
The plan-time trials (`RenderPlan._autotune`) keep whichever candidate is fastest on the machine at hand and never compare its
output with anything, so `test_every_tuning_candidate_gives_float64_gradients` forces every candidate the trials ran, one at a
time, and holds each to the float64 bars.

Bars (the BASELINE config-4 bars of tests/test_gpu_baseline_sizes.py): loss within 1e-5 relative, flat gradient bucket <= 1e-5
rel-L2, every kernel and bias <= 1e-5 rel-L2 -- unconditioned for the kink-free alpha = 1 twin, against the float64 oracle
evaluated on the HIP forward's own LeakyReLU branches for the released alpha = 0.3.
"""
import os

import pytest
import torch

import nlt_amd
from nlt_amd import capi as C
from nlt_amd import trainvali
from oracle import nlt_oracle as O
from gpu_util import (rel_l2, make_pair, to_device_batch, hip_activation_masks, _dump, _set_alpha, _oracle_grads,
                      _per_tensor, WGRAD_FNS, _spy_backward, _sweep_candidates)
from test_gpu_train_step import flat_oracle_grads, per_tensor_worst, FLAT_TOL, TENSOR_TOL

pytestmark = pytest.mark.gpu
DEPTH = 1024
SEED = 43
GRAD_TOL_FLAT = 1e-5
GRAD_TOL_TENSOR = 1e-5


def _threads():
    torch.set_num_threads(min(os.cpu_count() or 1, 16))


def _gw(mode, w):
    """Texels per grid row of a weight-gradient launch (engine.RenderPlan._wgrad_now)."""
    return w // 2 if mode == C.CONV_K2S2 else w


def _check_backward_coverage(pm, calls, uv):
    """The eager pass ran the launches this module exists for.  Level sizes come off the plan, not from this file."""
    D, cl = pm.plan.n_down, pm.plan._level_channels()
    wg = [c for c in calls if c[0] in WGRAD_FNS]
    deepest = uv >> D
    assert deepest < 4, "the deepest level (%d texels wide) does not need the first-generation weight gradient" % deepest
    first = [c for c in wg if c[0] == 'conv_backward_weights' and _gw(c[1], c[6]) < 4]
    assert first, "no level with gw < 4 went to the first-generation weight gradient: %s" % sorted({(c[0], c[6]) for c in wg})
    assert any(c[2] + c[3] >= cl[D] for c in first), "the first-generation kernel never saw a %d-channel level" % cl[D]
    tiled = [c for c in wg if c[0] == 'conv_backward_weights_tiled']
    assert any(c[2] + c[3] >= 1024 for c in tiled), "the tiled weight gradient served no layer with >= 1024 input channels"
    bott = pm.net['query'].layers[D + 1].convs()[0][0]           # deconv over concat(fm[D], fm[D]) (nlt.py:190)
    bc = [c for c in wg if c[9] is not None and c[9].data_ptr() == bott.dkernel.data_ptr()]
    assert len(bc) == 1, len(bc)
    _, mode, c0, c1, n, h, w, s0, s1, _ = bc[0]
    assert c0 + c1 == bott.cin == 4 * cl[D] and c0 == c1 and s0.data_ptr() == s1.data_ptr(), (c0, c1, bott.cin)
    assert any(c[0] == 'conv_backward_data' for c in calls), "the plan ran no backward-data launch"
    fam = {}
    for c in wg:
        fam.setdefault(c[0], set()).add((c[2] + c[3], c[5], c[6]))
    return {k: sorted(v) for k, v in fam.items()}


@pytest.mark.parametrize('uv,n,loss,alpha', [(512, 4, 'barron', 0.3), (512, 4, 'barron', 1.0), (256, 2, 'l2', 0.3),
                                             (256, 2, 'l2', 1.0)])
def test_depth1024_train_step_per_tensor_gradients(uv, n, loss, alpha, monkeypatch):
    """Loss and EVERY kernel / bias gradient of one depth-1024 train step (k = 1, camera at the UV size) against the float64
    oracle: (512, 4, barron, 0.3) is exactly dragon_sss.ini.  Three passes: autotuned + eager (the coverage of the deep
    backward launches is asserted on it), recorded into the launch tape, replayed from it -- each held to the bars."""
    _threads()
    om32, pm = make_pair(depth=DEPTH, uv=uv, im=uv, loss=loss, seed=SEED)
    _set_alpha(om32, pm, alpha)
    pm.build('cuda')
    batch, nn = O.synth_batch(n, uv, uv, uv, uv, uv, uv, k=1, seed=SEED + 100)
    lo, grads = _oracle_grads(loss, uv, uv, n, torch.float64, batch, nn, alpha, depth=DEPTH, seed=SEED)
    db = to_device_batch(batch, nn)
    calls = _spy_backward(monkeypatch, pm.plan)
    recs, cond = [], None
    for rep in range(3):
        if rep == 1:
            monkeypatch.undo()                              # (the spies only watch the eager pass)
        replays = pm.plan.tape_replays
        pred, gt, kw, _ = pm(db, mode='train')
        lp = pm.compute_loss(pred, gt, keep_batch=True).sum() / n
        pm.flat_params.grad = None
        lp.backward()
        torch.cuda.synchronize()
        lp = float(lp.detach())
        flat, worst = _per_tensor(pm, grads)
        rec = {'pass': ('eager', 'recorded', 'replayed')[rep], 'loss_hip': lp, 'loss_oracle_f64': lo, 'flat_rel': flat,
               'worst_unconditioned': worst}
        if rep == 0:
            rec['weight_gradient_kernels'] = _check_backward_coverage(pm, calls, uv)
        if rep == 2:
            assert pm.plan.tape_replays > replays, "the third pass did not replay the backward launch tape"
        if alpha != 1.0:
            masks = hip_activation_masks(pm)
            if cond is None or any(not all(torch.equal(a, b) for a, b in zip(masks[key], cond[0][key])) for key in masks):
                cond = (masks,) + _oracle_grads(loss, uv, uv, n, torch.float64, batch, nn, alpha, masks=masks, depth=DEPTH, seed=SEED)
            flat_m, worst_m = _per_tensor(pm, cond[2])
            rec.update({'loss_oracle_f64_hip_masks': cond[1], 'flat_rel_hip_masks': flat_m, 'worst_hip_masks': worst_m})
        recs.append(rec)
    _dump('depth1024_train_%d_n%d_%s_alpha%g' % (uv, n, loss, alpha), recs)
    for r in recs:
        assert abs(r['loss_hip'] - lo) <= 1e-5 * abs(lo), (r['pass'], r['loss_hip'], lo)
        assert r['flat_rel'] <= GRAD_TOL_FLAT, (r['pass'], r['flat_rel'])
        if alpha == 1.0:
            assert r['worst_unconditioned'][0][0] <= GRAD_TOL_TENSOR, (r['pass'], r['worst_unconditioned'][:4])
        else:
            assert abs(r['loss_hip'] - r['loss_oracle_f64_hip_masks']) <= 1e-5 * abs(lo), r['pass']
            assert r['flat_rel_hip_masks'] <= GRAD_TOL_FLAT, (r['pass'], r['flat_rel_hip_masks'])
            assert r['worst_hip_masks'][0][0] <= GRAD_TOL_TENSOR, (r['pass'], r['worst_hip_masks'][:4])


def test_depth1024_adam_and_clipnorm_steps_match_oracle(monkeypatch):
    """tests/test_gpu_train_step.py's three-step Adam-AMSGrad comparison at depth 1024 (256^2, the smallest UV the net takes: the
    bottleneck is 1 x 1 there; n = 2, l2): `distributed_train_step` + the fused optimizer over the 53.8 M-float bucket against
    `O.train_step` + KerasAdamAMSGrad, same bars as at depth 256; then one step with per-variable clip-by-norm
    (config mgm > 0 with NLT_APPLY_CLIPNORM=1, trainvali.make_optimizer) against the oracle's tf.clip_by_norm."""
    _threads()
    uv, n = 256, 2
    om, pm = make_pair(depth=DEPTH, uv=uv, im=uv, loss='l2', seed=SEED + 1)
    pm.build('cuda')
    batch, nn = O.synth_batch(n, uv, uv, uv, uv, uv, uv, k=1, seed=SEED + 101)
    db = to_device_batch(batch, nn)
    assert pm.flat_params.numel() >= 53_800_000
    opt_o = O.KerasAdamAMSGrad(om.parameters(), 1e-3)
    opt_p = nlt_amd.optim.AdamAMSGrad(pm, 1e-3)
    for step in range(3):
        lo, go = O.train_step(om, opt_o, batch, global_bs=n, nn_list=nn)
        lp, _ = trainvali.distributed_train_step(pm, db, opt_p, global_bs=n)
        torch.cuda.synchronize()
        assert abs(float(lp) - float(lo)) <= 2e-5 * max(1.0, abs(float(lo))), (step, float(lp), float(lo))
        ref = flat_oracle_grads(pm, go)
        rel = float((pm.flat_params.grad - ref).norm() / ref.norm())
        assert rel < FLAT_TOL, (step, rel)
        worst = per_tensor_worst(pm, go)
        assert worst[0] < TENSOR_TOL, (step, worst)
    worst = max(float((po.detach() - c.kernel.cpu()).abs().max()) for po, c in zip(om.parameters()[::2], pm._conv_layers()))
    assert worst < 2e-4, worst
    # one clip-by-norm step (fresh optimizer state on both sides)
    clip = 1e-3
    monkeypatch.setenv('NLT_APPLY_CLIPNORM', '1')
    opt_p = trainvali.make_optimizer(pm, nlt_amd.make_config(depth=DEPTH, uvh=uv, uvw=uv, imh=uv, imw=uv, mgm=clip, lr=1e-3))
    assert opt_p.clipnorm == clip
    opt_o = O.KerasAdamAMSGrad(om.parameters(), 1e-3)
    lo, go = O.train_step(om, opt_o, batch, global_bs=n, nn_list=nn, clipnorm=clip)
    lp, _ = trainvali.distributed_train_step(pm, db, opt_p, global_bs=n)
    torch.cuda.synchronize()
    assert abs(float(lp) - float(lo)) <= 2e-5 * max(1.0, abs(float(lo))), (float(lp), float(lo))
    ref = flat_oracle_grads(pm, go)
    assert float((pm.flat_params.grad - ref).norm() / ref.norm()) < 5e-4
    worst = max(float((po.detach() - c.kernel.cpu()).abs().max()) for po, c in zip(om.parameters()[::2], pm._conv_layers()))
    assert worst < 2e-4, worst


@pytest.mark.parametrize('mode', ['train', 'test'])
def test_every_tuning_candidate_gives_float64_gradients(mode):
    """Every (kind, hint) the plan-time trials ran at depth 1024 (256^2, k = 1, n = 2, alpha = 1: kink-free, so the unconditioned
    float64 bars hold) is forced, alone, on every launch it ran on; any of them may be the one the timing keeps on another machine.
    train: loss and every kernel / bias gradient against the float64 oracle (computed once); test: the rendered texels
    (fused-end inference plan, its own labels) <= 1e-4 rel-L2 against the oracle's `call`.  The families the sweep covered
    are asserted -- for the backward-data launches split-K in both forms, the LDS-tiled and the Winograd kernel; c32 in the
    forward -- so the sweep cannot pass by having nothing to force."""
    _threads()
    uv, n, alpha = 256, 2, 1.0
    om, pm = make_pair(depth=DEPTH, uv=uv, im=uv, loss='l2', seed=SEED + 2)
    _set_alpha(om, pm, alpha)
    pm.build('cuda')
    plan = pm.plan
    batch, nn = O.synth_batch(n, uv, uv, uv, uv, uv, uv, k=1, seed=SEED + 102)
    db = to_device_batch(batch, nn)

    if mode == 'train':
        lo, grads = _oracle_grads('l2', uv, uv, n, torch.float64, batch, nn, alpha, depth=DEPTH, seed=SEED + 2)
        ref = [g.cuda() for g in grads]
        names = ['conv%d.%s%s' % (li, nm, tuple(g.shape)) for li, _ in enumerate(pm._conv_layers())
                 for nm, g in zip(('dkernel', 'dbias'), grads[2 * li: 2 * li + 2])]

        def run():
            pred, gt, _, _ = pm(db, mode='train')
            lp = pm.compute_loss(pred, gt, keep_batch=True).sum() / n
            pm.flat_params.grad = None
            lp.backward()
            got = [getattr(c, nm).detach() for c in pm._conv_layers() for nm in ('dkernel', 'dbias')]
            num = torch.stack([(g.double() - r).norm() for g, r in zip(got, ref)])
            den = torch.stack([r.norm() for r in ref])
            errs = (num / den.clamp(min=1e-300)).tolist()
            worst = sorted(zip(errs, names), reverse=True)[:4]
            flat = float(num.square().sum().sqrt() / den.square().sum().sqrt())
            dl = abs(float(lp.detach()) - lo) / abs(lo)
            bad = dl > 1e-5 or flat > GRAD_TOL_FLAT or worst[0][0] > GRAD_TOL_TENSOR
            return bad, {'loss_rel': dl, 'flat_rel': flat, 'worst': worst}
    else:
        with torch.no_grad():
            o_pred_c, _, _, o_vis = om.call(batch, 'test', nn_list=nn)

        def run():
            with torch.no_grad():
                p_pred_c, _, _, p_vis = pm.call(db, 'test')
            torch.cuda.synchronize()
            e_uv, e_cam = rel_l2(p_vis['pred'].cpu(), o_vis['pred']), rel_l2(p_pred_c.cpu(), o_pred_c)
            return max(e_uv, e_cam) > 1e-4, {'rel_l2_pred_uv': e_uv, 'rel_l2_pred_camspc': e_cam}

    bad, base = run()                                       # autotuned: the forward (and in train mode the backward) trials
    assert not bad, ('autotuned plan', base)
    recs, failures, covered, n_tuned, n_cands = _sweep_candidates(plan, run)
    _dump('depth1024_candidate_sweep_%s' % mode, {'autotuned': base, 'forced': recs, 'covered': covered,
                                                 'tuned_labels': n_tuned, 'candidates': n_cands})
    assert not failures, "candidates off the float64 bars (candidate, worst): %s" % failures
    assert covered['fwd.c32'], "the forward trials ran no c32 launch"
    if mode == 'train':
        for fam in ('dgrad.splitk_one_launch', 'dgrad.splitk_two_launches', 'dgrad.lds', 'dgrad.wino'):
            assert covered[fam], "the backward trials never ran %s at depth 1024 / 256^2: %s" % (fam, covered)
