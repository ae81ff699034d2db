"""-m gpu: UV maps, warp grids and camera images that are NOT square, through every plan, against the oracle.

The reference keeps the axes apart everywhere: a UV map is uvh x uvw, the dataset resizes captures by height and keeps the aspect
ratio, the warp scales x by uvw and y by uvh, the camera image is imh x imw and the warp grid hc x wc is a third size.  A launch
that swaps h and w, a kernel that walks a row with the wrong extent, or a warp / resize adjoint with one scale for both axes is
invisible while h == w.  Non-square maps also reach weight-gradient grids no square map makes: at depth 256 (six stride-2 levels)
a 64 x 512 map ends in 1 x 8-texel levels (a grid 1-3 rows high: the tiled / narrow kernels' incremental row walk wraps the frame
index several times per 16-row step) and 512 x 64 in 8 x 1 levels (the first-generation kernel on a tall grid with gw < 4).

Bars are the suite's own for the same quantities (tests/test_gpu_model.py, test_gpu_baseline_sizes.py, test_gpu_infer.py,
test_gpu_bf16.py, test_gpu_train_step.py): rendered texels <= 1e-4 rel-L2, base / gt <= 1e-6, UV gather indices bit-exact; train
step loss and every kernel / bias <= 1e-5 against float64 (mask-conditioned at alpha = 0.3); f32x3_9 <= 1e-6; bf16 against the
bf16-operand oracle (5e-3 on the map leaving the bf16 region, 1e-4 on the texels)."""
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
from gpu_util import (rel_l2, make_pair, to_device_batch, hip_activation_masks, _dump, _set_alpha, _oracle_grads, _per_tensor,
                      WGRAD_FNS, _spy_backward, _sweep_candidates)
from test_gpu_train_step import flat_oracle_grads, per_tensor_worst, FLAT_TOL, TENSOR_TOL

pytestmark = pytest.mark.gpu
TOL = 1e-4
GRAD_TOL_FLAT = 1e-5
GRAD_TOL_TENSOR = 1e-5

# (uvh, uvw, hc, wc, imh, imw, k): both orientations of each UV shape; a warp grid whose aspect differs from the image's (the
# resize path) and one the image size itself (no resize)
SHAPES = [(64, 192, 32, 48, 48, 96, 1), (192, 64, 48, 32, 96, 48, 3),
          (64, 512, 40, 72, 40, 72, 3), (512, 64, 72, 40, 72, 40, 1)]
shape_id = lambda s: 'uv%dx%d-warp%dx%d-im%dx%d-k%d' % s


def _threads():
    torch.set_num_threads(min(os.cpu_count() or 1, 16))


def _indices_exact(vis, o_vis, uvh, uvw):
    fx, fy, inside = T.resampler_indices(o_vis['warp_px'].numpy(), uvh, uvw)
    idx = vis['uv_indices'].cpu().numpy()
    np.testing.assert_array_equal(idx[..., 0], fx)
    np.testing.assert_array_equal(idx[..., 1], fy)
    np.testing.assert_array_equal(idx[..., 2], inside.astype(np.int32))


def _forward_errors(om, pm, batch, nn, mode, reps=3):
    """`reps` calls of Model.call (plan-time trials, launch tape record, replay) against the oracle's call: errors of the last."""
    with torch.no_grad():
        o_pred_c, o_gt_c, _, o_vis = om.call(batch, mode, nn_list=nn)
    db = to_device_batch(batch, nn)
    for _ in range(reps):
        p_pred_c, p_gt_c, _, p_vis = pm.call(db, mode, want_indices=True)
    torch.cuda.synchronize()
    assert tuple(p_vis['pred'].shape[1:3]) == (om.uvh, om.uvw) and tuple(p_pred_c.shape[1:3]) == (om.imh, om.imw)
    rec = {'rel_l2_pred_uv': rel_l2(p_vis['pred'].cpu(), o_vis['pred']), 'rel_l2_pred_camspc': rel_l2(p_pred_c.cpu(), o_pred_c),
           'rel_l2_base_camspc': rel_l2(p_vis['base_camspc'].cpu(), o_vis['base_camspc'])}
    if mode != 'test':
        rec['rel_l2_gt_camspc'] = rel_l2(p_gt_c.cpu(), o_gt_c)
    _indices_exact(p_vis, o_vis, om.uvh, om.uvw)
    return rec


def _check_forward(rec):
    assert rec['rel_l2_pred_uv'] <= TOL and rec['rel_l2_pred_camspc'] <= TOL, rec
    assert rec['rel_l2_base_camspc'] <= 1e-6 and rec.get('rel_l2_gt_camspc', 0.0) <= 1e-6, rec


def _pair(shape, seed, depth=256, **kw):
    uvh, uvw, hc, wc, imh, imw, k = shape
    om, pm = make_pair(depth=depth, uvh=uvh, uvw=uvw, imh=imh, imw=imw, seed=seed, **kw)
    return om, pm


@pytest.mark.parametrize('mode', ['train', 'test'])
@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
def test_forward_fused_plan_vs_oracle(shape, mode):
    """Model.call on the autotuned fused plan, three calls (trials, tape record, replay), n = 2."""
    _threads()
    uvh, uvw, hc, wc, imh, imw, k = shape
    om, pm = _pair(shape, seed=uvh + uvw + k)
    batch, nn = O.synth_batch(2, uvh, uvw, hc, wc, imh, imw, k=k, seed=uvh + 2 * uvw)
    rec = _forward_errors(om, pm, batch, nn, mode)
    _dump('nonsquare_forward_%s_%s' % (shape_id(shape), mode), rec)
    _check_forward(rec)


@pytest.mark.parametrize('shape', SHAPES[:2], ids=shape_id)
def test_forward_direct_and_layerwise_plans_vs_oracle(shape):
    """The DIRECT conv kernels through the fused plan, and Model._call (the reference's layer-by-layer structure)."""
    _threads()
    uvh, uvw, hc, wc, imh, imw, k = shape
    om, pm = _pair(shape, seed=7 + k)
    batch, nn = O.synth_batch(2, uvh, uvw, hc, wc, imh, imw, k=k, seed=8 + k)
    pm.conv_algo = C.ALGO_DIRECT
    rec = _forward_errors(om, pm, batch, nn, 'train', reps=1)
    db = to_device_batch(batch, nn)
    x = torch.cat((db[1], db[2], db[3]), 3)
    y_obs = [(db[9][:, i] - db[8][:, i]).contiguous() for i in range(k)]
    got = pm._call(x, y_obs)
    with torch.no_grad():
        ref = om._call(torch.cat((batch[1], batch[2], batch[3]), 3), [r - b for b, r in nn])
    rec['rel_l2_layerwise'] = rel_l2(got.cpu(), ref)
    _dump('nonsquare_forward_direct_layerwise_%s' % shape_id(shape), rec)
    _check_forward(rec)
    assert rec['rel_l2_layerwise'] <= TOL, rec


def _gw(mode, w):
    return w // 2 if mode == C.CONV_K2S2 else w


def _gh(mode, h):
    return h // 2 if mode == C.CONV_K2S2 else h


def _grids(calls):
    """{function: sorted (gh, gw)} of the spied weight-gradient launches."""
    out = {}
    for c in calls:
        if c[0] in WGRAD_FNS:
            out.setdefault(c[0], set()).add((_gh(c[1], c[5]), _gw(c[1], c[6])))
    return {k: sorted(v) for k, v in out.items()}


TRAIN = [(64, 512, 'l2', 1.0), (64, 512, 'barron', 0.3), (512, 64, 'barron', 1.0), (512, 64, 'l2', 0.3)]


@pytest.mark.parametrize('uvh,uvw,loss,alpha', TRAIN)
def test_train_step_flat_and_tall_vs_float64(uvh, uvw, loss, alpha, monkeypatch):
    """One train step (n = 2, k = 1, warp 40 x 56, camera 56 x 72) against the float64 oracle, eager / recorded / replayed; the
    eager pass must reach the new grids: 64 x 512 a tiled or narrow weight gradient on a grid < 4 rows high, 512 x 64 a
    first-generation one on a grid < 4 texels wide and >= 4 rows high."""
    _threads()
    n, hc, wc, imh, imw, seed = 2, 40, 56, 56, 72, 61 + uvh // 64
    om32, pm = make_pair(depth=256, uvh=uvh, uvw=uvw, imh=imh, imw=imw, loss=loss, seed=seed)
    _set_alpha(om32, pm, alpha)
    pm.build('cuda')
    batch, nn = O.synth_batch(n, uvh, uvw, hc, wc, imh, imw, k=1, seed=seed + 100)
    dims = dict(uvh=uvh, uvw=uvw, imh=imh, imw=imw)
    lo, grads = _oracle_grads(loss, 0, 0, n, torch.float64, batch, nn, alpha, seed=seed, **dims)
    db = to_device_batch(batch, nn)
    calls = _spy_backward(monkeypatch, pm.plan)
    recs, cond = [], None
    for rep in range(3):
        if rep == 1:
            monkeypatch.undo()
        pred, gt, _, _ = pm(db, mode='train')
        lp = pm.compute_loss(pred, gt, keep_batch=True).sum() / n
        pm.flat_params.grad = None
        lp.backward()
        torch.cuda.synchronize()
        lp = float(lp.detach())
        flat, worst = _per_tensor(pm, grads)
        rec = {'pass': ('eager', 'recorded', 'replayed')[rep], 'loss_hip': lp, 'loss_oracle_f64': lo, 'flat_rel': flat,
               'worst_unconditioned': worst}
        if rep == 0:
            rec['weight_gradient_grids'] = _grids(calls)
        if alpha != 1.0:
            masks = hip_activation_masks(pm)
            if cond is None or any(not all(torch.equal(a, b) for a, b in zip(masks[key], cond[0][key])) for key in masks):
                cond = (masks,) + _oracle_grads(loss, 0, 0, n, torch.float64, batch, nn, alpha, masks=masks, seed=seed, **dims)
            flat_m, worst_m = _per_tensor(pm, cond[2])
            rec.update({'loss_oracle_f64_hip_masks': cond[1], 'flat_rel_hip_masks': flat_m, 'worst_hip_masks': worst_m})
        recs.append(rec)
    _dump('nonsquare_train_%dx%d_%s_alpha%g' % (uvh, uvw, loss, alpha), recs)
    for r in recs:
        assert abs(r['loss_hip'] - lo) <= 1e-5 * abs(lo), (r['pass'], r['loss_hip'], lo)
        assert r['flat_rel'] <= GRAD_TOL_FLAT, (r['pass'], r['flat_rel'])
        if alpha == 1.0:
            assert r['worst_unconditioned'][0][0] <= GRAD_TOL_TENSOR, (r['pass'], r['worst_unconditioned'][:4])
        else:
            assert abs(r['loss_hip'] - r['loss_oracle_f64_hip_masks']) <= 1e-5 * abs(lo), r['pass']
            assert r['flat_rel_hip_masks'] <= GRAD_TOL_FLAT, (r['pass'], r['flat_rel_hip_masks'])
            assert r['worst_hip_masks'][0][0] <= GRAD_TOL_TENSOR, (r['pass'], r['worst_hip_masks'][:4])
    grids = recs[0]['weight_gradient_grids']
    if uvh < uvw:
        flat = [g for fn in ('conv_backward_weights_tiled', 'conv_backward_weights_narrow') for g in grids.get(fn, []) if g[0] < 4]
        assert flat, "no tiled / narrow weight gradient ran on a grid < 4 rows high: %s" % grids
    else:
        tall = [g for g in grids.get('conv_backward_weights', []) if g[1] < 4 <= g[0]]
        assert tall, "no first-generation weight gradient ran on a grid < 4 wide, >= 4 high: %s" % grids


def test_adam_steps_at_64x512_match_oracle():
    """tests/test_gpu_train_step.py's three Adam-AMSGrad steps at 64 x 512 (warp 48 x 40, camera 40 x 64, k = 3, n = 2, l2)."""
    _threads()
    uvh, uvw, hc, wc, imh, imw, k = 64, 512, 48, 40, 40, 64, 3
    om, pm = make_pair(depth=256, uvh=uvh, uvw=uvw, imh=imh, imw=imw, loss='l2', seed=71)
    pm.build('cuda')
    batch, nn = O.synth_batch(2, uvh, uvw, hc, wc, imh, imw, k=k, seed=72)
    db = to_device_batch(batch, nn)
    opt_o = O.KerasAdamAMSGrad(om.parameters(), 1e-3)
    opt_p = nlt_amd.optim.AdamAMSGrad(pm, 1e-3)
    for step in range(3):
        lo, go = O.train_step(om, opt_o, batch, global_bs=2, nn_list=nn)
        lp, _ = trainvali.distributed_train_step(pm, db, opt_p, global_bs=2)
        torch.cuda.synchronize()
        assert abs(float(lp) - float(lo)) <= 2e-5 * max(1.0, abs(float(lo))), (step, float(lp), float(lo))
        ref = flat_oracle_grads(pm, go)
        rel = float((pm.flat_params.grad - ref).norm() / ref.norm())
        assert rel < FLAT_TOL, (step, rel)
        worst = per_tensor_worst(pm, go)
        assert worst[0] < TENSOR_TOL, (step, worst)
    worst = max(float((po.detach() - c.kernel.cpu()).abs().max()) for po, c in zip(om.parameters()[::2], pm._conv_layers()))
    assert worst < 2e-4, worst


@pytest.mark.parametrize('mode', ['train', 'test'])
def test_every_tuning_candidate_at_64x512(mode):
    """Every (kind, hint) the plan-time trials ran at 64 x 512 (depth 256, warp 40 x 72, camera 48 x 80, k = 1, n = 2, alpha = 1),
    forced alone on every launch it ran on (gpu_util._sweep_candidates).  train: loss and every kernel / bias gradient against
    float64; test: the rendered texels <= 1e-4 against the oracle's call.  Families asserted: the register-tiled wave tiles, the
    LDS-tiled, Winograd and c32 kernels in the forward; the LDS-tiled and Winograd kernels for backward-data.  Split-K runs where
    the trials give it launches (few GEMM rows, long K): it is forced like the rest and recorded, not required."""
    _threads()
    uvh, uvw, hc, wc, imh, imw, n, alpha = 64, 512, 40, 72, 48, 80, 2, 1.0
    om, pm = make_pair(depth=256, uvh=uvh, uvw=uvw, imh=imh, imw=imw, loss='l2', seed=81)
    _set_alpha(om, pm, alpha)
    pm.build('cuda')
    plan = pm.plan
    batch, nn = O.synth_batch(n, uvh, uvw, hc, wc, imh, imw, k=1, seed=82)
    db = to_device_batch(batch, nn)
    if mode == 'train':
        lo, grads = _oracle_grads('l2', 0, 0, n, torch.float64, batch, nn, alpha, seed=81, uvh=uvh, uvw=uvw, imh=imh, imw=imw)
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

    bad, base = run()
    assert not bad, ('autotuned plan', base)
    recs, failures, covered, n_tuned, n_cands = _sweep_candidates(plan, run)
    _dump('nonsquare_candidate_sweep_64x512_%s' % mode, {'autotuned': base, 'forced': recs, 'covered': covered,
                                                        'tuned_labels': n_tuned, 'candidates': n_cands})
    assert not failures, "candidates off the bars (candidate, worst): %s" % failures
    for fam in ('fwd.tile', 'fwd.lds', 'fwd.wino', 'fwd.c32'):
        assert covered[fam], "the forward trials never ran %s at 64 x 512: %s" % (fam, covered)
    if mode == 'train':
        for fam in ('dgrad.lds', 'dgrad.wino'):
            assert covered[fam], "the backward trials never ran %s at 64 x 512: %s" % (fam, covered)


def test_three_term_split_forward_at_192x64():
    """precision = f32x3_9 against the fp32 oracle: rendered texels <= 1e-6 rel-L2, gather indices bit-exact."""
    _threads()
    shape = SHAPES[1]
    uvh, uvw, hc, wc, imh, imw, k = shape
    om, pm = _pair(shape, seed=91, precision='f32x3_9')
    batch, nn = O.synth_batch(2, uvh, uvw, hc, wc, imh, imw, k=k, seed=92)
    rec = _forward_errors(om, pm, batch, nn, 'test')
    _dump('nonsquare_f32x3_9_%s' % shape_id(shape), rec)
    assert rec['rel_l2_pred_uv'] <= 1e-6 and rec['rel_l2_pred_camspc'] <= 1e-6 and rec['rel_l2_base_camspc'] <= 1e-6, rec


def test_bf16_forward_at_64x512():
    """precision = bf16 against OracleModel.set_precision('bf16'): <= 5e-3 on the map leaving the bf16 region, <= 1e-4 on the
    rendered texels (tests/test_gpu_bf16.py's bars)."""
    _threads()
    uvh, uvw, hc, wc, imh, imw, k = SHAPES[2]
    om = O.OracleModel(depth=256, uvh=uvh, uvw=uvw, imh=imh, imw=imw, seed=93)
    pb = get_model_class('nlt')(nlt_amd.make_config(depth=256, uvh=uvh, uvw=uvw, imh=imh, imw=imw, precision='bf16'))
    pb.load_weights(om.numpy_weights())
    pb.register_trainable()
    om.set_precision('bf16')
    batch, nn = O.synth_batch(2, uvh, uvw, hc, wc, imh, imw, k=k, seed=94)
    outs = []
    with torch.no_grad():
        om._call(torch.cat((batch[1], batch[2], batch[3]), 3), [r - b for b, r in nn], layer_outputs=outs)
        o_c, _, _, o_vis = om.call(batch, 'test', nn_list=nn)
    db = to_device_batch(batch, nn)
    for _ in range(3):
        p_c, _, _, p_vis = pb.call(db, 'test', want_indices=True)
    torch.cuda.synchronize()
    bufs = next(iter(pb.plan._bufs.values()))
    D = pb.plan.n_down
    assert bufs['fm'][3].dtype == torch.bfloat16 and bufs['dec'][D - 3].dtype == torch.float32
    rec = {'rel_l2_region_out': rel_l2(bufs['dec'][D - 3].cpu(), outs[D + 1 + D - 3]),
           'rel_l2_pred_uv': rel_l2(p_vis['pred'].cpu(), o_vis['pred']), 'rel_l2_pred_camspc': rel_l2(p_c.cpu(), o_c)}
    _dump('nonsquare_bf16_64x512', rec)
    assert rec['rel_l2_region_out'] <= 5e-3 and rec['rel_l2_pred_uv'] <= TOL and rec['rel_l2_pred_camspc'] <= TOL, rec
    _indices_exact(p_vis, o_vis, uvh, uvw)


def _agg_from_oracle(om, batches):
    with torch.no_grad():
        feats = [om._call(torch.cat((b[1], b[2], b[3]), 3), [b[5] - b[1]], return_feats=True)[1] for b, _ in batches]
    return [torch.cat([f[l] for f in feats], 0).mean(0, keepdim=True) for l in range(len(feats[0]))]


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[3]], ids=shape_id)
def test_inference_mode_vs_oracle_and_general_plan(shape):
    """The reference's inference mode (obs_override) on the fused override plan (front_ovr, map convs, dec_block and back map
    variants): <= 1e-4 against the oracle, <= 1e-5 against the general plan, replay bit-identical, indices bit-exact."""
    _threads()
    uvh, uvw, hc, wc, imh, imw, _ = shape
    n = 2
    om, pm = _pair(shape, seed=101)
    pm.build('cuda')
    agg = _agg_from_oracle(om, [O.synth_batch(2, uvh, uvw, hc, wc, imh, imw, k=1, seed=102)])
    batch, nn = O.synth_batch(n, uvh, uvw, hc, wc, imh, imw, k=1, seed=103)
    with torch.no_grad():
        o_pred_c, _, _, o_vis = om.call(batch, 'test', obs_override=[f.expand(n, -1, -1, -1) for f in agg], nn_list=nn)
    db = to_device_batch(batch, nn)
    dagg = [f.cuda() for f in agg]
    outs = []
    for _ in range(3):
        p_pred_c, _, _, p_vis = pm.call(db, 'test', obs_override=dagg, want_indices=True)
        outs.append(p_vis['pred'].clone())
    torch.cuda.synchronize()
    assert pm.plan._ovr is not None and pm.plan.tape_replays >= 1
    assert torch.equal(outs[1], outs[2])
    rec = {'rel_l2_pred_uv': rel_l2(p_vis['pred'].cpu(), o_vis['pred']), 'rel_l2_pred_camspc': rel_l2(p_pred_c.cpu(), o_pred_c)}
    _indices_exact(p_vis, o_vis, uvh, uvw)
    pm.plan.fuse_override = False
    g_vis = pm.call(db, 'test', obs_override=dagg)[3]
    pm.plan.fuse_override = True
    rec['rel_l2_vs_general_plan'] = rel_l2(p_vis['pred'].cpu(), g_vis['pred'].cpu())
    _dump('nonsquare_infer_%s' % shape_id(shape), rec)
    assert rec['rel_l2_pred_uv'] <= TOL and rec['rel_l2_pred_camspc'] <= TOL, rec
    assert rec['rel_l2_vs_general_plan'] <= 1e-5, rec


def _nonsquare_store(n_frames, uvh, uvw, hc, wc, imh, imw, seed):
    """datasets/synth.synthetic_store's layout (k = 1) with the axes apart: uint8 texels uvh x uvw, fp16 warp hc x wc (30 %
    background at (0, 0)), camera images imh x imw."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    R = lambda *s: torch.randint(0, 256, s, device='cuda', generator=g, dtype=torch.uint8)
    ids = ['trainvali_%09d_C%03d_L%03d' % (i, i, i) for i in range(n_frames)]
    warp = torch.rand((n_frames, hc, wc, 2), device='cuda', generator=g).half()
    warp[torch.rand((n_frames, hc, wc), device='cuda', generator=g) >= 0.7] = 0
    nn = {id_: {'cam': 'C%03d' % ((i + 1) % n_frames), 'light': 'L%03d' % ((i + 1) % n_frames)} for i, id_ in enumerate(ids)}
    return {'ids': ids, 'nn': nn, 'complete': [True] * n_frames,
            'diffuse': R(n_frames, uvh, uvw, 3), 'rgb': R(n_frames, uvh, uvw, 3), 'cvis': R(n_frames, uvh, uvw),
            'lvis': R(n_frames, uvh, uvw), 'rgb_camspc': R(n_frames, imh, imw, 3), 'uv2cam': warp}


@pytest.mark.parametrize('uvh,uvw,hc,wc,imh,imw', [(64, 192, 40, 56, 48, 96), (192, 64, 56, 40, 96, 48)])
def test_store_resident_inference_and_lanes(uvh, uvw, hc, wc, imh, imw):
    """nlt_test.infer over store-resident batches (the front launch reads the uint8 store by frame id, 1 / 255 in registers)
    against the assembled float batches, with test_gpu_infer's bars: rendered texels <= 1e-6 rel-L2, base_camspc and the UV
    gather indices bit-exact; RenderPipeline with 2 lanes equals one batch at a time bit for bit."""
    from nlt_amd import nlt_test
    from nlt_amd.datasets import get_dataset_class
    assert uvw % 8 == 0 and (uvh * uvw) % 16 == 0
    store = _nonsquare_store(9, uvh, uvw, hc, wc, imh, imw, seed=111)
    cfg = nlt_amd.make_config(depth=256, uvh=uvh, uvw=uvw, imh=imh, imw=imw, bs=2)
    pm = get_model_class('nlt')(cfg).build('cuda')
    pm.register_trainable()
    ds = get_dataset_class('nlt')(cfg, 'train', store, k=1, ring=0)
    agg = nlt_test.extract_feat(pm, [ds.load_batch(store['ids'][i:i + 2]) for i in (0, 2)])
    id_lists = [store['ids'][i:i + 2] for i in (4, 6, 7)]
    eager = [ds.load_batch(i) for i in id_lists]
    res = [ds.load_batch(i, resident=True) for i in id_lists]
    assert res[0][2] is None
    a = [pm.call(b, 'test', obs_override=agg, want_indices=True) for b in eager]
    b = [pm.call(x, 'test', obs_override=agg, want_indices=True) for x in res]
    torch.cuda.synchronize()
    assert pm.plan._ovr is not None
    for x, y in zip(a, b):
        assert tuple(y[3]['pred'].shape[1:3]) == (uvh, uvw) and tuple(y[0].shape[1:3]) == (imh, imw)
        assert rel_l2(y[3]['pred'].cpu(), x[3]['pred'].cpu()) <= 1e-6 and rel_l2(y[0].cpu(), x[0].cpu()) <= 1e-6
        assert torch.equal(x[3]['base_camspc'], y[3]['base_camspc']) and torch.equal(x[3]['uv_indices'], y[3]['uv_indices'])
    one = nlt_test.infer(pm, res, agg, lanes=1)
    two = nlt_test.infer(pm, res, agg, lanes=2)
    torch.cuda.synchronize()
    for x, y in zip(one, two):
        for key in ('pred', 'pred_camspc', 'base_camspc'):
            assert torch.equal(x[key], y[key]), key


def test_size_divisible_by_2_to_the_depth_in_one_axis_only_is_refused():
    """64 x 96 at depth 256: 96 is not a multiple of 2^6.  The train / test plan and the inference (obs_override) plan raise
    ValueError and launch nothing."""
    om, pm = make_pair(depth=256, uvh=64, uvw=96, imh=32, imw=48, seed=121)
    pm.build('cuda')
    batch, nn = O.synth_batch(2, 64, 96, 32, 48, 32, 48, k=1, seed=122)
    db = to_device_batch(batch, nn)
    launches = []
    real = pm.plan._launch
    pm.plan._launch = lambda *a, **kw: (launches.append(a[0]), real(*a, **kw))[1]
    for mode in ('train', 'test'):
        with pytest.raises(ValueError):
            pm.call(db, mode)
    agg = [torch.zeros((1, 64 >> l, 96 >> l, c), device='cuda') for l, c in enumerate(pm.plan._level_channels())]
    with pytest.raises(ValueError):
        pm.call(db, 'test', obs_override=agg)
    torch.cuda.synchronize()
    assert not launches, launches
    assert not pm.plan._bufs


# ---- depth 1024 (eight stride-2 levels): multiples of 256; the deepest levels are 1 x 2 and 2 x 1 texels

def test_depth1024_forward_at_256x512():
    _threads()
    shape = (256, 512, 128, 192, 160, 256, 1)
    uvh, uvw, hc, wc, imh, imw, k = shape
    om, pm = _pair(shape, seed=131, depth=1024)
    batch, nn = O.synth_batch(1, uvh, uvw, hc, wc, imh, imw, k=k, seed=132)
    rec = _forward_errors(om, pm, batch, nn, 'test')
    _dump('nonsquare_depth1024_forward_%s' % shape_id(shape), rec)
    _check_forward(rec)


def test_depth1024_train_step_at_512x256_vs_float64():
    """One alpha = 1 train step (n = 1, k = 1, warp 96 x 64, camera 128 x 96) against float64: loss, flat bucket and every
    kernel / bias <= 1e-5."""
    _threads()
    uvh, uvw, hc, wc, imh, imw, n = 512, 256, 96, 64, 128, 96, 1
    om32, pm = make_pair(depth=1024, uvh=uvh, uvw=uvw, imh=imh, imw=imw, loss='l2', seed=141)
    _set_alpha(om32, pm, 1.0)
    pm.build('cuda')
    batch, nn = O.synth_batch(n, uvh, uvw, hc, wc, imh, imw, k=1, seed=142)
    lo, grads = _oracle_grads('l2', 0, 0, n, torch.float64, batch, nn, 1.0, depth=1024, seed=141, uvh=uvh, uvw=uvw, imh=imh, imw=imw)
    db = to_device_batch(batch, nn)
    recs = []
    for rep in range(2):
        pred, gt, _, _ = pm(db, mode='train')
        lp = pm.compute_loss(pred, gt, keep_batch=True).sum() / n
        pm.flat_params.grad = None
        lp.backward()
        torch.cuda.synchronize()
        flat, worst = _per_tensor(pm, grads)
        recs.append({'loss_hip': float(lp.detach()), 'loss_oracle_f64': lo, 'flat_rel': flat, 'worst': worst})
    _dump('nonsquare_depth1024_train_512x256', recs)
    for r in recs:
        assert abs(r['loss_hip'] - lo) <= 1e-5 * abs(lo), r
        assert r['flat_rel'] <= GRAD_TOL_FLAT and r['worst'][0][0] <= GRAD_TOL_TENSOR, r
