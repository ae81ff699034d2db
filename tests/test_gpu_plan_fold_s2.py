"""-m gpu: a plan whose level-2 stride-1 observation launch also runs level 3's stride-2 observation conv (lds_hints['L2.o.s1'] =
engine.FOLD_HINT; csrc/conv_tile3.hip, conv_tile3w_s2_kernel), forced -- the plan-time trials choose it only where it wins.

  * `pred`, `pred_camspc` and the UV gather indices against the oracle at the f32x3_9 bars of tests/test_gpu_baseline_sizes.py;
  * fm[2] bit-equal to the plan that launches the two convs;
  * a two-lane RenderPipeline bit-identical to Model.call;
  * tuning export -> import -> the same launches;
  * a train step on the same model still launches the two convs.
"""
import numpy as np
import pytest
import torch

from nlt_amd import capi as C
from nlt_amd import engine
from nlt_amd.pipeline import RenderPipeline
from oracle import nlt_oracle as O
from oracle import tf_ops as T
from gpu_util import rel_l2, make_pair, to_device_batch

pytestmark = pytest.mark.gpu
TOL = 1e-6
UNFOLDED = 512 + 32


def _pair(uvh, uvw, hint, seed=4, **kw):
    om, pm = make_pair(depth=256, uvh=uvh, uvw=uvw, imh=uvh // 2, imw=uvw // 2, seed=seed, precision='f32x3_9', **kw)
    pm.plan.autotune = False
    pm.plan.lds_hints = {'L2.o.s1': hint}
    return om, pm


def _spy(pm):
    """Labels of the plan's launches, in order (launch tapes off: every pass goes through `_launch`)."""
    pm.plan.use_tape = False
    labels, real = [], pm.plan._launch

    def launch(label, nbytes, fn, *a, **kw):
        labels.append((label, fn.__name__))
        real(label, nbytes, fn, *a, **kw)
    pm.plan._launch = launch
    return labels


def _batch(uvh, uvw, n, k, seed):
    return O.synth_batch(n, uvh, uvw, uvh // 2, uvw // 2, uvh // 2, uvw // 2, k=k, seed=seed)


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('k', [1, 4])
@pytest.mark.parametrize('uvh,uvw', [(64, 64), (128, 64)])
def test_forced_fold_vs_the_oracle_and_the_two_launch_plan(uvh, uvw, k, n):
    om, pm = _pair(uvh, uvw, engine.FOLD_HINT)
    _, pu = _pair(uvh, uvw, UNFOLDED)
    batch, nn = _batch(uvh, uvw, n, k, 100 + k + n)
    with torch.no_grad():
        o_pred_c, _, _, o_vis = om.call(batch, 'test', nn_list=nn)
    db = to_device_batch(batch, nn)
    labels, labels_u = _spy(pm), _spy(pu)
    p_pred_c, _, _, p_vis = pm.call(db, 'test', want_indices=True)
    u_pred_c, _, _, u_vis = pu.call(db, 'test')
    torch.cuda.synchronize()
    assert ('L2.o.s1', 'conv_tile3w_s2_forward') in labels and not any(l == 'L3.o.s2' for l, _ in labels)
    assert ('L2.o.s1', 'conv_tile3r_forward') in labels_u and [l for l, _ in labels_u if l != 'L3.o.s2'] == [l for l, _ in labels]
    assert pm.plan.ran('lds') == {'L2.o.s1'}
    e_uv, e_cam = rel_l2(p_vis['pred'].cpu(), o_vis['pred']), rel_l2(p_pred_c.cpu(), o_pred_c)
    print("fold forced %dx%d k %d n %d: rel-L2 pred %.2e pred_camspc %.2e (two launches: %.2e %.2e)"
          % (uvh, uvw, k, n, e_uv, e_cam, rel_l2(u_vis['pred'].cpu(), o_vis['pred']), rel_l2(u_pred_c.cpu(), o_pred_c)))
    assert e_uv <= TOL and e_cam <= TOL and rel_l2(p_vis['base_camspc'].cpu(), o_vis['base_camspc']) <= 1e-6
    fx, fy, inside = T.resampler_indices(o_vis['warp_px'].numpy(), uvh, uvw)
    idx = p_vis['uv_indices'].cpu().numpy()
    np.testing.assert_array_equal(idx[..., 0], fx)
    np.testing.assert_array_equal(idx[..., 1], fy)
    np.testing.assert_array_equal(idx[..., 2], inside.astype(np.int32))
    fm2 = lambda m: next(iter(m.plan._bufs.values()))['fm'][2]
    assert torch.equal(fm2(pm), fm2(pu))


def test_two_lane_pipeline_equals_model_call():
    uvh, uvw, k = 128, 64, 4
    _, pm = _pair(uvh, uvw, engine.FOLD_HINT)
    batches = [to_device_batch(*_batch(uvh, uvw, 2, k, 200 + i)) for i in range(4)]
    ref = [pm.call(b, 'test') for b in batches]
    torch.cuda.synchronize()
    ref = [(r[0].clone(), {key: r[3][key].clone() for key in ('pred', 'pred_camspc')}) for r in ref]
    pipe = RenderPipeline(pm, 2)
    for rounds in range(3):                                              # eager pass, recorded launch tapes, replays
        outs = [t.result() for t in [pipe.submit(b, 'test') for b in batches]]
        torch.cuda.synchronize()
        for (r0, rv), out in zip(ref, outs):
            assert torch.equal(r0, out[0]) and all(torch.equal(rv[key], out[3][key]) for key in rv)
    assert pipe._lanes[1].plan is not pm.plan and pipe._lanes[1].plan.lds_hints == {'L2.o.s1': engine.FOLD_HINT}
    pipe.close()


def test_exported_tuning_imports_to_the_same_launches():
    uvh, uvw, k = 64, 64, 4
    _, pa = _pair(uvh, uvw, engine.FOLD_HINT)
    _, pb = _pair(uvh, uvw, 0)
    pb.plan.lds_hints = {}
    pb.plan.import_tuning(pa.plan.export_tuning())
    assert pb.plan.export_tuning() == pa.plan.export_tuning() and pb.plan.lds_hints['L2.o.s1'] == engine.FOLD_HINT
    db = to_device_batch(*_batch(uvh, uvw, 2, k, 300))
    la, lb = _spy(pa), _spy(pb)
    a, b = pa.call(db, 'test'), pb.call(db, 'test')
    torch.cuda.synchronize()
    assert la == lb and ('L2.o.s1', 'conv_tile3w_s2_forward') in la
    assert torch.equal(a[3]['pred'], b[3]['pred'])


def test_a_train_step_on_the_same_model_launches_the_two_convs():
    uvh, uvw = 64, 64
    _, pm = _pair(uvh, uvw, engine.FOLD_HINT)
    pm.build('cuda')
    db = to_device_batch(*_batch(uvh, uvw, 2, 1, 400))
    labels = _spy(pm)
    pm.call(db, 'test')
    assert ('L2.o.s1', 'conv_tile3w_s2_forward') in labels
    del labels[:]
    pred, gt, _, _ = pm(db, mode='train')
    loss = pm.compute_loss(pred, gt, keep_batch=True).sum()
    loss.backward()
    torch.cuda.synchronize()
    names = dict(labels)
    assert names['L2.o.s1'] == 'conv_tile3r_forward' and 'L3.o.s2' in names and 'conv_tile3w_s2_forward' not in names.values()
    assert torch.isfinite(pm.flat_params.grad).all()
