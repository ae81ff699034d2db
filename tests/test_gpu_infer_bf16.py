"""-m gpu: `precision = bf16` under the reference's inference mode -- nlt_test.infer -> Model.call(batch, 'test',
obs_override=feat_agg) (nlt/nlt_test.py:78-127, nlt/models/nlt.py:154-155,172-174) -- on the fused query-only plan with its
bf16 region (engine_infer.py: levels >= 3 and the expanding blocks j <= D - 3 on csrc/conv_bf16.hip, the concat convs through
nlt_conv_bf16_forward_map), against OracleModel.set_precision('bf16') called with obs_override.

The oracle rounds the same operands at the same places, so the plan differs from it by fp32 summation order.  Bars
(tests/test_gpu_bf16.py): <= 5e-3 rel-L2 on the map leaving the region, <= 1e-4 on the rendered texels, UV
gather indices bit-exact.  Those do not tell a bf16 region from an fp32 one (the two oracles are 1.3-1.7e-3 apart on the region's
output); what does: level 3's output -- two stacked bf16 convs, the first conv + map -- is BIT-EQUAL to the bf16 oracle's in
>= 98 % of its elements (a level computed in fp32 and rounded afterwards: 52-56 %).  The distances to the fp32 oracle and to
this build's fp32 override plan are printed, not asserted."""
import os

import numpy as np
import pytest
import torch

import nlt_amd
from nlt_amd import capi as C
from oracle import nlt_oracle as O
from oracle import tf_ops as T
from gpu_util import rel_l2, make_pair, to_device_batch

pytestmark = pytest.mark.gpu
TOL_REGION, TOL_PRED, MIN_EQUAL = 5e-3, 1e-4, 0.98
CAM = 32


def _agg_from_oracle(om, batches):
    """nlt_test.extract_feat on the (fp32) oracle: mean over all frames of every level's observation features of x = rgb - base."""
    with torch.no_grad():
        feats = [om._call(torch.cat((b[1], b[2], b[3]), 3), [b[5] - b[1]], return_feats=True)[1] for b, _ in batches]
    return [torch.cat([f[l] for f in feats], 0).mean(0, keepdim=True) for l in range(len(feats[0]))]


@pytest.mark.parametrize('depth,uvh,uvw,n', [(64, 32, 32, 3), (64, 48, 32, 2), (256, 64, 64, 2), (256, 128, 64, 1)])
def test_bf16_override_plan_vs_the_bf16_oracle(depth, uvh, uvw, n):
    """The smallest sizes at which every launch of the region exists (level D is 2x2, 3x2, 1x1, 2x1): plan-time trials, tape
    record, replay; the bottleneck's two-source form and the fp32 hand-over at block D - 3 are both on the path."""
    torch.set_num_threads(min(os.cpu_count() or 1, 64))
    seed = depth + uvh
    om, pm = make_pair(depth=depth, uvh=uvh, uvw=uvw, im=CAM, seed=seed, precision='bf16')
    pm.build('cuda')                                        # flat parameter bucket + pack registry: launch tapes need them
    agg = _agg_from_oracle(om, [O.synth_batch(2, uvh, uvw, CAM, CAM, CAM, CAM, k=1, seed=seed + 50)])
    batch, nn = O.synth_batch(n, uvh, uvw, CAM, CAM, CAM, CAM, k=1, seed=seed + 100)
    tiled = [f.expand(n, -1, -1, -1) for f in agg]
    with torch.no_grad():
        ref32 = om.call(batch, 'test', obs_override=tiled, nn_list=nn)[3]['pred']
        om.set_precision('bf16')
        outs = []
        om._call(torch.cat((batch[1], batch[2], batch[3]), 3), [r - b for b, r in nn], obs_override=tiled, layer_outputs=outs)
        o_pred_c, _, _, o_vis = om.call(batch, 'test', obs_override=tiled, nn_list=nn)
    db = to_device_batch(batch, nn)
    dagg = [f.cuda() for f in agg]
    preds = []
    for _ in range(3):                                      # plan-time trials, launch tape record, a replayed step
        p_pred_c, _, _, p_vis = pm.call(db, 'test', obs_override=dagg, want_indices=True)
        preds.append(p_vis['pred'].clone())
    torch.cuda.synchronize()
    assert pm.plan.precision == 'bf16' and pm.plan._ovr is not None and pm.plan.tape_replays >= 1
    assert torch.equal(preds[1], preds[2])                  # the replay reproduces the recorded pass bit for bit
    (bufs,) = pm.plan._bufs.values()
    D, cl = pm.plan.n_down, bufs['C']
    assert bufs['fm'][3].dtype == torch.bfloat16 and bufs['fm'][2].dtype == torch.float32
    assert bufs['dec'][D - 3].dtype == torch.float32 and bufs['dtmp'][D - 3].dtype == torch.bfloat16
    same = float((bufs['fm'][3][..., :cl[3]].float().cpu() == outs[3]).float().mean())
    e_region = rel_l2(bufs['dec'][D - 3].cpu(), outs[D + 1 + D - 3])
    e_uv, e_cam = rel_l2(p_vis['pred'].cpu(), o_vis['pred']), rel_l2(p_pred_c.cpu(), o_pred_c)
    e32 = rel_l2(p_vis['pred'].cpu(), ref32)
    pm.plan.precision, pm.plan.autotune = 'fp32', False     # this build's fp32 override plan on the same maps (no second round of trials)
    f_vis = pm.call(db, 'test', obs_override=dagg)[3]
    pm.plan.precision = 'bf16'
    e_plan32 = rel_l2(p_vis['pred'].cpu(), f_vis['pred'].cpu())
    print("bf16 override plan depth %d %dx%d x%d: fm[3] bit-equal %.4f, region out %.2e, pred %.2e, pred_camspc %.2e vs the bf16 "
          "oracle; pred vs the fp32 oracle %.2e, vs the fp32 override plan %.2e" % (depth, uvh, uvw, n, same, e_region, e_uv, e_cam, e32, e_plan32))
    assert same >= MIN_EQUAL
    assert e_region <= TOL_REGION
    assert e_uv <= TOL_PRED and e_cam <= TOL_PRED
    fx, fy, inside = T.resampler_indices(o_vis['warp_px'].numpy(), uvh, uvw)
    idx = p_vis['uv_indices'].cpu().numpy()
    np.testing.assert_array_equal(idx[..., 0], fx)
    np.testing.assert_array_equal(idx[..., 1], fy)
    np.testing.assert_array_equal(idx[..., 2], inside.astype(np.int32))


def test_bf16_infer_with_two_lanes_is_bit_identical_to_one():
    from nlt_amd import nlt_test
    depth, uv = 64, 32
    om, pm = make_pair(depth=depth, uv=uv, im=CAM, seed=11, precision='bf16')
    pm.build('cuda')
    agg = [f.cuda() for f in _agg_from_oracle(om, [O.synth_batch(2, uv, uv, CAM, CAM, CAM, CAM, k=1, seed=12)])]
    tests_ = [O.synth_batch(2, uv, uv, CAM, CAM, CAM, CAM, k=1, seed=20 + i) for i in range(4)]
    dbs = [to_device_batch(b, nn) for b, nn in tests_]
    one = nlt_test.infer(pm, dbs, agg)
    assert pm.plan._ovr is not None and pm.plan._ovr['stamp'][0] == 'bf16'
    (bufs,) = pm.plan._bufs.values()
    assert bufs['fm'][3].dtype == torch.bfloat16
    two = nlt_test.infer(pm, dbs, agg, lanes=2)
    torch.cuda.synchronize()
    for a, b in zip(one, two):
        assert torch.equal(a['pred'], b['pred']) and torch.equal(a['pred_camspc'], b['pred_camspc'])
    with torch.no_grad():
        om.set_precision('bf16')
        ref = om.call(tests_[3][0], 'test', obs_override=[f.cpu().expand(2, -1, -1, -1) for f in agg], nn_list=tests_[3][1])[3]['pred']
    assert rel_l2(one[3]['pred'].cpu(), ref) <= TOL_PRED


def test_bf16_infer_on_store_resident_batches():
    """Dataset.load_batch(resident=True) under precision = bf16: the override plan with its front launch on the uint8 store.
    Within 1e-4 of the float-batch bf16 result (no bit-level bar: the uint8 front differs from the float one by <= 1e-6, which
    can move a bf16 rounding); replays bit-identical."""
    from nlt_amd import nlt_test
    from nlt_amd.datasets import get_dataset_class
    from nlt_amd.datasets.synth import synthetic_store
    from nlt_amd.models import get_model_class
    uv, cam = 256, 128
    store = synthetic_store(9, uv, cam, seed=5, k=1)
    cfg = nlt_amd.make_config(depth=256, uvh=uv, uvw=uv, imh=cam, imw=cam, bs=2, precision='bf16')
    pm = get_model_class('nlt')(cfg).build('cuda')
    pm.register_trainable()
    ds = get_dataset_class('nlt')(cfg, 'train', store, k=1, ring=0)
    agg = nlt_test.extract_feat(pm, [ds.load_batch(store['ids'][i:i + 2]) for i in (0, 2)])   # (the observation net, layer by layer)
    id_lists = [store['ids'][i:i + 2] for i in (4, 6)]
    eager = [pm.call(ds.load_batch(i), 'test', obs_override=agg) for i in id_lists]
    res = [ds.load_batch(i, resident=True) for i in id_lists]
    assert res[0][2] is None
    got = [pm.call(b, 'test', obs_override=agg) for b in res]
    torch.cuda.synchronize()
    assert pm.plan._ovr is not None and pm.plan._ovr['stamp'][0] == 'bf16'
    (bufs,) = pm.plan._bufs.values()
    assert bufs['fm'][3].dtype == torch.bfloat16 and bufs['fm'][2].dtype == torch.float32
    for x, y in zip(eager, got):
        assert rel_l2(y[3]['pred'].cpu(), x[3]['pred'].cpu()) <= 1e-4 and rel_l2(y[0].cpu(), x[0].cpu()) <= 1e-4
    first = [y[3]['pred'].clone() for y in got]
    r0 = pm.plan.tape_replays
    for _ in range(3):
        again = [pm.call(x, 'test', obs_override=agg) for x in res]
    torch.cuda.synchronize()
    assert pm.plan.tape_replays > r0
    for x, y in zip(first, again):
        assert torch.equal(x, y[3]['pred'])
