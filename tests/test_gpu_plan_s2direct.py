"""-m gpu: a plan whose stride-2 encoder launches run on the texels-direct form of the three-term split conv (`lds_hints` =
engine.DIRECT_S2 + tn; csrc/conv_tile3.hip, conv_tile3d_kernel), forced on every stride-2 encoder label -- the plan-time trials
choose it only where it wins.

  * `pred`, `pred_camspc` and every level's feature map fm[l] bit-equal to the same plan with those launches on the streaming
    kernel (hint tn);
  * `pred`, `pred_camspc` against the oracle (<= 1e-4 rel-L2) and the UV gather indices bit-exact;
  * once more through the launch tape: the same bits.
"""
import numpy as np
import pytest
import torch

from nlt_amd import capi as C
from nlt_amd import engine
from oracle import nlt_oracle as O
from oracle import tf_ops as T
from gpu_util import rel_l2, make_pair, to_device_batch

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _pair(uvh, uvw, bit, tn, precision):
    om, pm = make_pair(depth=256, uvh=uvh, uvw=uvw, imh=uvh // 2, imw=uvw // 2, seed=4, precision=precision)
    pm.build('cuda')
    nlev = sum(pm.net['query'].is_contracting) - 1
    pm.plan.autotune = False
    pm.plan.lds_hints = {'L%d.%s.s2' % (l, p): bit + tn for l in range(1, nlev + 1) for p in 'qo'}
    return om, pm


def _count(monkeypatch):
    """The labels nlt_conv_tile3d_forward / nlt_conv_tile3_forward are launched under, through the adapters."""
    calls = {'conv_tile3d_forward': [], 'conv_tile3_forward': []}
    for name in calls:
        real = getattr(C, name)
        monkeypatch.setattr(C, name, (lambda real, name: lambda *a, **kw: (calls[name].append(a[1:3]), real(*a, **kw))[1])(real, name))
    return calls


# (uvh, uvw, k, n, precision, tn): tn = output channels per workgroup, + 256 = the observations as frames of their own
CASES = [(64, 64, 1, 1, 'f32x3_9', 32), (64, 64, 4, 3, 'f32x3_9', 32), (128, 64, 4, 1, 'f32x3_9', 32), (128, 64, 1, 3, 'f32x3_9', 64),
         (128, 64, 4, 3, 'f32x3', 32), (64, 64, 4, 3, 'f32x3_9', 256 + 64)]


@pytest.mark.parametrize('uvh,uvw,k,n,precision,tn', CASES)
def test_forced_direct_vs_the_streaming_plan_the_oracle_and_its_own_replay(monkeypatch, uvh, uvw, k, n, precision, tn):
    om, pd = _pair(uvh, uvw, engine.DIRECT_S2, tn, precision)
    _, ps = _pair(uvh, uvw, 0, tn, precision)
    batch, nn = O.synth_batch(n, uvh, uvw, uvh // 2, uvw // 2, uvh // 2, uvw // 2, k=k, seed=100 + k + n)
    with torch.no_grad():
        o_pred_c, _, _, o_vis = om.call(batch, 'test', nn_list=nn)
    db = to_device_batch(batch, nn)
    calls = _count(monkeypatch)
    d_pred_c, _, _, d_vis = pd.call(db, 'test', want_indices=True)
    n_direct, n_stream = len(calls['conv_tile3d_forward']), len(calls['conv_tile3_forward'])
    s_pred_c, _, _, s_vis = ps.call(db, 'test')
    torch.cuda.synchronize()
    # the forced plan sent stride-2 launches to the new entry; the other plan sent the SAME launches to the streaming kernel
    assert n_direct >= 2 and len(calls['conv_tile3d_forward']) == n_direct, calls
    assert len(calls['conv_tile3_forward']) - n_stream == n_direct + n_stream, calls
    assert pd.plan.ran('lds') == ps.plan.ran('lds') and all(label.endswith('.s2') for label in pd.plan.ran('lds'))
    assert torch.equal(d_vis['pred'], s_vis['pred']) and torch.equal(d_pred_c, s_pred_c)
    fm = lambda m: next(iter(m.plan._bufs.values()))['fm'][2:]           # (from the first level a forced launch feeds)
    assert len(fm(pd)) == len(fm(ps)) >= 2 and all(torch.equal(a, b) for a, b in zip(fm(pd), fm(ps)))
    e_uv, e_cam = rel_l2(d_vis['pred'].cpu(), o_vis['pred']), rel_l2(d_pred_c.cpu(), o_pred_c)
    print("direct forced %dx%d k %d n %d %s hint %d: %d launches, rel-L2 pred %.2e pred_camspc %.2e"
          % (uvh, uvw, k, n, precision, tn, n_direct, e_uv, e_cam))
    assert e_uv <= TOL and e_cam <= TOL
    fx, fy, inside = T.resampler_indices(o_vis['warp_px'].numpy(), uvh, uvw)
    idx = d_vis['uv_indices'].cpu().numpy()
    np.testing.assert_array_equal(idx[..., 0], fx)
    np.testing.assert_array_equal(idx[..., 1], fy)
    np.testing.assert_array_equal(idx[..., 2], inside.astype(np.int32))
    # second sight records the launch tape, the third replays it
    keep, keep_c = d_vis['pred'].clone(), d_pred_c.clone()
    before = pd.plan.tape_replays
    for _ in range(3):
        r_pred_c, _, _, r_vis = pd.call(db, 'test')
    torch.cuda.synchronize()
    assert pd.plan.tape_replays > before
    assert torch.equal(r_vis['pred'], keep) and torch.equal(r_pred_c, keep_c)
    assert all(torch.equal(a, b) for a, b in zip(fm(pd), fm(ps)))
