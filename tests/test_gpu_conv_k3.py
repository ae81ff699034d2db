"""-m gpu: kernel = 3 on csrc/conv_k3.hip.  Each 3x3 layer form (Conv2D / Conv2DTranspose, stride 1 / 2) through the layer
object and the layer-by-layer path's backward closure -- forward, dx, dkernel, dbias -- against float64 from
tests/conv_k3_ref.py, at the bound tests/test_gpu_conv.py holds k2 to (max abs error <= 2e-5 x the reference's max abs);
then whole kernel = 3 models against oracle.OracleModel, whose transposed conv is replaced by conv_k3_ref's (the oracle's
own crops the wrong ring at k3 s1: tests/test_conv_k3_ref.py)."""
import functools

import numpy as np
import pytest
import torch

import nlt_amd
from nlt_amd import capi as C
from nlt_amd import generic, trainvali
from nlt_amd.models import get_model_class
from nlt_amd.networks.elements import Act, Conv2D
from oracle import nlt_oracle as O
from oracle import tf_ops as T
import conv_k3_ref as R
from gpu_util import rel_l2, to_device_batch

pytestmark = pytest.mark.gpu

FORMS = [(1, False), (2, False), (1, True), (2, True)]
SHAPES = [(6, 10), (2, 2), (34, 18), (5, 7)]
CHANNELS = [(16, 16), (32, 16), (80, 8), (128, 16), (8, 4), (3, 16), (5, 3), (6, 10)]
CASES = [(s, tr, hw, ch) for (s, tr) in FORMS for hw in SHAPES for ch in CHANNELS if not (s == 2 and hw == (5, 7))]
ALPHA = 0.3


@functools.lru_cache(maxsize=None)
def _reference(stride, transpose, hw, ch):
    """Inputs (fp32) and the float64 pre-activation output with the gradients of <y, g>; shared by the act on / off cases."""
    (h, w), (cin, cout) = hw, ch
    gen = torch.Generator().manual_seed(1000 * stride + 100 * transpose + 7 * h + cin)
    x = torch.randn(2, h, w, cin, generator=gen)
    wk = torch.randn((3, 3, cout, cin) if transpose else (3, 3, cin, cout), generator=gen) * 0.2
    b = torch.randn(cout, generator=gen)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, wk, b))
    y = R.layer_f64(xd, wd, bd, stride, transpose)
    g = torch.randn(y.shape, generator=gen)
    return x, wk, b, g, y.detach(), xd, wd, bd, y


def _close(got, ref, what):
    err, scale = float((got.double().cpu() - ref).abs().max()), float(ref.abs().max())
    print('%s: max abs error %.3e, reference max abs %.3e (bound %.3e)' % (what, err, scale, 2e-5 * scale))
    assert err <= 2e-5 * scale, (what, err, scale)


@pytest.mark.parametrize('act', [False, True], ids=['linear', 'lrelu'])
@pytest.mark.parametrize('stride,transpose,hw,ch', CASES,
                         ids=['%s_s%d_%dx%d_%dto%d' % ('deconv' if tr else 'conv', s, hw[0], hw[1], ch[0], ch[1]) for s, tr, hw, ch in CASES])
def test_layer_forward_and_backward(stride, transpose, hw, ch, act):
    x, wk, b, g, ypre, xd, wd, bd, ygraph = _reference(stride, transpose, hw, ch)
    cout = ch[1]
    layer = Conv2D(cout, 3, stride, transpose)
    layer.set_weights(wk, b)
    a = Act(ALPHA) if act else None
    tape = generic.Tape(True)
    xin = tape.add(x.cuda(), (tape.leaf(x.cuda()),), lambda gr: (None,))         # not a network input: dx is wanted
    outs = []
    for _ in range(2):                                                            # twice into pre-filled destinations
        layer.dkernel = torch.full(tuple(wk.shape), 0.5, device='cuda')
        layer.dbias = torch.full((cout,), -2.0, device='cuda')
        node = generic.conv(tape, layer, xin, act=a)
        (dx,) = node.back(g.cuda())
        torch.cuda.synchronize()
        outs.append((node.value.cpu(), dx.cpu(), layer.dkernel.cpu(), layer.dbias.cpu()))
    assert all(torch.equal(p, q) for p, q in zip(*outs)), "two runs are bit-identical"
    y, dx, dk, db = outs[0]
    yref = T.leaky_relu(ypre, ALPHA) if act else ypre
    assert tuple(y.shape) == tuple(yref.shape)
    _close(y, yref, 'forward')
    gpre = g.double() * torch.where(y.double() > 0, 1.0, ALPHA) if act else g.double()   # the mask the device path takes from its own y
    rdx, rdw, rdb = torch.autograd.grad(ygraph, (xd, wd, bd), gpre, retain_graph=True)
    _close(dx, rdx, 'dx')
    _close(dk - 0.5, rdw, 'dkernel (accumulated on 0.5)')
    _close(db + 2.0, rdb, 'dbias (accumulated on -2)')


@pytest.mark.parametrize('stride,transpose', FORMS)
def test_direct_kernel_on_mfma_shapes_and_bad_arguments(stride, transpose):
    """The any-channel kernel on a shape the fast path would take; stride 2 on an odd size is an error status."""
    x, wk, b, g, ypre, *_ = _reference(stride, transpose, (6, 10), (16, 16))
    mode = Conv2D(16, 3, stride, transpose).mode
    out = torch.empty(tuple(ypre.shape), device='cuda')
    C.conv_k3_forward(mode, x.cuda(), wk.cuda(), b.cuda(), 16, out, act=False, algo=C.ALGO_DIRECT)
    _close(out, ypre, 'direct forward')
    with pytest.raises(C.NLTError):
        C.conv_k3_forward(mode, torch.zeros(1, 6, 10, 6, device='cuda'), torch.zeros(3, 3, 6, 6, device='cuda'), torch.zeros(6, device='cuda'),
                          6, torch.empty(1, 6, 10, 6, device='cuda'), algo=C.ALGO_MFMA)                 # 6 channels: no fast path
    if stride == 2:
        x57 = torch.zeros(2, 5, 7, 16, device='cuda')
        with pytest.raises(C.NLTError):
            Conv2D(16, 3, 2, transpose)(x57)
        with pytest.raises(C.NLTError):
            C.conv_k3_backward_weights(mode, x57, torch.zeros(2, 10, 14, 16, device='cuda'), 16,
                                       torch.zeros(3, 3, 16, 16, device='cuda'), torch.zeros(16, device='cuda'))


def test_k2_entry_points_refuse_the_new_modes():
    x = torch.zeros(1, 4, 4, 16, device='cuda')
    w = torch.zeros(3, 3, 16, 16, device='cuda')
    b = torch.zeros(16, device='cuda')
    for mode in (C.CONV_K3S1, C.CONV_K3S2, C.DECONV_K3S1, C.DECONV_K3S2):
        assert C.packed_weight_floats(mode, 16, 0, 16) <= 0
        assert not C.conv_tile_supported(mode, 16, 32, 32) and not C.conv_wino_supported(mode, 16, 32, 32)
        assert not C.conv_c32_supported(mode, 16, 32) and not C.wgrad_narrow_supported(mode, 16, 0, 1, 4, 4, 16)
        with pytest.raises(C.NLTError):
            C.conv_forward(mode, x, 16, 16, None, 0, 0, 1, 4, 4, w, None, b, 16, torch.empty_like(x), 16, algo=C.ALGO_DIRECT)
        with pytest.raises((C.NLTError, NotImplementedError)):
            C.conv_backward_weights(mode, x, 16, 16, None, 0, 0, 1, 4, 4, x, 16, 16, torch.zeros_like(w), torch.zeros_like(b))
        with pytest.raises(C.NLTError):
            C.conv_backward_weights_tiled(mode, x, 16, 16, None, 0, 0, 1, 4, 4, x, 16, 16, torch.zeros_like(w), torch.zeros_like(b))
        with pytest.raises(C.NLTError):
            C.pack_conv_weights(mode, w, 16, 0, 16)


# ---------------------------------------------------------------- whole models
def _pair(monkeypatch, depth=32, **kw):
    monkeypatch.setattr(T, 'conv2d_transpose_same', R.conv2d_transpose_same)
    om = O.OracleModel(depth=depth, kernel=3, uvh=128, uvw=128, imh=64, imw=64, seed=2, **kw)
    pm = get_model_class('nlt')(nlt_amd.make_config(depth=depth, kernel=3, uvh=128, uvw=128, imh=64, imw=64, **kw))
    pm.load_weights(om.numpy_weights())
    pm.register_trainable()
    return om, pm


MODELS = [dict(), dict(pool='avg', act='elu'), dict(use_obs=False)]


@pytest.mark.parametrize('kw', MODELS, ids=lambda kw: '+'.join('%s=%s' % x for x in kw.items()) or 'plain')
def test_kernel3_model_forward_and_train_step_vs_oracle(monkeypatch, kw):
    om, pm = _pair(monkeypatch, loss='l2', **kw)
    assert pm.generic
    pm.build('cuda')
    batch, nn = O.synth_batch(2, 128, 128, 64, 64, 64, 64, k=2, seed=9)
    db = to_device_batch(batch, nn)
    with torch.no_grad():
        ref = om.call(batch, 'vali', nn_list=nn)
    got = pm.call(db, 'vali', want_indices=True)
    torch.cuda.synchronize()
    e1, e2 = rel_l2(got[3]['pred'].cpu(), ref[3]['pred']), rel_l2(got[0].cpu(), ref[0])
    print('pred rel-L2 %.3e, pred_camspc rel-L2 %.3e (bound 1e-4)' % (e1, e2))
    assert e1 <= 1e-4 and e2 <= 1e-4
    po, go, _, _ = om.call(batch, 'train', nn_list=nn)
    lo = om.compute_loss(po, go, keep_batch=True).sum() / 2
    grads = torch.autograd.grad(lo, om.parameters(), allow_unused=True)   # (use_obs = False: the observation net is unused)
    pred, gt, _, _ = pm(db, mode='train')
    lp = pm.compute_loss(pred, gt, keep_batch=True).sum() / 2
    pm.flat_params.grad = None
    lp.backward()
    torch.cuda.synchronize()
    print('loss %.9e vs %.9e' % (float(lp.detach()), float(lo.detach())))
    assert abs(float(lp.detach()) - float(lo.detach())) <= 1e-5 * abs(float(lo.detach()))
    it = iter(grads)
    worst = 0.0
    for c in pm._conv_layers():
        for name in ('dkernel', 'dbias'):
            g = next(it)
            if g is None:
                assert not kw.get('use_obs', True) and not getattr(c, name).any()
                continue
            worst = max(worst, float((getattr(c, name).cpu() - g).norm() / (g.norm() + 1e-30)))
    print('worst per-tensor gradient rel-L2 %.3e (bound 5e-3)' % worst)
    assert worst <= 5e-3, worst
    opt = nlt_amd.optim.AdamAMSGrad(pm, 1e-3)
    loss, _ = trainvali.distributed_train_step(pm, db, opt, 2)
    assert np.isfinite(float(loss))


def test_kernel3_depth256_forward(monkeypatch):
    """The deepest level is 2 x 2 texels with 512 -> 256 channels: tiles larger than the image."""
    om, pm = _pair(monkeypatch, depth=256)
    pm.build('cuda')
    batch, nn = O.synth_batch(2, 128, 128, 64, 64, 64, 64, k=2, seed=5)
    with torch.no_grad():
        ref = om.call(batch, 'vali', nn_list=nn)
    got = pm.call(to_device_batch(batch, nn), 'vali')
    torch.cuda.synchronize()
    e1, e2 = rel_l2(got[3]['pred'].cpu(), ref[3]['pred']), rel_l2(got[0].cpu(), ref[0])
    print('pred rel-L2 %.3e, pred_camspc rel-L2 %.3e (bound 1e-4)' % (e1, e2))
    assert e1 <= 1e-4 and e2 <= 1e-4


def test_kernel3_test_mode_with_obs_override(monkeypatch):
    om, pm = _pair(monkeypatch)
    pm.build('cuda')
    n = 2
    batch, nn = O.synth_batch(n, 128, 128, 64, 64, 64, 64, k=2, seed=4)
    with torch.no_grad():
        x = torch.cat((batch[1], batch[2], batch[3]), 3)
        _, feats = om._call(x, [r - b for b, r in nn], return_feats=True)
        agg = [f.mean(0, keepdim=True) for f in feats]
        ref = om.call(batch, 'test', obs_override=[a.expand(n, -1, -1, -1) for a in agg], nn_list=nn)
    got = pm.call(to_device_batch(batch, nn), 'test', obs_override=[a.cuda() for a in agg])
    torch.cuda.synchronize()
    e1, e2 = rel_l2(got[3]['pred'].cpu(), ref[3]['pred']), rel_l2(got[0].cpu(), ref[0])
    print('obs_override: pred rel-L2 %.3e, pred_camspc rel-L2 %.3e (bound 1e-4)' % (e1, e2))
    assert e1 <= 1e-4 and e2 <= 1e-4


def test_kernel3_checkpoint_round_trip(monkeypatch, tmp_path):
    _, pm = _pair(monkeypatch, loss='l2')
    pm.build('cuda')
    batch, nn = O.synth_batch(2, 128, 128, 64, 64, 64, 64, k=2, seed=6)
    db = to_device_batch(batch, nn)
    opt = nlt_amd.optim.AdamAMSGrad(pm, 1e-3)
    trainvali.distributed_train_step(pm, db, opt, 2)
    want = pm.call(db, 'vali')[0].clone()
    path = trainvali.save_checkpoint(str(tmp_path / 'ckpt-1.pt'), pm, opt, step=1)
    pm2 = get_model_class('nlt')(nlt_amd.make_config(depth=32, kernel=3, uvh=128, uvw=128, imh=64, imw=64, loss='l2'))
    pm2.build('cuda'); pm2.register_trainable()
    assert trainvali.restore_checkpoint(path, pm2, nlt_amd.optim.AdamAMSGrad(pm2, 1e-3)) == 1
    got = pm2.call(db, 'vali')[0]
    torch.cuda.synchronize()
    assert torch.equal(got, want)
