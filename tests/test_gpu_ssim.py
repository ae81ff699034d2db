"""-m gpu: csrc/ssim.hip (nlt_ssim_loss, nlt_ssim_values) through _capi, losses.SSIM, metric.SSIM and the train step against
the float64 restatement of tf.image.ssim in tests/ssim_ref.py.

Tolerance rule (parity-unpinned: no TensorFlow to run): for each case e32 = |float32 restatement - float64 restatement| on the
same float32 inputs ("TF's own arithmetic"), and the HIP result must be within 4 * e32 + 1e-7 of float64 -- 4x is the margin
tests/test_gpu_wino.py gives a reformulated kernel over the plain one, 1e-7 covers an e32 that happens to be ~0.  Gradients: the
same rule on the max-norm error of the unit gradient scaled by its largest entry, e32 from the float32 torch restatement's
autograd."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import nlt_amd
from nlt_amd import capi as C
from nlt_amd import losses, metric
from oracle import nlt_oracle as O
from gpu_util import make_pair, to_device_batch
import ssim_ref as R

pytestmark = pytest.mark.gpu

# the tile a workgroup owns (kTileH x kTileW of csrc/ssim.hip): output positions in the forward, image pixels in the adjoint
TILE_H, TILE_W = 16, 32
# three tiles plus a remainder in each axis of the valid grid (and of the image: 63 = 3 * 16 + 15, 113 = 3 * 32 + 17)
BIG = (1, 10 + 3 * TILE_H + 5, 10 + 3 * TILE_W + 7)
SHAPES = [(1, 11, 11), (1, 11, 29), (1, 29, 11), (2, 12, 12), (3, 37, 53), BIG]
CASES = [(kind, s, c) for s in SHAPES for c in (3, 1) for kind in R.KINDS]
IDS = ['%s-%dx%dx%dx%d' % (k, s[0], s[1], s[2], c) for k, s, c in CASES]


def test_the_tile_constants_named_here_are_the_kernel_s():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'neural-light-transport_amd', 'csrc',
                            'ssim.hip')).read()
    m = re.search(r'constexpr int kTileW = (\d+), kTileH = (\d+);', src)
    assert m and (int(m.group(2)), int(m.group(1))) == (TILE_H, TILE_W)
    assert BIG[1] - 10 > 3 * TILE_H and (BIG[1] - 10) % TILE_H and BIG[2] - 10 > 3 * TILE_W and (BIG[2] - 10) % TILE_W


@functools.lru_cache(maxsize=None)
def reference(kind, shape, c):
    """(x = gt, y = pred, float64 loss / unit gradient, float32 restatement's loss / unit gradient); computed once, read only."""
    n, h, w = shape
    x, y = R.make_pair(kind, n, h, w, c, seed=h * 100 + w)
    l64, g64 = R.loss_and_unit_grad(x, y, 1.0, torch.float64)
    _, g32 = R.loss_and_unit_grad(x, y, 1.0, torch.float32)
    l32 = (np.float32(1) - R.ssim_np(x, y, 1.0, np.float32)) / np.float32(2)
    for a in (x, y, l64, g64, l32, g32):
        a.setflags(write=False)
    return x, y, l64, g64, l32, g32


@functools.lru_cache(maxsize=None)
def hip(kind, shape, c):
    x, y = reference(kind, shape, c)[:2]
    gt, pred = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    loss, dunit = C.ssim_loss(pred, gt, 1.0, True)
    only, none = C.ssim_loss(pred, gt, 1.0, False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(only, loss)     # the value does not depend on whether a gradient is wanted
    return loss.cpu().numpy().astype(np.float64), dunit.cpu().numpy().astype(np.float64)


def grad_error(got, want):
    """Per example: max-norm error scaled by the largest entry of `want`."""
    n = want.shape[0]
    return np.array([np.abs(got[f] - want[f]).max() / np.abs(want[f]).max() for f in range(n)])


@pytest.mark.parametrize('kind,shape,c', CASES, ids=IDS)
def test_loss_values(kind, shape, c):
    x, y, l64, g64, l32, g32 = reference(kind, shape, c)
    got, _ = hip(kind, shape, c)
    e32 = np.abs(l32.astype(np.float64) - l64)
    err = np.abs(got - l64)
    print("ssim loss %s %s c=%d: loss %s  e32 %s  hip %s" % (kind, shape, c, l64, e32, err))
    assert got.shape == (shape[0],)
    assert (err <= 4 * e32 + 1e-7).all(), (err, e32)
    if shape[0] > 1:
        assert len(set(np.round(l64, 9))) == shape[0]    # different images: a per-example mix-up would show


@pytest.mark.parametrize('kind,shape,c', CASES, ids=IDS)
def test_unit_gradient(kind, shape, c):
    x, y, l64, g64, l32, g32 = reference(kind, shape, c)
    _, got = hip(kind, shape, c)
    n, h, w = shape
    assert got.shape == (n, h, w, c) and np.isfinite(got).all()
    e32 = grad_error(g32.astype(np.float64), g64)
    err = grad_error(got, g64)
    print("ssim grad %s %s c=%d: e32 %s  hip %s" % (kind, shape, c, e32, err))
    assert (err <= 4 * e32 + 1e-7).all(), (err, e32)
    for f in range(n):
        big = np.abs(g64[f]).max()
        tol = (4 * e32[f] + 1e-7) * big
        # corner pixels: exactly one window reaches them; pixels 10 in from every edge: the full 11 x 11 footprint
        spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
        if h >= 21 and w >= 21:
            spots += [(10, 10), (h - 11, w - 11), (10, w - 11)]
        for (i, j) in spots:
            assert (np.abs(got[f, i, j] - g64[f, i, j]) <= tol).all(), (f, i, j)
            assert np.abs(g64[f, i, j]).max() > 0


def test_identical_images_give_exactly_one_and_zero_loss():
    x, _ = R.make_pair('near', 2, 37, 53, 3)
    t = torch.from_numpy(x).cuda()
    loss, _ = C.ssim_loss(t, t, 1.0, False)
    assert (loss == 0).all()
    assert C.ssim_values(t, t, 1.0).tolist() == [1.0, 1.0]


# ---------------------------------------------------------------------------------------------------- losses.SSIM
def test_losses_ssim_keep_batch_mean_weights_and_gradient_through_the_blend():
    n, h, w = 3, 23, 40
    x, y = R.make_pair('near', n, h, w, 3, seed=7)
    gt, pred = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    f = losses.SSIM(1 - 0)
    per = f(gt, pred, keep_batch=True)
    assert per.shape == (n,)
    l64 = R.loss_torch(torch.from_numpy(x), torch.from_numpy(y), 1.0).numpy()
    l32 = ((np.float32(1) - R.ssim_np(x, y, 1.0, np.float32)) / np.float32(2)).astype(np.float64)
    assert (np.abs(per.cpu().numpy() - l64) <= 4 * np.abs(l32 - l64) + 1e-7).all()
    mean = f(gt, pred)
    assert mean.dim() == 0 and float(mean) == float(per.mean())
    rng = np.random.RandomState(2)
    for wt in (rng.uniform(0.2, 1, (n, h, w, 1)).astype(np.float32), np.float32(0.7)):
        a = np.broadcast_to(wt, x.shape)
        xb, yb = (x * a).astype(np.float32), (y * a).astype(np.float32)      # alpha-blend against zeros, in float32 like _MulFn
        l64, g64 = R.loss_and_unit_grad(xb, yb, 1.0, torch.float64)
        _, g32 = R.loss_and_unit_grad(xb, yb, 1.0, torch.float32)
        l32 = ((np.float32(1) - R.ssim_np(xb, yb, 1.0, np.float32)) / np.float32(2)).astype(np.float64)
        p = pred.clone().requires_grad_(True)
        wt_dev = torch.from_numpy(wt).cuda() if wt.ndim else float(wt)
        got = f(gt, p, keep_batch=True, weights=wt_dev)
        assert (np.abs(got.detach().cpu().numpy() - l64) <= 4 * np.abs(l32 - l64) + 1e-7).all()
        got.sum().backward()
        # d/d pred = alpha * d/d(blended pred)
        want, want32 = g64 * a, g32.astype(np.float64) * a
        e32 = grad_error(want32, want)
        err = grad_error(p.grad.cpu().numpy().astype(np.float64), want)
        assert (err <= 4 * e32 + 1e-7).all(), (err, e32)
    # the upstream per-example gradient scales the rows (nlt_scale_rows)
    p = pred.clone().requires_grad_(True)
    up = torch.tensor([0.5, -2.0, 3.0], device='cuda')
    (f(gt, p, keep_batch=True) * up).sum().backward()
    _, dunit = C.ssim_loss(pred, gt, 1.0, True)
    assert torch.equal(p.grad, dunit * up[:, None, None, None])


# ---------------------------------------------------------------------------------------------------- metric.SSIM
@pytest.mark.parametrize('dtype', ['float32', 'uint8'])
def test_metric_ssim_inputs_and_batch(dtype):
    m = metric.SSIM(np.float32 if dtype == 'float32' else 'uint8')
    assert m.drange == (1.0 if dtype == 'float32' else 255.0)
    n, h, w = 3, 30, 45
    for kind in R.KINDS:
        x, y = R.make_pair(kind, n, h, w, 3, seed=11, max_val=m.drange)
        if dtype == 'uint8':
            x, y = np.clip(np.round(x), 0, 255).astype(np.uint8), np.clip(np.round(y), 0, 255).astype(np.uint8)
        else:
            x, y = np.clip(x, 0, 1), np.clip(y, 0, 1)
        per_image = []
        for views in (lambda a: a, lambda a: a[..., :1], lambda a: a[..., 0]):          # [H,W,3], [H,W,1], [H,W]
            a, b = views(x[0]), views(y[0])
            want = R.metric_ssim_np(a, b, m.drange, np.float64)
            e32 = abs(R.metric_ssim_np(a, b, m.drange, np.float32) - want)
            host = m(np.ascontiguousarray(a), np.ascontiguousarray(b))
            dev = m(torch.from_numpy(np.ascontiguousarray(a)).cuda(), torch.from_numpy(np.ascontiguousarray(b)).cuda())
            print("metric.SSIM %s %s %s: %.9f  e32 %.2e  hip %.2e" % (dtype, kind, a.shape, want, e32, abs(host - want)))
            assert isinstance(host, float) and host == dev
            assert abs(host - want) <= 4 * e32 + 1e-7, (kind, a.shape, host, want, e32)
        assert m(x[0][..., :1], y[0][..., :1]) == m(x[0][..., 0], y[0][..., 0])
        for c in (3, 1):
            per_image = [m(x[f][..., :c], y[f][..., :c]) for f in range(n)]
            got = m.batch(x[..., :c], y[..., :c])
            assert got == per_image and len(set(got)) == n                              # bit for bit, and no example mixed up


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    z = lambda *s: torch.zeros(s, device='cuda')
    with pytest.raises(C.NLTError):
        C.ssim_loss(z(1, 10, 16, 3), z(1, 10, 16, 3), 1.0, True)
    with pytest.raises(C.NLTError):
        C.ssim_loss(z(1, 16, 10, 3), z(1, 16, 10, 3), 1.0, False)
    with pytest.raises(C.NLTError):
        C.ssim_loss(z(1, 16, 16, 4), z(1, 16, 16, 4), 1.0, True)
    with pytest.raises(C.NLTError):
        C.ssim_values(z(1, 10, 16, 1), z(1, 10, 16, 1), 1.0)
    m = metric.SSIM(np.float32)
    with pytest.raises(C.NLTError):
        m(z(10, 16), z(10, 16))
    with pytest.raises(NotImplementedError):
        m(z(16, 16, 4), z(16, 16, 4))
    with pytest.raises(AssertionError):
        m(z(16, 16, 3), z(16, 17, 3))
    with pytest.raises(AssertionError):
        metric.PSNR(np.float32)(z(16, 16, 3), z(16, 17, 3))                             # like PSNR
    # a short workspace is refused on the host, before any launch
    ws = z(8)
    need = C.lib().nlt_ssim_workspace_floats(1, 16, 16, 3, 1)
    assert need == 2 + 3 * 3 * 36
    a, out = z(1, 16, 16, 3), z(1)
    s = torch.cuda.current_stream().cuda_stream
    assert C.lib().nlt_ssim_loss(a.data_ptr(), a.data_ptr(), 1, 16, 16, 3, 1.0, ws.data_ptr(), need - 1, out.data_ptr(),
                                 a.clone().data_ptr(), s) == -1


# ---------------------------------------------------------------------------------------------------- repeatability
@pytest.mark.parametrize('det', [False, True])
def test_two_calls_are_bit_identical(det):
    x, y = R.make_pair('noise', 3, 70, 121, 3, seed=5)
    gt, pred = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    with C.deterministic_scope(det):
        l0, d0 = C.ssim_loss(pred, gt, 1.0, True)
        l1, d1 = C.ssim_loss(pred, gt, 1.0, True)
        v0, v1 = C.ssim_values(pred, gt, 1.0), C.ssim_values(pred, gt, 1.0)
    assert torch.equal(l0, l1) and torch.equal(d0, d1) and torch.equal(v0, v1)
    plain = C.ssim_loss(pred, gt, 1.0, True)
    assert torch.equal(plain[0], l0) and torch.equal(plain[1], d0)                      # one form: the mode switches nothing


# ---------------------------------------------------------------------------------------------------- the train step
UV, CAM, N_EX, K = 64, 32, 2, 1          # the smallest model shape of tests/test_gpu_train_step.py


def _model(loss, seed=6, **kw):
    _, pm = make_pair(depth=256, uv=UV, im=CAM, loss=loss, seed=seed, **kw)
    pm.build('cuda')
    return pm


def _batch():
    return to_device_batch(*O.synth_batch(N_EX, UV, UV, CAM, CAM, CAM, CAM, k=K, seed=51))


def test_train_step_with_an_ssim_term():
    db = _batch()
    pm = _model('l2,0.5ssim')
    assert [(w, type(f).__name__) for w, f in pm.wloss] == [(1.0, 'L2'), (0.5, 'SSIM')]
    loss, vis = pm.train_forward_backward(db, N_EX)
    torch.cuda.synchronize()
    bucket = pm.flat_grads.clone()
    pred, gt = vis['pred_camspc'].cpu().numpy(), vis['gt_camspc'].cpu().numpy()
    l2 = ((pred.astype(np.float64) - gt) ** 2).mean(axis=(1, 2, 3))
    ssim = R.loss_torch(torch.from_numpy(gt), torch.from_numpy(pred), 1.0).numpy()
    want = float((l2 + 0.5 * ssim).sum() / N_EX)
    print("train step loss %.9f  want %.9f  rel %.2e" % (float(loss), want, abs(float(loss) - want) / abs(want)))
    assert abs(float(loss) - want) <= 1e-5 * abs(want)
    assert torch.isfinite(bucket).all() and float(bucket.abs().max()) > 0
    pl = _model('l2')
    pl.train_forward_backward(db, N_EX)
    torch.cuda.synchronize()
    assert pl.flat_grads.shape == bucket.shape and not torch.equal(pl.flat_grads, bucket)
    assert float((pl.flat_grads - bucket).norm()) > 1e-3 * float(pl.flat_grads.norm())   # the ssim term's gradient arrived


def test_deterministic_train_step_with_an_ssim_term_repeats_bit_for_bit():
    db = _batch()
    runs = []
    for _ in range(2):
        pm = _model('l2,0.5ssim', deterministic=True)
        assert pm.deterministic
        loss, _ = pm.train_forward_backward(db, N_EX)
        torch.cuda.synchronize()
        runs.append((loss.clone(), pm.flat_grads.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.isfinite(runs[0][1]).all() and float(runs[0][1].abs().max()) > 0
