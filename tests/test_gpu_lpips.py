"""-m gpu: csrc/lpips.hip -- every layer-level entry point alone, nlt_lpips_loss, losses.LPIPS, metric.LPIPS and the train step --
against the float64 restatement of LPIPS v0.1 (alex, lin) in tests/lpips_ref.py with random weights.

Tolerance rule (parity-unpinned: no TensorFlow and no real weights to run), the one of tests/test_gpu_ssim.py / test_gpu_wino.py:
the HIP result must be within 4 x e32 of float64, where e32 is the float32 torch restatement's error against float64 on the same
inputs.  e32 is taken per QUANTITY (one entry point's output) as the maximum over that quantity's cases of the relative error --
for maps and gradients the max-norm error scaled by the largest entry -- so one case where float32 happened to land close sets no
impossible bar.  Every case prints e32 and the measured error.  The pool forward is a selection: it is held to equality."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import nlt_amd
from nlt_amd import capi as C
from nlt_amd import losses, metric, lpips_weights
from oracle import nlt_oracle as O
from gpu_util import make_pair, to_device_batch
import lpips_ref as R

pytestmark = pytest.mark.gpu

# tile constants of csrc/lpips.hip (test_the_tile_constants_named_here_are_the_kernel_s)
C1_TILE, C2_TILE, C1_BWD_THREADS, POOL_THREADS, HEAD_TEXELS = 8, 8, 256, 256, 64
BIG = (1, 211, 215)             # maps 52 x 53 / 25 x 26 / 12 x 12
SHAPES = [(1, 31, 31), (2, 32, 35), (2, 47, 64), BIG]
W = R.random_weights(0)
CASES = [(kind, s) for s in SHAPES for kind in R.KINDS]
IDS = ['%s-%dx%dx%d' % ((k,) + s) for k, s in CASES]


def maps_of(shape):
    n, h, w = shape
    h1, w1 = (h - 7) // 4 + 1, (w - 7) // 4 + 1
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    return (h1, w1), (h2, w2), ((h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1)


def test_the_tile_constants_named_here_are_the_kernel_s():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'neural-light-transport_amd', 'csrc',
                            'lpips.hip')).read()
    for name, v in (('kC1Tile', C1_TILE), ('kC2Tile', C2_TILE), ('kC1BwdThreads', C1_BWD_THREADS), ('kPoolThreads', POOL_THREADS),
                    ('kHeadTexels', HEAD_TEXELS)):
        m = re.search(r'constexpr int %s = (\d+)[,;]' % name, src)
        assert m and int(m.group(1)) == v, name
    (h1, w1), (h2, w2), _ = maps_of(BIG)
    # more than three tiles plus a remainder in each axis of the two tiled convs' grids ...
    for extent, tile in ((h1, C1_TILE), (w1, C1_TILE), (h2, C2_TILE), (w2, C2_TILE)):
        assert extent > 3 * tile and extent % tile, (extent, tile)
    # ... and of the one-dimensional grids: conv1's backward (pixels of one phase), the head (texels), the pools (elements; the
    # backward's count at BIG is a multiple of the block, so the remainder comes from the (2,47,64) case)
    q = ((BIG[1] + 3) // 4) * ((BIG[2] + 3) // 4)
    assert q > 3 * C1_BWD_THREADS and q % C1_BWD_THREADS
    assert h1 * w1 > 3 * HEAD_TEXELS and (h1 * w1) % HEAD_TEXELS
    assert h2 * w2 * 64 > 3 * POOL_THREADS and (h2 * w2 * 64) % POOL_THREADS
    (a1, b1), _, _ = maps_of(SHAPES[2])
    assert 2 * a1 * b1 * 64 > 3 * POOL_THREADS and (2 * a1 * b1 * 64) % POOL_THREADS


def rel(got, want):
    """Max-norm error scaled by the largest entry of `want`."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32, order='C')).cuda()         # (a dense copy: the cached references are read-only)


def both(fn):
    """fn(dtype) -> NHWC tensor, for float64 and float32, as float64 NumPy arrays."""
    return fn(torch.float64).detach().numpy(), fn(torch.float32).detach().numpy().astype(np.float64)


def hold(quantity, cases, ref, hip):
    """The rule of the module docstring for one quantity: ref(case) -> (float64, float32 restatement), hip(case) -> array."""
    refs = [ref(c) for c in cases]
    e32 = max(rel(r32, r64) for r64, r32 in refs)
    worst = 0.0
    for c, (r64, _) in zip(cases, refs):
        got = hip(c)
        assert got.shape == r64.shape and np.isfinite(got).all(), (quantity, c)
        err = rel(got, r64)
        worst = max(worst, err)
        print("lpips %s %s: e32 (max over cases) %.3e  hip %.3e" % (quantity, c, e32, err))
    assert worst <= 4 * e32, (quantity, worst, e32)


# ---------------------------------------------------------------------------------------------------- layers alone
def _rand(shape, seed, relu=False):
    a = np.random.RandomState(seed).standard_normal(shape).astype(np.float32)
    return np.maximum(a + 0.3, 0) if relu else a


def test_conv1_forward_and_backward_data_alone():
    aff, wk, b = dev(R.affine()), dev(R.keras(W, 1)), dev(W['conv1_bias'])
    imgs = {s: R.make_pair('far', *s, seed=s[1])[0] for s in SHAPES}
    hold('conv1 forward', SHAPES,
         lambda s: both(lambda dt: R.nhwc(torch.relu(R.conv_pre(1, R.scaled(imgs[s], W, dt), W, dt)))),
         lambda s: C.lpips_conv1_forward(dev(imgs[s]), aff, wk, b).cpu().numpy())
    dpre = {s: _rand((s[0],) + maps_of(s)[0] + (64,), s[2]) for s in SHAPES}
    layer = lambda dt: (lambda x: R.nhwc(R.conv_pre(1, R.scaled(x, W, dt), W, dt)))
    hold('conv1 backward-data', SHAPES,
         lambda s: both(lambda dt: R.vjp(layer(dt), imgs[s], dpre[s], dt)),
         lambda s: C.lpips_conv1_backward_data(dev(dpre[s]), s[1], s[2], aff, wk).cpu().numpy())


def test_conv2_forward_and_backward_data_alone():
    wk, b = dev(R.keras(W, 2)), dev(W['conv2_bias'])
    sizes = [(s[0],) + maps_of(s)[1] for s in SHAPES]                                    # (n, h2, w2): 3x3, 3x3, 5x7, 25x26
    x = {s: _rand(s + (64,), s[1] * 7 + s[2], relu=True) for s in sizes}
    fwd = lambda dt: (lambda t: R.nhwc(R.conv_pre(2, R.nchw(t), W, dt)))
    hold('conv2 forward', sizes, lambda s: both(lambda dt: torch.relu(fwd(dt)(R._t(x[s], dt)))),
         lambda s: C.lpips_conv2_forward(dev(x[s]), wk, b).cpu().numpy())
    dpre = {s: _rand(s + (192,), s[1] * 11 + s[2]) for s in sizes}
    hold('conv2 backward-data', sizes, lambda s: both(lambda dt: R.vjp(fwd(dt), x[s], dpre[s], dt)),
         lambda s: C.lpips_conv2_backward_data(dev(dpre[s]), wk).cpu().numpy())


def test_pool_pair_alone():
    sizes = [(s[0],) + maps_of(s)[0] + (64,) for s in SHAPES] + [(s[0],) + maps_of(s)[1] + (192,) for s in SHAPES[2:]]
    x = {s: _rand(s, s[1] * 5 + s[2]) for s in sizes}
    pool = lambda t: R.nhwc(R.pool(R.nchw(t)))
    for s in sizes:
        got = C.lpips_pool_forward(dev(x[s])).cpu()
        assert torch.equal(got, pool(torch.from_numpy(x[s])))                           # a selection: exact
    dy = {s: _rand((s[0], (s[1] - 3) // 2 + 1, (s[2] - 3) // 2 + 1, s[3]), s[1] + s[2]) for s in sizes}
    hold('pool backward', sizes, lambda s: both(lambda dt: R.vjp(pool, x[s], dy[s], dt)),
         lambda s: C.lpips_pool_backward(dev(dy[s]), dev(x[s])).cpu().numpy())


def test_pool_backward_sends_a_tie_to_the_first_maximum_in_window_order():
    x = np.zeros((1, 5, 5, 64), np.float32)
    x[0, 1, 1] = x[0, 1, 2] = x[0, 2, 1] = 1.0              # window (0,0): first maximum at (1,1); window (0,1) [cols 2..4]: (1,2)
    dy = np.arange(1, 5, dtype=np.float32).reshape(1, 2, 2, 1).repeat(64, 3)
    got = C.lpips_pool_backward(dev(dy), dev(x)).cpu().numpy()
    want = np.zeros_like(x)
    want[0, 1, 1] = 1.0                                      # window (0,0)
    want[0, 1, 2] = 2.0                                      # window (0,1)
    want[0, 2, 1] = 3.0                                      # window (1,0) [rows 2..4]: its first maximum is (2,1)
    want[0, 2, 2] = 4.0                                      # window (1,1): all zero, the first element (2,2)
    assert np.array_equal(got, want)


def test_head_pair_alone():
    sizes = [(1, 7, 7, 64), (2, 3, 3, 192), (2, 2, 3, 384), (1, 1, 1, 256), (1, 52, 53, 64), (1, 25, 26, 192), (1, 12, 12, 384)]
    fp = {s: _rand(s, s[1] + s[3], relu=True) for s in sizes}
    fg = {s: _rand(s, s[2] + s[3] + 1, relu=True) for s in sizes}
    lin = {s: (np.random.RandomState(s[3]).uniform(0, 1, s[3]) / s[3]).astype(np.float32) for s in sizes}
    for s in sizes:
        assert (fp[s].sum(-1) > 0).all() and (fg[s].sum(-1) > 0).all()
    head = lambda s, dt: (lambda p: R.head(R.nchw(p), R.nchw(R._t(fg[s], dt)), lin[s], dt))
    hold('head forward', sizes, lambda s: both(lambda dt: head(s, dt)(R._t(fp[s], dt))),
         lambda s: C.lpips_head_forward(dev(fp[s]), dev(fg[s]), dev(lin[s])).cpu().numpy())
    ones = {s: np.ones(s[0], np.float32) for s in sizes}
    mask = lambda s, g: g * torch.as_tensor(fp[s] > 0, dtype=g.dtype)
    hold('head adjoint', sizes, lambda s: both(lambda dt: mask(s, R.vjp(head(s, dt), fp[s], ones[s], dt))),
         lambda s: C.lpips_head_backward(dev(fp[s]), dev(fg[s]), dev(lin[s])).cpu().numpy())
    dup = {s: _rand(s, 5) * 1e-3 for s in sizes}
    hold('head adjoint + upstream', sizes,
         lambda s: both(lambda dt: mask(s, R.vjp(head(s, dt), fp[s], ones[s], dt) + R._t(dup[s], dt))),
         lambda s: C.lpips_head_backward(dev(fp[s]), dev(fg[s]), dev(lin[s]), dev(dup[s])).cpu().numpy())


# ---------------------------------------------------------------------------------------------------- the whole loss
@functools.lru_cache(maxsize=None)
def blob():
    return torch.from_numpy(lpips_weights.blob(lpips_weights.validate(W))).cuda()


@functools.lru_cache(maxsize=None)
def reference(kind, shape):
    """(gt, pred, l64, g64, l32, g32) -- after lpips_ref.checked's assertions; computed once, read only."""
    n, h, w = shape
    gt, pred = R.make_pair(kind, n, h, w, seed=h * 100 + w)
    out = (gt, pred) + R.checked(gt, pred, W)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def hip(kind, shape):
    gt, pred = reference(kind, shape)[:2]
    g, p = dev(gt), dev(pred)
    loss, dunit = C.lpips_loss(p, g, blob(), True)
    only, none = C.lpips_loss(p, g, blob(), False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(only, loss)         # the value does not depend on whether a gradient is wanted
    return loss.cpu().numpy().astype(np.float64), dunit.cpu().numpy().astype(np.float64)


def test_loss_values():
    e32 = max(float((np.abs(reference(*c)[4] - reference(*c)[2]) / np.abs(reference(*c)[2])).max()) for c in CASES)
    worst = 0.0
    for kind, shape in CASES:
        l64 = reference(kind, shape)[2]
        got, _ = hip(kind, shape)
        err = float((np.abs(got - l64) / np.abs(l64)).max())
        worst = max(worst, err)
        print("lpips loss %s %s: loss %s  e32 (max over cases) %.3e  hip %.3e" % (kind, shape, l64, e32, err))
        assert got.shape == (shape[0],)
        if shape[0] > 1:
            assert len(set(np.round(l64, 9))) == shape[0]    # different images: a per-example mix-up would show
    assert worst <= 4 * e32, (worst, e32)


def test_unit_gradient():
    per = lambda a, b: max(rel(a[f], b[f]) for f in range(b.shape[0]))
    e32 = max(per(reference(*c)[5], reference(*c)[3]) for c in CASES)
    worst = 0.0
    for kind, shape in CASES:
        g64 = reference(kind, shape)[3]
        _, got = hip(kind, shape)
        assert got.shape == g64.shape and np.isfinite(got).all()
        err = per(got, g64)
        worst = max(worst, err)
        print("lpips grad %s %s: e32 (max over cases) %.3e  hip %.3e" % (kind, shape, e32, err))
    assert worst <= 4 * e32, (worst, e32)


def test_identical_images_give_exactly_zero_loss_and_gradient():
    x = dev(R.make_pair('far', 2, 47, 64, seed=9)[0])
    loss, dunit = C.lpips_loss(x, x.clone(), blob(), True)
    assert (loss == 0).all() and (dunit == 0).all()


@pytest.mark.parametrize('det', [False, True])
def test_two_calls_are_bit_identical(det):
    gt, pred = (dev(a) for a in R.make_pair('far', 2, 47, 64, seed=5))
    with C.deterministic_scope(det):
        l0, d0 = C.lpips_loss(pred, gt, blob(), True)
        l1, d1 = C.lpips_loss(pred, gt, blob(), True)
    assert torch.equal(l0, l1) and torch.equal(d0, d1)
    plain = C.lpips_loss(pred, gt, blob(), True)
    assert torch.equal(plain[0], l0) and torch.equal(plain[1], d0)                      # one form: the mode switches nothing


def test_refusals():
    z = lambda *s: torch.zeros(s, device='cuda')
    with pytest.raises(C.NLTError):
        C.lpips_loss(z(1, 30, 40, 3), z(1, 30, 40, 3), blob(), True)
    with pytest.raises(C.NLTError):
        C.lpips_loss(z(1, 40, 30, 3), z(1, 40, 30, 3), blob(), False)
    with pytest.raises(C.NLTError):
        C.lpips_loss(z(1, 40, 40, 1), z(1, 40, 40, 1), blob(), False)
    with pytest.raises(C.NLTError):
        C.lpips_loss(z(1, 40, 40, 3), z(1, 40, 40, 3), blob()[:-4], False)


# ---------------------------------------------------------------------------------------------------- losses.LPIPS
def test_losses_lpips_keep_batch_mean_weights_and_gradient_through_the_blend():
    n, h, w = 2, 33, 40
    x, y = R.make_pair('near', n, h, w, seed=7)
    gt, pred = dev(x), dev(y)
    f = losses.LPIPS(W)
    per = f(gt, pred, keep_batch=True)
    want, _ = C.lpips_loss(pred, gt, blob(), False)
    assert per.shape == (n,) and torch.equal(per, want)
    mean = f(gt, pred)
    assert mean.dim() == 0 and float(mean) == float(per.mean())
    wt = np.random.RandomState(2).uniform(0.5, 1, (n, h, w, 1)).astype(np.float32)
    a = np.broadcast_to(wt, x.shape)
    xb, yb = (x * a).astype(np.float32), (y * a).astype(np.float32)                      # alpha-blend against zeros, in float32 like _MulFn
    l64, g64, l32, g32 = R.checked(xb, yb, W)
    p = pred.clone().requires_grad_(True)
    got = f(gt, p, keep_batch=True, weights=dev(wt))
    e32, err = np.abs(l32 - l64) / l64, np.abs(got.detach().cpu().numpy() - l64) / l64
    got.sum().backward()
    ge32, gerr = rel(g32 * a, g64 * a), rel(p.grad.cpu().numpy(), g64 * a)               # d / d pred = alpha * d / d(blended pred)
    print("losses.LPIPS blend: loss e32 %s hip %s; grad e32 %.3e hip %.3e" % (e32, err, ge32, gerr))
    # (single case: the per-quantity e32 of test_loss_values / test_unit_gradient is not at hand, so this case's own)
    assert (err <= 4 * e32.max()).all() and gerr <= 4 * ge32
    p = pred.clone().requires_grad_(True)                     # the upstream per-example gradient scales the rows
    up = torch.tensor([0.5, -2.0], device='cuda')
    (f(gt, p, keep_batch=True) * up).sum().backward()
    _, dunit = C.lpips_loss(pred, gt, blob(), True)
    assert torch.equal(p.grad, dunit * up[:, None, None, None])


# ---------------------------------------------------------------------------------------------------- metric.LPIPS
@pytest.mark.parametrize('dtype', ['float32', 'uint8'])
def test_metric_lpips_single_image_and_batch(dtype):
    m = metric.LPIPS(np.float32 if dtype == 'float32' else 'uint8', W)
    n, h, w = 2, 35, 44
    x, y = R.make_pair('far', n, h, w, seed=11)
    if dtype == 'uint8':
        x, y = np.round(x * 255).astype(np.uint8), np.round(y * 255).astype(np.uint8)
    l64 = R.distance(x.astype(np.float64) / m.drange, y.astype(np.float64) / m.drange, W, torch.float64).numpy()
    host = m(x[0], y[0])
    assert isinstance(host, float) and host == m(torch.from_numpy(x[0]).cuda(), torch.from_numpy(y[0]).cuda())
    # bound: the train-step test's 1e-5 relative.  The metric divides by drange in float32 before the chain, which the float32
    # restatement of test_loss_values does not do, so that test's e32 is not this quantity's; the chain's own float32 error
    # (< 1e-6 relative there) plus one rounding of each input (6e-8 relative) stays two orders below the bound
    assert abs(host - l64[0]) <= 1e-5 * l64[0]
    got = m.batch(x, y)
    assert got == [m(x[f], y[f]) for f in range(n)] and len(set(got)) == n               # bit for bit, and no example mixed up
    one = m(x[0][..., :1], y[0][..., :1])                                                # one channel is tripled
    assert one == m(x[0][..., 0], y[0][..., 0]) == m(np.repeat(x[0][..., :1], 3, 2), np.repeat(y[0][..., :1], 3, 2))


# ---------------------------------------------------------------------------------------------------- the train step
UV, CAM, N_EX, K = 64, 32, 2, 1          # the smallest model shape of tests/test_gpu_train_step.py


@pytest.fixture(scope='module')
def weights_file(tmp_path_factory):
    p = str(tmp_path_factory.mktemp('lpips') / 'weights.npz')
    np.savez(p, **W)
    return p


def _model(loss, seed=6, **kw):
    _, pm = make_pair(depth=256, uv=UV, im=CAM, loss=loss, seed=seed, **kw)
    pm.build('cuda')
    return pm


def _batch():
    return to_device_batch(*O.synth_batch(N_EX, UV, UV, CAM, CAM, CAM, CAM, k=K, seed=51))


def test_train_step_with_an_lpips_term(weights_file):
    db = _batch()
    pm = _model('l2,0.5lpips', lpips_weights=weights_file)
    assert [(w, type(f).__name__) for w, f in pm.wloss] == [(1.0, 'L2'), (0.5, 'LPIPS')]
    loss, vis = pm.train_forward_backward(db, N_EX)
    torch.cuda.synchronize()
    bucket = pm.flat_grads.clone()
    pred, gt = vis['pred_camspc'].cpu().numpy(), vis['gt_camspc'].cpu().numpy()
    l2 = ((pred.astype(np.float64) - gt) ** 2).mean(axis=(1, 2, 3))
    lp = R.distance(gt, pred, W, torch.float64).numpy()
    want = float((l2 + 0.5 * lp).sum() / N_EX)
    print("train step loss %.9f  want %.9f  rel %.2e" % (float(loss), want, abs(float(loss) - want) / abs(want)))
    assert abs(float(loss) - want) <= 1e-5 * abs(want)
    assert torch.isfinite(bucket).all() and float(bucket.abs().max()) > 0
    pl = _model('l2')
    pl.train_forward_backward(db, N_EX)
    torch.cuda.synchronize()
    assert pl.flat_grads.shape == bucket.shape
    assert float((pl.flat_grads - bucket).norm()) > 1e-3 * float(pl.flat_grads.norm())   # the lpips term's gradient arrived


def test_deterministic_train_step_with_an_lpips_term_repeats_bit_for_bit(weights_file):
    db = _batch()
    runs = []
    for _ in range(2):
        pm = _model('l2,0.5lpips', deterministic=True, lpips_weights=weights_file)
        assert pm.deterministic
        loss, _ = pm.train_forward_backward(db, N_EX)
        torch.cuda.synchronize()
        runs.append((loss.clone(), pm.flat_grads.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.isfinite(runs[0][1]).all() and float(runs[0][1].abs().max()) > 0
