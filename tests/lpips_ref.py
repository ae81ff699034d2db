"""LPIPS v0.1 "alex / lin" restated from its published definition, in torch on the CPU (TEST-ONLY helper, not a test module).

Per image in [0, 1], NHWC: t = ((2x - 1) - shift) / scale; ReLU feature maps f1 = conv 11x11 s4 p2 (3 -> 64), f2 = conv 5x5 p2
(64 -> 192) of maxpool3x3s2(f1), f3 = conv 3x3 p1 (192 -> 384) of maxpool3x3s2(f2), f4 = conv 3x3 p1 (384 -> 256), f5 = conv 3x3 p1
(256 -> 256); n = f / (sqrt(sum_c f^2) + 1e-10); d_l = spatial mean of sum_c lin_l[c] (n_pred - n_gt)^2; the value is the sum of
the five d_l.  dtype picks float64 (the yardstick) or float32 ("the arithmetic a float32 framework would run").

Weights are random (`random_weights`): no real weights file is on hand, and parity with one is unpinned.  With autograd an
all-zero texel gives NaN, and a ReLU / max-pool kink that flips between float32 and float64 would pass as "rounding", so `checked`
asserts that the inputs it is given have neither."""
import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
CH = (3, 64, 192, 384, 256, 256)
KS = (11, 5, 3, 3, 3)
STRIDE = (4, 1, 1, 1, 1)
PAD = (2, 2, 1, 1, 1)
EPS = 1e-10
KINDS = ('near', 'far')


def random_weights(seed=0):
    """Published PyTorch layout: conv{l}_weight (O,I,kh,kw) He-uniform, conv{l}_bias U(0.02, 0.12) (so no texel's features are all
    zero), lin{l} (C,) = U(0,1) / C; float32."""
    rng = np.random.RandomState(seed)
    w = {}
    for l in range(1, 6):
        o, i, k = CH[l], CH[l - 1], KS[l - 1]
        b = np.sqrt(6.0 / (i * k * k))
        w['conv%d_weight' % l] = rng.uniform(-b, b, (o, i, k, k)).astype(np.float32)
        w['conv%d_bias' % l] = rng.uniform(0.02, 0.12, o).astype(np.float32)
        w['lin%d' % l] = (rng.uniform(0, 1, o) / o).astype(np.float32)
    return w


def keras(w, l):
    """conv l's kernel as the Keras array (kh,kw,I,O) the HIP entry points read."""
    return np.ascontiguousarray(np.transpose(w['conv%d_weight' % l], (2, 3, 1, 0)))


def affine(w=None):
    w = w or {}
    return np.concatenate([np.asarray(w.get('shift', SHIFT), np.float32), np.asarray(w.get('scale', SCALE), np.float32)])


def make_pair(kind, n, h, w, seed=0):
    """(gt, pred) float32 [n,h,w,3] in [0,1]: smooth ramps plus noise; 'near' = gt plus a little noise, 'far' = independent."""
    rng = np.random.RandomState(seed)

    def image():
        yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing='ij')
        base = np.stack([(np.sin(rng.uniform(2, 9) * yy + rng.uniform(0, 6)) * np.cos(rng.uniform(2, 9) * xx + rng.uniform(0, 6)))
                         for _ in range(3 * n)]).reshape(n, 3, h, w).transpose(0, 2, 3, 1)
        return np.clip(0.5 + 0.3 * base + rng.uniform(-0.2, 0.2, (n, h, w, 3)), 0, 1)
    gt = image()
    pred = np.clip(gt + rng.uniform(-0.05, 0.05, gt.shape), 0, 1) if kind == 'near' else image()
    return gt.astype(np.float32), pred.astype(np.float32)


def _t(a, dtype):
    return a.to(dtype) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a), dtype=dtype)


def nchw(x):
    return x.permute(0, 3, 1, 2)


def nhwc(x):
    return x.permute(0, 2, 3, 1)


def scaled(x, w, dtype):
    """x NHWC in [0,1] -> NCHW ((2x - 1) - shift) / scale."""
    a = affine(w)
    shift, scale = _t(a[:3], dtype).view(1, 3, 1, 1), _t(a[3:], dtype).view(1, 3, 1, 1)
    return (nchw(_t(x, dtype)) * 2 - 1 - shift) / scale


def conv_pre(l, x_nchw, w, dtype):
    """Pre-activation of conv l (1..5) on an NCHW input."""
    return F.conv2d(x_nchw, _t(w['conv%d_weight' % l], dtype), _t(w['conv%d_bias' % l], dtype), stride=STRIDE[l - 1], padding=PAD[l - 1])


def pool(x_nchw, indices=False):
    return F.max_pool2d(x_nchw, 3, 2, return_indices=indices)


def features(x, w, dtype, kinks=None):
    """The five ReLU maps (NCHW) of NHWC images in [0,1]; kinks (a list) collects every ReLU mask and pool argmax."""
    out, cur = [], scaled(x, w, dtype)
    for l in range(1, 6):
        if l in (2, 3):
            cur, idx = pool(cur, True)
            if kinks is not None:
                kinks.append(idx.detach().clone())
        pre = conv_pre(l, cur, w, dtype)
        if kinks is not None:
            kinks.append((pre > 0).detach().clone())
        cur = torch.relu(pre)
        out.append(cur)
    return out


def head(fp, fg, lin, dtype=None):
    """One level on NCHW maps: d [N] = spatial mean of sum_c lin[c] (fp / (|fp| + eps) - fg / (|fg| + eps))^2."""
    dtype = dtype or fp.dtype
    n_p = fp / (fp.pow(2).sum(1, keepdim=True).sqrt() + EPS)
    n_g = fg / (fg.pow(2).sum(1, keepdim=True).sqrt() + EPS)
    return ((n_p - n_g).pow(2) * _t(lin, dtype).view(1, -1, 1, 1)).sum(1).mean((1, 2))


def distance(gt, pred, w, dtype, kinks=None, check_zero=False):
    """LPIPS per example [N] (a tensor of `dtype`); pred may be a tensor that requires grad."""
    fp, fg = features(pred, w, dtype, kinks), features(gt, w, dtype, kinks)
    if check_zero:
        for l, (a, b) in enumerate(zip(fp, fg)):
            assert bool((a.detach().sum(1) > 0).all()) and bool((b.detach().sum(1) > 0).all()), "an all-zero texel at level %d" % (l + 1)
    total = 0
    for l in range(5):
        total = total + head(fp[l], fg[l], w['lin%d' % (l + 1)], dtype)
    return total


def loss_and_unit_grad(gt, pred, w, dtype=torch.float64, kinks=None, check_zero=False):
    """(loss [N], d loss[f] / d pred [N,H,W,3]) as NumPy arrays of `dtype`."""
    p = _t(pred, dtype).clone().requires_grad_(True)
    d = distance(_t(gt, dtype), p, w, dtype, kinks, check_zero)
    d.sum().backward()
    return d.detach().numpy(), p.grad.numpy()


def checked(gt, pred, w):
    """(l64, g64, l32, g32) after asserting: no all-zero texel at any level, finite float64 gradients, and float32 / float64
    agreeing on every ReLU mask and pool argmax (so no kink is mistaken for rounding)."""
    k64, k32 = [], []
    l64, g64 = loss_and_unit_grad(gt, pred, w, torch.float64, k64, True)
    l32, g32 = loss_and_unit_grad(gt, pred, w, torch.float32, k32, True)
    assert np.isfinite(g64).all() and np.isfinite(l64).all()
    assert len(k64) == len(k32) == 14
    for a, b in zip(k64, k32):
        assert torch.equal(a, b), "a ReLU mask or pool argmax differs between float32 and float64"
    return l64, g64, l32.astype(np.float64), g32.astype(np.float64)


def vjp(fn, x, dy, dtype):
    """d (fn(x) . dy) / d x for a layer `fn` on tensors of `dtype`."""
    xx = _t(x, dtype).clone().requires_grad_(True)
    (fn(xx) * _t(dy, dtype)).sum().backward()
    return xx.grad
