"""Test-side restatement of tf.image.ssim(img1, img2, max_val) of TF 2.2 (filter_size 11, filter_sigma 1.5, k1 0.01, k2 0.03),
written from the formulas alone:

    g[i]  = softmax_i(-(i - 5)^2 * 0.5 / 1.5^2), i = 0..10; the 2-D window is outer(g, g)
    F(.)  = per-channel 'VALID' correlation with that window -> (H - 10) x (W - 10)
    m0 = F(x), m1 = F(y), num0 = 2 m0 m1, den0 = m0^2 + m1^2, lum = (num0 + c1) / (den0 + c1)
    num1 = 2 F(x y), den1 = F(x^2 + y^2), cs = (num1 - num0 + c2) / (den1 - den0 + c2)
    ssim = mean over channels of the mean over positions of lum * cs          (one value per image)

`ssim_np(x, y, max_val, dtype)` runs every step in `dtype`: float64 is the truth, float32 is "TF's own arithmetic" (TF casts its
inputs to float32).  `ssim_torch` is the same thing on torch CPU tensors through F.conv2d, so autograd supplies gradients."""
import numpy as np
import torch
import torch.nn.functional as F

FILTER_SIZE, FILTER_SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03
LUMA = (0.2126, 0.7152, 0.0722)


def window(dtype=np.float64):
    dtype = np.dtype(dtype).type
    i = np.arange(FILTER_SIZE, dtype=dtype) - dtype((FILTER_SIZE - 1) / 2)
    e = -(i * i) * dtype(0.5 / FILTER_SIGMA ** 2)
    e = np.exp(e - e.max())
    return (e / e.sum()).astype(dtype)


def filter_valid(a, g):
    """[..., H, W, C] -> [..., H-10, W-10, C]: rows first, then columns, taps added in ascending order."""
    h, w = a.shape[-3], a.shape[-2]
    k = g.shape[0]
    if h < k or w < k:
        raise ValueError("image %dx%d is smaller than the %dx%d window" % (h, w, k, k))
    rows = sum(g[t] * a[..., :, t:w - k + 1 + t, :] for t in range(k))
    return sum(g[t] * rows[..., t:h - k + 1 + t, :, :] for t in range(k))


def ssim_map_np(x, y, max_val, dtype=np.float64):
    dtype = np.dtype(dtype).type
    x, y = np.asarray(x).astype(dtype), np.asarray(y).astype(dtype)
    assert x.shape == y.shape and x.ndim >= 3
    g = window(dtype)
    c1, c2 = dtype((K1 * max_val) ** 2), dtype((K2 * max_val) ** 2)
    m0, m1 = filter_valid(x, g), filter_valid(y, g)
    num0, den0 = m0 * m1 * dtype(2), m0 * m0 + m1 * m1
    lum = (num0 + c1) / (den0 + c1)
    num1, den1 = filter_valid(x * y, g) * dtype(2), filter_valid(x * x + y * y, g)
    cs = (num1 - num0 + c2) / (den1 - den0 + c2)
    return lum * cs


def ssim_np(x, y, max_val, dtype=np.float64):
    """x, y [H,W,C] or [N,H,W,C] -> float or [N] array of `dtype`."""
    m = ssim_map_np(x, y, max_val, dtype)
    return m.mean(axis=(-3, -2)).mean(axis=-1)


def luma_np(im):
    """[.., 3] -> [.., 1]: 0.2126 r + 0.7152 g + 0.0722 b in float64, then float32 (the metric's path into tf.image.ssim)."""
    im = np.asarray(im).astype(np.float64)
    if im.shape[-1] == 1:
        return im.astype(np.float32)
    lum = LUMA[0] * im[..., 0] + LUMA[1] * im[..., 1] + LUMA[2] * im[..., 2]
    return lum[..., None].astype(np.float32)


def metric_ssim_np(im1, im2, max_val, dtype=np.float64):
    """xm.metric.SSIM on [H,W] / [H,W,1] / [H,W,3]: luma first, then SSIM on the single channel."""
    im1, im2 = np.asarray(im1), np.asarray(im2)
    if im1.ndim == 2:
        im1, im2 = im1[..., None], im2[..., None]
    return float(ssim_np(luma_np(im1), luma_np(im2), max_val, dtype))


def ssim_torch(x, y, max_val, dtype=torch.float64):
    """x, y [N,H,W,C] torch CPU tensors -> [N]; differentiable."""
    x, y = x.to(dtype), y.to(dtype)
    n, h, w, c = x.shape
    if h < FILTER_SIZE or w < FILTER_SIZE:
        raise ValueError("image %dx%d is smaller than the window" % (h, w))
    g = torch.from_numpy(window(np.float64 if dtype == torch.float64 else np.float32))
    kern = torch.outer(g, g)[None, None].to(dtype)
    c1, c2 = (K1 * max_val) ** 2, (K2 * max_val) ** 2

    def filt(a):                                        # [N,H,W,C] -> [N*C,1,H-10,W-10]
        return F.conv2d(a.permute(0, 3, 1, 2).reshape(n * c, 1, h, w), kern)
    m0, m1 = filt(x), filt(y)
    num0, den0 = m0 * m1 * 2, m0 * m0 + m1 * m1
    lum = (num0 + c1) / (den0 + c1)
    num1, den1 = filt(x * y) * 2, filt(x * x + y * y)
    cs = (num1 - num0 + c2) / (den1 - den0 + c2)
    return (lum * cs).reshape(n, c, -1).mean(2).mean(1)


def loss_torch(gt, pred, max_val, dtype=torch.float64):
    """losses.SSIM with keep_batch=True: (1 - ssim(gt, pred)) / 2 per example."""
    return (1 - ssim_torch(gt, pred, max_val, dtype)) / 2


def loss_and_unit_grad(gt, pred, max_val, dtype=torch.float64):
    """([N] loss, [N,H,W,C] d loss[f] / d pred[f]) of `loss_torch`, both in `dtype`, as NumPy arrays."""
    with torch.enable_grad():                           # (also when called from inside an autograd.Function's forward)
        p = torch.as_tensor(pred).to(dtype).clone().requires_grad_(True)
        per = loss_torch(torch.as_tensor(gt), p, max_val, dtype)
        (d,) = torch.autograd.grad(per.sum(), p)        # examples are independent: the sum's gradient is the unit gradient
    return per.detach().numpy(), d.numpy()


# ---- the four kinds of input the issue measured the float32 restatement on ------------------------------------------------
KINDS = ('near', 'smooth', 'flat', 'noise')


def make_pair(kind, n, h, w, c, seed=0, max_val=1.0):
    """(x, y) float32 [N,H,W,C]; every example of a batch is a different image."""
    rng = np.random.RandomState(seed + 1000 * KINDS.index(kind))
    if kind == 'near':                                  # y = x + N(0, 0.02), x uniform
        x = rng.uniform(0, 1, (n, h, w, c))
        y = x + rng.normal(0, 0.02, x.shape)
    elif kind == 'smooth':                              # a smooth bright image and a slightly shifted copy
        yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing='ij')
        ph = rng.uniform(0, 2 * np.pi, (n, 1, 1, c))
        x = 0.8 + 0.15 * np.sin(3 * xx[None, ..., None] + ph) * np.cos(2 * yy[None, ..., None] + ph)
        y = 0.8 + 0.15 * np.sin(3 * xx[None, ..., None] + ph + 0.05) * np.cos(2 * yy[None, ..., None] + ph)
    elif kind == 'flat':                                # flat at 0.8 with 1e-3 noise: den1 - den0 cancels
        x = 0.8 + rng.normal(0, 1e-3, (n, h, w, c))
        y = 0.8 + rng.normal(0, 1e-3, (n, h, w, c))
    else:                                               # independent noise: SSIM about 0
        x = rng.uniform(0, 1, (n, h, w, c))
        y = rng.uniform(0, 1, (n, h, w, c))
    return (x * max_val).astype(np.float32), (y * max_val).astype(np.float32)
