"""Losses with the reference's call signatures (nlt/losses.py:39-53,75-87,90-118,121-169) on HIP kernels
(csrc/train_ops.hip, csrc/barron.hip, csrc/ssim.hip, csrc/lpips.hip); torch.autograd.Function is glue only."""
import os

import torch

from . import _capi as C
from . import lpips_weights


class _L2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt):
        pred, gt = pred.contiguous(), gt.contiguous()
        ctx.save_for_backward(pred, gt)
        return C.l2_loss_forward(pred, gt)

    @staticmethod
    def backward(ctx, gloss):
        pred, gt = ctx.saved_tensors
        return C.l2_loss_backward(pred, gt, gloss.contiguous()), None


class _BarronFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt):
        loss, dunit = C.barron_loss(pred.contiguous(), gt.contiguous(), bool(ctx.needs_input_grad[0]))
        ctx.dunit = dunit
        return loss

    @staticmethod
    def backward(ctx, gloss):
        return C.scale_rows(ctx.dunit, gloss.contiguous()), None


class _SSIMFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, max_val):
        loss, dunit = C.ssim_loss(pred.contiguous(), gt.contiguous(), max_val, bool(ctx.needs_input_grad[0]))
        ctx.dunit = dunit
        return loss

    @staticmethod
    def backward(ctx, gloss):
        return C.scale_rows(ctx.dunit, gloss.contiguous()), None, None


class _LPIPSFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, blob):
        loss, dunit = C.lpips_loss(pred.contiguous(), gt.contiguous(), blob, bool(ctx.needs_input_grad[0]))
        ctx.dunit = dunit
        return loss

    @staticmethod
    def backward(ctx, gloss):
        return C.scale_rows(ctx.dunit, gloss.contiguous()), None, None


class _L2WeightedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, weights):
        pred, gt = pred.contiguous(), gt.contiguous()
        ctx.save_for_backward(pred, gt, weights)
        return C.l2_loss_weighted_forward(pred, gt, weights)

    @staticmethod
    def backward(ctx, gloss):
        pred, gt, weights = ctx.saved_tensors
        return C.l2_loss_weighted_backward(pred, gt, weights, gloss.contiguous()), None, None


class _MulFn(torch.autograd.Function):
    """imgutil.alpha_blend(x, alpha) with no second tensor (nlt/util/img.py:74-89): x * alpha + 0 * (1 - alpha)."""

    @staticmethod
    def forward(ctx, x, alpha):
        ctx.save_for_backward(alpha)
        return C.mul_forward(x.contiguous(), alpha)

    @staticmethod
    def backward(ctx, g):
        (alpha,) = ctx.saved_tensors
        return C.mul_forward(g.contiguous(), alpha), None


def _sample_weight_map(weights, like):
    """Keras `sample_weight` against the per-texel loss map [N,H,W] (losses_utils.compute_weighted_loss: a trailing axis
    of 1 is squeezed, a missing trailing axis added, the rest must broadcast rank for rank) -> dense float32 [N,H,W]."""
    n, h, w = like.shape[:3]
    wt = torch.as_tensor(weights, dtype=torch.float32, device=like.device)
    if wt.dim() == 4 and wt.shape[-1] == 1:
        wt = wt[..., 0]
    elif wt.dim() == 2:
        wt = wt[..., None]
    if wt.dim() not in (0, 3):
        raise ValueError("sample weights of shape %s do not broadcast to the loss map %s" % (tuple(wt.shape), (n, h, w)))
    return wt.expand(n, h, w).contiguous()


class L2:
    """MeanSquaredError over channels, then mean over H,W: per-example [N] with keep_batch=True
    (what the train step injects, trainvali.py:275), scalar otherwise."""

    def __call__(self, gt, pred, keep_batch=False, weights=None):
        if weights is not None:                 # Keras sample_weight on the [N,H,W] loss map (nlt/losses.py:42-43)
            per = _L2WeightedFn.apply(pred, gt, _sample_weight_map(weights, pred))
            return per if keep_batch else per.mean()
        per = _L2Fn.apply(pred, gt)
        return per if keep_batch else per.mean()


class Barron:
    """robust_loss AdaptiveImageLossFunction as NLT fixes it: alpha = 1 (Charbonnier), scale = 0.01,
    sYUV, CDF9/7, 5 levels, wavelet_scale_base = 1 -- no trainable variables."""

    def __init__(self, imw, imh):
        self.imw, self.imh = imw, imh

    def __call__(self, gt, pred, keep_batch=False, weights=None):
        if weights is not None:                 # nlt/losses.py:107-110: gt and pred alpha-blended against zeros
            alpha = torch.as_tensor(weights, dtype=torch.float32, device=pred.device).expand(pred.shape).contiguous()
            gt, pred = _MulFn.apply(gt, alpha), _MulFn.apply(pred, alpha)
        assert tuple(pred.shape[1:3]) == (self.imh, self.imw), (tuple(pred.shape), self.imh, self.imw)
        per = _BarronFn.apply(pred, gt)
        return per if keep_batch else per.mean()


class SSIM:
    """(1 - tf.image.ssim(gt, pred, dynamic_range)) / 2 on the RGB channels as they are (nlt/losses.py:75-87); `weights`
    alpha-blends gt and pred against zeros first.  Scalar mean over the batch, the reference's only form; keep_batch=True
    returns the per-example [N] vector instead -- the one addition to the reference's class, whose __call__ takes no
    keep_batch and so cannot be called by its own train step (trainvali.py:275,299)."""

    def __init__(self, dynamic_range):
        self.dynamic_range = float(dynamic_range)       # i.e. max - min

    def __call__(self, gt, pred, keep_batch=False, weights=None):
        if weights is not None:
            alpha = torch.as_tensor(weights, dtype=torch.float32, device=pred.device).expand(pred.shape).contiguous()
            gt, pred = _MulFn.apply(gt, alpha), _MulFn.apply(pred, alpha)
        per = _SSIMFn.apply(pred, gt, self.dynamic_range)
        return per if keep_batch else per.mean()


class LPIPS:
    """LPIPS v0.1 "alex / lin" between gt and pred in [0, 1], [N,H,W,3] (nlt/losses.py:121-169) on csrc/lpips.hip.  `weights`: a
    path (`.npz` / `.pb`, lpips_weights.load) or the arrays themselves; parsed and validated here, on the host, and uploaded as
    one packed blob per device on first use.  The `weights=` argument of the call alpha-blends gt and pred against zeros first.
    per_ch=True (each channel tiled to three and averaged) is never asked for by the model and raises."""

    def __init__(self, weights, per_ch=False):
        if per_ch:
            raise NotImplementedError("losses.LPIPS(per_ch=True): the model never passes it (nlt/models/nlt.py:74-75)")
        self.per_ch = False
        self.arrays = lpips_weights.load(weights) if isinstance(weights, (str, bytes, os.PathLike)) else lpips_weights.validate(weights)
        self._blobs = {}

    def blob(self, device):
        """The packed weights on `device` (uploaded once)."""
        key = str(torch.device(device))
        if key not in self._blobs:
            self._blobs[key] = torch.from_numpy(lpips_weights.blob(self.arrays)).to(device)
        return self._blobs[key]

    def __call__(self, gt, pred, keep_batch=False, weights=None):
        assert gt.shape[3] == 3 and pred.shape[3] == 3, "Both ground truth and prediction must be of shape `(N, H, W, 3)`"
        if weights is not None:
            alpha = torch.as_tensor(weights, dtype=torch.float32, device=pred.device).expand(pred.shape).contiguous()
            gt, pred = _MulFn.apply(gt, alpha), _MulFn.apply(pred, alpha)
        per = _LPIPSFn.apply(pred, gt, self.blob(pred.device))
        return per if keep_batch else per.mean()
