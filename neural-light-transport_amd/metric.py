"""Image metrics with the reference's call signatures (third_party/xiuminglib/xiuminglib/metric.py) on libnlt_hip.so."""
import math

import numpy as np
import torch

from . import _capi as C
from . import losses, lpips_weights


DEVICE = 'cuda'


def _on_device(x):
    if torch.is_tensor(x):
        return x if x.device.type == torch.device(DEVICE).type else x.to(DEVICE)
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEVICE)


class Base:
    """xm.metric.Base (metric.py:35-72): `dtype` fixes the dynamic range -- 1 for float types, max - min for unsigned integer
    types."""

    def __init__(self, dtype):
        self.dtype = np.dtype(dtype)
        if self.dtype.kind == 'f':
            self.drange = 1.
        elif self.dtype.kind == 'u':
            info = np.iinfo(self.dtype)
            self.drange = float(info.max - info.min)
        else:
            raise NotImplementedError(self.dtype.kind)


class PSNR(Base):
    """xm.metric.PSNR (metric.py:105-151): Peak Signal-to-Noise Ratio in dB on luma (0.2126 r + 0.7152 g + 0.0722 b for
    3-channel inputs), float64 arithmetic, optional H x W logical mask.  `dtype` fixes the dynamic range the way
    metric.Base does: 1 for float types, max - min for unsigned integer types."""

    def __call__(self, im1, im2, mask=None):
        """im1, im2: [H,W] / [H,W,1] / [H,W,3] torch CUDA tensors (float32 storage) in [0, drange] -> float dB.
        NumPy arrays / host tensors (what the reference's vis_batch hands over) go up to `DEVICE` first: the sums are
        always the kernel's."""
        im1, im2 = _on_device(im1), _on_device(im2)
        if tuple(im1.shape) != tuple(im2.shape):
            raise AssertionError("The two images are not even of the same shape")
        if im1.dim() == 3 and im1.shape[2] not in (1, 3):
            raise NotImplementedError("%d-channel images" % im1.shape[2])
        a, b = im1.float().contiguous(), im2.float().contiguous()
        m = None if mask is None else mask.to(device=a.device, dtype=torch.uint8).contiguous()
        if m is not None and tuple(m.shape[:2]) != tuple(a.shape[:2]):
            raise AssertionError("Mask must be of shape %s, but is of shape %s" % (tuple(a.shape[:2]), tuple(m.shape)))
        se, n = C.psnr_sums(a, b, m).tolist()
        mse = se / n
        return 10 * math.log10((self.drange ** 2) / mse) if mse > 0 else float('inf')


class SSIM(Base):
    """xm.metric.SSIM (metric.py:154-184): tf.image.ssim(im1, im2, max_val=drange) of TF 2.2 on luma -- 3-channel inputs go to
    0.2126 r + 0.7152 g + 0.0722 b in float64 and then to float32 (TF casts), SSIM is taken on that single channel
    (csrc/ssim.hip).  `dtype` fixes the dynamic range exactly as for PSNR.  Parity-unpinned: no TensorFlow to run against;
    the semantics are restated in tests/ssim_ref.py."""

    def __call__(self, im1, im2):
        """im1, im2: [H,W] / [H,W,1] / [H,W,3] in [0, drange], device tensors, host tensors or NumPy arrays -> float."""
        im1, im2 = self._checked(im1, im2, 2)
        return self._values(im1[None], im2[None])[0]

    def batch(self, im1, im2):
        """im1, im2 [N,H,W,C] (C = 1 or 3) -> N floats, one launch; each equals the per-image call bit for bit."""
        im1, im2 = self._checked(im1, im2, 3)
        return self._values(im1, im2)

    @staticmethod
    def _checked(im1, im2, channel_axis):
        im1, im2 = _on_device(im1), _on_device(im2)
        if tuple(im1.shape) != tuple(im2.shape):
            raise AssertionError("The two images are not even of the same shape")
        if im1.dim() == channel_axis:
            im1, im2 = im1.unsqueeze(-1), im2.unsqueeze(-1)
        if im1.dim() != channel_axis + 1:
            raise ValueError("Input must be H-by-W or H-by-W-by-C (a batch: N-by-H-by-W-by-C), but is %dD" % im1.dim())
        if im1.shape[-1] not in (1, 3):
            raise NotImplementedError("%d-channel images" % im1.shape[-1])
        return im1.float().contiguous(), im2.float().contiguous()

    def _values(self, im1, im2):
        return C.ssim_values(im1, im2, self.drange).tolist()


class LPIPS(SSIM):
    """xm.metric.LPIPS (metric.py:187-258): LPIPS v0.1 "alex / lin" (lower is better) of im1 / drange and im2 / drange -- the
    minimum allowed is taken as 0, as there -- on csrc/lpips.hip; one-channel inputs are tripled.  `weight_pb`: the weights file
    (`.pb` or `.npz`); None takes what NLT_LPIPS_WEIGHTS names (nothing is bundled: lpips_weights.py), else NotImplementedError.
    Inputs and `.batch` are handled as for metric.SSIM.  Parity-unpinned: no TensorFlow and no real weights file to run against;
    the semantics are restated in tests/lpips_ref.py."""

    def __init__(self, dtype, weight_pb=None):
        super().__init__(dtype)
        path = weight_pb if weight_pb is not None else lpips_weights.configured_path()
        if path is None:
            raise NotImplementedError("metric.LPIPS: no weights are bundled; pass weight_pb or set %s" % lpips_weights.ENV)
        self._loss = losses.LPIPS(path)

    def _values(self, im1, im2):
        if im1.shape[-1] == 1:
            im1, im2 = im1.expand(-1, -1, -1, 3).contiguous(), im2.expand(-1, -1, -1, 3).contiguous()
        if self.drange != 1.:
            im1, im2 = im1 / self.drange, im2 / self.drange
        return C.lpips_loss(im1, im2, self._loss.blob(im1.device), False)[0].tolist()
