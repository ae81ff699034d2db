"""Experiment (run by hand on the GPU machine; not bench.py): the LPIPS chain of csrc/lpips.hip with random weights.
  1. nlt_lpips_loss, value + gradient and value only, at --frames x --size^2 (default 4 x 512^2), with the chain's fp32 FLOP count;
  2. the train step at the released 512^2 shape (depth 256, k = 1) with loss = barron against loss = barron,1e+0lpips.
    python tools/bench_lpips.py [--frames 4] [--size 512] [--steps 20]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                                     # noqa: E402
import nlt_amd                                                   # noqa: E402
from nlt_amd import capi as C, lpips_weights as LW               # noqa: E402
from nlt_amd.models import get_model_class                       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=4)
ap.add_argument('--size', type=int, default=512)
ap.add_argument('--steps', type=int, default=20)
a = ap.parse_args()
dev = torch.device('cuda', 0)


def random_weights(seed=0):
    rng = np.random.RandomState(seed)
    w = {}
    for l in range(1, 6):
        o, i, k, _ = LW.conv_shape(l)
        b = np.sqrt(6.0 / (i * k * k))
        w['conv%d_weight' % l] = rng.uniform(-b, b, (o, i, k, k)).astype(np.float32)
        w['conv%d_bias' % l] = rng.uniform(0.02, 0.12, o).astype(np.float32)
        w['lin%d' % l] = (rng.uniform(0, 1, o) / o).astype(np.float32)
    return w


def conv_flops(size):
    """fp32 FLOPs (2 per multiply-add) of the five convs on one image, per layer."""
    h1 = (size - 7) // 4 + 1
    h2 = (h1 - 3) // 2 + 1
    h3 = (h2 - 3) // 2 + 1
    maps = (h1, h2, h3, h3, h3)
    return [2.0 * m * m * LW.CHANNELS[l + 1] * LW.CHANNELS[l] * LW.KERNELS[l] ** 2 for l, m in enumerate(maps)]


def timed(fn, steps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


W = random_weights()
blob = torch.from_numpy(LW.blob(LW.validate(W))).to(dev)
n, s = a.frames, a.size
g = torch.Generator(device=dev).manual_seed(1)
gt = torch.rand((n, s, s, 3), device=dev, generator=g)
pred = (gt + 0.05 * torch.rand((n, s, s, 3), device=dev, generator=g)).clamp(0, 1)
per = conv_flops(s)
fwd, bwd = 2 * n * sum(per), n * sum(per)
print('chain FLOPs at %d x %d^2: forward (2 x %d images) %.1f GFLOP, backward-data (%d images) %.1f GFLOP' % (n, s, n, fwd / 1e9, n, bwd / 1e9))
t_val = timed(lambda: C.lpips_loss(pred, gt, blob, False), a.steps)
t_grad = timed(lambda: C.lpips_loss(pred, gt, blob, True), a.steps)
print('nlt_lpips_loss value only     : %.3f ms  (%.1f TFLOP/s fp32)' % (t_val * 1e3, fwd / t_val / 1e12))
print('nlt_lpips_loss value+gradient : %.3f ms  (%.1f TFLOP/s fp32)' % (t_grad * 1e3, (fwd + bwd) / t_grad / 1e12))

with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, 'lpips.npz')
    np.savez(path, **W)
    batch = bench.synth_device_batch(n, s, s, 1, dev, seed=3)
    for loss in ('barron', 'barron,1e+0lpips'):
        cfg = nlt_amd.make_config(depth=256, uvh=s, uvw=s, imh=s, imw=s, bs=n, loss=loss, lpips_weights=path)
        model = get_model_class('nlt')(cfg).build(dev)
        model.register_trainable()
        t = timed(lambda: model.train_forward_backward(batch, n), a.steps)
        print('train step %d x %d^2, loss = %-18s: %.3f ms' % (n, s, loss, t * 1e3))
        del model
