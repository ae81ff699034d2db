"""Experiment (run by hand on the GPU machine; not bench.py): relighting one view under an environment map at the released shape
(512^2 UV and camera maps, depth 256, bs 4) on a synthetic one-camera x --lights capture.
  1. ms per relit view for R = 1 and R = 120 probe rotations, and its parts timed alone: the renders (load_batch + Model.call in
     the inference mode, per chunk), the accumulation (nlt_relight_accumulate per chunk) and the finish (nlt_relight_finish);
  2. nlt_envmap_light_weights at --probe (1024x2048) x 300 lights, R = 1: time, and the result against the float64 NumPy loop of
     tests/relight_ref.py (max |err| over the bound 2^-23 |ref| + 1e-12; the loop's own time).
Every timed window is warmed on the shapes it uses and ends in a device synchronise.
    python tools/bench_relight.py [--lights 300] [--steps 5] [--probe 1024x2048] [--no-ref]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import nlt_amd                                                   # noqa: E402
from nlt_amd import capi as C, nlt_test, relight as RL           # noqa: E402
from nlt_amd.datasets import nlt as D                            # noqa: E402
from nlt_amd.datasets.synth import synthetic_store               # noqa: E402
from nlt_amd.models import get_model_class                       # noqa: E402
import relight_ref as R                                          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--lights', type=int, default=300)
ap.add_argument('--steps', type=int, default=5)
ap.add_argument('--size', type=int, default=512)
ap.add_argument('--probe', default='1024x2048')
ap.add_argument('--no-ref', action='store_true', help="skip the float64 NumPy loop (some ten seconds at 1024x2048)")
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_relight needs the GPU: there is no fallback"
torch.cuda.set_device(0)
BS, CAM = 4, 'C000'


def timed(fn, steps):
    """Seconds per call of fn, after two warm calls, over `steps` calls that end in one synchronise."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def one_camera_store(n_lights, size):
    """synthetic_store's frames renamed to one camera x n_lights lights, each light's neighbour the next one."""
    store = synthetic_store(n_lights, size, size, device='cuda', seed=0)
    ids = ['trainvali_%09d_%s_L%03d' % (i, CAM, i) for i in range(n_lights)]
    store['ids'] = ids
    store['nn'] = {id_: {'cam': CAM, 'light': 'L%03d' % ((i + 1) % n_lights)} for i, id_ in enumerate(ids)}
    return store


# ---------------------------------------------------------------- 1. the relit view
cfg = nlt_amd.make_config(uvh=a.size, uvw=a.size, imh=a.size, imw=a.size, bs=BS)
model = get_model_class('nlt')(cfg)
model.build('cuda')
model.register_trainable()
store = one_camera_store(a.lights, a.size)
ds = D.Dataset(cfg, 'train', store=store)
feat_agg = nlt_test.extract_feat(model, ds.build_pipeline(seed=0), 1)
ids = [i for i, _ in RL.view_samples(store, CAM)]
dirs = R.random_directions(a.lights, 1)
probe = (np.random.default_rng(2).random((64, 128, 3)) + 0.05).astype(np.float32)
chunks = [ids[i:i + BS] for i in range(0, len(ids), BS)]


def render_only():
    for c in chunks:
        model.call(ds.load_batch(c), 'test', obs_override=feat_agg)


print("relit view at %d^2, %d lights in chunks of %d (%d Model.calls):" % (a.size, a.lights, BS, len(chunks)))
t_render = timed(render_only, a.steps)
texels = a.size * a.size
for n_rot in (1, 120):
    w = RL.envmap_weights(probe, dirs, rotations=[2 * np.pi * t / n_rot for t in range(n_rot)])
    pred = torch.rand((BS, a.size, a.size, 3), device='cuda')
    acc = torch.zeros((n_rot, a.size, a.size, 3), device='cuda')

    def accumulate_only():
        for i, c in enumerate(chunks):
            C.relight_accumulate(pred[:len(c)], w, i * BS, acc, False)
    t_acc = timed(accumulate_only, a.steps)
    t_fin = timed(lambda: C.relight_finish(acc, 1.0, True), a.steps)
    t_all = timed(lambda: RL.relight(model, ds, CAM, w, feat_agg=feat_agg), a.steps)
    # bytes the accumulation has to move: per chunk, acc read + written once and the chunk's predictions once per r-tile of 8
    moved = sum(4.0 * 3 * texels * (2 * n_rot + len(c) * -(-n_rot // 8)) for c in chunks)
    print("  R = %3d: %8.2f ms per view | alone: render %8.2f ms, accumulate %8.2f ms (%.0f GB/s of the bytes it needs), finish %6.3f ms"
          % (n_rot, 1e3 * t_all, 1e3 * t_render, 1e3 * t_acc, moved / t_acc / 1e9, 1e3 * t_fin))
    if t_acc > t_render:
        print("           the accumulation takes longer than the renders at R = %d: the r-tile (8) and the per-chunk pass over acc "
              "are the next thing to tune" % n_rot)
    del acc, pred

# ---------------------------------------------------------------- 2. the weights
he, we = (int(x) for x in a.probe.split('x'))
big = (np.random.default_rng(3).random((he, we, 3)) + 0.05).astype(np.float32)
dirs300, eye = R.random_directions(300, 4), np.eye(3, dtype=np.float32)[None]
dev = lambda x: torch.from_numpy(x).cuda()
args = (dev(big), dev(dirs300), dev(eye))
t_w = timed(lambda: C.envmap_light_weights(*args), a.steps)
print("envmap_light_weights %dx%d x 300 lights, R = 1: %.3f ms" % (he, we, 1e3 * t_w))
if not a.no_ref:
    t0 = time.perf_counter()
    idx, margin = R.nearest_lights(he, we, dirs300, eye)
    ref = R.envmap_light_weights(big, dirs300, eye, idx=idx)
    t_ref = time.perf_counter() - t0
    got = C.envmap_light_weights(*args).cpu().numpy().astype(np.float64)
    ratio = np.abs(got - ref) / (2.0 ** -23 * np.abs(ref) + 1e-12)
    print("  float64 NumPy loop: %.1f s; rel-L2 of all weights %.3e; max |err| / (2^-23 |ref| + 1e-12) = %.3f; %d of %d pixels have a "
          "float64 margin between their two best lights under 1e-5 (smallest %.2e: under ~2e-7 the float32 dot products may pick "
          "the other light, and that pixel's energy moves)"
          % (t_ref, float(np.linalg.norm(got - ref) / np.linalg.norm(ref)), float(ratio.max()), int((margin < 1e-5).sum()), he * we,
             float(margin.min())))
