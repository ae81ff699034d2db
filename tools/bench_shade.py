"""Experiment (run by hand on the GPU machine; not bench.py): nlt_render_direct (csrc/raycast.hip) on the icosphere of 327 680
triangles (20 * 4^7) of tools/bench_raycast.py, same camera and light.
  1. 512 x 512 at 1, 4 and 16 samples per pixel: ms and Mrays/s, counting the primary rays and the shadow rays actually cast (one
     per hit sample that faces the light), timed with device events after two warm calls; beside them the parent's equivalent --
     nlt_raycast_camera + nlt_raycast_shadow at 512 x 512, measured here too, scaled by the sample count;
  2. where one `render_view` + `write_sample` sample (512 x 512, uvs 1024, 16 samples) spends its time.
    python tools/bench_shade.py [--level 7] [--steps 20]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import nlt_amd                                                   # noqa: E402,F401
from nlt_amd import capi as C                                    # noqa: E402
from nlt_amd.data_gen import mesh as M, render as RD, shade as SH  # noqa: E402
import raycast_ref as R                                          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--level', type=int, default=7)
ap.add_argument('--steps', type=int, default=20)
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_shade needs the GPU: there is no fallback"
torch.cuda.set_device(0)


def timed(fn, steps=a.steps):
    """Milliseconds per call between two device events, after two warm calls."""
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def wall(fn, steps=3):
    """Milliseconds per call on the host clock, each window ending in a synchronise."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


cam = R.make_cam('B', (1.8, -1.6, 1.9), (0.0, 0.0, 0.0), focal_length=35.0, sensor_width=24.0, sensor_height=24.0)
light = dict(name='L', position=[2.5, 1.0, 2.0], size=0.1)
v, f = R.icosphere(a.level)
mesh = M.Mesh(v, f.tolist())
imh = 512
_, inv, (imh, imw) = M.camera_matrix(cam, imh)
print("icosphere level %d: %d triangles, %d x %d pixels" % (a.level, mesh.n_tris, imh, imw))

# ---------------------------------------------------------------- the parent's two launches
args = (*mesh.bvh, mesh.n_tris, mesh._tri2face)
t_cam = timed(lambda: C.raycast_camera(*args, inv.reshape(-1), cam['position'], imh, imw))
locs, normals, valid, _ = C.raycast_camera(*args, inv.reshape(-1), cam['position'], imh, imw)
frac_facing = float((C.cosine_map(locs, normals, valid, None, light['position'], want_u8=False)[0] > 0).sum()) / max(int(valid.sum()), 1)
t_sh = timed(lambda: C.raycast_shadow(*mesh.bvh, mesh.n_tris, locs, valid, light['position']))
hits = int(valid.sum())
base_rays = imh * imw + hits
print("  nlt_raycast_camera %.3f ms + nlt_raycast_shadow %.3f ms = %.3f ms for %d + %d rays = %.1f Mrays/s"
      % (t_cam, t_sh, t_cam + t_sh, imh * imw, hits, base_rays / (t_cam + t_sh) / 1e3))

# ---------------------------------------------------------------- 1. nlt_render_direct
for smooth in (False, True):
    mat = SH.Material(smooth=smooth)
    for spp in (1, 4, 16):
        s = SH.spp_side(spp)
        t = timed(lambda: SH.render_direct(mesh, cam, light, imh, spp, mat), steps=max(3, a.steps // spp))
        _, cov = SH.render_direct(mesh, cam, light, imh, spp, mat)
        primary = imh * imw * spp
        hit_samples = int(round(float(cov.double().sum()) * spp))
        facing = hit_samples * frac_facing          # shadow rays: hit samples that face the light (the fraction measured at 1 spp)
        rays = primary + facing
        print("  render_direct %s spp %2d: %8.3f ms = %7.1f Mrays/s (%d primary + ~%d shadow rays) | parent's two launches x %d: %8.3f ms"
              % ('smooth' if smooth else 'flat  ', spp, t, rays / t / 1e3, primary, int(facing), spp, (t_cam + t_sh) * spp))

# ---------------------------------------------------------------- 2. one whole sample
n_faces = mesh.n_tris
side = int(np.ceil(np.sqrt(n_faces)))
cell = np.stack((np.arange(n_faces) % side, np.arange(n_faces) // side), 1).astype(np.float64)
corner = np.array([(0.1, 0.1), (0.9, 0.1), (0.1, 0.9)])
dense = {'uv': (cell[:, None, :] + corner[None]) / side, 'counts': np.full(n_faces, 3)}
mat = SH.Material()
out = tempfile.mkdtemp(prefix='bench_shade_')
try:
    t_view = wall(lambda: SH.render_view(mesh, dense, cam, light, imh, 1024, 16, mat, 20.0))
    sample = SH.render_view(mesh, dense, cam, light, imh, 1024, 16, mat, 20.0)
    t_write = wall(lambda: RD.write_sample(os.path.join(out, 's'), sample, cam, light, {'cam': 'B', 'light': 'L'}))
    t_shade = timed(lambda: SH.render_direct(mesh, cam, light, imh, 16, mat), steps=3)
    print("one sample at %d^2, uvs 1024, spp 16: render_view %.1f ms (of which nlt_render_direct %.2f ms) + write_sample %.1f ms"
          % (imh, t_view, t_shade, t_write))
finally:
    shutil.rmtree(out, ignore_errors=True)
