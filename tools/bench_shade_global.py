"""Experiment (run by hand on the GPU machine; not bench.py): nlt_render_global (csrc/raycast.hip) beside nlt_render_direct from
the same run, on the icosphere of 327 680 triangles (20 * 4^7) of tools/bench_shade.py, same camera and light, 512 x 512 at 16
samples per pixel, flat shading, (bounce rays, light points) = (0, 1), (4, 1), (8, 4); light radius 0.1.
Reported: ms (device events after two warm calls) and Mrays/s counting every traversal -- the primary rays, one shadow ray per
hit sample and light point that faces it (the facing fraction is measured at the pixel centres for the light's centre), one
bounce ray per hit sample and table point (flat shading: none is dropped by the geometric-normal rule), and the secondary
hits' shadow rays.  The icosphere is convex: every bounce ray misses, there are no secondary shadow rays and the count is
exact up to the facing fraction.  `--bumpy` repeats the legs on the same mesh with its radius modulated (concave: bounce rays
hit); there the secondary shadow rays are not counted, so its Mrays/s is a lower bound.
    python tools/bench_shade_global.py [--level 7] [--steps 5] [--bumpy]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import nlt_amd                                                   # noqa: E402,F401
from nlt_amd import capi as C                                    # noqa: E402
from nlt_amd.data_gen import mesh as M, shade as SH              # noqa: E402
import raycast_ref as R                                          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--level', type=int, default=7)
ap.add_argument('--steps', type=int, default=5)
ap.add_argument('--spp', type=int, default=16)
ap.add_argument('--bumpy', action='store_true')
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_shade_global needs the GPU: there is no fallback"
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


cam = R.make_cam('B', (1.8, -1.6, 1.9), (0.0, 0.0, 0.0), focal_length=35.0, sensor_width=24.0, sensor_height=24.0)
light = dict(name='L', position=[2.5, 1.0, 2.0], size=0.1)
mat = SH.Material(smooth=False)
v, f = R.icosphere(a.level)
meshes = [('icosphere', v)]
if a.bumpy:
    meshes.append(('bumpy', v * (1.0 + 0.12 * np.sin(9.0 * v[:, :1]) * np.sin(7.0 * v[:, 1:2]) * np.sin(8.0 * v[:, 2:3]))))
for name, verts in meshes:
    mesh = M.Mesh(verts, f.tolist())
    _, inv, (imh, imw) = M.camera_matrix(cam, 512)
    locs, normals, valid, _ = C.raycast_camera(*mesh.bvh, mesh.n_tris, mesh._tri2face, inv.reshape(-1), cam['position'], imh, imw)
    cos = C.cosine_map(locs, normals, valid, None, light['position'], want_u8=False)[0]
    # the kernel shades two-sided: a hit faces the light when the light is on the viewer's side of its plane
    to_cam = torch.tensor(cam['position'], dtype=torch.float64, device=locs.device) - locs
    side = (normals * to_cam).sum(-1)
    facing = float((((cos > 0) == (side > 0)) & (valid > 0)).sum()) / max(int(valid.sum()), 1)
    print("%s level %d: %d triangles, %d x %d pixels, %d samples per pixel, %.3f of the hits face the light"
          % (name, a.level, mesh.n_tris, imh, imw, a.spp, facing))
    t = timed(lambda: SH.render_direct(mesh, cam, light, imh, a.spp, mat))
    _, cov = SH.render_direct(mesh, cam, light, imh, a.spp, mat)
    primary = imh * imw * a.spp
    hit_samples = int(round(float(cov.double().sum()) * a.spp))
    rays = primary + hit_samples * facing
    print("  nlt_render_direct              : %8.3f ms = %7.1f Mrays/s (%d primary + ~%d shadow rays)"
          % (t, rays / t / 1e3, primary, int(hit_samples * facing)))
    for n_b, n_l in ((0, 1), (4, 1), (8, 4)):
        t = timed(lambda: SH.render_global(mesh, cam, light, imh, a.spp, mat, bounces=n_b, light_samples=n_l))
        _, _, ind = SH.render_global(mesh, cam, light, imh, a.spp, mat, bounces=n_b, light_samples=n_l)
        shadow, bounce = hit_samples * facing * n_l, hit_samples * n_b
        rays = primary + shadow + bounce
        print("  nlt_render_global n_b %d n_l %d : %8.3f ms = %7.1f Mrays/s%s (%d primary + ~%d shadow + %d bounce rays); %d pixels "
              "with indirect light" % (n_b, n_l, t, rays / t / 1e3, ' (lower bound)' if name == 'bumpy' and n_b else '', primary,
                                       int(shadow), bounce, int((ind > 0).any(-1).sum())))
