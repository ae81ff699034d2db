"""Experiment (run by hand on the GPU machine; not bench.py): the mesh ray casts of csrc/raycast.hip on an icosphere of 327 680
triangles (20 * 4^7).
  1. the hierarchy build (Morton codes, the stable sort, leaves and levels), nlt_raycast_camera at 512 x 512 and nlt_raycast_shadow
     on its hits: ms and Mrays/s, timed with device events after two warm calls;
  2. for scale, the same two launches on a 4 096-triangle mesh with the hierarchy as built and with pruning disabled (every box
     replaced by one that holds everything, so each ray tests every triangle);
  3. where a 512^2 and a 1024^2 `render_geometry` sample (uvs 1024) spends its time: the two ray casts, the bidirectional mapping
     (dense unwrap table; at 512^2 also the dict form's per-pixel loop) and the two capture launches.
    python tools/bench_raycast.py [--level 7] [--steps 20]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import nlt_amd                                                   # noqa: E402,F401
from nlt_amd import capi as C                                    # noqa: E402
from nlt_amd.data_gen import mesh as M, render as RD             # noqa: E402
import raycast_ref as R                                          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--level', type=int, default=7)
ap.add_argument('--steps', type=int, default=20)
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_raycast needs the GPU: there is no fallback"
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
    """Milliseconds per call on the host clock (host-bound steps), each window ending in a synchronise."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def casts(mesh, cam, imh, light, label, steps=a.steps):
    _, inv, (imh, imw) = M.camera_matrix(cam, imh)
    args = (*mesh.bvh, mesh.n_tris, mesh._tri2face)
    t_cam = timed(lambda: C.raycast_camera(*args, inv.reshape(-1), cam['position'], imh, imw), steps)
    locs, _, valid, _ = C.raycast_camera(*args, inv.reshape(-1), cam['position'], imh, imw)
    hits = int(valid.sum())
    t_sh = timed(lambda: C.raycast_shadow(*mesh.bvh, mesh.n_tris, locs, valid, light), steps)
    occ = int(C.raycast_shadow(*mesh.bvh, mesh.n_tris, locs, valid, light).sum())
    print("  %-34s camera %dx%d: %8.3f ms = %8.1f Mrays/s (%d hits) | shadow: %8.3f ms = %8.1f Mrays/s (%d occluded)"
          % (label, imh, imw, t_cam, imh * imw / t_cam / 1e3, hits, t_sh, hits / t_sh / 1e3, occ))
    return t_cam, t_sh


cam = R.make_cam('B', (1.8, -1.6, 1.9), (0.0, 0.0, 0.0), focal_length=35.0, sensor_width=24.0, sensor_height=24.0)
light = (2.5, 1.0, 2.0)

# ---------------------------------------------------------------- 1. the big mesh
v, f = R.icosphere(a.level)
mesh = M.Mesh(v, f.tolist())
tv = mesh._tri_verts
lo, hi = v.min(0), v.max(0)
print("icosphere level %d: %d triangles, depth %d, hierarchy %.1f MB" % (a.level, mesh.n_tris, int(np.log2((mesh.bvh[1].numel() // 6 + 1) // 2)),
                                                                       8e-6 * (mesh.bvh[0].numel() + mesh.bvh[1].numel())))
print("  hierarchy build (morton + stable sort + leaves + levels): %.3f ms" % timed(lambda: C.bvh_build(tv, lo, hi)))
casts(mesh, cam, 512, light, 'as built')

# ---------------------------------------------------------------- 2. pruning on / off at 4 096 triangles
v4, f4 = R.icosphere(4)
small = M.Mesh(v4, f4[:4096].tolist())
p_cam, p_sh = casts(small, cam, 512, light, '4 096 triangles, as built')
nodes = small.bvh[1].view(-1, 6)
nodes[:, :3], nodes[:, 3:] = -1e300, 1e300
u_cam, u_sh = casts(small, cam, 512, light, '4 096 triangles, pruning disabled', steps=3)
print("  pruning buys x%.0f (camera), x%.0f (shadow) at 4 096 triangles; unpruned = %.1f G ray-triangle tests/s in float64"
      % (u_cam / p_cam, u_sh / p_sh, 512 * 512 * 4096 / u_cam / 1e6))

# ---------------------------------------------------------------- 3. one render_geometry sample
n_faces = mesh.n_tris
side = int(np.ceil(np.sqrt(n_faces)))
cell = np.stack((np.arange(n_faces) % side, np.arange(n_faces) // side), 1).astype(np.float64)
corner = np.array([(0.1, 0.1), (0.9, 0.1), (0.1, 0.9)])
dense = {'uv': (cell[:, None, :] + corner[None]) / side, 'counts': np.full(n_faces, 3)}
light_d = dict(name='L', position=list(light))
for imh in (512, 1024):
    inter = M.shadow(mesh, light_d, M.backproject(mesh, cam, imh))
    imw = inter['hw'][1]
    xs, ys = np.meshgrid(range(imw), range(imh))
    xys = np.dstack((xs, ys)).reshape(-1, 2)
    t_rays = wall(lambda: M.shadow(mesh, light_d, M.backproject(mesh, cam, imh)))
    t_map = wall(lambda: RD.calc_bidir_mapping(dense, None, xys, inter, 1024))
    uv2cam, cam2uv = RD.calc_bidir_mapping(dense, None, xys, inter, 1024)
    alpha = (inter['valid'] * 255).view(imh, imw)

    def capture():
        cv, lv, _, _ = C.capture_camspc(inter['locs'], inter['normals'], inter['valid'], inter['occluded'], cam['position'], light,
                                        alpha, uv2cam.contiguous())
        C.capture_uvspc(cam2uv.contiguous(), cv, lv, None)
    t_cap = timed(capture)
    t_all = wall(lambda: M.render_geometry(mesh, dense, cam, light_d, imh, 1024))
    print("render_geometry at %d^2, uvs 1024: %.1f ms | ray casts (with the face_i copy to the host) %.2f ms, mapping (dense table) "
          "%.1f ms, the two capture launches %.3f ms" % (imh, t_all, t_rays, t_map, t_cap))
    if imh == 512:
        table = {i: [[3 * i + k, 3 * i + k, float(dense['uv'][i, k, 0]), float(dense['uv'][i, k, 1])] for k in range(3)] for i in range(n_faces)}
        print("  mapping with the dict table (a Python loop over %d hit pixels): %.0f ms"
              % (int(inter['valid'].sum()), wall(lambda: RD.calc_bidir_mapping(table, None, xys, inter, 1024), steps=1)))
