"""Experiment (run by hand on the GPU machine; not bench.py): the UV unwrap (csrc/unwrap.hip, data_gen/unwrap.py) on the icosphere
of 327 680 triangles (20 * 4^7) of the other data-gen benchmarks, at angle limits 66 and 89 (area weight 0, margin 0.002).
Per stage: milliseconds on the host clock, each window ending in a device synchronise (stages b and d read a device value every
round, so the host is part of them), the mean of `--steps` calls after two warm ones; the rounds of stages b and d, the groups and
the islands; and, for scale, the wall time of the NumPy restatement tests/unwrap_ref.py (one run).
    python tools/bench_unwrap.py [--level 7] [--steps 5] [--no_ref]"""
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
from nlt_amd.data_gen import unwrap as U                         # noqa: E402
import unwrap_ref as R                                           # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--level', type=int, default=7)
ap.add_argument('--steps', type=int, default=5)
ap.add_argument('--no_ref', action='store_true', help="skip the NumPy restatement")
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_unwrap needs the GPU: there is no fallback"
torch.cuda.set_device(0)


def wall(fn, steps=a.steps):
    """(milliseconds per call on the host clock, the last call's result); every window ends in a synchronise."""
    for _ in range(2):
        out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps, out


v, f = R.icosphere(a.level)
faces = f.tolist()
verts, _, loop_verts, face_off = U.mesh_arrays(dict(vertices=v, faces=faces))
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
d_verts, d_lv, d_fo = dev(verts), dev(loop_verts), dev(face_off)
print("icosphere level %d: %d faces, %d loops, %d vertices" % (a.level, len(faces), len(loop_verts), len(verts)))

for angle in (66., 89.):
    cos_half, cos_full = U.angle_cosines(angle)
    t_a, (_, unit, area, ok) = wall(lambda: C.unwrap_frames(d_verts, d_lv, d_fo))
    t_b, (vectors, seeds) = wall(lambda: C.unwrap_vectors(unit, area, ok, cos_half, cos_full, 0.0, 1.0))
    vectors = vectors.contiguous()
    t_c, group = wall(lambda: C.unwrap_assign(unit, ok, vectors))
    t_d, (label, loop_face, island_rounds) = wall(lambda: C.unwrap_islands(d_lv, d_fo, len(verts), group))
    t0 = time.perf_counter()
    island_labels, island = U.island_numbers(label.cpu().numpy())
    frames = np.stack([np.stack(U.projection_basis(x)) for x in vectors.cpu().numpy()])
    d_island, d_frames = dev(island), dev(frames)
    t_host1 = 1e3 * (time.perf_counter() - t0)
    t_e, (puv, boxes) = wall(lambda: C.unwrap_boxes(d_verts, d_lv, loop_face, group, d_island, d_frames, len(island_labels)))
    t0 = time.perf_counter()
    b = boxes.cpu().numpy()
    scale, rot, offsets = U.pack_islands(b[:, 2:] - b[:, :2], island_labels, 0.002)
    d_rot, d_off = dev(rot.astype(np.uint8)), dev(offsets)
    t_f = 1e3 * (time.perf_counter() - t0)
    t_g, uv = wall(lambda: C.unwrap_uv(puv, d_fo, d_island, boxes, d_rot, d_off, scale, 3))
    t_all, u = wall(lambda: U.smart_unwrap(dict(vertices=v, faces=faces), angle, 0.0, 0.002), steps=max(1, a.steps // 2))
    print("angle limit %g: %d groups in %d rounds, %d islands in %d rounds, scale %.4f" % (angle, len(seeds), len(seeds), len(island_labels),
                                                                                       island_rounds, scale))
    print("  a frames %.3f ms | b vectors %.3f ms (%.3f per round) | c assign %.3f ms | d islands %.3f ms (sort + %d rounds) | island numbers "
          "and frames (host) %.3f ms | e boxes %.3f ms | f packing (host) %.3f ms | g uv %.3f ms"
          % (t_a, t_b, t_b / len(seeds), t_c, t_d, island_rounds, t_host1, t_e, t_f, t_g))
    print("  smart_unwrap end to end (mesh lists in, table arrays out, host conversions included): %.1f ms" % t_all)
    if not a.no_ref:
        t0 = time.perf_counter()
        r = R.unwrap(v, faces, angle, 0.0, 0.002)
        print("  NumPy restatement: %.1f ms; uv bit-equal: %s" % (1e3 * (time.perf_counter() - t0), bool(np.array_equal(r['uv'], u.dense['uv']))))
