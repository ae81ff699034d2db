"""TEST-ONLY: the float64 NumPy brute force csrc/raycast.hip is held to, bit for bit -- every ray against every triangle, the
hit test of include/nlt_hip.h written out operation by operation (NumPy's element-wise ufuncs never fuse a multiply with an add),
the argmin with ties to the lowest index, and the camera-ray and shadow rules.  No hierarchy, no pruning: what a traversal may
not change.  Also the small scene builders the host and GPU tests share."""
import numpy as np

INF = np.inf


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), -1)


def degenerate(tri_verts):
    """[T] bool: e1 x e2 is the zero vector or not finite -- such a triangle is never hit."""
    with np.errstate(all='ignore'):
        n = cross(tri_verts[:, 1] - tri_verts[:, 0], tri_verts[:, 2] - tri_verts[:, 0])
    return ~np.isfinite(n).all(-1) | (n == 0).all(-1)


def hit_distances(o, d, tri_verts):
    """o, d [R,3], tri_verts [T,3,3] -> t [R,T] float64, +inf where the ray misses the triangle."""
    o, d = o[:, None, :], d[:, None, :]
    v0 = tri_verts[None, :, 0]
    with np.errstate(all='ignore'):
        e1, e2 = tri_verts[None, :, 1] - v0, tri_verts[None, :, 2] - v0
        p = cross(d, e2)
        det = dot(e1, p)
        ok = np.isfinite(det) & (det != 0) & ~degenerate(tri_verts)[None, :]
        inv = 1.0 / det
        s = o - v0
        u = dot(s, p) * inv
        ok &= (u >= 0) & (u <= 1)
        q = cross(s, e1)
        v = dot(d, q) * inv
        ok &= (v >= 0) & (u + v <= 1)
        t = dot(e2, q) * inv
        ok &= t >= 0
    return np.where(ok, t, INF)


def closest(o, d, tri_verts, tri2face=None, chunk=256):
    """-> (t [R] float64, +inf = miss; tri [R] int32, -1 = miss; face [R] int32)."""
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    t = np.empty(len(o))
    tri = np.empty(len(o), np.int32)
    for a in range(0, len(o), chunk):
        tt = hit_distances(o[a:a + chunk], d[a:a + chunk], tri_verts)
        k = tt.argmin(1)                                            # the first minimum: ties to the lowest index
        t[a:a + chunk] = tt[np.arange(len(k)), k]
        tri[a:a + chunk] = k
    tri[t == INF] = -1
    face = tri.copy() if tri2face is None else np.where(tri >= 0, np.asarray(tri2face)[np.maximum(tri, 0)], -1).astype(np.int32)
    return t, tri, face


def unit_towards(src, to):
    """dir = (to - src) / |to - src| per component, and |to - src|."""
    with np.errstate(all='ignore'):
        w = to - src
        length = np.sqrt(dot(w, w))
        return w / length[..., None], length


def camera_rays(cam_mat_inv, cam_loc, imh, imw):
    """backproject_to_3d's rays, row-major pixels: ray_to = from_homo(Minv . (x, y, 1, 1)), dir normalised."""
    m = np.asarray(cam_mat_inv, np.float64).reshape(4, 4)
    xs, ys = np.meshgrid(np.arange(imw, dtype=np.float64), np.arange(imh, dtype=np.float64))
    x, y = xs.reshape(-1), ys.reshape(-1)
    h = [((m[r, 0] * x + m[r, 1] * y) + m[r, 2]) + m[r, 3] for r in range(4)]
    to = np.stack((h[0] / h[3], h[1] / h[3], h[2] / h[3]), -1)
    d, _ = unit_towards(np.asarray(cam_loc, np.float64), to)
    return d


def backproject(tri_verts, tri2face, cam_mat_inv, cam_loc, imh, imw):
    """The dense intersect as NumPy arrays: locs, normals [P,3], valid uint8 [P], face_i int32 [P]."""
    cam_loc = np.asarray(cam_loc, np.float64)
    d = camera_rays(cam_mat_inv, cam_loc, imh, imw)
    t, tri, face = closest(np.broadcast_to(cam_loc, d.shape), d, tri_verts, tri2face)
    hit = tri >= 0
    k = np.maximum(tri, 0)
    with np.errstate(all='ignore'):
        loc = cam_loc + t[:, None] * d
        c = cross(tri_verts[k, 1] - tri_verts[k, 0], tri_verts[k, 2] - tri_verts[k, 0])
        nrm = c / np.sqrt(dot(c, c))[:, None]
    z = np.zeros(3)
    return dict(locs=np.where(hit[:, None], loc, z), normals=np.where(hit[:, None], nrm, z), valid=hit.astype(np.uint8),
                face_i=face, hw=(imh, imw))


def shadow(tri_verts, locs, valid, light_loc):
    """data_gen/render.py:238-254 -> occluded uint8 [P]."""
    light = np.asarray(light_loc, np.float64)
    d, full = unit_towards(light, np.asarray(locs, np.float64))
    d = np.where(np.asarray(valid)[:, None] > 0, d, 1.0)            # (invalid pixels cast nothing; any ray will do)
    t, tri, _ = closest(np.broadcast_to(light, d.shape), d, tri_verts)
    with np.errstate(all='ignore'):
        reach = np.abs(t - full) <= 1e-8 + 1e-5 * np.abs(full)      # np.isclose's defaults, written out
    return ((np.asarray(valid) > 0) & (tri >= 0) & ~reach).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def soup(n, seed, degenerates=False):
    """n random triangles in the unit cube (edge lengths up to 0.3).  degenerates: every 5th triangle has zero area (three equal
    vertices, or collinear ones with e2 = 2 e1 exactly) and one vertex of triangle 1 sits at 1e6."""
    rng = np.random.default_rng(seed)
    c = rng.random((n, 1, 3))
    tv = c + (rng.random((n, 3, 3)) - 0.5) * 0.3
    if degenerates:
        for i in range(0, n, 5):
            if (i // 5) % 2:
                tv[i, 1] = tv[i, 0]; tv[i, 2] = tv[i, 0]
            else:
                e = np.round((rng.random(3) - 0.5) * 64) / 256          # few mantissa bits: v0 + e, v0 + 2e are exact
                tv[i, 0] = np.round(tv[i, 0] * 256) / 256
                tv[i, 1] = tv[i, 0] + e; tv[i, 2] = tv[i, 0] + 2 * e
        if n > 1:
            tv[1, 2] = (1e6, -1e6, 1e6)
    return np.ascontiguousarray(tv)


def rays_into(n, seed, lo=0.0, hi=1.0):
    """n rays from a sphere around the box [lo, hi]^3 towards random points inside it (unit directions)."""
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3))
    o = (lo + hi) / 2 + o / np.linalg.norm(o, axis=1, keepdims=True) * (hi - lo) * 2.5
    d, _ = unit_towards(o, lo + rng.random((n, 3)) * (hi - lo))
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def icosphere(level):
    """Unit icosphere: 20 * 4^level triangles (vertices [V,3], faces [T,3] int)."""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = np.array(v, np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = np.array(f, np.int64)
    for _ in range(level):
        edges = np.sort(np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]])), 1)
        uniq, inv = np.unique(edges, axis=0, return_inverse=True)
        mid = v[uniq[:, 0]] + v[uniq[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = len(v) + inv.reshape(3, -1)                             # midpoints of edges 01, 12, 20 per face
        v = np.concatenate((v, mid))
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        f = np.concatenate((np.stack((a, m[0], m[2]), 1), np.stack((b, m[1], m[0]), 1), np.stack((c, m[2], m[1]), 1),
                            np.stack((m[0], m[1], m[2]), 1)))
    return v, f


def look_at(position, target, up=(0.0, 0.0, 1.0)):
    """Blender 'XYZ' Euler angles of a camera at `position` looking at `target` (the camera looks down its -z, y up)."""
    position, target = np.asarray(position, np.float64), np.asarray(target, np.float64)
    z = position - target
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    r = np.stack((x, y, z), 1)                                      # camera -> world; r = Rz Ry Rx
    ry = -np.arcsin(np.clip(r[2, 0], -1, 1))
    rx = np.arctan2(r[2, 1], r[2, 2])
    rz = np.arctan2(r[1, 0], r[0, 0])
    return [float(rx), float(ry), float(rz)]


def make_cam(name, position, target, focal_length=50.0, sensor_width=36.0, sensor_height=24.0, up=(0.0, 0.0, 1.0)):
    return dict(name=name, position=[float(x) for x in position], rotation=look_at(position, target, up), focal_length=focal_length,
                sensor_width=sensor_width, sensor_height=sensor_height, clip_start=0.1, clip_end=100.0)


# ---------------------------------------------------------------------------------------------------------------------
# the two mesh fixtures and what the tests build around them
# ---------------------------------------------------------------------------------------------------------------------
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
BUNNY, CUBE = os.path.join(GOLDEN, 'bun_zipper_res4.ply'), os.path.join(GOLDEN, 'cube.obj')


def grid_unwrap(n_faces, verts_per_face=3):
    """{face: [[loop, vert, u, v], ...]}: one small chart per face on a square grid of cells (enough for the mapping tests)."""
    side = int(np.ceil(np.sqrt(n_faces)))
    corner = np.array([(0.1, 0.1), (0.9, 0.1), (0.9, 0.9), (0.1, 0.9)])[:verts_per_face] if verts_per_face == 4 else \
        np.array([(0.1, 0.1), (0.9, 0.1), (0.1, 0.9)])
    table = {}
    for f in range(n_faces):
        cell = np.array([f % side, f // side], np.float64)
        table[f] = [[verts_per_face * f + k, verts_per_face * f + k] + list((cell + corner[k]) / side) for k in range(verts_per_face)]
    return table


def bunny_cam(name='B01', offset=(0.12, -0.05, 0.33), sensor=(32.0, 24.0), aim=(0.0, 0.0, 0.0)):
    """A camera looking at the bunny's centroid (+ aim) from centroid + offset; 32 x 24 mm sensor: imw = imh * 4 / 3."""
    from nlt_amd.data_gen.mesh import load_mesh
    c = load_mesh(BUNNY)['vertices'].mean(0)
    return make_cam(name, c + np.asarray(offset), c + np.asarray(aim), sensor_width=sensor[0], sensor_height=sensor[1])
