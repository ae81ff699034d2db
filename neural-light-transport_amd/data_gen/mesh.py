"""A mesh, a cam.json and a light.json -> the dense `intersect` data_gen/render.py takes, without Blender: the two ray casts the
reference does in Python over a mathutils BVH -- xm.blender.camera.backproject_to_3d (camera.py:512-654) and the shadow rays of
calc_light_cosines (data_gen/render.py:238-254) -- on csrc/raycast.hip.  Host code here is file parsing, the camera matrix and
the plumbing around three launches.  What is restated rather than pinned against Blender is listed in DESIGN.md section 8."""
import struct

import numpy as np
import torch

from .. import _capi as C
from .render import _params, render_sample

_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


def _load_ply(path):
    with open(path, 'rb') as h:
        raw = h.read()
    end = raw.find(b'end_header')
    if not raw.startswith(b'ply') or end < 0:
        raise ValueError("%s is not a PLY file" % path)
    body = raw.index(b'\n', end) + 1
    fmt, elements = None, []
    for line in raw[:end].decode('ascii').splitlines():
        w = line.split()
        if not w or w[0] in ('ply', 'comment', 'obj_info'):
            continue
        if w[0] == 'format':
            fmt = w[1]
        elif w[0] == 'element':
            elements.append((w[1], int(w[2]), []))
        elif w[0] == 'property':
            # (name, value dtype, count dtype or None)
            elements[-1][2].append((w[-1], _PLY_TYPES[w[3]], _PLY_TYPES[w[2]]) if w[1] == 'list' else (w[2], _PLY_TYPES[w[1]], None))
    if fmt not in ('ascii', 'binary_little_endian'):
        raise ValueError("%s: PLY format %r is not supported (ascii and binary_little_endian are)" % (path, fmt))
    vertices, faces = None, None
    tokens, pos = (raw[body:].split(), 0) if fmt == 'ascii' else (None, body)
    for name, count, props in elements:
        scalar = all(c is None for _, _, c in props)
        cols, lists = {}, {}
        if scalar and fmt == 'ascii':
            block = np.array(tokens[pos:pos + count * len(props)], dtype=np.float64).reshape(count, len(props))
            pos += count * len(props)
            # a value is what its declared type holds (a `float` property is a float32), as in the binary form
            cols = {p[0]: block[:, i].astype(p[1]) for i, p in enumerate(props)}
        elif scalar:
            dt = np.dtype([(p[0], '<' + p[1]) for p in props])
            block = np.frombuffer(raw, dt, count, pos)
            pos += count * dt.itemsize
            cols = {p[0]: block[p[0]] for p in props}
        else:
            lists = {p[0]: [] for p in props if p[2] is not None}
            for _ in range(count):
                for pname, vt, ct in props:
                    if fmt == 'ascii':
                        n = 1 if ct is None else int(tokens[pos])
                        pos += 0 if ct is None else 1
                        vals = tokens[pos:pos + n]
                        pos += n
                    else:
                        n = 1
                        if ct is not None:
                            n = int(np.frombuffer(raw, '<' + ct, 1, pos)[0])
                            pos += np.dtype(ct).itemsize
                        vals = np.frombuffer(raw, '<' + vt, n, pos)
                        pos += n * np.dtype(vt).itemsize
                    if ct is not None:
                        lists[pname].append([int(v) for v in vals])
        if name == 'vertex':
            vertices = np.stack([cols[k].astype(np.float64) for k in ('x', 'y', 'z')], 1)
        elif name == 'face':
            key = next((k for k in ('vertex_indices', 'vertex_index') if k in lists), None)
            if key is None:
                raise ValueError("%s: the face element has no vertex_indices list" % path)
            faces = lists[key]
    if vertices is None or faces is None:
        raise ValueError("%s: a vertex and a face element are needed" % path)
    return dict(vertices=np.ascontiguousarray(vertices), faces=faces, loop_uvs=None)


def _load_obj(path):
    verts, vts, faces, face_vts = [], [], [], []
    with open(path, 'r', errors='replace') as h:
        for line in h:
            w = line.split('#', 1)[0].split()
            if not w:
                continue
            if w[0] == 'v':
                verts.append([float(x) for x in w[1:4]])
            elif w[0] == 'vt':
                vts.append([float(w[1]), float(w[2]) if len(w) > 2 else 0.0])
            elif w[0] == 'f':
                vi, ti = [], []
                for tok in w[1:]:
                    part = tok.split('/')
                    i = int(part[0])
                    vi.append(i - 1 if i > 0 else len(verts) + i)
                    if len(part) > 1 and part[1]:
                        j = int(part[1])
                        ti.append(j - 1 if j > 0 else len(vts) + j)
                    else:
                        ti.append(None)
                faces.append(vi)
                face_vts.append(ti)
    loop_uvs = None
    if vts:
        # loops without a `vt` get (0, 0), the value Blender's importer leaves in the UV layer for them
        loop_uvs = [np.array([vts[j] if j is not None else (0.0, 0.0) for j in ti], np.float64).reshape(-1, 2) for ti in face_vts]
    return dict(vertices=np.array(verts, np.float64).reshape(-1, 3), faces=faces, loop_uvs=loop_uvs)


def load_mesh(path):
    """.ply (ascii / binary_little_endian; vertex x y z, any other scalar property skipped; face lists of any length) or .obj
    (v, vt, f as v, v/vt, v/vt/vn, v//vn; negative indices; polygons) -> {'vertices': float64 [V,3], 'faces': list of vertex-index
    lists, 'loop_uvs': per face a float64 [n,2] array, or None when the file has no UVs}.  No library."""
    ext = path.lower().rsplit('.', 1)[-1]
    if ext == 'ply':
        return _load_ply(path)
    if ext == 'obj':
        return _load_obj(path)
    raise ValueError("%s: .ply and .obj meshes are read" % path)


def write_ply(path, vertices, faces, binary=True):
    """vertices [V,3] as float32 `x y z`, faces as `list uchar int`: the inverse of `load_mesh` for what the ray casts use."""
    v = np.asarray(vertices, np.float32)
    head = ("ply\nformat %s 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nelement face %d\n"
            "property list uchar int vertex_indices\nend_header\n" % ('binary_little_endian' if binary else 'ascii', len(v), len(faces)))
    with open(path, 'wb') as h:
        h.write(head.encode('ascii'))
        if binary:
            h.write(v.astype('<f4').tobytes())
            for f in faces:
                h.write(struct.pack('<B%di' % len(f), len(f), *f))
        else:
            for row in v:
                h.write((' '.join(repr(float(x)) for x in row) + '\n').encode('ascii'))
            for f in faces:
                h.write((' '.join(str(x) for x in [len(f)] + list(f)) + '\n').encode('ascii'))


class Mesh:
    """World-space triangles of one object and their hierarchy on `device`.  vertices [V,3], faces: vertex-index lists (polygons
    are fan-triangulated as (0, i, i+1); `tri2face` [T] leads back to the polygon), matrix_world: the object's 4 x 4, applied on
    the host in float64.  device = None keeps everything on the host (no hierarchy: parsing and triangulation only)."""

    def __init__(self, vertices, faces, matrix_world=None, device='cuda', loop_uvs=None):
        v = np.array(vertices, np.float64).reshape(-1, 3)
        if matrix_world is not None:
            m = np.asarray(matrix_world, np.float64).reshape(4, 4)
            v = v @ m[:3, :3].T + m[:3, 3]
        self.vertices, self.faces, self.loop_uvs = np.ascontiguousarray(v), [list(f) for f in faces], loop_uvs
        tris, tri2face = [], []
        for fi, f in enumerate(self.faces):
            for i in range(1, len(f) - 1):
                tris.append((f[0], f[i], f[i + 1]))
                tri2face.append(fi)
        if not tris:
            raise ValueError("the mesh has no triangle")
        self.tris = np.array(tris, np.int64)
        self.tri2face = np.array(tri2face, np.int32)
        self.tri_verts = np.ascontiguousarray(self.vertices[self.tris])            # [T,3,3]
        self.n_tris = len(self.tris)
        self.device = device
        if device is not None:
            used = self.tri_verts.reshape(-1, 3)
            used = used[np.isfinite(used).all(1)]
            lo, hi = (used.min(0), used.max(0)) if len(used) else (np.zeros(3), np.zeros(3))
            self._tri_verts = torch.from_numpy(self.tri_verts).to(device)
            self._tri2face = torch.from_numpy(self.tri2face).to(device)
            self.bvh = C.bvh_build(self._tri_verts, lo, hi)                         # built once

    @classmethod
    def load(cls, path, matrix_world=None, device='cuda'):
        d = load_mesh(path)
        return cls(d['vertices'], d['faces'], matrix_world, device, d['loop_uvs'])

    def raycast(self, origins, dirs):
        """origins, dirs [R,3] (float64 tensors on the mesh's device, or arrays) -> (t, tri, face) device tensors."""
        dev = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, np.float64))).to(self.device).contiguous()
        return C.raycast(*self.bvh, self.n_tris, self._tri2face, dev(origins), dev(dirs))


def corner_normals(mesh):
    """Area-weighted vertex normals of `mesh`, gathered per triangle corner through `mesh.tris` -> float64 [T,3,3] on the host.
    A vertex's normal is the sum of e1 x e2 (twice the area times the unit normal) over the triangles that use it, divided by its
    length; degenerate triangles add nothing, and a vertex whose sum is zero keeps a zero normal (the kernel then falls back to
    the geometric normal where the blend vanishes)."""
    tv = mesh.tri_verts
    with np.errstate(all='ignore'):
        c = np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0])
    c[~np.isfinite(c).all(1)] = 0.0
    n = np.zeros_like(mesh.vertices)
    for k in range(3):
        np.add.at(n, mesh.tris[:, k], c)
    length = np.sqrt((n * n).sum(1, keepdims=True))
    n = np.divide(n, length, out=np.zeros_like(n), where=length > 0)
    return np.ascontiguousarray(n[mesh.tris])


def unwrap_from_obj(mesh):
    """The {face: [[loop, vert, u, v], ...]} table of data_gen/uv_unwrap.py:59-63 from the UVs the mesh file itself carries
    (`Mesh.load` / `load_mesh` of an .obj with `vt`).  No unwrapping is done here: a mesh without UVs raises (data_gen/unwrap.py
    unwraps one)."""
    faces, uvs = (mesh['faces'], mesh['loop_uvs']) if isinstance(mesh, dict) else (mesh.faces, mesh.loop_uvs)
    if uvs is None:
        raise ValueError("the mesh carries no UVs (no `vt` in the file): unwrap it with data_gen.unwrap.smart_unwrap "
                         "(`--uv_unwrap smart`, or python -m nlt_amd.data_gen.unwrap_main) and pass that table")
    table, loop = {}, 0
    for fi, (f, uv) in enumerate(zip(faces, uvs)):
        table[fi] = [[loop + k, int(vi), float(uv[k, 0]), float(uv[k, 1])] for k, vi in enumerate(f)]
        loop += len(f)
    return table


def dense_unwrap(cached_unwrap):
    """The dict table as the dense form `calc_bidir_mapping` also takes: {'uv': float64 [F,Vmax,2], 'counts': int64 [F]}."""
    n = max(cached_unwrap) + 1
    counts = np.zeros(n, np.int64)
    for f, rows in cached_unwrap.items():
        counts[f] = len(rows)
    uv = np.zeros((n, int(counts.max()), 2), np.float64)
    for f, rows in cached_unwrap.items():
        uv[f, :len(rows)] = np.asarray(rows, np.float64)[:, 2:]
    return {'uv': uv, 'counts': counts}


def euler_xyz_matrix(rotation):
    """Blender's 'XYZ' Euler angles (radians) -> the 3 x 3 rotation Rz . Ry . Rx."""
    x, y, z = (float(a) for a in rotation)
    cx, sx, cy, sy, cz, sz = np.cos(x), np.sin(x), np.cos(y), np.sin(y), np.cos(z), np.sin(z)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


def safe_cast_to_int(x):
    if x != int(x):
        raise ValueError("failed to safely cast %f to an integer" % x)
    return int(x)


def camera_matrix(cam, imh):
    """get_camera_matrix(keep_disparity=True) (camera.py:257-395) for a cam.json: horizontal sensor fit, square pixels, 100 %
    scale; imw as data_gen/render.py:119-121.  Returns (the 4 x 4 world -> (x d, y d, d, 1) matrix, its inverse, (imh, imw))."""
    cam = _params(cam)
    imw = safe_cast_to_int(imh / cam['sensor_height'] * cam['sensor_width'])
    f, sw, sh = float(cam['focal_length']), float(cam['sensor_width']), float(cam['sensor_height'])
    s_x, s_y = imw / sw, imh / sh
    int_mat = np.array([[s_x * f, 0, imw / 2, 0], [0, s_y * f, imh / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
    t = np.asarray(cam['position'], np.float64)
    world2cam = euler_xyz_matrix(cam['rotation']).T
    cam2cv = np.diag([1.0, -1.0, -1.0])
    ext = np.eye(4)
    ext[:3, :3] = cam2cv @ world2cam
    ext[:3, 3] = cam2cv @ (world2cam @ -t)
    mat = int_mat @ ext
    return mat, np.linalg.inv(mat), (int(imh), imw)


def backproject(mesh, cam, imh):
    """backproject_to_3d for every pixel -> the dense intersect of data_gen/render.py ('locs', 'normals', 'valid' on the device,
    'face_i' on the host as `calc_bidir_mapping` reads it, 'hw')."""
    cam = _params(cam)
    _, inv, (imh, imw) = camera_matrix(cam, imh)
    locs, normals, valid, face_i = C.raycast_camera(*mesh.bvh, mesh.n_tris, mesh._tri2face, inv.reshape(-1), cam['position'], imh, imw)
    return {'locs': locs, 'normals': normals, 'valid': valid, 'face_i': face_i.cpu().numpy(), 'hw': (imh, imw)}


def shadow(mesh, light, intersect):
    """Fills intersect['occluded'] (uint8 [P]) from shadow rays of the light.json `light`; returns intersect."""
    light = _params(light)
    intersect['occluded'] = C.raycast_shadow(*mesh.bvh, mesh.n_tris, intersect['locs'], intersect['valid'], light['position'])
    return intersect


def render_geometry(mesh, cached_unwrap, cam, light, imh, uvs, rgb_camspc=None, alpha=None):
    """Every buffer of a sample for a camera and a light the capture does not hold: both ray casts, then `render_sample` with
    alpha = 255 * valid (the binary hit mask; Cycles' anti-aliased alpha is out of scope) unless an `alpha` [imh,imw] uint8 is
    given (data_gen/shade.py passes the supersampled coverage).  rgb_camspc = None: a complete test sample for `write_sample`."""
    cam, light = _params(cam), _params(light)
    intersect = shadow(mesh, light, backproject(mesh, cam, imh))
    if alpha is None:
        alpha = (intersect['valid'] * 255).view(intersect['hw'])
    return render_sample(intersect, cached_unwrap, cam, light, uvs, rgb_camspc=rgb_camspc, alpha=alpha)
