"""CPU: the ray-cast reference (tests/raycast_ref.py) against analytic scenes, the mesh loaders on the two fixtures of
tests/golden, the camera matrix, the dense unwrap table of calc_bidir_mapping against the dict form (on the emulated adapters the
capture-writer test uses), and the argument checks of every entry of csrc/raycast.hip (nothing is launched)."""
import numpy as np
import pytest
import torch

import capture_ref
import fake_capi
import raycast_ref as R
from nlt_amd import capi as C
from nlt_amd.data_gen import mesh as M
from nlt_amd.data_gen import render as RD


# ---------------------------------------------------------------- the reference against analytic scenes
def test_unit_square_under_vertical_rays():
    tv = np.array([[[0, 0, 0], [1, 0, 0], [1, 1, 0]], [[0, 0, 0], [1, 1, 0], [0, 1, 0]]], np.float64)
    g = (np.arange(8) + 0.5) / 8
    xs, ys = np.meshgrid(g, g + 0.01)                               # (off the diagonal, which both triangles share)
    o = np.stack((xs.ravel(), ys.ravel(), np.full(64, 2.5)), 1)
    o = np.concatenate((o, [[1.5, 0.5, 2.5], [-0.1, 0.2, 2.5]]))    # two rays beside the square
    d = np.tile([0.0, 0.0, -1.0], (len(o), 1))
    t, tri, face = R.closest(o, d, tv, tri2face=np.array([7, 7], np.int32))
    assert np.array_equal(t[:64], np.full(64, 2.5)) and np.all(np.isinf(t[64:])) and np.array_equal(tri[64:], [-1, -1])
    assert np.array_equal(tri[:64], (o[:64, 1] > o[:64, 0]).astype(np.int32)) and np.array_equal(face[:64], np.full(64, 7))
    assert np.array_equal(face[64:], [-1, -1])
    # through the camera path: loc, normal
    cam = R.make_cam('C', (0.5, 0.5, 3.0), (0.5, 0.5, 0.0), sensor_width=32.0, sensor_height=24.0, up=(0.0, 1.0, 0.0))
    _, inv, (imh, imw) = M.camera_matrix(cam, 6)
    x = R.backproject(tv, None, inv, cam['position'], imh, imw)
    hit = x['valid'] > 0
    assert hit.any() and np.abs(x['locs'][hit][:, 2]).max() < 1e-14 and np.array_equal(x['normals'][hit], np.tile([0.0, 0.0, 1.0], (hit.sum(), 1)))
    assert np.array_equal(x['locs'][~hit], np.zeros(((~hit).sum(), 3))) and np.array_equal(x['face_i'][~hit], np.full((~hit).sum(), -1))


def test_icosphere_hits_lie_within_the_chord_error():
    v, f = R.icosphere(2)
    assert len(f) == 320
    tv = v[f]
    n = R.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0])
    inradius = np.abs(R.dot(n / np.linalg.norm(n, axis=1, keepdims=True), tv[:, 0])).min()
    o, d = R.rays_into(500, 3, lo=-0.3, hi=0.3)
    t, tri, _ = R.closest(o, d, tv)
    assert (tri >= 0).all()
    r = np.linalg.norm(o + t[:, None] * d, axis=1)
    assert r.max() <= 1 + 1e-12 and r.min() >= inradius - 1e-12 and inradius > 0.95


def test_degenerate_triangles_and_parallel_rays_miss():
    tv = np.array([[[0, 0, 0], [0, 0, 0], [0, 0, 0]],                           # a point
                   [[0, 0, 0], [0.25, 0.5, 0.125], [0.5, 1.0, 0.25]],           # collinear, e2 = 2 e1
                   [[0, 0, 1], [1, 0, 1], [0, 1, 1]]], np.float64)              # a real one at z = 1
    assert np.array_equal(R.degenerate(tv), [True, True, False])
    o = np.array([[0.0, 0.0, 5.0], [0.5, 1.0, 5.0], [0.2, 0.2, 1.0], [0.2, 0.2, 5.0]])
    d = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])   # ray 2 lies in the plane z = 1
    t, tri, _ = R.closest(o, d, tv[:2])
    assert np.all(np.isinf(t)) and np.array_equal(tri, [-1] * 4)
    t, tri, _ = R.closest(o, d, tv)
    assert np.array_equal(tri, [2, -1, -1, 2]) and np.array_equal(t[[0, 3]], [4.0, 4.0])


# ---------------------------------------------------------------- loaders
def test_bunny_ply_ascii_and_binary(tmp_path):
    b = M.load_mesh(R.BUNNY)
    assert b['vertices'].shape == (453, 3) and b['vertices'].dtype == np.float64 and len(b['faces']) == 948 and b['loop_uvs'] is None
    assert all(len(f) == 3 for f in b['faces']) and b['faces'][-3] == [409, 412, 410] and b['faces'][-1] == [435, 423, 430]
    assert np.array_equal(b['vertices'][0], np.array([-0.0312216, 0.126304, 0.00514924], np.float32).astype(np.float64))
    for binary in (True, False):
        path = str(tmp_path / ('b%d.ply' % binary))
        M.write_ply(path, b['vertices'], b['faces'], binary=binary)
        again = M.load_mesh(path)
        assert np.array_equal(again['vertices'], b['vertices']) and again['faces'] == b['faces']
    # polygons of any length, extra properties and another element, binary
    path = str(tmp_path / 'poly.ply')
    with open(path, 'wb') as h:
        h.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty double x\nproperty double y\nproperty double z\n"
                b"property uchar red\nelement face 2\nproperty list uchar int vertex_indices\nproperty float quality\nend_header\n")
        pts = np.arange(15, dtype=np.float64).reshape(5, 3) / 7
        for p in pts:
            h.write(p.astype('<f8').tobytes() + b'\x09')
        h.write(b'\x05' + np.array([0, 1, 2, 3, 4], '<i4').tobytes() + np.float32(1).tobytes())
        h.write(b'\x03' + np.array([4, 2, 0], '<i4').tobytes() + np.float32(2).tobytes())
    p = M.load_mesh(path)
    assert np.array_equal(p['vertices'], pts) and p['faces'] == [[0, 1, 2, 3, 4], [4, 2, 0]]


def test_cube_obj_triangulation_and_unwrap(tmp_path):
    c = M.load_mesh(R.CUBE)
    assert c['vertices'].shape == (8, 3) and [len(f) for f in c['faces']] == [4] * 6
    assert c['faces'][0] == [0, 1, 2, 3] and c['faces'][1] == [4, 7, 6, 5]
    m = M.Mesh(c['vertices'], c['faces'], device=None, loop_uvs=c['loop_uvs'])
    assert m.n_tris == 12 and np.array_equal(m.tri2face, np.repeat(np.arange(6), 2))
    assert np.array_equal(m.tris[:4], [[0, 1, 2], [0, 2, 3], [4, 7, 6], [4, 6, 5]])
    table = M.unwrap_from_obj(m)
    assert table[0] == [[0, 0, 0.0, 0.0], [1, 1, 1.0, 0.0], [2, 2, 1.0, 1.0], [3, 3, 0.0, 1.0]]      # the file's own comment
    assert table[1] == [[4, 4, 0.0, 0.0], [5, 7, 0.0, 0.0], [6, 6, 0.0, 0.0], [7, 5, 0.0, 0.0]]      # (faces without vt: (0, 0))
    assert sorted(table) == list(range(6))
    with pytest.raises(ValueError, match='no UVs'):
        M.unwrap_from_obj(M.load_mesh(R.BUNNY))
    # v, v/vt, v/vt/vn, negative indices; the world matrix on the host
    path = str(tmp_path / 'n.obj')
    with open(path, 'w') as h:
        h.write("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0.25 0.5\nvt 0.75 0.5\nvt 0.5 1\nf -4 -3 -2\nf 1/1 3/2 4/3\nf 1/1/1 2/2/1 3/3/1 4/1/1\n")
    n = M.load_mesh(path)
    assert n['faces'] == [[0, 1, 2], [0, 2, 3], [0, 1, 2, 3]] and np.array_equal(n['loop_uvs'][1], [[0.25, 0.5], [0.75, 0.5], [0.5, 1.0]])
    world = np.array([[0, -2, 0, 5], [2, 0, 0, 6], [0, 0, 2, 7], [0, 0, 0, 1]], np.float64)
    mw = M.Mesh(n['vertices'], n['faces'], world, device=None)
    assert np.array_equal(mw.vertices, [[5, 6, 7], [5, 8, 7], [3, 8, 7], [3, 6, 7]]) and mw.n_tris == 4


# ---------------------------------------------------------------- camera matrix
def test_camera_matrix():
    c = M.load_mesh(R.BUNNY)['vertices'].mean(0)
    cam = R.bunny_cam()
    mat, inv, (imh, imw) = M.camera_matrix(cam, 48)
    assert (imh, imw) == (48, 64) and np.abs(mat @ inv - np.eye(4)).max() < 1e-12
    p = mat @ np.append(c, 1.0)
    assert np.abs(p[:2] / p[2] - (imw / 2, imh / 2)).max() < 1e-9 and p[2] > 0
    assert M.camera_matrix(dict(cam, sensor_width=36.0), 48)[2] == (48, 72)
    with pytest.raises(ValueError):
        M.camera_matrix(dict(cam, sensor_width=35.0), 48)               # 70.0 is fine, 48 / 24 * 35.1 is not
        M.camera_matrix(dict(cam, sensor_width=35.1), 48)
    # the reference's hits project back onto their pixels
    b = M.load_mesh(R.BUNNY)
    m = M.Mesh(b['vertices'], b['faces'], device=None)
    x = R.backproject(m.tri_verts, m.tri2face, inv, cam['position'], imh, imw)
    hit = x['valid'] > 0
    assert 0.2 < hit.mean() < 0.9
    q = np.concatenate((x['locs'][hit], np.ones((hit.sum(), 1))), 1) @ mat.T
    xs, ys = np.meshgrid(np.arange(imw), np.arange(imh))
    want = np.stack((xs.ravel(), ys.ravel()), 1)[hit]
    assert np.abs(q[:, :2] / q[:, 2:3] - want).max() < 1e-9
    # Blender's 'XYZ' Euler order: Rz . Ry . Rx
    r = M.euler_xyz_matrix([0.3, -0.7, 1.9])
    assert np.abs(r @ r.T - np.eye(3)).max() < 1e-15 and abs(r[2, 0] - np.sin(0.7)) < 1e-15


# ---------------------------------------------------------------- dense unwrap table
@pytest.mark.parametrize('which', ['cube', 'bunny'])
def test_dense_unwrap_table_equals_the_dict_form(monkeypatch, which):
    fake_capi.install(monkeypatch)
    capture_ref.install(monkeypatch)
    if which == 'cube':
        m = M.Mesh.load(R.CUBE, device=None)
        table = M.unwrap_from_obj(m)
        for f in range(1, 6):                                           # (give the faces without vt a chart of their own)
            table[f] = [[r[0], r[1], (f % 3 + u) / 3, (f // 3 + v) / 2] for r, (u, v) in zip(table[f], [(0.1, 0.1), (0.9, 0.1), (0.9, 0.9), (0.1, 0.9)])]
        cam, imh, uvs = R.make_cam('Q', (3.0, -4.0, 2.5), (0.0, 0.0, 0.0), sensor_width=35.0, sensor_height=25.0), 5, 8
    else:
        m = M.Mesh.load(R.BUNNY, device=None)
        table, cam, imh, uvs = R.grid_unwrap(948), R.bunny_cam(), 24, 32
    _, inv, (imh, imw) = M.camera_matrix(cam, imh)
    x = R.backproject(m.tri_verts, m.tri2face, inv, cam['position'], imh, imw)
    assert (x['face_i'] >= 0).sum() > 5
    inter = {'face_i': x['face_i'], 'valid': torch.from_numpy(x['valid'])}
    xs, ys = np.meshgrid(range(imw), range(imh))
    xys = np.dstack((xs, ys)).reshape(-1, 2)
    dense = M.dense_unwrap(table)
    assert dense['uv'].shape == (len(table), 4 if which == 'cube' else 3, 2)
    a = RD.calc_bidir_mapping(table, None, xys, inter, uvs)
    b = RD.calc_bidir_mapping(dense, None, xys, inter, uvs)
    for p, q in zip(a, b):
        assert p.dtype == q.dtype == torch.float64 and p.shape == q.shape and p.numpy().tobytes() == q.numpy().tobytes()
    assert float(a[0].abs().sum()) > 0 and float(a[1].abs().sum()) > 0


# ---------------------------------------------------------------- argument checks: answered before any launch
def test_bad_arguments_return_status_codes_without_a_gpu():
    L = C.lib()
    n, p, big = None, 4096, 1 << 31                                     # (p: a non-null fake pointer, checked, never dereferenced)
    assert [L.nlt_bvh_tris_doubles(x) for x in (0, -3, big, 1, 4, 5, 1000)] == [-1, -1, -1, 40, 40, 80, 256 * 40]
    assert [L.nlt_bvh_nodes_doubles(x) for x in (0, -3, big, 1, 4, 5, 1000)] == [-1, -1, -1, 6, 6, 18, 511 * 6]
    assert L.nlt_bvh_morton(n, 4, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, n, n) == -1
    assert L.nlt_bvh_morton(p, 0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, p, n) == -1
    assert L.nlt_bvh_morton(p, big, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, p, n) == -2
    assert L.nlt_bvh_build(n, n, 5, n, 80, n, 18, n) == -1
    assert L.nlt_bvh_build(p, p, 0, p, 80, p, 18, n) == -1 and L.nlt_bvh_build(p, p, -1, p, 80, p, 18, n) == -1
    assert L.nlt_bvh_build(p, p, 5, p, 79, p, 18, n) == -1 and L.nlt_bvh_build(p, p, 5, p, 80, p, 17, n) == -1
    assert L.nlt_bvh_build(p, p, big, p, 1 << 40, p, 1 << 40, n) == -2
    assert L.nlt_raycast(n, n, 5, n, n, n, 7, n, n, n, n) == -1
    assert L.nlt_raycast(p, p, 0, n, p, p, 7, p, p, p, n) == -1 and L.nlt_raycast(p, p, 5, n, p, p, -1, p, p, p, n) == -1
    assert L.nlt_raycast(p, p, 5, n, p, p, 0, p, p, p, n) == -1
    assert L.nlt_raycast(p, p, big, n, p, p, 7, p, p, p, n) == -2 and L.nlt_raycast(p, p, 5, n, p, p, big, p, p, p, n) == -2
    assert L.nlt_raycast_camera(n, n, 5, n, n, 4, 4, n, n, n, n, n) == -1
    assert L.nlt_raycast_camera(p, p, 0, n, p, 4, 4, p, p, p, p, n) == -1 and L.nlt_raycast_camera(p, p, 5, n, p, 0, 4, p, p, p, p, n) == -1
    assert L.nlt_raycast_camera(p, p, 5, n, p, 4, -4, p, p, p, p, n) == -1
    assert L.nlt_raycast_camera(p, p, big, n, p, 4, 4, p, p, p, p, n) == -2 and L.nlt_raycast_camera(p, p, 5, n, p, 40000, 40000, p, p, p, p, n) == -2
    assert L.nlt_raycast_shadow(n, n, 5, n, n, 16, 0.0, 0.0, 1.0, n, n) == -1
    assert L.nlt_raycast_shadow(p, p, 0, p, p, 16, 0.0, 0.0, 1.0, p, n) == -1 and L.nlt_raycast_shadow(p, p, 5, p, p, -16, 0.0, 0.0, 1.0, p, n) == -1
    assert L.nlt_raycast_shadow(p, p, big, p, p, 16, 0.0, 0.0, 1.0, p, n) == -2 and L.nlt_raycast_shadow(p, p, 5, p, p, big, 0.0, 0.0, 1.0, p, n) == -2
