"""-m gpu: csrc/raycast.hip against the float64 brute force of tests/raycast_ref.py, BIT FOR BIT -- t, tri, face, locs, normals,
valid and occluded, misses included.  Every scene is a legal one for which the brute force is well defined: tree shapes from one
leaf to padded power-of-two trees, exact ties on shared edges and duplicate triangles, zero-thickness boxes with +0 / -0 /
denormal direction components, degenerate triangles and a far vertex, the camera and shadow forms on the two mesh fixtures, and the
path from a mesh file to Model.call."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import nlt_amd
import raycast_ref as R
from nlt_amd import capi as C
from nlt_amd.data_gen import mesh as M
from nlt_amd.data_gen import render as RD

pytestmark = pytest.mark.gpu

N_RAYS = 4099                                                           # not a multiple of 64 or 256


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same(got, want, what=''):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.nonzero(bits(got).reshape(-1) != bits(want).reshape(-1))[0]
    assert bad.size == 0, "%s: %d element(s) differ, first at %d: %r != %r" % (what, bad.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def soup_mesh(tv, tri2face=None):
    """A Mesh straight from triangles [T,3,3] (each its own face unless tri2face says otherwise)."""
    m = M.Mesh(tv.reshape(-1, 3), np.arange(tv.shape[0] * 3).reshape(-1, 3), device='cuda')
    assert np.array_equal(m.tri_verts, tv)
    if tri2face is not None:
        m.tri2face = np.asarray(tri2face, np.int32)
        m._tri2face = torch.from_numpy(m.tri2face).cuda()
    return m


def check_cast(tv, o, d, tri2face=None, what=''):
    m = soup_mesh(tv, tri2face)
    t, tri, face = m.raycast(o, d)
    wt, wtri, wface = R.closest(o, d, tv, tri2face)
    same(t, wt, what + ' t'); same(tri, wtri, what + ' tri'); same(face, wface, what + ' face')
    return wt, wtri


# ---------------------------------------------------------------- tree shape
@pytest.mark.parametrize('n', [1, 3, 4, 5, 8, 9, 17, 1000])
def test_tree_shapes_and_permutation(n):
    tv = R.soup(n, seed=n)
    o, d = R.rays_into(N_RAYS, seed=100 + n)
    wt, wtri = check_cast(tv, o, d, what='soup %d' % n)
    assert (wtri >= 0).any() and (n > 17 or (wtri < 0).any())
    perm = np.random.default_rng(n).permutation(n)
    t, tri, _ = soup_mesh(tv[perm]).raycast(o, d)
    same(t, wt, 'permuted t')
    tri = tri.cpu().numpy()
    same(np.where(tri >= 0, perm[np.maximum(tri, 0)], -1).astype(np.int32), wtri, 'un-permuted tri')


# ---------------------------------------------------------------- ties
def test_shared_edges_and_duplicate_triangles():
    a = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    b = [[1, 0, 0], [1, 1, 0], [0, 1, 0]]
    pair = np.array([a, b], np.float64)
    targets = np.array([[0.5, 0.5, 0], [1, 0, 0], [0, 1, 0], [0.25, 0.25, 0], [0.75, 0.75, 0], [0.25, 0.75, 0], [0.625, 0.375, 0],
                        [0.2, 0.3, 0], [0.9, 0.8, 0], [1.5, 0.5, 0]], np.float64)
    origins = np.array([[0.5, 0.5, 2.0], [0.3, 0.2, 2.0], [-1.0, 3.0, 1.5], [0.5, 0.5, -1.0]])
    o = np.repeat(origins, len(targets), 0)
    d = np.tile(targets, (len(origins), 1)) - o                       # directions as given (not normalised) ...
    o, d = np.concatenate((o, o)), np.concatenate((d, R.unit_towards(o, o + d)[0]))        # ... and normalised
    wt, wtri = check_cast(pair, o, d, what='pair')
    assert (wtri[:len(targets)][[3, 4, 7, 8]] >= 0).all() and wtri[9] == -1
    # the pair twice: every triangle has an exact duplicate at a higher index, which must never win
    wt2, wtri2 = check_cast(np.concatenate((pair, pair)), o, d, tri2face=[5, 6, 7, 8], what='duplicated pair')
    same(wt2, wt); same(wtri2, wtri)
    _, wtri3 = check_cast(np.concatenate((pair[::-1], R.soup(9, 5) + [0, 0, 4.0], pair)), o, d, what='duplicates across leaves')
    assert (wtri3[wtri >= 0] < 2).all()                               # (the duplicates at 11, 12 sit in another leaf)


# ---------------------------------------------------------------- boxes
def _quad(axis, c=0.5):
    """Two triangles of the unit square in the plane x[axis] = c."""
    b, k = [i for i in range(3) if i != axis]
    p = np.full((4, 3), c)
    p[:, b] = [0, 1, 1, 0]
    p[:, k] = [0, 0, 1, 1]
    return np.array([[p[0], p[1], p[2]], [p[0], p[2], p[3]]])


def _box_rays():
    o, d = [], []
    grid = [0.0, 0.25, 0.5, 1.0]
    for axis in range(3):
        b, k = [i for i in range(3) if i != axis]
        for u in grid:
            for v in grid:
                tgt = np.full(3, 0.5)
                tgt[b], tgt[k] = u, v
                for sign in (1.0, -1.0):
                    for zero in (0.0, -0.0, 5e-324, -5e-324):
                        dd = np.full(3, zero)
                        dd[axis] = -sign
                        for dist in (2.0, 0.25, 0.0):                   # outside, inside the mesh box, on the triangle (t = 0)
                            oo = tgt.copy()
                            oo[axis] += sign * dist
                            o.append(oo); d.append(dd)
                # rays lying in the plane of the quad (and of its zero-thickness box)
                for bb in (b, k):
                    for sign in (1.0, -1.0):
                        oo, dd = tgt.copy(), np.zeros(3)
                        oo[bb] += 2 * sign
                        dd[bb] = -sign
                        o.append(oo); d.append(dd)
    # through the corners of the boxes, diagonally and in a face
    for corner in ([0, 0, 0.5], [1, 1, 0.5], [0.5, 0, 1], [0.5, 1, 1], [1, 0.5, 0], [0, 0.5, 1], [0, 0, 0], [1, 1, 1]):
        for dd in ([-1, -1, -1], [1, 1, 1], [-1, -1, 0], [0, -1, -1], [-1, 0, -1], [1, -1, 0], [-1, 2, -0.5]):
            dd = np.array(dd, np.float64)
            o.append(np.array(corner, np.float64) - 2 * dd); d.append(dd)
    return np.array(o), np.array(d)


@pytest.mark.parametrize('scene', ['x', 'y', 'z', 'xyz', 'xyz+soup'])
def test_flat_boxes_zero_components_and_grazing_rays(scene):
    o, d = _box_rays()
    tv = np.concatenate([_quad('xyz'.index(c)) for c in scene.split('+')[0]])
    if scene.endswith('soup'):
        tv = np.concatenate((tv, R.soup(40, 9)))
    wt, wtri = check_cast(tv, o, d, what=scene)
    assert (wt == 0).any() and (wt == 2).any() and (wtri < 0).any()


# ---------------------------------------------------------------- degenerate input
def test_degenerate_triangles_and_a_far_vertex():
    tv = R.soup(203, seed=7, degenerates=True)
    assert R.degenerate(tv).sum() == 41
    o, d = R.rays_into(N_RAYS, seed=8)
    far = tv[1]
    w = np.random.default_rng(2).dirichlet((1, 1, 1), 64)              # rays at points of the triangle with the far vertex
    o2 = np.tile([0.5, 0.5, 3.0], (64, 1))
    d2, _ = R.unit_towards(o2, w @ far)
    wt, wtri = check_cast(tv, np.concatenate((o, o2)), np.concatenate((d, d2)), what='degenerate soup')
    assert not np.isin(wtri, np.nonzero(R.degenerate(tv))[0]).any() and (wtri == 1).any()
    # only degenerate triangles: nothing to hit
    t, tri, face = soup_mesh(tv[R.degenerate(tv)]).raycast(o, d)
    same(t, np.full(N_RAYS, np.inf)); same(tri, np.full(N_RAYS, -1, np.int32)); same(face, np.full(N_RAYS, -1, np.int32))


def test_all_miss_launch():
    tv = R.soup(17, seed=3)
    o, d = R.rays_into(N_RAYS, seed=4)
    t, tri, face = soup_mesh(tv).raycast(o, -d)
    same(t, np.full(N_RAYS, np.inf)); same(tri, np.full(N_RAYS, -1, np.int32)); same(face, np.full(N_RAYS, -1, np.int32))
    same(t, R.closest(o, -d, tv)[0])


# ---------------------------------------------------------------- camera
def _check_camera(mesh, cam, imh):
    got = M.backproject(mesh, cam, imh)
    _, inv, (imh, imw) = M.camera_matrix(cam, imh)
    want = R.backproject(mesh.tri_verts, mesh.tri2face, inv, cam['position'], imh, imw)
    assert got['hw'] == (imh, imw)
    for k in ('locs', 'normals', 'valid', 'face_i'):
        same(got[k], want[k], k)
    return got, want


@pytest.fixture(scope='module')
def bunny():
    return M.Mesh.load(R.BUNNY)


def test_camera_bunny(bunny):
    _, want = _check_camera(bunny, R.bunny_cam(), 48)
    assert want['hw'] == (48, 64) and 0.2 < want['valid'].mean() < 0.9
    _, half = _check_camera(bunny, R.bunny_cam('B02', aim=(0.09, 0.0, 0.0)), 48)        # the mesh half out of frame
    cols = np.nonzero(half['valid'].reshape(48, 64).any(0))[0]
    assert half['valid'].any() and (cols.min() == 0 or cols.max() == 63) and half['valid'].sum() < want['valid'].sum()


def test_camera_cube_polygons():
    cube = M.Mesh.load(R.CUBE)
    cam = R.make_cam('Q', (3.0, -4.0, 2.5), (0.0, 0.0, 0.0), sensor_width=35.0, sensor_height=25.0)
    _, want = _check_camera(cube, cam, 5)
    assert want['hw'] == (5, 7) and want['valid'].any() and want['face_i'].max() <= 5 and len(set(want['face_i'][want['valid'] > 0])) >= 2


# ---------------------------------------------------------------- shadow
def _check_shadow(mesh, inter, light):
    got = M.shadow(mesh, dict(name='L', position=list(light)), dict(inter))['occluded']
    want = R.shadow(mesh.tri_verts, inter['locs'].cpu().numpy(), inter['valid'].cpu().numpy(), light)
    same(got, want, 'occluded')
    return want


def test_shadow_of_one_quad_on_another():
    lower = [[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]]
    upper = [[-0.5, -0.5, 1], [0.5, -0.5, 1], [0.5, 0.5, 1], [-0.5, 0.5, 1]]
    mesh = M.Mesh(np.array(lower + upper, np.float64), [[0, 1, 2, 3], [4, 5, 6, 7]])
    cam = R.make_cam('S', (3.0, -4.0, 6.0), (0.0, 0.0, 0.0), sensor_width=32.0, sensor_height=24.0)
    inter, want = _check_camera(mesh, cam, 36)
    light = (0.1, 0.2, 5.0)
    occ = _check_shadow(mesh, inter, light)
    locs, face = want['locs'], want['face_i']
    q = np.asarray(light) + (locs - light) * (4.0 / 5.0)                # where light -> loc crosses z = 1 (for the lower quad)
    under = (np.abs(q[:, 0]) < 0.49) & (np.abs(q[:, 1]) < 0.49)
    clear = (np.abs(q[:, 0]) > 0.51) | (np.abs(q[:, 1]) > 0.51)
    assert (face == 0).sum() > 50 and (face == 1).sum() > 5 and ((face == 0) & under).sum() > 3
    assert occ[(face == 0) & under].all() and not occ[(face == 0) & clear].any() and not occ[face == 1].any() and not occ[face < 0].any()


def test_shadow_bunny_self_shadow_and_isclose(bunny):
    inter, want = _check_camera(bunny, R.bunny_cam(), 48)
    c = bunny.vertices.mean(0)
    light = c + (0.4, 0.1, 0.05)                                        # from the side: part of what the camera sees is in shadow
    occ = _check_shadow(bunny, inter, light)
    v = want['valid'] > 0
    assert 0.05 < occ[v].mean() < 0.95
    # lit pixels whose shadow ray ends within isclose of the full distance but not bit-equal to it
    d, full = R.unit_towards(np.asarray(light), want['locs'])
    t = bunny.raycast(np.broadcast_to(light, d.shape)[v], d[v])[0].cpu().numpy()
    lit = occ[v] == 0
    assert (lit & (t != full[v]) & np.isfinite(t)).any()


# ---------------------------------------------------------------- end to end
def test_render_geometry_equals_render_sample_on_the_reference_intersect(bunny):
    cam, light = R.bunny_cam(), dict(name='L1', position=list(bunny.vertices.mean(0) + (0.3, -0.2, 0.3)))
    table = R.grid_unwrap(948)
    got = M.render_geometry(bunny, table, cam, light, 24, 32)
    dense = M.render_geometry(bunny, M.dense_unwrap(table), cam, light, 24, 32)
    _, inv, (imh, imw) = M.camera_matrix(cam, 24)
    assert (imh, imw) == (24, 32)
    x = R.backproject(bunny.tri_verts, bunny.tri2face, inv, cam['position'], imh, imw)
    x['occluded'] = R.shadow(bunny.tri_verts, x['locs'], x['valid'], light['position'])
    inter = {k: (v if k in ('face_i', 'hw') else torch.from_numpy(v).cuda()) for k, v in x.items()}
    want = RD.render_sample(inter, table, cam, light, 32, alpha=torch.from_numpy((x['valid'] * 255).reshape(imh, imw)).cuda())
    assert set(got) == set(want) == set(dense) and 'rgb.png' not in got and x['occluded'].any()
    for k, w in want.items():
        same(got[k], w.cpu().numpy(), k); same(dense[k], w.cpu().numpy(), k + ' (dense table)')
    assert tuple(got['cvis.png'].shape) == (32, 32) and tuple(got['uv2cam.npy'].shape) == (24, 32, 2) and int(got['cvis.png'].max()) > 0


def test_mesh_to_model_call(bunny, tmp_path):
    """A few trainvali_* samples and one test_* sample written by the CLI at a camera not among them -> postprocess -> load_store
    -> Dataset(mode='test') -> Model.call(batch, 'test')."""
    from nlt_amd.data_gen import postproc, render_main
    from nlt_amd.datasets import nlt as D
    from nlt_amd.models import get_model_class
    from oracle import nlt_oracle as O
    root = str(tmp_path / 'capture')
    c = bunny.vertices.mean(0)
    cams = {'C1': R.bunny_cam('C1'), 'C2': R.bunny_cam('C2', offset=(-0.2, -0.1, 0.28)), 'C9': R.bunny_cam('C9', offset=(0.02, -0.25, 0.25))}
    lights = {n: dict(name=n, position=list(c + p), size=0.1) for n, p in (('L1', (0.3, -0.2, 0.3)), ('L2', (-0.3, 0.1, 0.3)), ('L9', (0.0, -0.3, 0.4)))}
    cam_nn, light_nn = {'C1': 'C2', 'C2': 'C1', 'C9': 'C1'}, {'L1': 'L2', 'L2': 'L1', 'L9': 'L2'}
    uvs, imh = 64, 24
    table = M.dense_unwrap(R.grid_unwrap(948))
    n = 0
    for cn in ('C1', 'C2'):
        for ln in ('L1', 'L2'):
            geo = M.render_geometry(bunny, table, cams[cn], lights[ln], imh, uvs)
            rgb = geo['lvis_camspc.png'].unsqueeze(-1).expand(-1, -1, 3).contiguous()      # "ground truth": the quantised light cosines
            sample = M.render_geometry(bunny, table, cams[cn], lights[ln], imh, uvs, rgb_camspc=rgb)
            RD.write_sample(os.path.join(root, 'trainvali_%09d_%s_%s' % (n, cn, ln)), sample, cams[cn], lights[ln], (cam_nn, light_nn))
            n += 1
    files = {}
    for name, obj in (('C9', cams['C9']), ('L9', lights['L9']), ('cam_nn', cam_nn), ('light_nn', light_nn)):
        files[name] = str(tmp_path / (name + '.json'))
        with open(files[name], 'w') as h:
            json.dump(obj, h)
    with open(str(tmp_path / 'unwrap.pickle'), 'wb') as h:
        pickle.dump(R.grid_unwrap(948), h)
    test_dir = os.path.join(root, 'test_000000000_C9_L9')
    written = render_main.main(['--mesh', R.BUNNY, '--uv_unwrap', str(tmp_path / 'unwrap.pickle'), '--cam_json', files['C9'], '--light_json',
                                files['L9'], '--cam_nn_json', files['cam_nn'], '--light_nn_json', files['light_nn'], '--imh', str(imh), '--uvs',
                                str(uvs), '--outdir', test_dir])
    assert 'cvis.png' in written and 'rgb.png' not in written and os.path.exists(os.path.join(test_dir, 'nn.json'))
    postproc.postprocess(root)
    store = D.load_store(root, device='cuda')
    assert len(store['ids']) == 5 and all(store['complete'])
    kw = dict(depth=32, uvh=uvs, uvw=uvs, imh=imh, imw=32)
    cfg = nlt_amd.make_config(data_root=root, bs=1, **kw)
    ds = D.Dataset(cfg, 'test', store=store)
    assert ds.files == ['test_000000000_C9_L9']
    pm = get_model_class('nlt')(cfg)
    pm.load_weights(O.OracleModel(seed=3, **kw).numpy_weights())
    batch = ds.load_batch(ds.files)
    assert batch[7] == ['trainvali_000000001_C1_L2']
    pred_camspc = pm.call(batch, 'test')[0]
    torch.cuda.synchronize()
    assert tuple(pred_camspc.shape) == (1, imh, 32, 3) and bool(torch.isfinite(pred_camspc).all()) and float(pred_camspc.abs().sum()) > 0
