"""CPU: the unwrap's NumPy restatement (tests/unwrap_ref.py) and its host code (data_gen/unwrap.py: projection_basis,
pack_islands, the pickle, the argument checks, the CLI parsers) against closed forms and properties.  The restatement is what
csrc/unwrap.hip is held to bit for bit in tests/test_gpu_unwrap.py, so what is proved of it here carries over."""
import itertools
import os
import pickle

import numpy as np
import pytest

import unwrap_ref as R
from nlt_amd import capi as C
from nlt_amd.data_gen import capture_main as CM
from nlt_amd.data_gen import mesh as M
from nlt_amd.data_gen import render_main as RM
from nlt_amd.data_gen import unwrap as U
from nlt_amd.data_gen import unwrap_main as UM

MARGIN = 0.002
_cache = {}


def ref(name, angle=66., aw=0.):
    """One restatement run per (mesh, parameters), shared and left unchanged."""
    key = (name, angle, aw)
    if key not in _cache:
        verts, faces = MESHES[name]()
        _cache[key] = (np.asarray(verts, np.float64), faces, R.unwrap(verts, faces, angle, aw, MARGIN))
    return _cache[key]


def _ico(level):
    return lambda: tuple(a.tolist() if i else a for i, a in enumerate(R.icosphere(level)))


MESHES = {'cube': R.cube_mesh, 'bunny': R.bunny_mesh, 'ico0': _ico(0), 'ico1': _ico(1), 'ico2': _ico(2), 'tetra': R.tetrahedron,
          'grid': lambda: R.grid_mesh(5), 'folded': lambda: R.two_triangles(True), 'coplanar': lambda: R.two_triangles(False),
          'mixed': R.mixed_mesh}
PROPERTY_MESHES = ['bunny', 'ico0', 'ico1', 'ico2', 'cube']


# --------------------------------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize('angle', [1., 30., 66., 89.])
def test_cube_six_vectors_six_islands_and_large_charts(angle):
    verts, faces, r = ref('cube', angle)
    assert len(r['vectors']) == 6 and sorted(r['groups']) == list(range(6)) and len(r['island_labels']) == 6
    for f in range(6):
        assert np.allclose(r['vectors'][r['groups'][f]], r['unit'][f], rtol=0, atol=1e-14)
    assert sorted(r['labels']) == list(range(6))
    # three squares per shelf fit once (2 scale + 2 margin) <= 1/3, and one 0.97 step of slack is allowed: side >= 0.97 (1/3 - 2 margin)
    sides = (r['boxes'][:, 2:] - r['boxes'][:, :2]) * r['scale']
    assert 0.97 * (1 / 3 - 2 * MARGIN) >= 0.3 and sides.min() >= 0.3, sides


def test_regular_tetrahedron_has_four_groups():
    for angle in (1., 66., 89.):
        _, _, r = ref('tetra', angle)
        assert len(r['vectors']) == 4 and len(r['island_labels']) == 4


def test_flat_grid_is_one_island_and_an_exact_similarity():
    verts, faces, r = ref('grid')
    assert len(r['vectors']) == 1 and np.array_equal(r['vectors'][0], [0., 0., 1.]) and len(r['island_labels']) == 1
    assert set(r['labels']) == {0} and not r['rot'][0]
    xy = verts[np.array(faces)][..., :2]
    assert np.array_equal(r['uv'], (xy - xy.reshape(-1, 2).min(0)) * r['scale'] + r['offsets'][0])


def test_two_triangles_folded_and_coplanar():
    assert len(ref('folded')[2]['island_labels']) == 2 and len(ref('folded')[2]['vectors']) == 2
    assert len(ref('coplanar')[2]['island_labels']) == 1 and list(ref('coplanar')[2]['labels']) == [0, 0]


def test_tree_sum_is_the_stated_pairing():
    rng = np.random.default_rng(0)
    for n in (1, 2, 255, 256, 257, 70000):
        x = rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-8, 8, size=(n, 1))
        level = x
        while True:                                                 # the rule, written as scalar loops over one block at a time
            out = []
            for b in range(0, len(level), 256):
                blk = np.zeros((256, 3)); blk[:len(level[b:b + 256])] = level[b:b + 256]
                for s in (128, 64, 32, 16, 8, 4, 2, 1):
                    for i in range(s):
                        blk[i] = blk[i] + blk[i + s]
                out.append(blk[0])
            level = np.array(out)
            if len(level) == 1:
                break
        assert np.array_equal(R.tree_sum(x), level[0])


def test_ties_go_to_the_lowest_index_on_an_octahedron():
    verts, faces = R.octahedron()
    r = R.unwrap(verts, faces, 66., 0., MARGIN)
    # eight equal areas: face 0 seeds; its opposite face 6 is the one farthest away; then six faces tie at a dot of 1/3 (the sums
    # (p + p) - p, (p - p) + p and (-p + p) + p are all exactly p): the lowest index, 1, goes next
    assert r['seeds'][:3] == [0, 6, 1] and sorted(r['seeds']) == list(range(8))
    assert len(r['vectors']) == 8 and list(r['groups']) == [r['seeds'].index(f) for f in range(8)]


def test_degenerate_and_nan_faces_join_nothing():
    verts, faces = R.grid_mesh(2)
    verts = np.concatenate((verts, [[np.nan, 0, 0]]))
    faces = faces + [[0, 0, 1], [0, 1, len(verts) - 1], [0, 1]]
    r = R.unwrap(verts, faces, 66., 0., MARGIN)
    assert list(r['ok']) == [1] * 8 + [0, 0, 0] and list(r['groups'][8:]) == [-1] * 3 and list(r['labels'][8:]) == [-1] * 3
    assert not r['uv'][8:].any() and np.isfinite(r['uv']).all() and len(r['island_labels']) == 1


# --------------------------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize('name', PROPERTY_MESHES)
def test_uvs_lie_in_the_unit_square_and_boxes_keep_their_margin(name):
    _, faces, r = ref(name)
    assert r['uv'].min() >= 0.0 and r['uv'].max() <= 1.0
    wh = r['boxes'][:, 2:] - r['boxes'][:, :2]
    tw, th = np.where(r['rot'], wh[:, 1], wh[:, 0]) * r['scale'], np.where(r['rot'], wh[:, 0], wh[:, 1]) * r['scale']
    lo, hi = r['offsets'], r['offsets'] + np.stack((tw, th), 1)
    # every loop of an island lies in its placed box (to rounding), and two boxes are 2 margin apart on some axis (to rounding)
    for f in range(len(faces)):
        i = r['island'][f]
        uv = r['uv'][f, :r['counts'][f]]
        assert (uv >= lo[i] - 1e-12).all() and (uv <= hi[i] + 1e-12).all()
    gap_x = np.maximum(lo[:, None, 0] - hi[None, :, 0], lo[None, :, 0] - hi[:, None, 0])
    gap_y = np.maximum(lo[:, None, 1] - hi[None, :, 1], lo[None, :, 1] - hi[:, None, 1])
    gap = np.maximum(gap_x, gap_y)
    np.fill_diagonal(gap, np.inf)
    assert gap.min() >= 2 * MARGIN - 1e-12, gap.min()


def _uv_area(uv):
    a = 0.0
    for i in range(1, len(uv) - 1):
        e1, e2 = uv[i] - uv[0], uv[i + 1] - uv[0]
        a += 0.5 * (e1[0] * e2[1] - e1[1] * e2[0])
    return a


@pytest.mark.parametrize('name', PROPERTY_MESHES + ['mixed'])
def test_a_faces_uv_area_is_its_projected_area(name):
    """Signed: positive, because the charts are turned, never mirrored, and every face looks along its group's vector."""
    _, faces, r = ref(name)
    for f in range(len(faces)):
        want = r['scale'] ** 2 * r['area'][f] * float(R.dot(r['unit'][f], r['vectors'][r['groups'][f]]))
        got = _uv_area(r['uv'][f, :r['counts'][f]])
        assert want > 0 and abs(got - want) <= 1e-12 * want + 1e-18, (f, got, want)


def _overlap(a, b, eps=1e-12):
    """Separating-axis test of two convex polygons: True when their interiors overlap by more than eps."""
    for poly in (a, b):
        for i in range(len(poly)):
            e = poly[(i + 1) % len(poly)] - poly[i]
            axis = np.array([-e[1], e[0]])
            length = np.hypot(*axis)
            if length == 0:
                continue
            axis = axis / length
            pa, pb = a @ axis, b @ axis
            if pa.max() <= pb.min() + eps or pb.max() <= pa.min() + eps:
                return False
    return True


@pytest.mark.parametrize('name', ['cube', 'ico1'])
def test_no_two_faces_overlap_on_a_convex_mesh(name):
    _, faces, r = ref(name)
    polys = [r['uv'][f, :r['counts'][f]] for f in range(len(faces))]
    for i, j in itertools.combinations(range(len(polys)), 2):
        assert not _overlap(polys[i], polys[j]), (i, j)


def test_bunny_fill_groups_and_islands():
    _, _, r = ref('bunny')
    wh = r['boxes'][:, 2:] - r['boxes'][:, :2]
    fill = float((wh[:, 0] * wh[:, 1]).sum() * r['scale'] ** 2)
    print("bunny at (66, 0, 0.002): %d groups, %d islands, scale %.6f, box fill %.4f" % (len(r['vectors']), len(r['island_labels']), r['scale'], fill))
    assert fill >= 0.55


# --------------------------------------------------------------------------------------------------------------------- host code
def test_projection_basis_is_a_right_handed_orthonormal_frame():
    rng = np.random.default_rng(3)
    vecs = list(np.eye(3)) + list(-np.eye(3)) + [v / np.linalg.norm(v) for v in rng.normal(size=(50, 3))]
    for n in vecs:
        u, v = U.projection_basis(n)
        assert np.allclose([u @ u, v @ v, u @ v, u @ n, v @ n], [1, 1, 0, 0, 0], atol=1e-15) and np.allclose(np.cross(u, v), n, atol=1e-15)
    u, v = U.projection_basis([0., 0., 1.])
    assert np.array_equal(u, [1., 0., 0.]) and np.array_equal(v, [0., 1., 0.])


def test_pack_islands_turns_sorts_and_shelves():
    wh = np.array([[0.5, 1.0], [2.0, 1.0], [1.0, 1.0], [0.2, 0.1]])
    scale, rot, off = U.pack_islands(wh, [7, 3, 5, 9], 0.01)
    assert list(rot) == [True, False, False, False]
    # turned heights: 0.5, 1, 1, 0.1 -> order by height descending, ties to the lower label: 3 (label 3), 5, 7, 9
    tw, th = np.where(rot, wh[:, 1], wh[:, 0]) * scale, np.where(rot, wh[:, 0], wh[:, 1]) * scale
    assert np.allclose(off[1], (0.01, 0.01)) and (off >= 0.01 - 1e-15).all() and (off + np.stack((tw, th), 1) <= 0.99 + 1e-12).all()
    first = scale / min(1 / np.sqrt((wh[:, 0] * wh[:, 1]).sum()), 0.98 / 2.0)
    k = np.log(first) / np.log(0.97)
    assert abs(k - round(k)) < 1e-9 and round(k) >= 0
    assert off[2][0] > off[1][0] or off[2][1] > off[1][1]
    with pytest.raises(ValueError):
        U.pack_islands(wh, [0, 1, 2, 3], 0.5)
    with pytest.raises(ValueError, match='do not fit'):
        U.pack_islands(np.ones((90000, 2)), np.arange(90000), 0.002)


def test_pickle_round_trip_and_forced_extension(tmp_path):
    _, faces, r = ref('mixed')
    u = U.Unwrap(dense={'uv': r['uv'], 'counts': r['counts']}, faces=faces)
    table = u.table()
    path = U.write_unwrap(str(tmp_path / 'mixed_uv'), table)
    assert path.endswith('mixed_uv.pickle') and os.path.exists(path) and U.write_unwrap(path, table) == path
    with open(path, 'rb') as h:
        raw = pickle.load(h)
    back = U.read_unwrap(path)
    loop = 0
    for f, verts in enumerate(faces):
        assert isinstance(raw[f], np.ndarray) and raw[f].dtype == np.float64 and raw[f].shape == (len(verts), 4)
        assert list(raw[f][:, 0]) == list(range(loop, loop + len(verts))) and list(raw[f][:, 1]) == verts
        assert np.array_equal(back[f], table[f])
        loop += len(verts)
    dense = M.dense_unwrap(back)
    assert np.array_equal(dense['uv'], r['uv']) and np.array_equal(dense['counts'], r['counts'])


def test_argument_checks():
    verts, faces = R.cube_mesh()
    for bad in (0.5, 90., float('nan')):
        with pytest.raises(ValueError, match='angle_limit'):
            U.smart_unwrap(dict(vertices=verts, faces=faces), angle_limit=bad, device='cpu')
    with pytest.raises(ValueError, match='area_weight'):
        U.smart_unwrap(dict(vertices=verts, faces=faces), area_weight=1.5, device='cpu')
    with pytest.raises(ValueError, match='margin'):
        U.smart_unwrap(dict(vertices=verts, faces=faces), margin=0.5, device='cpu')
    with pytest.raises(ValueError, match='vertex outside'):
        U.mesh_arrays(dict(vertices=verts, faces=[[0, 1, 8]]))
    with pytest.raises(ValueError, match='no face'):
        U.mesh_arrays(dict(vertices=verts, faces=[]))
    v2, f2 = R.icosphere(2)
    with pytest.raises(ValueError, match='max_groups'):
        R.unwrap(v2, f2.tolist(), 1., 0., MARGIN, max_groups=256)
    with pytest.raises(ValueError, match='no UVs.*smart_unwrap'):
        M.unwrap_from_obj(dict(faces=faces, loop_uvs=None))


def test_cli_parsers(capsys):
    a = UM.parse_args(['--mesh', 'm.ply', '--outpath', 'u'])
    assert (a.angle_limit, a.area_weight, a.margin) == (89., 1., 0.002)
    a = UM.parse_args(['--mesh', 'm.ply', '--outpath', 'u', '--angle_limit', '66', '--area_weight', '0', '--margin', '0.01'])
    assert (a.angle_limit, a.area_weight, a.margin) == (66., 0., 0.01)
    with pytest.raises(SystemExit):
        UM.parse_args(['--mesh', 'm.ply', '--outpath', 'u', '--angle_limit', '90'])
    base = ['--mesh', 'm.ply', '--outroot', 'o']
    a = CM.parse_args(base + ['--uv_unwrap', 'smart'])
    assert (a.uv_unwrap, a.angle_limit, a.area_weight, a.margin) == ('smart', 89., 1., 0.002)
    a = CM.parse_args(base + ['--uv_unwrap', 'smart', '--angle_limit', '66', '--area_weight', '0.5', '--margin', '0.004'])
    assert (a.angle_limit, a.area_weight, a.margin) == (66., 0.5, 0.004)
    a = CM.parse_args(base + ['--uv_unwrap', 'u.pickle'])
    assert (a.uv_unwrap, a.angle_limit, a.area_weight, a.margin) == ('u.pickle', None, None, None)
    rbase = ['--mesh', 'm.ply', '--cam_json', 'c', '--light_json', 'l', '--cam_nn_json', 'cn', '--light_nn_json', 'ln', '--outdir', 'o']
    a = RM.parse_args(rbase + ['--uv_unwrap', 'smart', '--margin', '0.01'])
    assert (a.angle_limit, a.area_weight, a.margin) == (89., 1., 0.01)
    for parse, args in ((CM.parse_args, base), (RM.parse_args, rbase)):
        for flag in ('--angle_limit', '--area_weight', '--margin'):
            with pytest.raises(SystemExit):
                parse(args + ['--uv_unwrap', 'u.pickle', flag, '0.5'])
            assert 'smart only' in capsys.readouterr().err
        with pytest.raises(SystemExit):
            parse(args + ['--uv_unwrap', 'smart', '--angle_limit', '0.5'])


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    L, n, p, big = C.lib(), None, 4096, 1 << 31
    assert L.nlt_unwrap_workspace_bytes(0) == -1 and L.nlt_unwrap_workspace_bytes(big) == -1
    # 3 doubles per tree block on every level, then a (value, index) candidate per block of 256 faces
    assert L.nlt_unwrap_workspace_bytes(256) == (3 + 2) * 8 and L.nlt_unwrap_workspace_bytes(257) == (3 * 2 + 3 + 2 * 2) * 8
    assert L.nlt_unwrap_workspace_bytes(256 * 256 + 1) == (3 * 257 + 3 * 2 + 3 + 2 * 257) * 8
    assert L.nlt_unwrap_frames(n, 8, n, 24, n, 6, n, n, n, n, n) == -1 and L.nlt_unwrap_frames(p, 8, p, 24, p, 0, p, p, p, p, n) == -1
    assert L.nlt_unwrap_frames(p, big, p, 24, p, 6, p, p, p, p, n) == -2
    assert L.nlt_unwrap_seed(n, n, 6, n, n, 40, n, n) == -1 and L.nlt_unwrap_seed(p, p, 6, p, p, 39, p, n) == -1
    assert L.nlt_unwrap_gather(p, p, p, 6, 6, 0.8, 0.0, 1.0, p, 40, p, n) == -1 and L.nlt_unwrap_gather(p, p, p, 6, 0, 0.8, 0.0, 1.0, p, 39, p, n) == -1
    assert L.nlt_unwrap_farthest(p, p, p, p, 6, p, 1, p, 39, p, n) == -1 and L.nlt_unwrap_farthest(p, p, p, n, 6, p, 1, p, 40, p, n) == -1
    assert L.nlt_unwrap_assign(p, p, 6, p, 0, p, n) == -1 and L.nlt_unwrap_assign(p, p, big, p, 1, p, n) == -2
    assert L.nlt_unwrap_edge_keys(p, 0, p, 6, 8, p, p, n) == -1 and L.nlt_unwrap_islands_init(n, 6, p, n) == -1
    assert L.nlt_unwrap_islands_round(p, p, p, 24, p, 6, p, n, n) == -1
    assert L.nlt_unwrap_boxes(p, p, p, 24, p, p, 6, p, 1, p, p, 7, n) == -1 and L.nlt_unwrap_boxes(p, p, p, 24, p, p, 6, p, 0, p, p, 6, n) == -1
    assert L.nlt_unwrap_uv(p, 24, p, p, 6, p, p, p, 6, 1.0, 0, p, n) == -1 and L.nlt_unwrap_uv(p, 24, p, p, 6, p, p, n, 6, 1.0, 4, p, n) == -1
