"""-m gpu: csrc/unwrap.hip through data_gen.unwrap.smart_unwrap against the NumPy restatement tests/unwrap_ref.py, BIT for bit:
n, unit, area, ok, the projection vectors and their seeds, groups, labels, puv, boxes and the dense uv (tests/test_host_unwrap.py
holds the restatement to closed forms).  Cases: the tree sum's block edges (1, 2, 255, 256, 257 faces; 81 920 faces for a third
level), the fixtures, degenerate / NaN / non-manifold / duplicate faces, exact ties, labels that travel far against the index
order, a permuted face order, repeat calls and a second stream.  One restatement run per case, shared and left unchanged."""
import numpy as np
import pytest
import torch

import unwrap_ref as R
from nlt_amd import capi as C
from nlt_amd.data_gen import unwrap as U

pytestmark = pytest.mark.gpu

MARGIN = 0.002
_ref = {}


def ref(key, make, angle=66., aw=0.):
    if (key, angle, aw) not in _ref:
        verts, faces = make()
        faces = [list(map(int, f)) for f in faces]
        _ref[(key, angle, aw)] = (np.asarray(verts, np.float64), faces, R.unwrap(verts, faces, angle, aw, MARGIN))
    return _ref[(key, angle, aw)]


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == 'f':                                         # a NaN is a NaN, whatever its payload; every other value by its bits
        nan = np.isnan(a)
        return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64)))
    return bool(np.array_equal(a, b))


def device_run(verts, faces, angle=66., aw=0.):
    return U.smart_unwrap(dict(vertices=verts, faces=faces), angle, aw, MARGIN, intermediates=True)


def assert_same(u, r, what=''):
    pairs = [('n', u.n, r['n']), ('unit', u.unit, r['unit']), ('area', u.area, r['area']), ('ok', u.ok, r['ok']),
             ('vectors', u.vectors, r['vectors']), ('seeds', np.array(u.seeds), np.array(r['seeds'])), ('groups', u.groups, r['groups']),
             ('labels', u.labels, r['labels']), ('puv', u.puv, r['puv']), ('boxes', u.boxes, r['boxes']),
             ('scale', np.float64(u.scale), np.float64(r['scale'])), ('rot', u.rot, r['rot']), ('offsets', u.offsets, r['offsets']),
             ('uv', u.dense['uv'], r['uv']), ('counts', u.dense['counts'], r['counts'])]
    for name, got, want in pairs:
        assert bits_equal(got, want), "%s%s differs from the restatement" % (what, name)


def check(key, make, angle=66., aw=0.):
    verts, faces, r = ref(key, make, angle, aw)
    u = device_run(verts, faces, angle, aw)
    assert_same(u, r, '%s (%g, %g): ' % (key, angle, aw))
    return u, r


def _grid_prefix(n):
    verts, faces = R.grid_mesh(12)
    return verts, faces[:n]


@pytest.mark.parametrize('n', [1, 2, 255, 256, 257])
def test_tree_sum_block_edges_on_a_flat_grid(n):
    """Every face is gathered by the first round, so the one sum runs over all n faces: one block short, full, and one over."""
    u, r = check('grid%d' % n, lambda: _grid_prefix(n), 66., 1.)
    assert len(u.vectors) == 1 and len(u.island_labels) == 1 and u.rounds['vectors'] == 1


@pytest.mark.parametrize('n', [1, 2, 255, 256, 257])
def test_tree_sum_block_edges_on_a_soup(n):
    u, r = check('soup%d' % n, lambda: R.soup_mesh(n, seed=5), 89., 1.)
    assert len(u.island_labels) == n                                # nothing is welded: one island per face


def test_third_tree_level_on_icosphere_6():
    u, r = check('ico6', lambda: R.icosphere(6))
    assert len(u.groups) == 81920 > 256 * 256 and u.rounds['vectors'] == len(r['vectors'])
    print("icosphere 6: %d groups, %d islands, %d island rounds" % (len(u.vectors), len(u.island_labels), u.rounds['islands']))


@pytest.mark.parametrize('key,make,angle,aw', [('cube', R.cube_mesh, 66., 0.), ('cube', R.cube_mesh, 1., 1.), ('mixed', R.mixed_mesh, 66., 0.),
                                               ('mixed', R.mixed_mesh, 20., 0.5), ('bunny', R.bunny_mesh, 66., 0.), ('bunny', R.bunny_mesh, 89., 1.)])
def test_fixtures(key, make, angle, aw):
    u, r = check(key, make, angle, aw)
    assert u.dense['uv'].min() >= 0 and u.dense['uv'].max() <= 1
    if key == 'bunny':
        print("bunny (%g, %g): %d groups, %d islands, scale %.6f, %d island rounds" % (angle, aw, len(u.vectors), len(u.island_labels), u.scale,
                                                                                       u.rounds['islands']))


def _bad_faces():
    """A flat grid with: two fins on the boundary edge (0, 1) of face 0 (three faces on one edge; the fins' normals are 26.6
    degrees off the grid's, so they share its group), zero-area faces (a repeated vertex, three collinear ones), a face at a NaN
    vertex and one at an infinite one, a two-loop face -- all five on that edge too, after the fins in loop order, so the run of
    equal keys links face 0, the fins and nothing else -- and one face three times."""
    verts, faces = R.grid_mesh(3)
    k = len(verts)
    verts = np.concatenate((verts, [[np.nan, 0.1, 0.2], [np.inf, 0.0, 0.0], [0.125, 0.1, -0.05], [0.125, -0.1, -0.05]]))
    faces = faces + [[0, 1, k + 2], [1, 0, k + 3], [0, 0, 1], [0, 1, 2], [0, 1, k], [4, 5, k + 1], [0, 1], list(faces[3]), list(faces[3])]
    return verts, faces


def test_bad_faces():
    u, r = check('bad', _bad_faces)
    assert list(u.ok[18:]) == [1, 1, 0, 0, 0, 0, 0, 1, 1] and list(u.groups[20:25]) == [-1] * 5 and list(u.labels[20:25]) == [-1] * 5
    assert not u.dense['uv'][20:25].any() and np.isfinite(u.dense['uv']).all()
    assert len(u.vectors) == 1 and not u.labels[:20].any() and not u.labels[25:].any()      # fins and duplicates join the grid's island


def test_ties_go_to_the_lowest_index():
    u, r = check('octa', R.octahedron)
    assert u.seeds[:3] == [0, 6, 1] and list(u.groups) == [u.seeds.index(f) for f in range(8)]


def test_labels_travel_along_a_permuted_ribbon():
    u, r = check('ribbon', lambda: R.ribbon(4000, seed=9))
    assert len(u.vectors) == 1 and not u.labels.any()               # one island, and its label is face 0
    print("ribbon of 4000 permuted triangles: %d island rounds" % u.rounds['islands'])
    assert u.rounds['islands'] < C.UNWRAP_MAX_ISLAND_ROUNDS


def test_a_permuted_face_order_gives_the_same_partition():
    """The island stage alone on icosphere 3 (1280 faces, every edge shared by exactly two), with the groups of the unpermuted run
    carried along: the partition does not depend on which face index a label starts from, the labels are the components' smallest
    indices in either order, and they are the restatement's.  (On an edge that MORE than two faces of different groups share, the
    links follow the sorted run, so there the partition may depend on the face order: include/nlt_hip.h.)"""
    verts, faces, r = ref('ico3', lambda: R.icosphere(3))
    perm = np.random.default_rng(2).permutation(len(faces))
    _, lv, fo = R.mesh_arrays(verts, [faces[i] for i in perm])
    group = np.ascontiguousarray(r['groups'][perm])
    label, _, _ = C.unwrap_islands(torch.from_numpy(lv).cuda(), torch.from_numpy(fo).cuda(), len(verts), torch.from_numpy(group).cuda())
    label = label.cpu().numpy()
    inv = np.argsort(perm)
    want = {frozenset(int(inv[f]) for f in part) for part in R.partition(r['labels'])}
    assert len(want) > 1 and R.partition(label) == want
    for part in want:
        assert all(label[f] == min(part) for f in part)
    assert bits_equal(label, R.islands(lv, fo, len(verts), group)[0])


def test_repeat_calls_and_a_second_stream_give_equal_bits():
    verts, faces, r = ref('bunny', R.bunny_mesh)
    a = device_run(verts, faces)
    b = device_run(verts, faces)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = device_run(verts, faces)
    side.synchronize()
    for other in (b, c):
        for name in ('n', 'unit', 'area', 'ok', 'vectors', 'groups', 'labels', 'puv', 'boxes'):
            assert bits_equal(getattr(a, name), getattr(other, name)), name
        assert bits_equal(a.dense['uv'], other.dense['uv'])
    assert_same(c, r, 'second stream: ')


def test_max_groups_is_a_hard_cap():
    verts, faces = R.icosphere(2)
    with pytest.raises(ValueError, match='max_groups'):
        U.smart_unwrap(dict(vertices=verts, faces=faces.tolist()), angle_limit=1.)
    u = U.smart_unwrap(dict(vertices=verts, faces=faces.tolist()), angle_limit=1., max_groups=320)
    assert len(u.vectors) == 320 and len(u.island_labels) == 320


def test_table_and_mesh_object():
    """`smart_unwrap` of a `Mesh` works from its world-space vertices, and `.table()` is the pickle's layout."""
    from nlt_amd.data_gen.mesh import Mesh, dense_unwrap
    verts, faces, r = ref('mixed', R.mixed_mesh)
    m = np.eye(4); m[:3, :3] = np.diag([2.0, 2.0, 2.0]); m[:3, 3] = (1.0, -2.0, 0.5)
    u = U.smart_unwrap(Mesh(verts, faces, matrix_world=m, device=None))
    r2 = R.unwrap(verts @ m[:3, :3].T + m[:3, 3], faces, 66., 0., MARGIN)
    assert bits_equal(u.dense['uv'], r2['uv']) and bits_equal(u.boxes, r2['boxes'])
    table = u.table()
    assert [list(table[f][:, 1]) for f in range(len(faces))] == faces and table[5].shape == (5, 4)
    assert list(np.concatenate([table[f][:, 0] for f in range(len(faces))])) == list(range(sum(len(f) for f in faces)))
    assert bits_equal(dense_unwrap(table)['uv'], u.dense['uv'])
