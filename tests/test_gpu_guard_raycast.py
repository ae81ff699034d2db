"""-m gpu: memory discipline of csrc/raycast.hip with tests/guard_util.py -- nlt_bvh_morton + nlt_bvh_build and the three launch
forms.  Every tensor argument is a guarded view under the three fills, the adapters' own allocations (the Morton codes, the two
hierarchy buffers, every output) are guarded through `guarded_allocs`: bands and read-only operands intact, outputs fully written
and the same bits under every fill and on plain tensors (tests/test_gpu_raycast.py holds those to the brute force).  The hierarchy
buffers are exactly the queried sizes and start as the fill, so every element of them is written; the traversal's stack lives in
LDS and is written before it is read (a fill cannot reach it; equal bits across runs is what shows here).  Shapes: 9 triangles
(three leaves padded to four), 133 rays and 11 x 7 pixels (partial last workgroups).  All rays of the nlt_raycast case hit, so
every t is finite, as guard_util's finiteness check wants."""
import numpy as np
import pytest
import torch

import guard_util as G
import raycast_ref as R
from nlt_amd import capi as C

pytestmark = pytest.mark.gpu

N_TRIS = 9
TV = R.soup(N_TRIS, seed=21)
TRI2FACE = torch.arange(N_TRIS, dtype=torch.int32) // 2
f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _plain_bvh():
    tris, nodes = C.bvh_build(f64(TV).cuda(), TV.reshape(-1, 3).min(0), TV.reshape(-1, 3).max(0))
    torch.cuda.synchronize()
    return tris.cpu(), nodes.cpu()


def test_bvh_build(monkeypatch):
    lo, hi = TV.reshape(-1, 3).min(0), TV.reshape(-1, 3).max(0)
    res, state, want = G.bitwise_case(monkeypatch, lambda t: C.bvh_build(t['tri_verts'], lo, hi), dict(tri_verts=f64(TV)))
    L = C.lib()
    sizes = [g.shape for g in state['nan'][1].made]
    assert sizes == [(N_TRIS,), (L.nlt_bvh_tris_doubles(N_TRIS),), (L.nlt_bvh_nodes_doubles(N_TRIS),)] == [(9,), (160,), (42,)]
    tris = want['ret0'].view(16, 10)
    assert sorted(int(x) for x in tris[:, 9]) == [-1] * 7 + list(range(9))          # every triangle once, 7 empty slots
    assert torch.equal(tris[12:], torch.tensor([[0.0] * 9 + [-1.0]] * 4, dtype=torch.float64))      # the padding leaf
    nodes = want['ret1'].view(7, 6)
    assert torch.equal(nodes[6], torch.tensor([1.0, 1, 1, -1, -1, -1], dtype=torch.float64))         # its box: empty
    assert torch.equal(nodes[0, :3], f64(lo)) and torch.equal(nodes[0, 3:], f64(hi))                 # the root: the mesh's box


def test_raycast(monkeypatch):
    tris, nodes = _plain_bvh()
    rng = np.random.default_rng(5)
    o = np.tile([0.5, 0.5, 3.0], (133, 1)) + rng.random((133, 3)) * 0.1
    d, _ = R.unit_towards(o, TV.mean(1)[rng.integers(0, N_TRIS, 133)])               # at centroids: every ray hits something
    ins = dict(tris=tris, nodes=nodes, tri2face=TRI2FACE, origins=f64(o), dirs=f64(d))
    res, _, want = G.bitwise_case(monkeypatch, lambda t: C.raycast(t['tris'], t['nodes'], N_TRIS, t['tri2face'], t['origins'], t['dirs']), ins)
    assert bool((want['ret1'] >= 0).all()) and torch.equal(want['ret2'], want['ret1'] // 2)


def test_raycast_camera_and_shadow(monkeypatch):
    tris, nodes = _plain_bvh()
    from nlt_amd.data_gen.mesh import camera_matrix
    cam = R.make_cam('G', (0.6, -1.2, 2.4), (0.5, 0.5, 0.5), sensor_width=33.0, sensor_height=21.0)
    _, inv, (imh, imw) = camera_matrix(cam, 7)
    assert (imh, imw) == (7, 11)
    ins = dict(tris=tris, nodes=nodes, tri2face=TRI2FACE)
    call = lambda t: C.raycast_camera(t['tris'], t['nodes'], N_TRIS, t['tri2face'], inv.reshape(-1), cam['position'], imh, imw)
    _, _, want = G.bitwise_case(monkeypatch, call, ins)
    locs, valid = want['ret0'], want['ret2']
    assert 0 < int(valid.sum()) < imh * imw and tuple(locs.shape) == (imh * imw, 3)
    ins = dict(tris=tris, nodes=nodes, locs=locs, valid=valid)
    call = lambda t: C.raycast_shadow(t['tris'], t['nodes'], N_TRIS, t['locs'], t['valid'], (0.2, 0.4, 3.0))
    _, _, want = G.bitwise_case(monkeypatch, call, ins)
    assert tuple(want['ret'].shape) == (imh * imw,) and not bool(want['ret'][valid == 0].any())
