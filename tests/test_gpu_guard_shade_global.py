"""-m gpu: memory discipline of nlt_render_global (csrc/raycast.hip) with tests/guard_util.py, as tests/test_gpu_guard_shade.py
does it for nlt_render_direct.  The hierarchy, both attribute arrays and both sample tables are guarded views of exactly the
stated size under the three fills, the adapter's three outputs are guarded through `guarded_allocs` and start as the fill: bands
and read-only operands intact, every output element written (a fill left behind is not finite, or differs between fills) and
the same bits under every fill and on plain tensors (tests/test_gpu_shade_global.py holds those to the brute force).  A table
read outside its [n_sets, n, c] elements would bring a fill into the picture.  The NULL forms: no attribute arrays, no bounce
table (n_b = 0), no rgb_indirect.  Shapes: a ground quad under 7 random triangles (bounce rays from the ground reach them, some
of them lit) = 9 triangles (three leaves padded to four), 11 x 7 pixels (a partial last workgroup),
2 x 2 samples, 3 light points in 5 sets and 4 bounce rays in 3 sets (the set index wraps)."""
import numpy as np
import pytest
import torch

import guard_util as G
import raycast_ref as R
from nlt_amd import capi as C
from nlt_amd.data_gen import shade as SH
from nlt_amd.data_gen.mesh import camera_matrix
from test_gpu_guard_shade import CAM, LIGHT, f64

pytestmark = pytest.mark.gpu

_G = [(-0.5, -0.5, 0.0), (1.5, -0.5, 0.0), (1.5, 1.6, 0.0), (-0.5, 1.6, 0.0)]
TV = np.concatenate((np.array([[_G[0], _G[1], _G[2]], [_G[0], _G[2], _G[3]]]), R.soup(7, seed=22)))
N_TRIS = len(TV)


def _plain_bvh():
    tris, nodes = C.bvh_build(f64(TV).cuda(), TV.reshape(-1, 3).min(0), TV.reshape(-1, 3).max(0))
    torch.cuda.synchronize()
    return tris.cpu(), nodes.cpu()


@pytest.mark.parametrize('attributes,bounce,indirect', [(True, True, True), (False, True, True), (True, False, True), (True, True, False)])
def test_render_global(monkeypatch, attributes, bounce, indirect):
    tris, nodes = _plain_bvh()
    _, inv, (imh, imw) = camera_matrix(CAM, 7)
    assert (imh, imw) == (7, 11)
    rng = np.random.default_rng(4)
    ins = dict(tris=tris, nodes=nodes, tri_normals=f64(rng.normal(size=(N_TRIS, 3, 3))) if attributes else None,
               tri_rgb=f64(rng.random((N_TRIS, 3, 3))) if attributes else None, light_pts=f64(np.array(SH.light_table(3, 5))),
               bounce_pts=f64(np.array(SH.bounce_table(4, 3))) if bounce else None)       # (copies: the tables are read-only)
    call = lambda t: C.render_global(t['tris'], t['nodes'], N_TRIS, t['tri_normals'], t['tri_rgb'], inv.reshape(-1), CAM['position'], imh,
                                     imw, 2, LIGHT, 4.0, (0.8, 0.7, 0.6), 0.04, 0.5, 0.3, t['light_pts'], t['bounce_pts'],
                                     want_indirect=indirect)
    _, state, want = G.bitwise_case(monkeypatch, call, ins)
    shapes = [(imh * imw, 3), (imh * imw,)] + ([(imh * imw, 3)] if indirect else [])
    assert [g.shape for g in state['nan'][1].made] == shapes
    rgb, cov = want['ret0'], want['ret1']
    assert tuple(rgb.shape) == (imh * imw, 3) and tuple(cov.shape) == (imh * imw,)
    assert 0 < int((cov > 0).sum()) < imh * imw and bool(((cov > 0) & (cov < 1)).any()) and bool((rgb > 0).any())
    assert not bool(rgb[cov == 0].any())
    if indirect:
        ind = want['ret2']
        assert tuple(ind.shape) == (imh * imw, 3) and bool((ind > 0).any()) == bounce and not bool(ind[cov == 0].any())
        assert bool((ind <= rgb).all())
