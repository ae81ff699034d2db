"""-m gpu: memory discipline of nlt_render_direct (csrc/raycast.hip) with tests/guard_util.py, as tests/test_gpu_guard_raycast.py
does it for the ray casts.  The hierarchy and both attribute arrays are guarded views under the three fills, the adapter's two
outputs are guarded through `guarded_allocs` and start as the fill: bands and read-only operands intact, every output element
written (a fill left behind is not finite, or differs between fills) and the same bits under every fill and on plain tensors
(tests/test_gpu_shade.py holds those to the brute force).  The traversal's stack lives in LDS and is written before it is read.
Shapes: 9 triangles (three leaves padded to four), 11 x 7 pixels (a partial last workgroup), 2 x 2 samples."""
import numpy as np
import pytest
import torch

import guard_util as G
import raycast_ref as R
from nlt_amd import capi as C
from nlt_amd.data_gen.mesh import camera_matrix

pytestmark = pytest.mark.gpu

N_TRIS = 9
TV = R.soup(N_TRIS, seed=21)
f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
CAM = R.make_cam('G', (0.6, -1.2, 2.4), (0.5, 0.5, 0.5), sensor_width=33.0, sensor_height=21.0)
LIGHT = (0.2, 0.4, 3.0)


def _plain_bvh():
    tris, nodes = C.bvh_build(f64(TV).cuda(), TV.reshape(-1, 3).min(0), TV.reshape(-1, 3).max(0))
    torch.cuda.synchronize()
    return tris.cpu(), nodes.cpu()


@pytest.mark.parametrize('attributes', [True, False])
def test_render_direct(monkeypatch, attributes):
    tris, nodes = _plain_bvh()
    _, inv, (imh, imw) = camera_matrix(CAM, 7)
    assert (imh, imw) == (7, 11)
    rng = np.random.default_rng(4)
    ins = dict(tris=tris, nodes=nodes, tri_normals=f64(rng.normal(size=(N_TRIS, 3, 3))) if attributes else None,
               tri_rgb=f64(rng.random((N_TRIS, 3, 3))) if attributes else None)
    call = lambda t: C.render_direct(t['tris'], t['nodes'], N_TRIS, t['tri_normals'], t['tri_rgb'], inv.reshape(-1), CAM['position'], imh,
                                     imw, 2, LIGHT, 4.0, (0.8, 0.7, 0.6), 0.04, 0.5)
    _, state, want = G.bitwise_case(monkeypatch, call, ins)
    assert [g.shape for g in state['nan'][1].made] == [(imh * imw, 3), (imh * imw,)]
    rgb, cov = want['ret0'], want['ret1']
    assert tuple(rgb.shape) == (imh * imw, 3) and tuple(cov.shape) == (imh * imw,)
    assert 0 < int((cov > 0).sum()) < imh * imw and bool(((cov > 0) & (cov < 1)).any()) and bool((rgb > 0).any())
    assert not bool(rgb[cov == 0].any())
