"""-m gpu: memory discipline of the capture writer's three launches (csrc/assemble.hip: nlt_capture_camspc, nlt_capture_uvspc,
nlt_diffuse_bases) with tests/guard_util.py.  Every input is a guarded view of exactly the stated size and must come back
unmodified; the outputs the adapters allocate are guarded, fill-initialised allocations of exactly the described elements
(`guarded_allocs`): nothing beyond them may be touched, and nothing of the fill may survive in them or reach them -- the results
are bit-identical under the three fills and bit for bit what the same adapter gives on plain tensors.

Sizes: the smallest odd shapes -- one pixel / texel, and odd sides that are no multiple of the 256-thread block with more than
one block (for nlt_diffuse_bases: the UV half and the camera half meeting inside a block)."""
import numpy as np
import pytest
import torch

from nlt_amd import capi as C
import guard_util as G

pytestmark = pytest.mark.gpu


def _unit_map(rng, *shape):
    m = rng.random(shape + (2,)) * 1.1 - 0.05
    m[rng.random(shape) < 0.3] = 0
    return m


@pytest.mark.parametrize('imh,imw', [(1, 1), (17, 19)])
@pytest.mark.parametrize('masked', [True, False])
def test_capture_camspc(monkeypatch, imh, imw, masked):
    rng = np.random.default_rng(imh + masked)
    p = imh * imw
    T = torch.from_numpy
    ins = dict(locs=T(rng.random((p, 3)) * 4 - 2), normals=T(rng.random((p, 3)) * 2 - 1), valid=T((rng.random(p) > 0.2).astype(np.uint8)),
               occluded=T((rng.random(p) < 0.3).astype(np.uint8)) if masked else None,
               alpha=T(rng.choice(np.array([0, 1, 254, 255], np.uint8), (imh, imw))) if masked else None,
               uv2cam=T(_unit_map(rng, imh, imw)))
    G.bitwise_case(monkeypatch, lambda t: C.capture_camspc(t['locs'], t['normals'], t['valid'], t['occluded'], (0.3, -2.5, 1.0),
                                                           (-1.0, 0.5, 2.0), t['alpha'], t['uv2cam']), ins)


@pytest.mark.parametrize('imh,imw,uvs', [(1, 1, 1), (5, 7, 19)])
@pytest.mark.parametrize('ldm,ld_rgb', [(2, 3), (3, 4), (2, None)])
def test_capture_uvspc(monkeypatch, imh, imw, uvs, ldm, ld_rgb):
    rng = np.random.default_rng(uvs + ldm)
    T = torch.from_numpy
    U8 = lambda *s: T(rng.integers(0, 256, s, dtype=np.uint8))
    cam2uv = _unit_map(rng, uvs, uvs)
    if ldm == 3:
        cam2uv = np.dstack((cam2uv, rng.random((uvs, uvs))))
    ins = dict(cam2uv=T(cam2uv), cvis_camspc=U8(imh, imw), lvis_camspc=U8(imh, imw), rgb_camspc=None if ld_rgb is None else U8(imh, imw, ld_rgb))
    G.bitwise_case(monkeypatch, lambda t: C.capture_uvspc(t['cam2uv'], t['cvis_camspc'], t['lvis_camspc'], t['rgb_camspc']), ins)


@pytest.mark.parametrize('f,h,w,imh,imw', [(1, 1, 1, 1, 1), (3, 11, 9, 7, 5)])
def test_diffuse_bases(monkeypatch, f, h, w, imh, imw):
    rng = np.random.default_rng(f + h)
    T = torch.from_numpy
    albedo = rng.random((h, w, 3))
    albedo[0, 0, 0] = 1.0
    ins = dict(albedo=T(albedo), lvis=T(rng.integers(0, 256, (f, h, w), dtype=np.uint8)), uv2cam=T(_unit_map(rng, f, imh, imw).astype(np.float16)))
    G.bitwise_case(monkeypatch, lambda t: C.diffuse_bases(t['albedo'], t['lvis'], t['uv2cam']), ins)
