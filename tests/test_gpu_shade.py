"""-m gpu: nlt_render_direct (csrc/raycast.hip) against the float64 brute force of tests/shade_ref.py, BIT FOR BIT on the float32
outputs -- rgb_linear and coverage, misses, back-lit and shadowed pixels included.  That is derived, not a tolerance: every
operation is an IEEE + - * / sqrt in float64 with contraction off, in the order include/nlt_hip.h states, then one rounding.
Shapes are the smallest at which the kernel can still go wrong: a 13 x 9 image (a partial last workgroup of 64 lanes), 1, 4 and 9
samples per pixel, one leaf to a few hundred triangles.  Each case's reference is computed once (`ref`) and shared; the
non-vacuity conditions at the end are asserted on the references alone."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import raycast_ref as R
import shade_ref as S
from nlt_amd import capi as C
from nlt_amd.data_gen import mesh as M
from nlt_amd.data_gen import shade as SH

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same(got, want, what=''):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.nonzero(bits(got).reshape(-1) != bits(want).reshape(-1))[0]
    assert bad.size == 0, "%s: %d element(s) differ, first at %d: %r != %r" % (what, bad.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


# ---------------------------------------------------------------- scenes (host only: nothing here touches the GPU)
@functools.lru_cache(None)
def host_mesh(name):
    if name == 'cube':
        return M.Mesh.load(R.CUBE, device=None)
    if name == 'bunny':
        return M.Mesh.load(R.BUNNY, device=None)
    if name == 'occluder':
        # a ground quad and, above it, two separate triangles at z = 1 (one wound clockwise)
        v = np.array([[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0], [-0.6, -0.5, 1], [0.5, -0.6, 1], [0.1, 0.6, 1],
                      [0.9, 0.9, 1], [0.8, 0.0, 1], [1.7, 0.4, 1]], np.float64)
        return M.Mesh(v, [[0, 1, 2, 3], [4, 5, 6], [7, 8, 9]], device=None)
    if name == 'soup':
        tv = R.soup(60, seed=11, degenerates=True)                      # every 5th triangle degenerate, one vertex at 1e6
        return M.Mesh(tv.reshape(-1, 3), np.arange(180).reshape(-1, 3).tolist(), device=None)
    raise KeyError(name)


@functools.lru_cache(None)
def dev_mesh(name):
    h = host_mesh(name)
    return M.Mesh(h.vertices, h.faces)


def cube_cam():
    return R.make_cam('Q', (3.0, -4.0, 2.5), (0.0, 0.0, 0.0), sensor_width=26.0, sensor_height=18.0)          # 13 x 9 at imh = 9


def occluder_cam():
    return R.make_cam('S', (3.0, -4.0, 6.0), (0.0, 0.0, 0.0), sensor_width=32.0, sensor_height=24.0)


def soup_cam():
    return R.make_cam('D', (0.4, -1.6, 1.3), (0.5, 0.5, 0.5), focal_length=30.0, sensor_width=26.0, sensor_height=18.0)


def bunny_light(offset):
    return tuple(host_mesh('bunny').vertices.mean(0) + np.asarray(offset))


def bunny_rgb():
    return np.random.default_rng(3).random((len(host_mesh('bunny').vertices), 3))


# name -> (mesh, camera, imh, samples per side, light position, Material arguments, intensity)
CASES = {}
for s_ in (1, 2, 3):
    # the cube is [-1, 1]^3; the camera sees +x, -y and +z.  Light A: +x lit, -y grazing (the light is 0.002 outside its plane),
    # +z unlit (the light is below it).  Light B is inside the cube: every visible face is lit from behind and black.
    CASES['cube lit/grazing/unlit S=%d' % s_] = ('cube', cube_cam, 9, s_, (5.0, -1.002, 0.5), dict(smooth=False), 30.0)
    CASES['cube light inside S=%d' % s_] = ('cube', cube_cam, 9, s_, (0.1, 0.2, -0.3), dict(smooth=False), 30.0)
CASES['cube smooth ks=0'] = ('cube', cube_cam, 9, 2, (4.0, -3.0, 5.0), dict(ks=0.0, smooth=True), 30.0)
CASES['cube alpha=1'] = ('cube', cube_cam, 9, 2, (4.0, -3.0, 5.0), dict(roughness=1.0, smooth=False, kd=(0.2, 0.5, 0.9)), 30.0)
CASES['occluder cast shadow S=1'] = ('occluder', occluder_cam, 18, 1, (0.1, 0.2, 5.0), dict(smooth=False), 20.0)
CASES['occluder shadow edges S=3'] = ('occluder', occluder_cam, 18, 3, (0.1, 0.2, 5.0), dict(smooth=False), 20.0)
CASES['occluder light in the plane z=1'] = ('occluder', occluder_cam, 18, 2, (3.0, 0.3, 1.0), dict(smooth=False), 20.0)
CASES['bunny smooth vertex_rgb'] = ('bunny', R.bunny_cam, 24, 2, lambda: bunny_light((0.4, 0.1, 0.05)), lambda: dict(vertex_rgb=bunny_rgb()), 0.1)
CASES['bunny flat constant'] = ('bunny', R.bunny_cam, 24, 2, lambda: bunny_light((0.4, 0.1, 0.05)), dict(smooth=False), 0.1)
CASES['bunny narrow highlight alpha=0.05'] = ('bunny', R.bunny_cam, 24, 2, lambda: bunny_light((0.1, -0.1, 0.35)), dict(roughness=0.05, ks=0.5), 0.1)
CASES['soup with degenerate triangles'] = ('soup', soup_cam, 9, 2, (0.2, -1.0, 2.5), dict(smooth=False), 5.0)


def case(name):
    mesh, cam, imh, s, light, mat, intensity = CASES[name]
    light = light() if callable(light) else light
    mat = mat() if callable(mat) else mat
    return mesh, cam(), imh, s, dict(name='L', position=[float(x) for x in light], size=0.1), SH.Material(**mat), intensity


@functools.lru_cache(None)
def ref(name):
    """The brute force for a case: computed once, shared, never modified."""
    mesh, cam, imh, s, light, mat, intensity = case(name)
    h = host_mesh(mesh)
    _, inv, (imh, imw) = M.camera_matrix(cam, imh)
    out = S.render(h.tri_verts, inv, cam['position'], imh, imw, s, light['position'], intensity, mat.kd, mat.ks, mat.roughness,
                   tri_normals=M.corner_normals(h) if mat.smooth else None,
                   tri_rgb=None if mat.vertex_rgb is None else mat.vertex_rgb[h.tris])
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize('name', sorted(CASES))
def test_bit_equal_to_the_brute_force(name):
    mesh, cam, imh, s, light, mat, intensity = case(name)
    want = ref(name)
    rgb, cov = SH.render_direct(dev_mesh(mesh), cam, light, imh, s * s, mat, intensity)
    rgb2, cov2 = SH.render_direct(dev_mesh(mesh), cam, light, imh, s * s, mat, intensity)
    torch.cuda.synchronize()
    print("%s: %d pixels, %d partly covered, %d lit, %d with spec, %d in cast shadow, %d flipped"
          % (name, want['hits'].size, ((want['coverage'] > 0) & (want['coverage'] < 1)).sum(), (want['lit'] > 0).sum(),
             (want['spec_lit'] > 0).sum(), (want['shadowed'] > 0).sum(), want['flipped'].sum()))
    same(cov, want['coverage'], name + ' coverage')
    same(rgb, want['rgb'], name + ' rgb_linear')
    assert torch.equal(rgb.view(torch.int32), rgb2.view(torch.int32)) and torch.equal(cov.view(torch.int32), cov2.view(torch.int32))
    dark = torch.from_numpy(want['lit'] == 0).cuda()                                     # a miss, back-lit or occluded: exactly 0
    assert not bool(rgb[dark].view(torch.int32).any())
    if s == 1:
        valid = M.backproject(dev_mesh(mesh), cam, imh)['valid']
        assert torch.equal(cov, valid.float())


def test_what_the_cube_cases_show():
    """Conditions on the inputs: light A leaves a lit, a grazing and an unlit face in view; light B leaves nothing lit."""
    a, b = ref('cube lit/grazing/unlit S=1'), ref('cube light inside S=1')
    h = host_mesh('cube')
    cam = cube_cam()
    _, inv, (imh, imw) = M.camera_matrix(cam, 9)
    face = R.backproject(h.tri_verts, h.tri2face, inv, cam['position'], imh, imw)['face_i']
    faces = sorted(set(face[face >= 0]))
    assert (imh, imw) == (9, 13) and len(faces) == 3 and imh * imw % 64 != 0
    mean = {f: a['rgb'][face == f].max() for f in faces}
    order = sorted(mean.values())
    assert order[0] == 0.0 and 0.0 < order[1] < 0.01 * order[2]                          # unlit, grazing, lit
    assert (b['hits'] > 0).sum() > 30 and not b['rgb'].any() and not b['lit'].any() and not b['shadowed'].any()


def test_attribute_arrays_null_and_given_and_bad_normals():
    """Straight through the adapter: NULL / non-NULL tri_normals and tri_rgb in the four combinations on the soup, with corner normals
    that are random (so many hits are shaded on a flipped normal), all zero for one triangle, infinite for another and NaN for a
    third (those fall back to the geometric normal)."""
    h, m = host_mesh('soup'), dev_mesh('soup')
    cam = soup_cam()
    _, inv, (imh, imw) = M.camera_matrix(cam, 9)
    rng = np.random.default_rng(5)
    normals = rng.normal(size=(h.n_tris, 3, 3))
    t, tri, _ = R.closest(np.broadcast_to(np.asarray(cam['position']), (imh * imw, 3)), R.camera_rays(inv, cam['position'], imh, imw), h.tri_verts)
    seen = [int(k) for k in np.unique(tri[tri >= 0])]
    assert len(seen) >= 6
    normals[seen[0]] = 0.0; normals[seen[1]] = np.inf; normals[seen[2], 1, 1] = np.nan
    rgb = rng.random((h.n_tris, 3, 3))
    light, kw = (0.2, -1.0, 2.5), dict(intensity=5.0, kd=(0.7, 0.6, 0.5), ks=0.04, alpha=0.5)
    flipped = 0
    for tn, tc in ((None, None), (normals, None), (None, rgb), (normals, rgb)):
        want = S.render(h.tri_verts, inv, cam['position'], imh, imw, 2, light, tri_normals=tn, tri_rgb=tc, **kw)
        dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
        got_rgb, got_cov = C.render_direct(*m.bvh, m.n_tris, dev(tn), dev(tc), inv.reshape(-1), cam['position'], imh, imw, 2, light,
                                           kw['intensity'], kw['kd'], kw['ks'], kw['alpha'])
        same(got_cov, want['coverage'], 'coverage'); same(got_rgb, want['rgb'], 'rgb_linear')
        assert np.isfinite(want['rgb']).all() and want['rgb'].any()
        flipped += int(want['flipped'].sum()) if tn is not None else 0
    assert flipped >= 10
    with pytest.raises(C.NLTError):
        C.render_direct(*m.bvh, m.n_tris, torch.zeros((3, 3, 3), dtype=torch.float64).cuda(), None, inv.reshape(-1), cam['position'], imh, imw,
                        2, light, 1.0, (1, 1, 1), 0.04, 0.5)


def test_degenerate_triangles_are_never_hit():
    h = host_mesh('soup')
    cam = soup_cam()
    _, inv, (imh, imw) = M.camera_matrix(cam, 9)
    assert R.degenerate(h.tri_verts).sum() == 12
    only = M.Mesh(h.tri_verts[R.degenerate(h.tri_verts)].reshape(-1, 3), np.arange(36).reshape(-1, 3).tolist())
    rgb, cov = SH.render_direct(only, cam, dict(position=[0.2, -1.0, 2.5]), 9, 4, SH.Material(smooth=False), 5.0)
    assert not bool(rgb.view(torch.int32).any()) and not bool(cov.view(torch.int32).any())


def test_refusals_launch_nothing():
    m = dev_mesh('cube')
    cam = cube_cam()
    _, inv, _ = M.camera_matrix(cam, 9)
    host = (ctypes.c_double * 19)(*([float(x) for x in inv.reshape(-1)] + cam['position']))
    rgb = torch.full((9 * 13, 3), 7.0, device='cuda')
    cov = torch.full((9 * 13,), 7.0, device='cuda')
    L = C.lib()

    def call(imh=9, imw=13, s=1, n_tris=m.n_tris, tris=m.bvh[0].data_ptr(), out=rgb.data_ptr()):
        return L.nlt_render_direct(tris, m.bvh[1].data_ptr(), n_tris, None, None, ctypes.addressof(host), imh, imw, s, 1.0, 2.0, 3.0, 1.0,
                                   0.8, 0.8, 0.8, 0.04, 0.5, out, cov.data_ptr(), None)
    assert call(s=0) == -1 and call(s=9) == -1 and call(s=-1) == -1 and call(imh=0) == -1 and call(imw=0) == -1
    assert call(n_tris=0) == -1 and call(tris=None) == -1 and call(out=None) == -1
    assert call(n_tris=1 << 31) == -2 and call(imh=1 << 15, imw=1 << 15) == -2          # 3 * pixels >= 2^31
    torch.cuda.synchronize()
    assert bool((rgb == 7.0).all()) and bool((cov == 7.0).all())
    assert call(s=8) == 0 and call() == 0                                                # the ends of the range are taken
    torch.cuda.synchronize()
    assert not bool((rgb == 7.0).any()) and not bool((cov == 7.0).any())
    for spp in (0, 2, 81):
        with pytest.raises(ValueError):
            SH.render_direct(m, cam, dict(position=[1.0, 2.0, 3.0]), 9, spp, SH.Material())


def test_the_cases_are_not_vacuous():
    """Conditions on the inputs, counted on the references' output (never on the kernel's)."""
    refs = [ref(n) for n in sorted(CASES)]
    partly = sum(int(((r['coverage'] > 0) & (r['coverage'] < 1)).sum()) for r in refs)
    spec = sum(int((r['spec_lit'] > 0).sum()) for r in refs)
    shadow = sum(int((r['shadowed'] > 0).sum()) for r in refs)
    flipped = sum(int(r['flipped'].sum()) for r in refs)
    print("partly covered %d, lit with spec %d, in cast shadow %d, flipped hits %d" % (partly, spec, shadow, flipped))
    assert partly >= 20 and spec >= 20 and shadow >= 20 and flipped >= 10
    edge = ref('occluder shadow edges S=3')
    n = edge['hits']
    assert int(((edge['shadowed'] > 0) & (edge['shadowed'] < n) & (edge['lit'] > 0)).sum()) >= 3      # pixels across a shadow edge
    plane = ref('occluder light in the plane z=1')
    assert plane['rgb'].any() and (plane['hits'] > plane['lit']).any()
    narrow, wide = ref('bunny narrow highlight alpha=0.05'), ref('bunny flat constant')
    assert 0 < (narrow['spec_lit'] > 0).sum() and np.isfinite(narrow['rgb']).all() and np.isfinite(wide['rgb']).all()
    # ks = 0 leaves Schlick's (1 - vh)^5 term, alpha = 1 the constant D = 1 / pi: both still have a specular part
    assert ref('cube smooth ks=0')['spec_lit'].any() and ref('cube alpha=1')['spec_lit'].any()
