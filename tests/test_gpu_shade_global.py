"""-m gpu: nlt_render_global (csrc/raycast.hip) against the float64 brute force of tests/shade_global_ref.py, BIT FOR BIT on the
three float32 outputs -- rgb_linear, rgb_indirect and coverage.  That is derived, not a tolerance: every operation is an IEEE
+ - * / sqrt in float64 with contraction off, in the order include/nlt_hip.h states, then one rounding; the tables are the same
float64 numbers on both sides.  Shapes are the smallest at which the kernel can still go wrong: the scenes of
tests/test_gpu_shade.py (a 13 x 9 image: a partial last workgroup; 1, 4 and 9 samples per pixel; 1 to 5 bounce rays and 1 to 3
light points; as many table sets as samples, fewer, and one more, which checks the modulo), a corner of two coloured quads
(colour bleeding) and a floor under a ceiling lit from below the floor (indirect light only).  Each case's reference is computed
once (`ref`) and shared; the non-vacuity conditions at the end are asserted on the references alone."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import raycast_ref as R
import shade_global_ref as G
from nlt_amd import capi as C
from nlt_amd.data_gen import mesh as M
from nlt_amd.data_gen import shade as SH
from test_gpu_shade import bunny_light, bunny_rgb, cube_cam, occluder_cam, same, soup_cam
from test_gpu_shade import host_mesh as _host_mesh

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- scenes (host only: nothing here touches the GPU)
@functools.lru_cache(None)
def host_mesh(name):
    if name == 'corner':
        # a floor x in [0, 3], a wall in the plane x = 0 and a small awning at z = 2 whose shadow falls on both, each with
        # vertices of its own
        v = np.array([[0, -2, 0], [3, -2, 0], [3, 2, 0], [0, 2, 0], [0, -2, 0], [0, 2, 0], [0, 2, 2.5], [0, -2, 2.5],
                      [0.3, -0.5, 2], [1.3, -0.5, 2], [1.3, 0.8, 2], [0.3, 0.8, 2]], np.float64)
        return M.Mesh(v, [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]], device=None)
    if name == 'room':
        # a floor and, 1.5 above it, a smaller ceiling; the light of this case lies below the floor's plane, beside the floor
        v = np.array([[-2, -2, 0], [1.9, -2, 0], [1.9, 2, 0], [-2, 2, 0], [-1, -1, 1.5], [1.3, -1, 1.5], [1.3, 1, 1.5], [-1, 1, 1.5]], np.float64)
        return M.Mesh(v, [[0, 1, 2, 3], [4, 5, 6, 7]], device=None)
    return _host_mesh(name)


@functools.lru_cache(None)
def dev_mesh(name):
    h = host_mesh(name)
    return M.Mesh(h.vertices, h.faces)


def corner_cam():
    return R.make_cam('K', (4.0, -3.0, 3.0), (0.5, 0.0, 0.5), sensor_width=32.0, sensor_height=24.0)


def room_cam():
    return R.make_cam('M', (3.0, -5.0, 1.1), (0.0, 0.0, 0.6), sensor_width=32.0, sensor_height=24.0)


def corner_rgb():
    return np.array([[0.9, 0.15, 0.1], [0.8, 0.2, 0.1], [0.9, 0.3, 0.2], [0.7, 0.1, 0.1], [0.1, 0.8, 0.3], [0.2, 0.9, 0.2], [0.1, 0.7, 0.4], [0.3, 0.8, 0.1],
                     [0.5, 0.5, 0.9], [0.4, 0.5, 0.8], [0.5, 0.4, 0.9], [0.5, 0.6, 0.7]])


# name -> (mesh, camera, imh, S, light, Material arguments, intensity, light_radius, n_l, n_b, n_lsets, n_bsets)
CASES = {}
for s_ in (1, 2, 3):
    for nb_ in (1, 5):
        for nl_ in (1, 3):
            for sets_ in sorted({1, s_ * s_, s_ * s_ + 1}):
                CASES['cube S=%d n_b=%d n_l=%d sets=%d' % (s_, nb_, nl_, sets_)] = \
                    ('cube', cube_cam, 9, s_, (5.0, -1.002, 0.5), dict(smooth=False), 30.0, 0.3, nl_, nb_, sets_, sets_)
CASES['corner colour bleeding'] = ('corner', corner_cam, 18, 2, (2.5, 1.0, 3.0), lambda: dict(vertex_rgb=corner_rgb(), smooth=False), 20.0,
                                   0.4, 2, 6, 4, 3)
CASES['room indirect only'] = ('room', room_cam, 18, 2, (4.0, 0.5, -1.0), dict(smooth=False, kd=(0.9, 0.6, 0.3)), 20.0, 0.2, 2, 4, 4, 4)
CASES['occluder penumbrae'] = ('occluder', occluder_cam, 18, 2, (0.1, 0.2, 5.0), dict(smooth=False), 20.0, 0.5, 4, 2, 4, 4)
CASES['occluder light in the plane z=1'] = ('occluder', occluder_cam, 18, 1, (3.0, 0.3, 1.0), dict(smooth=False), 20.0, 0.3, 3, 3, 2, 1)
CASES['bunny smooth vertex_rgb n_b=4'] = ('bunny', R.bunny_cam, 24, 1, lambda: bunny_light((0.4, 0.1, 0.05)),
                                          lambda: dict(vertex_rgb=bunny_rgb()), 0.1, 0.03, 2, 4, 1, 1)
CASES['soup with degenerate triangles'] = ('soup', soup_cam, 9, 2, (0.2, -1.0, 2.5), dict(smooth=False), 5.0, 0.25, 2, 3, 4, 4)


def case(name):
    mesh, cam, imh, s, light, mat, intensity, radius, n_l, n_b, n_lsets, n_bsets = CASES[name]
    light = light() if callable(light) else light
    mat = mat() if callable(mat) else mat
    return (mesh, cam(), imh, s, [float(x) for x in light], SH.Material(**mat), intensity, radius, SH.light_table(n_l, n_lsets),
            SH.bounce_table(n_b, n_bsets))


@functools.lru_cache(None)
def ref(name):
    """The brute force for a case: computed once, shared, never modified."""
    mesh, cam, imh, s, light, mat, intensity, radius, lpts, bpts = case(name)
    h = host_mesh(mesh)
    _, inv, (imh, imw) = M.camera_matrix(cam, imh)
    out = G.render(h.tri_verts, inv, cam['position'], imh, imw, s, light, intensity, mat.kd, mat.ks, mat.roughness,
                   tri_normals=M.corner_normals(h) if mat.smooth else None,
                   tri_rgb=None if mat.vertex_rgb is None else mat.vertex_rgb[h.tris], light_radius=radius, light_pts=lpts, bounce_pts=bpts)
    for v in out.values():
        v.setflags(write=False)
    return out


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float64)).cuda()                # (a copy: the tables are read-only)


def launch(name, **kw):
    mesh, cam, imh, s, light, mat, intensity, radius, lpts, bpts = case(name)
    m = dev_mesh(mesh)
    _, inv, (imh, imw) = M.camera_matrix(cam, imh)
    return C.render_global(*m.bvh, m.n_tris, *mat.arrays(m), inv.reshape(-1), cam['position'], imh, imw, s, light, intensity, mat.kd,
                           mat.ks, mat.roughness, radius, dev(lpts), dev(bpts), **kw)


@pytest.mark.parametrize('name', sorted(CASES))
def test_bit_equal_to_the_brute_force(name):
    want = ref(name)
    rgb, cov, ind = launch(name)
    rgb2, cov2, ind2 = launch(name)
    torch.cuda.synchronize()
    print("%s: %d pixels, %d hit, %d with indirect light, %d in a penumbra, bounce rays: %d skipped, %d missed, %d hit"
          % (name, want['hits'].size, (want['hits'] > 0).sum(), want['rgb_indirect'].any(1).sum(),
             ((want['light_occluded'] > 0) & (want['light_unoccluded'] > 0)).sum(), want['bounce_skipped'].sum(),
             want['bounce_missed'].sum(), want['bounce_hit'].sum()))
    same(cov, want['coverage'], name + ' coverage')
    same(ind, want['rgb_indirect'], name + ' rgb_indirect')
    same(rgb, want['rgb'], name + ' rgb_linear')
    for a, b in ((rgb, rgb2), (cov, cov2), (ind, ind2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert np.isfinite(want['rgb']).all()
    # without rgb_indirect (NULL) the other two outputs are the same bits
    rgb3, cov3, none = launch(name, want_indirect=False)
    assert none is None and torch.equal(rgb3.view(torch.int32), rgb.view(torch.int32)) and torch.equal(cov3.view(torch.int32), cov.view(torch.int32))


def test_the_host_path_uses_one_table_set_per_sample():
    """shade.render_global: the light JSON's size is the radius, n_sets = S^2 -- the case 'cube S=2 n_b=5 n_l=3 sets=4'."""
    name = 'cube S=2 n_b=5 n_l=3 sets=4'
    mesh, cam, imh, s, light, mat, intensity, radius, lpts, bpts = case(name)
    want = ref(name)
    got = SH.render_global(dev_mesh(mesh), cam, dict(name='L', position=light, size=radius), imh, s * s, mat, intensity, bounces=5, light_samples=3)
    for g, k in zip(got, ('rgb', 'coverage', 'rgb_indirect')):
        same(g, want[k], k)
    other = SH.render_global(dev_mesh(mesh), cam, dict(name='L', position=light, size=7.0), imh, s * s, mat, intensity, bounces=5, light_samples=3,
                             light_size=radius)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, other))


@pytest.mark.parametrize('name', ['cube S=3 n_b=1 n_l=1 sets=9', 'occluder penumbrae', 'bunny smooth vertex_rgb n_b=4'])
def test_degenerate_arguments_are_render_direct_bit_for_bit(name):
    """n_b = 0 with a NULL bounce table, n_l = 1, light_radius = 0, against nlt_render_direct's own output; and n_b = 0 with a
    sized light against the brute force."""
    mesh, cam, imh, s, light, mat, intensity, radius, lpts, _ = case(name)
    m, h = dev_mesh(mesh), host_mesh(mesh)
    _, inv, (imh, imw) = M.camera_matrix(cam, imh)
    args = (*m.bvh, m.n_tris, *mat.arrays(m), inv.reshape(-1), cam['position'], imh, imw, s, light, intensity, mat.kd, mat.ks, mat.roughness)
    rgb0, cov0 = C.render_direct(*args)
    rgb, cov, ind = C.render_global(*args, 0.0, dev(SH.light_table(1, 2)), None)
    torch.cuda.synchronize()
    assert bool(rgb0.any()) and torch.equal(rgb.view(torch.int32), rgb0.view(torch.int32)) and torch.equal(cov.view(torch.int32), cov0.view(torch.int32))
    assert not bool(ind.view(torch.int32).any())
    if mesh != 'bunny':
        want = G.render(h.tri_verts, inv, cam['position'], imh, imw, s, light, intensity, mat.kd, mat.ks, mat.roughness,
                        tri_normals=M.corner_normals(h) if mat.smooth else None, light_radius=radius, light_pts=lpts, bounce_pts=None)
        rgb, cov, ind = C.render_global(*args, radius, dev(lpts), None)
        same(rgb, want['rgb'], 'rgb_linear'); same(cov, want['coverage'], 'coverage'); same(ind, want['rgb_indirect'], 'rgb_indirect')
        assert not want['rgb_indirect'].any() and ((want['light_occluded'] > 0) | (want['light_not_facing'] > 0)).any()


def test_attribute_arrays_null_and_given():
    """Straight through the adapter: NULL / non-NULL tri_normals and tri_rgb in the four combinations on the soup, with random corner
    normals (many hits, primary and secondary, are shaded on a flipped normal; bounce rays leave below the geometric surface and are
    skipped), all zero for one triangle, infinite for another and NaN for a third (those fall back to the geometric normal)."""
    h, m = host_mesh('soup'), dev_mesh('soup')
    cam = soup_cam()
    _, inv, (imh, imw) = M.camera_matrix(cam, 9)
    rng = np.random.default_rng(5)
    normals = rng.normal(size=(h.n_tris, 3, 3))
    t, tri, _ = R.closest(np.broadcast_to(np.asarray(cam['position']), (imh * imw, 3)), R.camera_rays(inv, cam['position'], imh, imw), h.tri_verts)
    seen = [int(k) for k in np.unique(tri[tri >= 0])]
    normals[seen[0]] = 0.0; normals[seen[1]] = np.inf; normals[seen[2], 1, 1] = np.nan
    rgb = rng.random((h.n_tris, 3, 3))
    light, kw = (0.2, -1.0, 2.5), dict(intensity=5.0, kd=(0.7, 0.6, 0.5), ks=0.04, alpha=0.5)
    lpts, bpts = SH.light_table(2, 3), SH.bounce_table(3, 2)
    skipped = hit = 0
    for tn, tc in ((None, None), (normals, None), (None, rgb), (normals, rgb)):
        want = G.render(h.tri_verts, inv, cam['position'], imh, imw, 2, light, tri_normals=tn, tri_rgb=tc, light_radius=0.2, light_pts=lpts,
                        bounce_pts=bpts, **kw)
        got = C.render_global(*m.bvh, m.n_tris, dev(tn), dev(tc), inv.reshape(-1), cam['position'], imh, imw, 2, light, kw['intensity'],
                              kw['kd'], kw['ks'], kw['alpha'], 0.2, dev(lpts), dev(bpts))
        for g, k in zip(got, ('rgb', 'coverage', 'rgb_indirect')):
            same(g, want[k], k)
        assert np.isfinite(want['rgb']).all() and want['rgb'].any()
        skipped += int(want['bounce_skipped'].sum()) if tn is not None else 0
        hit += int(want['bounce_hit'].sum())
    assert skipped >= 10 and hit >= 10
    bad = torch.zeros((3, 3, 3), dtype=torch.float64).cuda()
    for a in ((bad, None, dev(lpts), dev(bpts)), (None, None, dev(lpts[..., :2]), dev(bpts)), (None, None, dev(lpts), dev(lpts))):
        with pytest.raises(C.NLTError):
            C.render_global(*m.bvh, m.n_tris, a[0], a[1], inv.reshape(-1), cam['position'], imh, imw, 2, light, 1.0, (1, 1, 1), 0.04, 0.5, 0.2,
                            a[2], a[3])


def test_refusals_launch_nothing():
    m = dev_mesh('cube')
    cam = cube_cam()
    _, inv, _ = M.camera_matrix(cam, 9)
    host = (ctypes.c_double * 19)(*([float(x) for x in inv.reshape(-1)] + cam['position']))
    outs = [torch.full((9 * 13, 3), 7.0, device='cuda'), torch.full((9 * 13,), 7.0, device='cuda'), torch.full((9 * 13, 3), 7.0, device='cuda')]
    lpts, bpts = dev(SH.light_table(64, 1)), dev(SH.bounce_table(64, 1))
    L = C.lib()

    def call(s=1, n_tris=m.n_tris, radius=0.1, lp=lpts.data_ptr(), n_l=2, n_lsets=1, bp=bpts.data_ptr(), n_b=2, n_bsets=1, out=outs[0].data_ptr(),
             imh=9, imw=13):
        return L.nlt_render_global(m.bvh[0].data_ptr(), m.bvh[1].data_ptr(), n_tris, None, None, ctypes.addressof(host), imh, imw, s, 1.0, 2.0,
                                   3.0, 1.0, 0.8, 0.8, 0.8, 0.04, 0.5, radius, lp, n_l, n_lsets, bp, n_b, n_bsets, out, outs[1].data_ptr(),
                                   outs[2].data_ptr(), None)
    assert call(s=0) == -1 and call(s=9) == -1 and call(n_tris=0) == -1 and call(out=None) == -1 and call(lp=None) == -1
    assert call(bp=None) == -1 and call(n_l=0) == -1 and call(n_l=65) == -1 and call(n_b=-1) == -1 and call(n_b=65) == -1
    assert call(n_lsets=0) == -1 and call(n_bsets=0) == -1 and call(radius=-1.0) == -1 and call(radius=float('nan')) == -1
    assert call(radius=float('inf')) == -1 and call(n_tris=1 << 31) == -2 and call(imh=1 << 15, imw=1 << 15) == -2
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)
    assert call(n_l=64, n_b=64) == 0 and call(bp=None, n_b=0) == 0 and call(radius=0.0, n_l=1) == 0        # the ends of the ranges are taken
    torch.cuda.synchronize()
    assert not any(bool((o == 7.0).any()) for o in outs)


def test_the_cases_are_not_vacuous():
    """Conditions on the inputs, counted on the references' output (never on the kernel's)."""
    refs = {n: ref(n) for n in sorted(CASES)}
    tot = lambda k: sum(int(r[k].sum()) for r in refs.values())
    indirect_only = sum(int((~r['direct'].any(1) & r['rgb_indirect'].any(1)).sum()) for r in refs.values())
    penumbra = sum(int(((r['light_occluded'] > 0) & (r['light_unoccluded'] > 0)).sum()) for r in refs.values())
    print("pixels with D = 0 and I > 0: %d, with some but not all light points occluded: %d; bounce rays skipped %d, missed %d, hit %d; "
          "secondary hits lit %d, shadowed %d, flipped %d" % (indirect_only, penumbra, tot('bounce_skipped'), tot('bounce_missed'),
                                                              tot('bounce_hit'), tot('secondary_lit'), tot('secondary_shadowed'), tot('secondary_flipped')))
    assert indirect_only >= 10 and penumbra >= 10 and tot('bounce_skipped') >= 10 and tot('bounce_missed') >= 100
    assert tot('secondary_lit') >= 100 and tot('secondary_shadowed') >= 10 and tot('secondary_flipped') >= 10
    room = refs['room indirect only']
    # the light is below the floor's plane: the floor is lit by the ceiling's underside alone (which the camera also sees, lit)
    assert int((~room['direct'].any(1) & room['rgb_indirect'].any(1)).sum()) >= 10 and room['direct'].any()
    corner = refs['corner colour bleeding']
    # colour bleeding: floor pixels (red) receive green from the wall -- their indirect green exceeds their indirect red's share
    assert (corner['rgb_indirect'][:, 1] > corner['rgb_indirect'][:, 0]).sum() >= 10
    pen = refs['occluder penumbrae']
    assert int(((pen['light_occluded'] > 0) & (pen['light_unoccluded'] > 0)).sum()) >= 5
    bunny = refs['bunny smooth vertex_rgb n_b=4']
    assert bunny['bounce_skipped'].sum() >= 5 and bunny['bounce_hit'].sum() >= 20
    # the modulo: with one set more than samples, and with one set for several samples, the picture differs from one set per sample
    a, b, c = (refs['cube S=2 n_b=5 n_l=3 sets=%d' % k]['rgb'] for k in (1, 4, 5))
    assert not np.array_equal(a, b) and not np.array_equal(b, c)
