"""CPU: tests/shade_ref.py (the brute force nlt_render_direct is held to on the GPU) against closed forms, and the host logic of
data_gen/rig.py and data_gen/capture_main.py.

The closed-form scenes use a camera on the z axis at height 16 looking straight down at the plane z = 0 with a square 24 mm sensor,
a 48 mm lens and an 8 x 8 image: pixel (px, py) sees the world point (px - 4, 4 - py, 0), so sample positions and triangle edges
can be placed by hand."""
import math

import numpy as np
import pytest
import torch

import raycast_ref as R
import shade_ref as S
from nlt_amd.data_gen import capture_main as CM
from nlt_amd.data_gen import mesh as M
from nlt_amd.data_gen import rig as RIG
from nlt_amd.data_gen import shade as SH

EPS32 = float(np.finfo(np.float32).eps)
H = 16.0
CAM = R.make_cam('Z', (0.0, 0.0, H), (0.0, 0.0, 0.0), focal_length=48.0, sensor_width=24.0, sensor_height=24.0, up=(0.0, 1.0, 0.0))
_, INV, (IMH, IMW) = M.camera_matrix(CAM, 8)
BIG = np.array([[[-300.0, -300.0, 0.0], [300.0, -300.0, 0.0], [0.0, 500.0, 0.0]]])          # counter-clockwise: normal +z
CENTRE = 4 * IMW + 4                                                                          # pixel (4, 4) looks at the origin


def render(tv, spp_side, light, **kw):
    return S.render(tv, INV, CAM['position'], IMH, IMW, spp_side, light, **kw)


def closed_form(d, intensity, kd, ks, alpha):
    """Camera and light both on the normal: n = wo = wi = h, so nh = vh = ci = co = 1, D = 1 / (pi alpha^2), G1 = 1, F = ks."""
    spec0 = ks / (4.0 * math.pi * alpha * alpha)
    return intensity / (d * d) * (np.asarray(kd) / math.pi + spec0)


def test_the_camera_of_these_tests_maps_pixels_to_the_plane_as_stated():
    assert (IMH, IMW) == (8, 8)
    d = S.sample_rays(INV, CAM['position'], np.array([4.0, 5.0, 0.0]), np.array([4.0, 2.0, 7.0]))
    hit = np.asarray(CAM['position']) + d * (H / -d[:, 2:3])
    assert np.allclose(hit, [[0, 0, 0], [1, 2, 0], [-4, -3, 0]], atol=1e-12)


@pytest.mark.parametrize('ks,alpha', [(0.04, 0.5), (0.0, 0.5), (0.3, 0.05), (0.04, 1.0)])
def test_single_triangle_facing_camera_and_light(ks, alpha):
    d, kd, intensity = 5.0, (0.9, 0.5, 0.2), 3.0
    out = render(BIG, 1, (0.0, 0.0, d), intensity=intensity, kd=kd, ks=ks, alpha=alpha)
    want = closed_form(d, intensity, kd, ks, alpha)
    got = out['rgb'][CENTRE].astype(np.float64)
    assert np.all(np.abs(got - want) <= 2 * EPS32 * want), (got, want)
    assert np.all(out['coverage'] == 1.0) and out['lit'][CENTRE] == 1 and out['flipped'].sum() == 0
    assert (out['spec_lit'][CENTRE] == 1) == (ks > 0)
    # supersampling a constant-coverage pixel changes nothing but the sample positions: the centre pixel stays within the
    # variation of the shading over one pixel (a smooth function; at alpha = 0.05 the highlight is narrower than that)
    if alpha >= 0.5:
        out3 = render(BIG, 3, (0.0, 0.0, d), intensity=intensity, kd=kd, ks=ks, alpha=alpha)
        assert np.allclose(out3['rgb'][CENTRE], want, rtol=0.05) and np.all(out3['coverage'] == 1.0)


def test_occluder_between_light_and_surface_gives_exactly_zero():
    """Light at z = 40, camera at z = 16, occluder at z = 28: above the camera, so only light rays cross it."""
    occluder = np.array([[[-0.5, -0.5, 28.0], [0.5, -0.5, 28.0], [0.0, 1.0, 28.0]]])
    tv = np.concatenate((BIG, occluder))
    light = (0.0, 0.0, 40.0)
    free = render(BIG, 1, light)
    out = render(tv, 1, light)
    assert free['rgb'][CENTRE].min() > 0
    assert np.all(out['rgb'][CENTRE] == 0.0) and out['shadowed'][CENTRE] == 1 and out['coverage'][CENTRE] == 1.0
    # the shadow of the occluder on z = 0 is its image scaled by 40 / 12 about the axis: within |x| < 1.7, -1.7 < y < 3.4, so
    # the image corners (|x| >= 3, |y| >= 3) stay lit and equal to the render without it
    for p in (0, IMW - 1, (IMH - 1) * IMW, IMH * IMW - 1):
        assert out['lit'][p] == 1 and np.array_equal(out['rgb'][p], free['rgb'][p])


def test_half_plane_edge_coverage_and_alpha():
    """A triangle with a vertical edge at x = 1.2: the S = 4 sample columns of pixel column 5 lie at x = 0.625, 0.875, 1.125, 1.375,
    so three of four are covered: coverage 12 / 16 exactly.  Columns 0 .. 4 are covered, 6 and 7 are not."""
    tv = np.array([[[1.2, -300.0, 0.0], [1.2, 300.0, 0.0], [-500.0, 0.0, 0.0]]])
    out = render(tv, 4, (0.0, 0.0, 5.0))
    cov = out['coverage'].reshape(IMH, IMW)
    assert cov.dtype == np.float32
    assert np.all(cov[:, :5] == 1.0) and np.all(cov[:, 5] == np.float32(12 / 16)) and np.all(cov[:, 6:] == 0.0)
    assert np.all(out['rgb'].reshape(IMH, IMW, 3)[:, 6:] == 0.0)
    full = render(BIG, 4, (0.0, 0.0, 5.0))['rgb'].reshape(IMH, IMW, 3)
    edge = out['rgb'].reshape(IMH, IMW, 3)[:, 5]
    assert np.all(edge > 0.5 * full[:, 5]) and np.all(edge < full[:, 5])                # 12 of 16 samples, the nearer ones
    alpha = SH.to_uint8(torch.from_numpy(cov)).numpy()
    assert alpha.dtype == np.uint8 and set(alpha[:, 5]) == {191} and set(alpha[:, 4]) == {255} and set(alpha[:, 6]) == {0}   # int(.75*255)


def test_back_facing_triangle_is_shaded_on_its_flipped_normal():
    d, kd = 5.0, (0.9, 0.5, 0.2)
    back = np.ascontiguousarray(BIG[:, [0, 2, 1]])                                       # clockwise: normal -z
    out = render(back, 1, (0.0, 0.0, d), kd=kd)
    want = closed_form(d, 1.0, kd, 0.04, 0.5)
    got = out['rgb'][CENTRE].astype(np.float64)
    assert np.all(np.abs(got - want) <= 2 * EPS32 * want) and out['flipped'][CENTRE] == 1 and out['flipped'].sum() == IMH * IMW
    # a light behind the (two-sided) surface as the camera sees it: black
    below = render(back, 1, (0.0, 0.0, -d), kd=kd)
    assert np.all(below['rgb'] == 0.0) and below['lit'].sum() == 0 and np.all(below['coverage'] == 1.0)


def test_vertex_attributes_blend_with_the_barycentrics():
    """Corner colours red, green, blue on BIG: the centre pixel's kd is the barycentric blend at the origin, which is
    (0.3125, 0.3125, 0.375) for these vertices; corner normals all +z change nothing, all-zero ones fall back to the geometric one."""
    rgb = np.eye(3)[None]
    light, kw = (0.0, 0.0, 5.0), dict(ks=0.0)
    got = render(BIG, 1, light, tri_rgb=rgb, **kw)['rgb'][CENTRE].astype(np.float64)
    want = closed_form(5.0, 1.0, (0.3125, 0.3125, 0.375), 0.0, 0.5)
    assert np.all(np.abs(got - want) <= 2 * EPS32 * want)
    base = render(BIG, 1, light, **kw)['rgb']
    up = np.tile([0.0, 0.0, 1.0], (1, 3, 1))
    assert np.array_equal(render(BIG, 1, light, tri_normals=up, **kw)['rgb'], base)
    assert np.array_equal(render(BIG, 1, light, tri_normals=np.zeros((1, 3, 3)), **kw)['rgb'], base)
    tilted = render(BIG, 1, light, tri_normals=np.tile([0.6, 0.0, 0.8], (1, 3, 1)), **kw)['rgb'][CENTRE].astype(np.float64)
    assert np.all(np.abs(tilted - 0.8 * base[CENTRE]) <= 4 * EPS32 * base[CENTRE])       # ci = 0.8


def test_corner_normals_are_area_weighted_and_skip_degenerate_triangles():
    # two triangles at a right angle sharing the edge 0-2: e1 x e2 = (0, 0, 1) and (2, 0, 0), so the shared vertices get (2, 0, 1) / sqrt 5
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 2]])
    fold = M.Mesh(v, [[0, 1, 2], [0, 2, 3]], device=None)
    s = np.array([2.0, 0, 1]) / np.sqrt(5.0)
    assert np.allclose(M.corner_normals(fold), [[s, [0, 0, 1], s], [s, s, [1, 0, 0]]], atol=1e-15)
    vs, fs = R.icosphere(2)
    ball = M.Mesh(vs, fs.tolist(), device=None)
    n = M.corner_normals(ball)
    assert n.shape == (ball.n_tris, 3, 3) and np.allclose(np.linalg.norm(n, axis=2), 1.0)
    assert ((n * ball.tri_verts).sum(2) > 0.999).all()                                   # on a sphere: radial to within 2.6 degrees
    cube = M.Mesh.load(R.CUBE, device=None)                                              # quads: fan-triangulated first
    assert M.corner_normals(cube).shape == (12, 3, 3)
    lone = M.Mesh(np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0]]), [[0, 1, 2]], device=None)
    assert np.array_equal(M.corner_normals(lone), np.zeros((1, 3, 3)))


# ---------------------------------------------------------------- rig
@pytest.mark.parametrize('hemisphere', [False, True])
def test_rig_names_projection_and_euler_round_trip(hemisphere):
    target = np.array([0.3, -0.2, 0.5])
    cams, lights = RIG.light_stage(7, 5, 2.5, target, focal_length=50.0, sensor=(32.0, 24.0), hemisphere=hemisphere)
    assert len(cams) == 7 and len(lights) == 5
    assert len({c['name'] for c in cams} | {l['name'] for l in lights}) == 12
    assert all(set(c) == {'name', 'position', 'rotation', 'focal_length', 'sensor_width', 'sensor_height', 'clip_start', 'clip_end'} for c in cams)
    assert all(set(l) == {'name', 'position', 'size'} for l in lights)
    again = RIG.light_stage(7, 5, 2.5, target, hemisphere=hemisphere)
    assert again == (cams, lights)                                                      # deterministic
    for c in cams + lights:
        p = np.asarray(c['position'])
        assert abs(np.linalg.norm(p - target) - 2.5) <= 1e-12 and (not hemisphere or p[2] > target[2])
    pos = np.array([c['position'] for c in cams] + [l['position'] for l in lights])
    dist = np.linalg.norm(pos[:, None] - pos[None], axis=2) + 10 * np.eye(len(pos))
    assert dist.min() > 0.1                                                             # no light sits in a camera
    for c in cams:
        mat, _, (imh, imw) = M.camera_matrix(c, 24)
        assert (imh, imw) == (24, 32)
        h = mat @ np.append(target, 1.0)
        assert h[2] > 0 and np.allclose(h[:2] / h[2], [imw / 2, imh / 2], rtol=0, atol=1e-9)
        r = M.euler_xyz_matrix(c['rotation'])
        assert np.allclose(r @ r.T, np.eye(3), atol=1e-14)
        back = -r[:, 2]                                                                  # the camera looks down its -z
        assert np.allclose(back, (target - c['position']) / 2.5, atol=1e-12)
        assert np.allclose(M.euler_xyz_matrix(RIG.look_at_euler(c['position'], target)), r, atol=1e-14)
        assert r[2, 1] >= -1e-12                                                        # y up: the image is not upside down


def test_rig_phase_gives_held_out_positions_and_straight_down_works():
    cams, _ = RIG.light_stage(4, 4, 2.0, (0, 0, 0))
    held, _ = RIG.light_stage(4, 4, 2.0, (0, 0, 0), phase=1.0, cam_prefix='VC')
    a, b = np.array([c['position'] for c in cams]), np.array([c['position'] for c in held])
    assert np.allclose(a[:, 2], b[:, 2]) and np.linalg.norm(a[:, None] - b[None], axis=2).min() > 0.1
    assert [c['name'] for c in held] == ['VC000', 'VC001', 'VC002', 'VC003']
    r = M.euler_xyz_matrix(RIG.look_at_euler((0.0, 0.0, 3.0), (0.0, 0.0, 0.0)))
    assert np.allclose(r[:, 2], [0, 0, 1], atol=1e-14) and np.allclose(r @ r.T, np.eye(3), atol=1e-14)


# ---------------------------------------------------------------- driver plumbing
def _numpy_neighbors(phys_and_virt, phys, k=1, device=None):
    """get_neighbors' rule on the host: the nearest physical entry at non-zero distance, the first minimum."""
    out = {}
    for ref in phys_and_virt:
        d = np.array([np.linalg.norm(np.asarray(ref['position']) - np.asarray(p['position'])) for p in phys])
        d[d == 0] = np.inf
        out[ref['name']] = phys[int(d.argmin())]['name']
    return out


def test_parse_args_and_rig_of_the_driver():
    a = CM.parse_args(['--mesh', 'm.ply', '--uv_unwrap', 'u.pickle', '--outroot', 'out', '--n_cams', '3', '--n_lights', '4', '--n_test', '2',
                       '--kd', '0.1,0.2,0.3', '--flat', '--spp', '4'])
    assert (a.n_cams, a.n_lights, a.n_test, a.imh, a.uvs, a.spp) == (3, 4, 2, 512, 1024, 4)
    assert a.kd == (0.1, 0.2, 0.3) and a.flat and a.exposure is None and a.ks == 0.04 and a.roughness == 0.5
    for bad in (['--spp', '5'], ['--spp', '0'], ['--spp', '100'], ['--kd', '1,2']):
        with pytest.raises(SystemExit):
            CM.parse_args(['--mesh', 'm', '--uv_unwrap', 'u', '--outroot', 'o'] + bad)
    assert [SH.spp_side(s) for s in (1, 4, 9, 16, 64)] == [1, 2, 3, 4, 8]
    cams, lights, pairs, rig = CM.build_rig(a, np.array([0.0, 0.0, 1.0]), 2.0)
    assert len(cams) == 3 and len(lights) == 4 and len(pairs) == 2 and rig['radius'] == 9.0 and rig['target'] == [0.0, 0.0, 1.0]
    names = [c['name'] for c in cams] + [c['name'] for c, _ in pairs] + [l['name'] for l in lights] + [l['name'] for _, l in pairs]
    assert len(set(names)) == len(names) and not any('_' in n for n in names)
    held = np.array([c['position'] for c, _ in pairs])
    assert np.linalg.norm(held[:, None] - np.array([c['position'] for c in cams])[None], axis=2).min() > 0.1


def test_neighbor_tables_are_get_neighbors_on_the_same_dicts(monkeypatch):
    from nlt_amd.data_gen import get_neighbors as GN
    calls = []

    def spy(phys_and_virt, phys, k=1, device='cuda'):
        calls.append(([o['name'] for o in phys_and_virt], [o['name'] for o in phys]))
        return _numpy_neighbors(phys_and_virt, phys)
    monkeypatch.setattr(GN, 'get_neighbors', spy)
    cams, lights = RIG.light_stage(3, 4, 2.0, (0, 0, 0))
    tc, tl = RIG.light_stage(2, 2, 2.0, (0, 0, 0), phase=1.0, cam_prefix='VC', light_prefix='VL')
    cam_nn, light_nn = CM.neighbor_tables(cams, lights, tc, tl)
    assert calls == [(['C000', 'C001', 'C002', 'VC000', 'VC001'], ['C000', 'C001', 'C002']),
                     (['L000', 'L001', 'L002', 'L003', 'VL000', 'VL001'], ['L000', 'L001', 'L002', 'L003'])]
    assert cam_nn == _numpy_neighbors(cams + tc, cams) and light_nn == _numpy_neighbors(lights + tl, lights)
    assert all(v in {'C000', 'C001', 'C002'} and v != k for k, v in cam_nn.items())


def test_default_exposure_maps_a_white_lambert_surface_to_point_eight():
    """The rule, and that it is the rule of the renderer: a white Lambert surface (kd = 1, ks = 0) facing a light 5 away."""
    e = CM.default_exposure(5.0, intensity=3.0)
    assert e == 0.8 * math.pi * 25.0 / 3.0
    out = render(BIG, 1, (0.0, 0.0, 5.0), intensity=3.0, kd=(1.0, 1.0, 1.0), ks=0.0)
    assert np.allclose(e * out['rgb'][CENTRE].astype(np.float64), 0.8, rtol=4 * EPS32, atol=0)
    centre, half = CM.mesh_box(M.Mesh.load(R.CUBE, device=None))
    cube = M.load_mesh(R.CUBE)['vertices']
    assert np.allclose(centre, (cube.min(0) + cube.max(0)) / 2) and np.isclose(half, np.linalg.norm(cube.max(0) - cube.min(0)) / 2)


def test_material_checks_its_arguments():
    with pytest.raises(ValueError):
        SH.Material(kd=(1, 2))
    m = SH.Material(vertex_rgb=np.zeros((5, 3)), smooth=False)
    assert m.to_json() == dict(kd=[0.8, 0.8, 0.8], vertex_rgb=True, ks=0.04, roughness=0.5, smooth=False)
    for bad in (0, 2, 81, 3.5):
        with pytest.raises(ValueError):
            SH.spp_side(bad)
