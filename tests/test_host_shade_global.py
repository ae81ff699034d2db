"""CPU: tests/shade_global_ref.py (the brute force nlt_render_global is held to on the GPU) against closed forms, and the host
logic around the new entry point: the two sample tables of data_gen/shade.py, `render_view`'s choice of entry point,
capture_main's flags and the argument checks, which answer before any launch.

The closed-form scenes use the camera of tests/test_host_shade.py: on the z axis at height 16, looking straight down at z = 0,
8 x 8 pixels; pixel (px, py) sees the world point (px - 4, 4 - py, 0).  Tolerance of the closed forms: that file's, 2 float32
epsilons of the expected value (one rounding to float32 of a float64 result that carries a few float64 roundings)."""
import ctypes
import json
import math
import types

import numpy as np
import pytest
import torch

import raycast_ref as R
import shade_global_ref as G
import shade_ref as S
from nlt_amd import capi as C
from nlt_amd.data_gen import capture_main as CM
from nlt_amd.data_gen import mesh as M
from nlt_amd.data_gen import shade as SH
from test_gpu_shade import cube_cam, host_mesh, occluder_cam
from test_host_shade import BIG, CAM, CENTRE, EPS32, IMH, IMW, INV


def quad(x0, x1, y0, y1, z):
    """Two counter-clockwise (normal +z) triangles."""
    a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
    return np.array([[a, b, c], [a, c, d]], np.float64)


def render(tv, spp_side, light, **kw):
    return G.render(tv, INV, CAM['position'], IMH, IMW, spp_side, light, **kw)


# A floor x in [2, 4.4] and, 2 above the floor point (3, 0, 0) that pixel (7, 4) sees, a small ceiling.  (3, 0, 0) lies off the
# floor's diagonal: a primary hit exactly on an edge two triangles share leaves from one of them only, and its bounce rays hit the
# coplanar neighbour at t = 0 -- the definition masks the hit triangle alone.  The primary ray crosses z = 2 at x = 2.625, beside the ceiling.  The light at (8, 0, -1) lies below the floor's plane (the floor point does not face it)
# and sees the ceiling's underside: its ray to (3, 0, 2) crosses z = 0 at x = 6.33, beside the floor.
FLOOR, CEILING = quad(2.0, 4.4, -1.0, 1.0, 0.0), quad(2.8, 3.4, -0.2, 0.2, 2.0)
ROOM = np.concatenate((FLOOR, CEILING))
PIXEL = 4 * IMW + 7
LIGHT = (8.0, 0.0, -1.0)
STRAIGHT_UP = np.zeros((1, 1, 2))                                  # one bounce ray: the direction n itself
KD_FLOOR, KD_CEIL = np.array([0.9, 0.5, 0.2]), np.array([0.3, 0.6, 0.8])


def room_rgb(ceil):
    return np.concatenate((np.broadcast_to(KD_FLOOR, (2, 3, 3)), np.broadcast_to(ceil, (2, 3, 3))))


def test_one_bounce_closed_form():
    intensity = 7.0
    out = render(ROOM, 1, LIGHT, intensity=intensity, tri_rgb=room_rgb(KD_CEIL), bounce_pts=STRAIGHT_UP)
    r2 = 5.0 ** 2 + 3.0 ** 2
    want = KD_FLOOR * (intensity / r2 * (3.0 / math.sqrt(r2)) * KD_CEIL / math.pi)
    got = out['rgb'][PIXEL].astype(np.float64)
    assert np.all(np.abs(got - want) <= 2 * EPS32 * want), (got, want)
    assert np.array_equal(out['rgb_indirect'][PIXEL], out['rgb'][PIXEL]) and np.all(out['direct'][PIXEL] == 0.0)
    assert out['hits'][PIXEL] == 1 and out['light_not_facing'][PIXEL] == 1 and out['bounce_hit'][PIXEL] == 1
    assert out['secondary_lit'][PIXEL] == 1 and out['secondary_flipped'][PIXEL] == 1       # the ceiling's normal is +z: flipped
    # the ceiling wound the other way: the same light
    other = render(np.concatenate((FLOOR, CEILING[:, [0, 2, 1]])), 1, LIGHT, intensity=intensity, tri_rgb=room_rgb(KD_CEIL),
                   bounce_pts=STRAIGHT_UP)
    assert other['secondary_flipped'][PIXEL] == 0
    assert np.all(np.abs(other['rgb'][PIXEL].astype(np.float64) - want) <= 2 * EPS32 * want)
    # the mean over two identical bounce rays is the one ray's value
    twice = render(ROOM, 1, LIGHT, intensity=intensity, tri_rgb=room_rgb(KD_CEIL), bounce_pts=np.zeros((1, 2, 2)))
    assert np.all(np.abs(twice['rgb'][PIXEL].astype(np.float64) - want) <= 2 * EPS32 * want) and twice['bounce_hit'][PIXEL] == 2


def test_no_second_surface_gives_the_direct_render():
    """A lone quad and a lone triangle.  Samples on the quad's diagonal hit the coplanar other triangle at t = 0; that hit's normal
    is turned away from the ray, so away from the light above: it adds exactly nothing as well."""
    light = (0.5, 0.3, 5.0)
    table = SH.bounce_table(4, 4)
    for tv in (quad(-3.0, 3.0, -3.0, 3.0, 0.0), BIG):
        out = render(tv, 2, light, kd=(0.9, 0.5, 0.2), bounce_pts=table)
        want = S.render(tv, INV, CAM['position'], IMH, IMW, 2, light, kd=(0.9, 0.5, 0.2))
        assert not out['rgb_indirect'].any() and out['secondary_lit'].sum() == 0
        assert out['bounce_hit'].sum() + out['bounce_missed'].sum() == 4 * out['hits'].sum() and out['bounce_skipped'].sum() == 0
        assert tv is not BIG or out['bounce_hit'].sum() == 0
        assert out['rgb'].any() and np.array_equal(out['rgb'].view(np.int32), want['rgb'].view(np.int32))
        assert np.array_equal(out['coverage'], want['coverage'])


def test_black_second_surface_gives_exactly_zero():
    lit = render(ROOM, 1, LIGHT, tri_rgb=room_rgb(KD_CEIL), bounce_pts=STRAIGHT_UP)
    black = render(ROOM, 1, LIGHT, tri_rgb=room_rgb(np.zeros(3)), bounce_pts=STRAIGHT_UP)
    assert lit['rgb_indirect'][PIXEL].min() > 0 and black['secondary_lit'][PIXEL] == 1
    assert not black['rgb_indirect'][PIXEL].any() and not black['rgb'][PIXEL].any()


def test_penumbra_two_of_four_light_points():
    """Light centre (0, 0, 40), radius 1; a half plane x < 0 at z = 28 (above the camera: only light rays cross it).  The rays from
    the four light points to the origin cross z = 28 at x = 0.7 * Lk.x = 0.7, -0.7, 0.42, -0.42: two pass, two are blocked."""
    half = np.array([[[0.0, -300.0, 28.0], [0.0, 300.0, 28.0], [-500.0, 0.0, 28.0]]])
    tv = np.concatenate((BIG, half))
    pts = np.array([[[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.6, 0.8, 0.0], [-0.6, 0.8, 0.0]]])
    centre, kw = np.array([0.0, 0.0, 40.0]), dict(intensity=90.0, kd=(0.9, 0.5, 0.2))
    out = render(tv, 1, centre, light_radius=1.0, light_pts=pts, **kw)
    assert out['light_unoccluded'][CENTRE] == 2 and out['light_occluded'][CENTRE] == 2 and out['light_not_facing'][CENTRE] == 0
    want = sum(S.render(BIG, INV, CAM['position'], IMH, IMW, 1, centre + pts[0, k], intensity=90.0 / 4, kd=kw['kd'])['rgb'][CENTRE]
               .astype(np.float64) for k in (0, 2))
    got = out['rgb'][CENTRE].astype(np.float64)
    assert np.all(want > 0) and np.all(np.abs(got - want) <= 2 * EPS32 * want), (got, want)
    free = render(BIG, 1, centre, light_radius=1.0, light_pts=pts, **kw)
    assert free['light_unoccluded'][CENTRE] == 4 and np.all(free['rgb'][CENTRE] > 1.9 * out['rgb'][CENTRE])
    # a pixel well inside the lit half and one well inside the shadow: all or nothing
    assert out['light_unoccluded'][4 * IMW + 7] == 4 and out['light_occluded'][4 * IMW + 0] == 4 and not out['rgb'][4 * IMW + 0].any()


@pytest.mark.parametrize('scene', ['cube', 'occluder'])
def test_degenerate_arguments_are_the_direct_reference_bit_for_bit(scene):
    h = host_mesh(scene)
    cam, imh, light = (cube_cam(), 9, (5.0, -1.002, 0.5)) if scene == 'cube' else (occluder_cam(), 18, (0.1, 0.2, 5.0))
    _, inv, (imh, imw) = M.camera_matrix(cam, imh)
    kw = dict(intensity=20.0, kd=(0.7, 0.6, 0.5), ks=0.04, alpha=0.5, tri_normals=M.corner_normals(h))
    want = S.render(h.tri_verts, inv, cam['position'], imh, imw, 2, light, **kw)
    got = G.render(h.tri_verts, inv, cam['position'], imh, imw, 2, light, light_radius=0.0, light_pts=SH.light_table(1, 4), **kw)
    assert want['rgb'].any() and np.array_equal(got['rgb'].view(np.int32), want['rgb'].view(np.int32))
    assert np.array_equal(got['coverage'].view(np.int32), want['coverage'].view(np.int32)) and not got['rgb_indirect'].any()
    assert np.array_equal(got['light_unoccluded'], want['lit']) and np.array_equal(got['light_occluded'], want['shadowed'])


# ---------------------------------------------------------------- the tables
@pytest.mark.parametrize('n,n_sets', [(1, 1), (5, 4), (4, 9), (64, 3)])
def test_tables_shapes_ranges_and_the_round_robin_deal(n, n_sets):
    b, l = SH.bounce_table(n, n_sets), SH.light_table(n, n_sets)
    assert b.shape == (n_sets, n, 2) and l.shape == (n_sets, n, 3) and b.dtype == l.dtype == np.float64
    assert not b.flags.writeable and not l.flags.writeable and b.flags.c_contiguous and l.flags.c_contiguous
    assert SH.bounce_table(n, n_sets) is b and SH.light_table(n, n_sets) is l                      # cached per argument pair
    assert ((b * b).sum(-1) <= 1.0).all()
    assert np.abs(np.sqrt((l * l).sum(-1)) - 1.0).max() <= 2 * np.finfo(np.float64).eps
    # deterministic: the same numbers from the definition, point q in set q mod n_sets at row q // n_sets
    total = n * n_sets
    q = np.arange(total, dtype=np.float64)
    r, phi = np.sqrt((q + 0.5) / total), q * (np.pi * (3.0 - np.sqrt(5.0)))
    disc = np.stack((r * np.cos(phi), r * np.sin(phi)), 1)
    from nlt_amd.data_gen.rig import fibonacci_sphere
    sphere = fibonacci_sphere(total)
    sphere = sphere / np.sqrt((sphere * sphere).sum(1))[:, None]
    for k in range(total):
        assert np.array_equal(b[k % n_sets, k // n_sets], disc[k]) and np.array_equal(l[k % n_sets, k // n_sets], sphere[k])
    if n_sets > 1 and n > 1:
        # every set spans the disc: its radii reach into the outer and the inner half
        rad = np.sqrt((b * b).sum(-1))
        assert (rad.max(1) > 0.7).all() and (rad.min(1) < 0.7).all()


def test_tables_edge_arguments():
    assert SH.bounce_table(0, 4).shape == (4, 0, 2)
    for bad in ((-1, 1), (1, 0)):
        with pytest.raises(ValueError):
            SH.bounce_table(*bad)
    for bad in ((0, 1), (1, 0)):
        with pytest.raises(ValueError):
            SH.light_table(*bad)


# ---------------------------------------------------------------- render_view and the driver
class _FakeCapi:
    def __init__(self):
        self.calls = []

    def render_direct(self, *a):
        self.calls.append(('direct', a))
        return torch.zeros((9 * 13, 3)), torch.zeros(9 * 13)

    def render_global(self, *a):
        self.calls.append(('global', a))
        return torch.zeros((9 * 13, 3)), torch.zeros(9 * 13), torch.zeros((9 * 13, 3))

    def relight_finish(self, acc, exposure, to_srgb):
        return acc[0]


def test_render_view_reaches_the_new_binding_only_when_asked(monkeypatch):
    fake = _FakeCapi()
    monkeypatch.setattr(SH, 'C', fake)
    monkeypatch.setattr(SH, 'render_geometry', lambda *a, **kw: kw)
    mesh = types.SimpleNamespace(bvh=(None, None), n_tris=12, device='cpu')
    cam, light, mat = cube_cam(), dict(name='L', position=[5.0, -1.0, 0.5], size=0.125), SH.Material(smooth=False)
    out = SH.render_view(mesh, None, cam, light, 9, 32, 4, mat, 2.0)
    assert [c[0] for c in fake.calls] == ['direct'] and out['rgb_camspc'].shape == (9, 13, 3) and out['alpha'].shape == (9, 13)
    for kw, want in ((dict(bounces=3), (0.125, 1, 3)), (dict(light_samples=2), (0.125, 2, 0)), (dict(light_size=0.0), (0.0, 1, 0)),
                     (dict(bounces=2, light_samples=5, light_size=0.5), (0.5, 5, 2))):
        del fake.calls[:]
        SH.render_view(mesh, None, cam, light, 9, 32, 4, mat, 2.0, **kw)
        (kind, a), = fake.calls
        radius, lpts, bpts = a[-3:]
        assert kind == 'global' and radius == want[0] and tuple(lpts.shape) == (4, want[1], 3) and lpts.dtype == torch.float64
        assert (bpts is None) if want[2] == 0 else (tuple(bpts.shape) == (4, want[2], 2) and bpts.dtype == torch.float64)
        assert np.array_equal(lpts.numpy(), SH.light_table(want[1], 4))
    for bad in (dict(bounces=65), dict(light_samples=0), dict(light_size=-1.0), dict(light_size=float('nan'))):
        with pytest.raises(ValueError):
            SH.render_view(mesh, None, cam, light, 9, 32, 4, mat, 2.0, **bad)


def test_capture_main_flags_reach_the_renderer_the_light_jsons_and_capture_json(monkeypatch, tmp_path):
    base = ['--mesh', 'm.ply', '--uv_unwrap', 'u.pickle', '--outroot', 'o', '--n_cams', '2', '--n_lights', '2', '--n_test', '1', '--spp', '4']
    a = CM.parse_args(base)
    assert (a.bounces, a.light_samples, a.light_size) == (0, 1, None)
    for bad in (['--bounces', '-1'], ['--bounces', '65'], ['--light_samples', '0'], ['--light_samples', '65'], ['--light_size', '-0.1'],
                ['--light_size', 'nan']):
        with pytest.raises(SystemExit):
            CM.parse_args(base + bad)
    _, lights, pairs, _ = CM.build_rig(a, np.zeros(3), 1.0)
    assert all(l['size'] == 0.1 for l in lights) and pairs[0][1]['size'] == 0.1                   # as before without the flag
    a = CM.parse_args(base + ['--bounces', '2', '--light_samples', '3', '--light_size', '0.05'])
    assert (a.bounces, a.light_samples, a.light_size) == (2, 3, 0.05)
    cams, lights, pairs, rig = CM.build_rig(a, np.zeros(3), 1.0)
    assert all(l['size'] == 0.05 for l in lights) and pairs[0][1]['size'] == 0.05
    seen, written = [], []
    monkeypatch.setattr(CM, 'render_view', lambda *args: seen.append(args) or {})
    monkeypatch.setattr(CM, 'write_sample', lambda path, sample, cam, light, nn, workers=None: written.append(light))
    monkeypatch.setattr(CM, 'neighbor_tables', lambda *args, **kw: ({}, {}))
    monkeypatch.setattr(CM.postproc, 'postprocess', lambda *args, **kw: {})
    root = str(tmp_path / 'cap')
    for kw in (dict(), dict(bounces=a.bounces, light_samples=a.light_samples, light_size=a.light_size)):
        del seen[:], written[:]
        _, info = CM.write_capture(host_mesh('cube'), {'uv': None}, root, cams, lights, pairs, imh=9, uvs=8, spp=4, rig=rig, **kw)
        want = (kw.get('bounces', 0), kw.get('light_samples', 1), kw.get('light_size'))
        assert len(seen) == 5 and all(s[-3:] == want for s in seen) and all(l['size'] == 0.05 for l in written)
        rec = json.load(open(root + '.capture.json'))
        assert rec == info and (rec['bounces'], rec['light_samples'], rec['light_size']) == want


def test_default_exposure_is_a_rule_of_the_direct_light():
    assert 'direct light' in CM.default_exposure.__doc__ and CM.default_exposure(5.0, 3.0) == 0.8 * math.pi * 25.0 / 3.0


# ---------------------------------------------------------------- the entry point without a GPU
def test_bad_arguments_return_status_codes_without_a_gpu():
    """Every call below is refused by the argument checks, so nothing is launched: safe on a machine with no GPU."""
    L = C.lib()
    P = 4096                                            # a non-null fake pointer: checked, never dereferenced here
    host = (ctypes.c_double * 19)(*([0.0] * 19))
    ok = dict(tris=P, nodes=P, n_tris=12, cam=ctypes.addressof(host), imh=9, imw=13, s=2, radius=0.1, lpts=P, n_l=2, n_lsets=4, bpts=P,
              n_b=3, n_bsets=4, rgb=P, cov=P, ind=P)

    def call(**kw):
        a = dict(ok, **kw)
        return L.nlt_render_global(a['tris'], a['nodes'], a['n_tris'], None, None, a['cam'], a['imh'], a['imw'], a['s'], 1.0, 2.0, 3.0, 1.0,
                                   0.8, 0.8, 0.8, 0.04, 0.5, a['radius'], a['lpts'], a['n_l'], a['n_lsets'], a['bpts'], a['n_b'],
                                   a['n_bsets'], a['rgb'], a['cov'], a['ind'], None)
    for name in ('tris', 'nodes', 'cam', 'lpts', 'rgb', 'cov'):
        assert call(**{name: None}) == -1, name
    assert call(bpts=None) == -1                                                         # NULL bounce table with n_b > 0
    for kw in (dict(n_l=0), dict(n_l=65), dict(n_l=-1), dict(n_b=-1), dict(n_b=65), dict(n_lsets=0), dict(n_bsets=0), dict(n_bsets=-3),
               dict(radius=-0.5), dict(radius=float('nan')), dict(radius=float('inf')), dict(s=0), dict(s=9), dict(imh=0), dict(imw=0),
               dict(n_tris=0)):
        assert call(**kw) == -1, kw
    assert call(n_tris=1 << 31) == -2 and call(imh=1 << 15, imw=1 << 15) == -2
    assert 'nlt_render_global' in C.SIGNATURES
