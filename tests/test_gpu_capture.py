"""-m gpu: the capture writer's three fused launches (csrc/assemble.hip: nlt_capture_camspc, nlt_capture_uvspc, nlt_diffuse_bases)
bit for bit against tests/capture_ref.py's compositions of oracle/buffers.py, and the written capture read back on the device
(load_store -> Dataset.load_batch, eager and store-resident, at the stored and at another trained resolution).
Integers, bytes and float16 bit patterns throughout: every assertion is np.array_equal."""
import numpy as np
import pytest
import torch

import capture_ref as R
import nlt_amd
from nlt_amd import capi as C
from nlt_amd.data_gen import postproc as P
from nlt_amd.datasets import nlt as D
from oracle import buffers as B

pytestmark = pytest.mark.gpu

_dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
_bits = lambda a: a.view(np.uint16)


def unit_map(rng, h, w, zeros=0.0, ties=0.0):
    """A [h,w,2] float64 map over [-0.05, 1.05] (the .png clip is exercised on both sides); `zeros`: share of exact (0, 0)
    entries (background); `ties`: share of values moved onto -- or 2^-40 relative beside -- the midpoint of two neighbouring
    float16 values, where a conversion that rounds to float32 first goes the wrong way."""
    m = rng.random((h, w, 2)) * 1.1 - 0.05
    if ties:
        lo = m.astype(np.float16)
        hi = np.nextafter(lo, np.float16(2))
        mid = (lo.astype(np.float64) + hi.astype(np.float64)) / 2          # exact: 12 significant bits
        mid = mid * (1 + rng.choice([0.0, 2.0 ** -40, -2.0 ** -40], m.shape))
        m = np.where(rng.random(m.shape) < ties, mid, m)
    if zeros:
        m[rng.random((h, w)) < zeros] = 0
    return m


# ----------------------------------------------------------------------------- nlt_capture_camspc
@pytest.mark.parametrize('imh,imw', [(1, 1), (37, 53), (512, 512)])
def test_capture_camspc_bit_exact(imh, imw):
    rng = np.random.default_rng(imh * 7 + imw)
    p = imh * imw
    valid = (rng.random(p) > 0.2).astype(np.uint8)
    valid[0] = 1
    occluded = (rng.random(p) < 0.3).astype(np.uint8)
    locs, normals = rng.random((p, 3)) * 4 - 2, rng.random((p, 3)) * 2 - 1
    normals[0] = 0                                                  # one zero normal (normalises to itself)
    if p > 1:
        occluded[0], occluded[1], valid[1] = 0, 1, 1                # a lit and a shadowed hit whatever the draw
    alpha = rng.choice(np.array([0, 1, 254, 255], np.uint8), (imh, imw))
    uv2cam = unit_map(rng, imh, imw, ties=0.25)
    cam, light = (0.3, -2.5, 1.0), (-1.0, 0.5, 2.0)
    for a, oc in ((alpha, occluded), (None, None)):
        got = C.capture_camspc(_dev(locs), _dev(normals), _dev(valid), _dev(oc), cam, light, _dev(a), _dev(uv2cam))
        want = R.capture_camspc_np(locs, normals, valid, oc, cam, light, a, uv2cam)
        torch.cuda.synchronize()
        cvis, lvis, f16, png = (t.cpu().numpy() for t in got)
        assert f16.dtype == np.float16 and f16.shape == (imh, imw, 2) and png.shape == (imh, imw, 3)
        assert np.array_equal(cvis, want[0]) and np.array_equal(lvis, want[1])
        assert np.array_equal(_bits(f16), _bits(want[2])) and np.array_equal(png, want[3])
    if p > 1:                                                       # the case reached what it is meant to
        shadowed = R.capture_camspc_np(locs, normals, valid, occluded, cam, light, None, uv2cam)[1]
        assert (want[1] != shadowed).any() and (want[1] > 0).any() and (want[0] > 0).any()      # cast shadows reached lvis alone
        twice = uv2cam.astype(np.float32).astype(np.float16)        # rounding twice differs somewhere: the ties are live
        assert (_bits(twice) != _bits(uv2cam.astype(np.float16))).any()
        assert (png[:, :, :2] == 255).any() and (png[:, :, :2] == 0).any() and not png[:, :, 2].any()


# ----------------------------------------------------------------------------- nlt_capture_uvspc
@pytest.mark.parametrize('imh,imw,uvs', [(9, 12, 16), (37, 53, 40), (512, 512, 1024)])
@pytest.mark.parametrize('ldm,ld_rgb', [(2, 3), (3, 4), (2, None)])
def test_capture_uvspc_bit_exact(imh, imw, uvs, ldm, ld_rgb):
    rng = np.random.default_rng(imh + uvs + ldm)
    cam2uv = unit_map(rng, uvs, uvs, zeros=0.3)
    if ldm == 3:
        cam2uv = np.dstack((cam2uv, rng.random((uvs, uvs))))        # (add_b_ch's third channel: never read)
    U8 = lambda *s: rng.integers(0, 256, s, dtype=np.uint8)
    cvis_c, lvis_c = U8(imh, imw), U8(imh, imw)
    rgb_c = None if ld_rgb is None else U8(imh, imw, ld_rgb)
    got = C.capture_uvspc(_dev(cam2uv), _dev(cvis_c), _dev(lvis_c), _dev(rgb_c))
    torch.cuda.synchronize()
    want = (B.remap_u8(cvis_c, cam2uv), B.remap_u8(lvis_c, cam2uv),
            None if rgb_c is None else B.remap_u8(np.ascontiguousarray(rgb_c[:, :, :3]), cam2uv)) + R.map_files(cam2uv)
    assert (got[2] is None) == (rgb_c is None)
    for g, w, name in zip(got, want, ('cvis', 'lvis', 'rgb', 'cam2uv.npy', 'cam2uv.png')):
        if w is not None:
            g = g.cpu().numpy()
            assert g.dtype == w.dtype and g.shape == w.shape, name
            assert np.array_equal(g.view(np.uint16) if g.dtype == np.float16 else g, w.view(np.uint16) if w.dtype == np.float16 else w), name


def test_capture_uvspc_identity_mapping_is_a_copy():
    """cam2uv = (j / w, i / h): every texel lands on a pixel centre of the fixed-point grid -> the source itself, its top-left
    pixel (where the background samples from) forced black."""
    s = 16
    rng = np.random.default_rng(1)
    j, i = np.meshgrid(np.arange(s), np.arange(s))
    cam2uv = np.dstack((j / s, i / s)).astype(np.float64)
    src = [rng.integers(1, 256, (s, s), dtype=np.uint8), rng.integers(1, 256, (s, s), dtype=np.uint8), rng.integers(1, 256, (s, s, 4), dtype=np.uint8)]
    got = C.capture_uvspc(_dev(cam2uv), *[_dev(a) for a in src])
    torch.cuda.synchronize()
    for g, a in zip(got[:3], (src[0], src[1], src[2][:, :, :3])):
        want = a.copy()
        want[0, 0] = 0
        assert np.array_equal(g.cpu().numpy(), want)


# ----------------------------------------------------------------------------- nlt_diffuse_bases
@pytest.mark.parametrize('f,h,w,imh,imw', [(1, 2, 2, 1, 1), (7, 33, 21, 19, 23), (4, 256, 256, 128, 128)])
def test_diffuse_bases_bit_exact(f, h, w, imh, imw):
    rng = np.random.default_rng(f + h)
    albedo = B.albedo_from_frames(rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8))
    assert (albedo == 1).any()
    lvis = rng.integers(0, 256, (f, h, w), dtype=np.uint8)
    lvis[rng.random((f, h, w)) < 0.1] = 255
    uv2cam = np.stack([unit_map(rng, imh, imw, zeros=0.3) for _ in range(f)]).astype(np.float16)
    diffuse, cam = C.diffuse_bases(_dev(albedo), _dev(lvis), _dev(uv2cam))
    torch.cuda.synchronize()
    want_d = np.stack([B.diffuse_base(albedo, l) for l in lvis])
    want_c = np.stack([B.remap_u8(d, m.astype(np.float16)) for d, m in zip(want_d, uv2cam)])
    assert np.array_equal(diffuse.cpu().numpy(), want_d)
    assert np.array_equal(cam.cpu().numpy(), want_c)
    # and the adapters the parent commit had give the same bytes (the fused launch replaces a Python loop of them)
    old_d, old_c = P.compute_diffuse_bases(_dev(albedo), _dev(lvis), _dev(uv2cam))
    assert torch.equal(old_d, diffuse) and torch.equal(torch.stack(old_c), cam)


# ----------------------------------------------------------------------------- the written capture, read back on the device
@pytest.fixture(scope='module')
def capture(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('gpu') / 'capture')
    given = R.write_capture(root, 'cuda')
    P.postprocess(root, chunk=2)
    exp = {}
    for id_, cam, light in R.SAMPLES:
        inter, rgba, alpha, sample = given[id_]
        exp[id_] = R.expected_sample(inter, rgba, alpha, cam, light, sample['_uv2cam'], sample['_cam2uv'])
    order = sorted(exp)
    albedo = B.albedo_from_frames(np.stack([exp[i]['rgb.png'] for i in order if i.startswith('trainvali_')]))
    diffuse, _ = R.diffuse_bases_np(albedo, np.stack([exp[i]['lvis.png'] for i in order]), np.stack([exp[i]['uv2cam.npy'] for i in order]))
    zeros = np.zeros((R.UVS, R.UVS, 3), np.uint8)
    st = {'diffuse': diffuse, 'cvis': np.stack([exp[i]['cvis.png'] for i in order]), 'lvis': np.stack([exp[i]['lvis.png'] for i in order]),
          'rgb': np.stack([exp[i].get('rgb.png', zeros) for i in order])}
    return root, order, exp, st


def _neighbours(files):
    by = {(c, l): i for i, c, l in R.SAMPLES}
    of = {i: (c, l) for i, c, l in R.SAMPLES}
    return [by[(R.CAM_NN[of[i][0]], R.LIGHT_NN[of[i][1]])] for i in files]


@pytest.mark.parametrize('mode', ['train', 'test'])
def test_written_capture_loads_into_batches_on_the_device(capture, mode):
    root, order, exp, st = capture
    store = D.load_store(root, device='cuda')
    assert store['ids'] == order and all(store['complete'])
    for k, v in st.items():
        assert np.array_equal(store[k].cpu().numpy(), v), k          # the files hold the oracle's bytes
    cfg = nlt_amd.make_config(data_root=root, uvh=R.UVS, uvw=R.UVS, imh=R.IMH, imw=R.IMW, holdout_cam='P02', holdout_light='L2', bs=2)
    ds = D.Dataset(cfg, mode, store=store)
    nn_names = _neighbours(ds.files)
    ref = B.assemble_batch(st, [order.index(i) for i in ds.files], [[order.index(i)] for i in nn_names], mode)
    warp = np.stack([exp[i]['uv2cam.npy'] for i in ds.files]).astype(np.float32)
    eager = ds.load_batch(ds.files, resident=False)
    res = ds.load_batch(ds.files, resident=True)
    flt = res[1].materialize()
    torch.cuda.synchronize()
    assert eager[7] == nn_names and res[7] == nn_names
    for j, k in ((1, 'base'), (2, 'cvis'), (3, 'lvis'), (5, 'rgb'), (8, 'nn_base'), (9, 'nn_rgb')):
        assert np.array_equal(eager[j].cpu().numpy(), ref[k]), k
        assert np.array_equal(flt[k].cpu().numpy(), ref[k]), k
    assert np.array_equal(eager[4].cpu().numpy(), warp) and np.array_equal(flt['warp'].cpu().numpy(), warp)


def test_written_capture_at_another_trained_resolution(capture):
    """uvh = 24, (imh, imw) = (12, 18) over files stored at 16 and 8 x 12: every buffer normalised and resized as `_load_data`
    does per sample (normalize_uint -> cv2.resize INTER_LINEAR on float64 -> float32), the warp left alone."""
    root, order, exp, st = capture
    cfg = nlt_amd.make_config(data_root=root, uvh=24, uvw=24, imh=12, imw=18, holdout_cam='P02', holdout_light='L2', bs=2)
    ds = D.Dataset(cfg, 'train')                                    # (reads the capture through cfg's data_root)
    b = ds.load_batch(ds.files)
    torch.cuda.synchronize()
    nn_names = _neighbours(ds.files)
    rs = lambda a, h, w: B.cv_resize_linear(B.normalize_uint(a), h, w).astype(np.float32)
    d = lambda i: st['diffuse'][order.index(i)]
    for j, (id_, nn) in enumerate(zip(ds.files, nn_names)):
        assert np.array_equal(b[1][j].cpu().numpy(), rs(d(id_), 24, 24))
        assert np.array_equal(b[2][j].cpu().numpy()[..., 0], rs(exp[id_]['cvis.png'], 24, 24))
        assert np.array_equal(b[3][j].cpu().numpy()[..., 0], rs(exp[id_]['lvis.png'], 24, 24))
        assert np.array_equal(b[5][j].cpu().numpy(), rs(exp[id_]['rgb.png'], 24, 24))
        assert np.array_equal(b[6][j].cpu().numpy(), rs(exp[id_]['rgb_camspc.png'][:, :, :3], 12, 18))
        assert np.array_equal(b[8][j, 0].cpu().numpy(), rs(d(nn), 24, 24))
        assert np.array_equal(b[9][j, 0].cpu().numpy(), rs(exp[nn]['rgb.png'], 24, 24))
        assert np.array_equal(b[10][j].cpu().numpy(), rs(exp[nn]['rgb_camspc.png'][:, :, :3], 12, 18))
    assert tuple(b[4].shape) == (len(ds.files), R.IMH, R.IMW, 2)
