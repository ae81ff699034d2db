"""CPU: the host half of nlt_amd.relight -- the lat-long convention, the Radiance decoder, the capture's lights and views, the
normalisation.  Nothing here loads libnlt_hip.so: where a test needs per-light weights, the float64 restatement of
tests/relight_ref.py stands in for the adapter."""
import json
import os

import numpy as np
import pytest
import torch

from nlt_amd import relight as RL
import relight_ref as R


# ---------------------------------------------------------------------------------------------------- direction convention
@pytest.mark.parametrize('he,we', [(2, 4), (4, 8)])
def test_pixels_land_on_the_expected_hemispheres(he, we):
    """z-up: the top rows look up; phi runs from -pi (column 0) through 0 (the centre, +x) to +pi, so the middle columns look
    along +x, the outer ones along -x, the left half along -y and the right half along +y."""
    d = R.pixel_directions(he, we)
    assert np.allclose(np.linalg.norm(d, axis=2), 1.0, atol=1e-15)
    assert (d[:he // 2, :, 2] > 0).all() and (d[he // 2:, :, 2] < 0).all()
    assert (d[:, we // 4:3 * we // 4, 0] > 0).all() and (d[:, :we // 4, 0] < 0).all() and (d[:, 3 * we // 4:, 0] < 0).all()
    assert (d[:, :we // 2, 1] < 0).all() and (d[:, we // 2:, 1] > 0).all()
    assert np.isclose(R.solid_angles(he, we).sum() * we, 4 * np.pi, rtol=0.2 if he == 2 else 0.05)
    # six axis-aligned lights: every pixel's nearest light is the axis its direction has the largest component along
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    idx, _ = R.nearest_lights(he, we, axes, np.eye(3)[None])
    for i in range(he):
        for j in range(we):
            a = int(np.argmax(np.abs(d[i, j])))
            assert idx[0, i, j] == 2 * a + (0 if d[i, j, a] > 0 else 1), (i, j)
    # a quarter turn about +z carries +x to +y: what was nearest +x is nearest +y afterwards
    turned, _ = R.nearest_lights(he, we, axes, RL.rotations_about_z([np.pi / 2]))
    assert ((idx[0] == 0) == (turned[0] == 2)).all() and ((idx[0] == 4) == (turned[0] == 4)).all()


def test_light_directions_are_unit_vectors_from_the_centre():
    d = RL.light_directions([[3, 0, 0], [1, 1, 1], [0, -2, 5]], center=(1, 0, 0))
    assert d.dtype == np.float32 and d.shape == (3, 3)
    assert np.allclose(d[0], [1, 0, 0]) and np.allclose(d[1], [0, 2 ** -0.5, 2 ** -0.5]) and np.allclose(np.linalg.norm(d, axis=1), 1, atol=1e-6)
    with pytest.raises(ValueError, match='centre'):
        RL.light_directions([[1, 0, 0]], center=(1, 0, 0))


# ---------------------------------------------------------------------------------------------------- .hdr decoder
def _picture(h, w, seed):
    """Values RGBE holds exactly: 8-bit mantissas under one shared exponent per pixel, a black pixel, long constant runs."""
    rng = np.random.default_rng(seed)
    mant = rng.integers(0, 256, (h, w, 3))
    mant[np.arange(h * w).reshape(h, w) % 7 == 0, rng.integers(0, 3)] = 200                # the top bit set somewhere: a normalised pixel
    mant[:, :, 0] |= 128
    expo = rng.integers(-6, 7, (h, w))
    img = mant * 2.0 ** (expo[:, :, None] - 8)
    img[0, 1] = 0
    img[h - 1, 2:] = img[h - 1, 2]                                   # a run to the end of the line
    return img.astype(np.float32)


@pytest.mark.parametrize('rle', [False, True])
def test_hdr_decoder_is_exact_on_files_the_test_encodes(tmp_path, rle):
    img = _picture(5, 11, seed=3 + rle)
    rgbe = R.encode_rgbe(img)
    data = R.hdr_bytes(rgbe, rle)
    assert (len(data) != len(R.hdr_bytes(rgbe, False))) == rle       # the run-length form really is another byte stream
    path = str(tmp_path / 'probe.hdr')
    with open(path, 'wb') as h:
        h.write(data)
    got = RL.read_envmap(path)
    assert got.dtype == np.float32 and got.shape == img.shape and np.array_equal(got, img)
    np.save(str(tmp_path / 'probe.npy'), img)
    assert np.array_equal(RL.read_envmap(str(tmp_path / 'probe.npy')), img)


def test_hdr_decoder_refuses_what_it_does_not_read(tmp_path):
    rgbe = R.encode_rgbe(_picture(2, 8, 1))
    good = R.hdr_bytes(rgbe, False)
    with pytest.raises(ValueError, match='resolution'):
        RL.decode_hdr(good.replace(b'-Y 2 +X 8', b'+Y 2 +X 8'))
    with pytest.raises(ValueError, match='xyze'):
        RL.decode_hdr(good.replace(b'32-bit_rle_rgbe', b'32-bit_rle_xyze'))
    with pytest.raises(ValueError, match='RADIANCE'):
        RL.decode_hdr(b'P6\n' + good)
    with pytest.raises(ValueError, match='ends early'):
        RL.decode_hdr(good[:-5])
    with pytest.raises(ValueError, match='.npy and Radiance'):
        RL.read_envmap(str(tmp_path / 'probe.exr'))
    np.save(str(tmp_path / 'flat.npy'), np.zeros((4, 8)))
    with pytest.raises(ValueError, match=r'\[He,We,3\]'):
        RL.read_envmap(str(tmp_path / 'flat.npy'))


# ---------------------------------------------------------------------------------------------------- lights and views
LIGHTS = {'L003': [0.0, 1.0, 5.0], 'L001': [1.0, 3.0, 2.0], 'L002': [-2.0, -2.0, 3.5]}


def _capture(root, samples, incomplete=(), positions=None):
    """A hand-written index + light.json files: samples = [(id, light name)]."""
    index = {}
    for id_, light in samples:
        os.makedirs(os.path.join(root, id_), exist_ok=True)
        with open(os.path.join(root, id_, 'light.json'), 'w') as h:
            json.dump({'name': light, 'position': (positions or {}).get(id_, LIGHTS[light])}, h)
        index[id_] = {'light': os.path.join(id_, 'light.json'), 'complete': id_ not in incomplete}
    with open(root.rstrip('/') + '.json', 'w') as h:
        json.dump(index, h)


SAMPLES = [('trainvali_000000000_C01_L003', 'L003'), ('trainvali_000000001_C01_L001', 'L001'), ('trainvali_000000002_C02_L001', 'L001'),
           ('trainvali_000000003_C01_L002', 'L002'), ('trainvali_000000004_C02_L002', 'L002'), ('test_000000000_C01_L003', 'L003')]


def test_load_lights_and_view_samples(tmp_path):
    root = str(tmp_path / 'capture')
    _capture(root, SAMPLES, incomplete=('trainvali_000000003_C01_L002',))
    assert RL.load_lights(root) == {k: tuple(v) for k, v in LIGHTS.items()}
    want = [('trainvali_000000001_C01_L001', 'L001'), ('trainvali_000000000_C01_L003', 'L003')]      # by light name; the incomplete one skipped
    assert RL.view_samples(root, 'C01') == want
    store = {'ids': [i for i, _ in SAMPLES], 'complete': [i != 'trainvali_000000003_C01_L002' for i, _ in SAMPLES]}
    assert RL.view_samples(store, 'C01') == want
    assert RL.view_samples(store, 'C02') == [('trainvali_000000002_C02_L001', 'L001'), ('trainvali_000000004_C02_L002', 'L002')]
    with pytest.raises(ValueError, match=r"camera 'C07'; cameras: C01, C02"):
        RL.view_samples(store, 'C07')
    # a light only an incomplete sample shows is not listed; the test sample's is (its trainvali twin is complete)
    _capture(root, SAMPLES, incomplete=('trainvali_000000003_C01_L002', 'trainvali_000000004_C02_L002'))
    assert sorted(RL.load_lights(root)) == ['L001', 'L003']
    with pytest.raises(FileNotFoundError):
        RL.load_lights(str(tmp_path / 'nowhere'))


def test_one_light_name_with_two_positions_is_an_error(tmp_path):
    root = str(tmp_path / 'capture')
    _capture(root, SAMPLES, positions={'trainvali_000000002_C02_L001': [1.0, 3.0, 2.5]})
    with pytest.raises(ValueError, match="light 'L001' has two positions"):
        RL.load_lights(root)


# ---------------------------------------------------------------------------------------------------- normalisation
def _ref_adapter(envmap, dirs, rot):
    w = R.envmap_light_weights(envmap.numpy(), dirs.numpy(), rot.numpy())
    return torch.from_numpy(w.astype(np.float32))


def test_a_uniform_white_probe_normalises_to_one(monkeypatch):
    monkeypatch.setattr(RL.C, 'envmap_light_weights', _ref_adapter)
    dirs = R.random_directions(5, seed=2)
    white = np.ones((4, 8, 3), np.float32)
    for rotations, n in ((None, 1), ([0.3, 1.1], 2), (R.random_rotations(3, 4), 3)):
        w = RL.envmap_weights(white, dirs, rotations=rotations, device='cpu')
        assert tuple(w.shape) == (n, 5, 3) and w.dtype == torch.float32
        assert np.allclose(w.double().sum(1).mean(1).numpy(), 1.0, atol=1e-6)
    raw = RL.envmap_weights(white, dirs, normalize=False, device='cpu')
    assert np.isclose(float(raw.double().sum()) / 3, R.solid_angles(4, 8).sum() * 8, rtol=1e-6)      # the raw integrals: the sphere's area
    # normalising is by the IDENTITY probe's sum: a tinted probe keeps its tint, a rotation does not change the scale
    tinted = white * np.array([2.0, 1.0, 0.5], np.float32)
    w = RL.envmap_weights(tinted, dirs, rotations=[0.7], device='cpu')
    assert np.allclose(w.double().sum(1).numpy()[0], np.array([2.0, 1.0, 0.5]) * 3 / 3.5, atol=1e-6)
    with pytest.raises(ValueError, match='energy'):
        RL.envmap_weights(np.zeros((4, 8, 3), np.float32), dirs, device='cpu')
