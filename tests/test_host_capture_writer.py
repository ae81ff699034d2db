"""The capture writer on the host (data_gen.render.render_sample / write_sample, data_gen.postproc.postprocess / gen_file_list):
a tiny capture -- 2 cameras x 2 lights as trainvali_*, one test_* sample without rgb_camspc, uvs = 16, camera 8 x 12 -- is
written the way the reference's data_gen/render.py:150-206 and postproc.py:50-122 lay it out and read back.  The C-ABI
adapters are the CPU emulation of tests/fake_capi.py; the three capture adapters are tests/capture_ref.py's compositions of
oracle/buffers.py.  Every comparison is on bytes, integers or float16 bit patterns."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import capture_ref as R
import fake_capi
import nlt_amd
from nlt_amd.data_gen import postproc as P
from nlt_amd.datasets import nlt as D
from oracle import buffers as B

SAMPLE_FILES = {'uv2cam.png', 'cam2uv.png', 'uv2cam.npy', 'cam2uv.npy', 'lvis_camspc.png', 'cvis_camspc.png', 'cvis.png', 'lvis.png',
                'cam.json', 'light.json', 'nn.json'}
TRAINVALI_ONLY = {'rgb_camspc.png', 'alpha.png', 'rgb.png'}
POSTPROC_FILES = {'diffuse.png', 'diffuse_camspc.png'}
IDS = [s[0] for s in R.SAMPLES]
TEST_ID = IDS[-1]


def decode(path):
    with open(path, 'rb') as h:
        img = Image.open(h)
        img.load()
    return np.array(img)


def build(tmp_path, monkeypatch, postprocess=True, **kw):
    fake_capi.install(monkeypatch)
    R.install(monkeypatch)
    root = str(tmp_path / 'capture')
    given = R.write_capture(root, 'cpu', **kw)
    if postprocess:
        P.postprocess(root, device='cpu')
    return root, given


def expected(given):
    """{id: {file: array}} from the oracle compositions, the diffuse bases included."""
    exp = {}
    for id_, cam, light in R.SAMPLES:
        inter, rgba, alpha, sample = given[id_]
        exp[id_] = R.expected_sample(inter, rgba, alpha, cam, light, sample['_uv2cam'], sample['_cam2uv'])
    albedo = B.albedo_from_frames(np.stack([exp[i]['rgb.png'] for i in sorted(IDS) if i.startswith('trainvali_')]))
    order = sorted(IDS)
    diffuse, cam = R.diffuse_bases_np(albedo, np.stack([exp[i]['lvis.png'] for i in order]), np.stack([exp[i]['uv2cam.npy'] for i in order]))
    for j, i in enumerate(order):
        exp[i]['diffuse.png'], exp[i]['diffuse_camspc.png'] = diffuse[j], cam[j]
    return exp


def test_each_directory_holds_exactly_the_reference_file_set(tmp_path, monkeypatch):
    root, _ = build(tmp_path, monkeypatch)
    assert sorted(os.listdir(root)) == sorted(IDS)
    for id_ in IDS:
        want = SAMPLE_FILES | POSTPROC_FILES | (TRAINVALI_ONLY if id_.startswith('trainvali_') else set())
        assert set(os.listdir(os.path.join(root, id_))) == want, id_
    assert not os.path.exists(os.path.join(root, TEST_ID, 'rgb.png'))
    with open(os.path.join(root, IDS[0], 'nn.json')) as h:
        text = h.read()
    assert json.loads(text) == {'cam': 'P02', 'light': 'L2'} and text == json.dumps(json.loads(text), indent=4, sort_keys=True)
    with open(os.path.join(root, IDS[0], 'cam.json')) as h:
        assert json.load(h) == {'name': 'P01', 'position': R.CAMS['P01']}


def test_every_file_decodes_to_the_oracle_composition(tmp_path, monkeypatch):
    root, given = build(tmp_path, monkeypatch)
    exp = expected(given)
    for id_ in IDS:
        for name, want in exp[id_].items():
            path = os.path.join(root, id_, name)
            if name.endswith('.npy'):
                got = np.load(path)
                assert got.dtype == np.float16 and got.shape == want.shape
                assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), (id_, name)
            else:
                got = decode(path)
                assert got.dtype == np.uint8 and np.array_equal(got, want), (id_, name)
        alpha = given[id_][2]
        u = np.load(os.path.join(root, id_, 'uv2cam.npy'))
        assert u.shape == (R.IMH, R.IMW, 2) and np.load(os.path.join(root, id_, 'cam2uv.npy')).shape == (R.UVS, R.UVS, 2)
        assert not decode(os.path.join(root, id_, 'uv2cam.png'))[:, :, 2].any()                    # blue = 0
        if alpha is not None:
            assert set(np.unique(alpha)) == {0, 254, 255}
            assert not u[alpha < 255].any() and u[alpha == 255].any()
            # cam2uv stays unmasked: it is the float64 map the mapping kernel returned, cast once
            assert np.array_equal(np.load(os.path.join(root, id_, 'cam2uv.npy')), given[id_][3]['_cam2uv'].astype(np.float16))
            assert decode(os.path.join(root, id_, 'rgb_camspc.png')).shape == (R.IMH, R.IMW, 4)     # as given: RGBA
    # the masked map differs from the unmasked one somewhere (the mask did something), and misses / occlusion reached the files
    id0 = IDS[0]
    assert given[id0][3]['_uv2cam'][given[id0][2] < 255].any()
    assert (exp[id0]['cvis_camspc.png'] != exp[id0]['lvis_camspc.png']).any()


def test_debug_writes_the_three_reprojections(tmp_path, monkeypatch):
    root, given = build(tmp_path, monkeypatch, postprocess=False, debug_first=True)
    inter, rgba, alpha, sample = given[IDS[0]]
    masked = sample['_uv2cam'].copy()
    masked[alpha < 255] = 0
    for k in ('cvis', 'lvis', 'rgb'):
        got = decode(os.path.join(root, IDS[0], k + '_camspc_repro.png'))
        assert np.array_equal(got, B.remap_u8(sample[k + '.png'], masked)), k
    assert not os.path.exists(os.path.join(root, IDS[1], 'cvis_camspc_repro.png'))


def test_index_has_the_reference_keys_and_tracks_missing_files(tmp_path, monkeypatch):
    root, _ = build(tmp_path, monkeypatch)
    out_json = root + '.json'                                       # the default: where load_store looks
    with open(out_json) as h:
        text = h.read()
    index = json.loads(text)
    assert text == json.dumps(index, indent=4, sort_keys=True) and sorted(index) == sorted(IDS)
    common = {'cam', 'cvis', 'diffuse', 'light', 'lvis', 'nn', 'uv2cam', 'complete'}
    for id_, entry in index.items():
        assert set(entry) == common | ({'alpha', 'rgb', 'rgb_camspc'} if id_.startswith('trainvali_') else set()), id_
        assert entry['complete'] is True
        for k, v in entry.items():
            if k != 'complete':
                assert not os.path.isabs(v) and v.split(os.sep)[0] == id_ and os.path.exists(os.path.join(root, v)), (id_, k, v)
        assert entry['uv2cam'] == os.path.join(id_, 'uv2cam.npy') and entry['diffuse'] == os.path.join(id_, 'diffuse.png')
    os.remove(os.path.join(root, IDS[1], 'lvis.png'))
    other = str(tmp_path / 'elsewhere' / 'index.json')
    again = P.gen_file_list(root, other)
    with open(other) as h:
        assert json.load(h) == again
    assert [i for i in again if not again[i]['complete']] == [IDS[1]]


@pytest.mark.parametrize('mode', ['train', 'test'])
def test_load_store_and_batches_equal_the_oracle_assembly(tmp_path, monkeypatch, mode):
    root, given = build(tmp_path, monkeypatch)
    exp = expected(given)
    order = sorted(IDS)
    store = D.load_store(root, device='cpu')
    assert store['ids'] == order and all(store['complete'])
    zeros = np.zeros((R.UVS, R.UVS, 3), np.uint8)
    st = {'diffuse': np.stack([exp[i]['diffuse.png'] for i in order]), 'cvis': np.stack([exp[i]['cvis.png'] for i in order]),
          'lvis': np.stack([exp[i]['lvis.png'] for i in order]), 'rgb': np.stack([exp[i].get('rgb.png', zeros) for i in order])}
    for k, v in st.items():
        assert np.array_equal(store[k].numpy(), v), k
    assert np.array_equal(store['uv2cam'].numpy().view(np.uint16), np.stack([exp[i]['uv2cam.npy'] for i in order]).view(np.uint16))
    cfg = nlt_amd.make_config(data_root=root, uvh=R.UVS, uvw=R.UVS, imh=R.IMH, imw=R.IMW, holdout_cam='P02', holdout_light='L2', bs=2)
    ds = D.Dataset(cfg, mode, store=store, device='cpu')
    want_files = [TEST_ID] if mode == 'test' else [i for i, c, l in R.SAMPLES if i.startswith('trainvali_') and (c, l) != ('P02', 'L2')]
    assert ds.files == sorted(want_files)
    by_cam_light = {(c, l): i for i, c, l in R.SAMPLES}
    cam_light = {i: (c, l) for i, c, l in R.SAMPLES}
    nn_names = [by_cam_light[(R.CAM_NN[cam_light[i][0]], R.LIGHT_NN[cam_light[i][1]])] for i in ds.files]    # through the written nn.json
    b = ds.load_batch(ds.files)
    assert b[7] == nn_names
    ref = B.assemble_batch(st, [order.index(i) for i in ds.files], [[order.index(i)] for i in nn_names], mode)
    for j, k in ((1, 'base'), (2, 'cvis'), (3, 'lvis'), (5, 'rgb'), (8, 'nn_base'), (9, 'nn_rgb')):
        assert b[j].dtype == torch.float32 and np.array_equal(b[j].numpy(), ref[k]), k
    assert np.array_equal(b[4].numpy(), np.stack([exp[i]['uv2cam.npy'] for i in ds.files]).astype(np.float32))
    if mode == 'train':
        assert np.array_equal(b[6].numpy(), np.stack([B.normalize_uint(exp[i]['rgb_camspc.png'][:, :, :3]).astype(np.float32) for i in ds.files]))


def test_postprocess_in_chunks_writes_the_same_bytes(tmp_path, monkeypatch):
    root, _ = build(tmp_path, monkeypatch, postprocess=False)

    def run(chunk):
        P.postprocess(root, chunk=chunk, device='cpu')
        out = {}
        for id_ in IDS:
            for name in sorted(POSTPROC_FILES):
                path = os.path.join(root, id_, name)
                with open(path, 'rb') as h:
                    out[(id_, name)] = h.read()
                os.remove(path)
        with open(root + '.json', 'rb') as h:
            out['index'] = h.read()
        return out
    whole, chunked = run(64), run(2)
    assert len(whole) == 2 * len(IDS) + 1 and whole == chunked


def test_bad_arguments_are_refused_before_any_launch():
    """The real library (no GPU needed: the argument checks run before anything is launched): null pointer / empty shape ->
    NLT_ERR_BAD_ARG (-1), a side above 32767 -> NLT_ERR_UNSUPPORTED (-2)."""
    from nlt_amd import capi as C
    L = C.lib()
    n, p = None, 4096                                               # (a non-null fake pointer: checked, never dereferenced)
    assert L.nlt_capture_camspc(n, n, n, n, 0., 0., 0., 0., 0., 0., n, n, 4, 4, n, n, n, n, n) == -1
    assert L.nlt_capture_camspc(p, p, p, n, 0., 0., 0., 0., 0., 0., n, p, 0, 4, p, p, p, p, n) == -1
    assert L.nlt_capture_camspc(p, p, p, n, 0., 0., 0., 0., 0., 0., n, p, 4, 32768, p, p, p, p, n) == -2
    assert L.nlt_capture_uvspc(n, 2, 4, 4, n, n, n, 0, 4, 4, n, n, n, n, n, n) == -1
    assert L.nlt_capture_uvspc(p, 1, 4, 4, p, p, n, 0, 4, 4, p, p, n, p, p, n) == -1
    assert L.nlt_capture_uvspc(p, 2, 4, 4, p, p, p, 3, 4, 4, p, p, n, p, p, n) == -1       # rgb_camspc without rgb
    assert L.nlt_capture_uvspc(p, 2, 32768, 4, p, p, n, 0, 4, 4, p, p, n, p, p, n) == -2
    assert L.nlt_diffuse_bases(n, n, n, 1, 4, 4, 2, 2, n, n, n) == -1
    assert L.nlt_diffuse_bases(p, p, p, 0, 4, 4, 2, 2, p, p, n) == -1
    assert L.nlt_diffuse_bases(p, p, p, 1, 4, 4, 2, 40000, p, p, n) == -2
