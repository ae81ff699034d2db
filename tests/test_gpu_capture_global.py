"""-m gpu: python -m nlt_amd.data_gen.capture_main with --bounces 2 --light_samples 2 --light_size 0.05 end to end on the bunny fixture
(one chart per face as the unwrap), at the sizes of tests/test_gpu_capture_main.py: 2 cameras x 2 lights at 24 x 32 pixels, a
64 x 64 texture, 4 samples per pixel -> the writer's file set, the flags in capture.json and the light JSONs, rgb_camspc the bytes
of `render_view` with those arguments and not those of the default capture, the index `load_store` reads and one batch through
Model.call."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import nlt_amd
import raycast_ref as R
from nlt_amd.data_gen import capture_main as CM
from nlt_amd.data_gen import mesh as M
from nlt_amd.data_gen import shade as SH
from nlt_amd.datasets import nlt as D
from nlt_amd.models import get_model_class
from test_gpu_capture_main import FILES, IMH, IMW, SPP

pytestmark = pytest.mark.gpu

UVS = 64
FLAGS = ['--bounces', '2', '--light_samples', '2', '--light_size', '0.05']


def test_a_global_capture_differs_from_the_default_one_and_feeds_the_model(tmp_path):
    unwrap = str(tmp_path / 'unwrap.pickle')
    with open(unwrap, 'wb') as h:
        pickle.dump(R.grid_unwrap(948), h)
    base = ['--mesh', R.BUNNY, '--uv_unwrap', unwrap, '--n_cams', '2', '--n_lights', '2', '--n_test', '0', '--imh', str(IMH), '--uvs', str(UVS),
            '--spp', str(SPP), '--hemisphere']
    plain, glob = str(tmp_path / 'plain'), str(tmp_path / 'global')
    _, info0 = CM.main(base + ['--outroot', plain])
    index, info = CM.main(base + ['--outroot', glob] + FLAGS)
    assert (info0['bounces'], info0['light_samples'], info0['light_size']) == (0, 1, None)
    assert (info['bounces'], info['light_samples'], info['light_size']) == (2, 2, 0.05) and json.load(open(glob + '.capture.json')) == info
    assert info['exposure'] == info0['exposure']                                         # `default_exposure`: a rule of the direct light
    names = sorted(index)
    assert names == ['trainvali_%09d_C%03d_L%03d' % (2 * c + l, c, l) for c in range(2) for l in range(2)]
    mesh, dense = M.Mesh.load(R.BUNNY), M.dense_unwrap(R.grid_unwrap(948))
    differ = 0
    for d in names:
        assert set(os.listdir(os.path.join(glob, d))) == FILES and index[d]['complete']
        cam, light = json.load(open(os.path.join(glob, d, 'cam.json'))), json.load(open(os.path.join(glob, d, 'light.json')))
        assert light['size'] == 0.05 and json.load(open(os.path.join(plain, d, 'light.json')))['size'] == 0.1
        rgb, rgb0 = D.read_png(os.path.join(glob, d, 'rgb_camspc.png')), D.read_png(os.path.join(plain, d, 'rgb_camspc.png'))
        want = SH.render_view(mesh, dense, cam, light, IMH, UVS, SPP, SH.Material(), info['exposure'], bounces=2, light_samples=2, light_size=0.05)
        assert rgb.shape == (IMH, IMW, 3) and np.array_equal(rgb, want['rgb_camspc.png'].cpu().numpy())
        differ += int((rgb != rgb0).any(-1).sum())
        # the geometry buffers are those of the light's centre: the same files in both captures
        for f in ('alpha.png', 'lvis_camspc.png', 'cvis_camspc.png', 'uv2cam.npy'):
            assert open(os.path.join(glob, d, f), 'rb').read() == open(os.path.join(plain, d, f), 'rb').read(), (d, f)
    print("%d pixels of rgb_camspc differ between the two captures" % differ)
    assert differ > 50
    store = D.load_store(glob, device='cuda')
    assert len(store['ids']) == 4 and all(store['complete'])
    cfg = nlt_amd.make_config(data_root=glob, bs=2, depth=32, uvh=UVS, uvw=UVS, imh=IMH, imw=IMW)
    train = D.Dataset(cfg, 'train', store=store)
    pm = get_model_class('nlt')(cfg)
    pm.build('cuda'); pm.register_trainable()
    batch = train.load_batch(sorted(train.files)[:2])
    pred = pm.call(batch, 'train')[0]
    torch.cuda.synchronize()
    assert tuple(pred.shape) == (2, IMH, IMW, 3) and bool(torch.isfinite(pred).all()) and float(batch[6].max()) > 0
