"""-m gpu: python -m nlt_amd.data_gen.capture_main end to end on the cube fixture (its own `vt` as the unwrap): 2 cameras x 3 lights
and one held-out test sample at 24 x 32 pixels, a 32 x 32 texture and 4 samples per pixel -> the writer's file set, rgb_camspc.png
the bytes of `render_view`, an anti-aliased alpha, the index `load_store` reads, one batch through Model.call and a train step, the
test sample through Model.call(..., 'test').  One capture is written per module and shared."""
import json
import os

import numpy as np
import pytest
import torch

import nlt_amd
import raycast_ref as R
from nlt_amd import trainvali
from nlt_amd.data_gen import capture_main as CM
from nlt_amd.data_gen import mesh as M
from nlt_amd.data_gen import shade as SH
from nlt_amd.datasets import nlt as D
from nlt_amd.models import get_model_class

pytestmark = pytest.mark.gpu

IMH, IMW, UVS, SPP = 24, 32, 32, 4
FILES = {'alpha.png', 'cam.json', 'cam2uv.npy', 'cam2uv.png', 'cvis.png', 'cvis_camspc.png', 'light.json', 'lvis.png', 'lvis_camspc.png',
         'nn.json', 'rgb.png', 'rgb_camspc.png', 'uv2cam.npy', 'uv2cam.png', 'diffuse.png', 'diffuse_camspc.png'}


@pytest.fixture(scope='module')
def capture(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('shade') / 'cube')
    index, info = CM.main(['--mesh', R.CUBE, '--uv_unwrap', R.CUBE, '--outroot', root, '--n_cams', '2', '--n_lights', '3', '--n_test', '1',
                           '--imh', str(IMH), '--uvs', str(UVS), '--spp', str(SPP), '--flat', '--kd', '0.9,0.6,0.3'])
    return root, index, info


def _png(path):
    return D.read_png(path)


def test_every_sample_directory_holds_the_writers_file_set(capture):
    root, index, info = capture
    dirs = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))
    want = ['test_000000000_VC000_VL000'] + ['trainvali_%09d_C%03d_L%03d' % (3 * c + l, c, l) for c in range(2) for l in range(3)]
    assert dirs == want and sorted(index) == want and all(index[d]['complete'] for d in want)
    for d in dirs:
        assert set(os.listdir(os.path.join(root, d))) == FILES, d
    with open(root + '.capture.json') as h:
        rec = json.load(h)
    lights = [json.load(open(os.path.join(root, 'trainvali_%09d_C000_L%03d' % (l, l), 'light.json'))) for l in range(3)]
    centre, half = CM.mesh_box(M.Mesh.load(R.CUBE, device=None))
    dist = np.mean([np.linalg.norm(np.asarray(l['position']) - centre) for l in lights])
    assert rec == info and np.isclose(rec['rig']['radius'], 4.5 * half) and np.isclose(dist, rec['rig']['radius'])
    assert np.isclose(rec['exposure'], CM.default_exposure(dist)) and rec['material']['kd'] == [0.9, 0.6, 0.3] and not rec['material']['smooth']
    nn = json.load(open(os.path.join(root, 'test_000000000_VC000_VL000', 'nn.json')))
    assert nn['cam'] in ('C000', 'C001') and nn['light'] in ('L000', 'L001', 'L002')


def test_rgb_camspc_is_render_view_and_alpha_is_anti_aliased(capture):
    root, _, info = capture
    mesh = M.Mesh.load(R.CUBE)
    unwrap = M.dense_unwrap(M.unwrap_from_obj(M.Mesh.load(R.CUBE, device=None)))
    mat = SH.Material(kd=(0.9, 0.6, 0.3), smooth=False)
    seen = []
    for l in range(3):
        d = os.path.join(root, 'trainvali_%09d_C000_L%03d' % (l, l))
        cam, light = json.load(open(os.path.join(d, 'cam.json'))), json.load(open(os.path.join(d, 'light.json')))
        sample = SH.render_view(mesh, unwrap, cam, light, IMH, UVS, SPP, mat, info['exposure'])
        rgb = _png(os.path.join(d, 'rgb_camspc.png'))
        assert rgb.shape == (IMH, IMW, 3) and np.array_equal(rgb, sample['rgb_camspc.png'].cpu().numpy())
        assert np.array_equal(_png(os.path.join(d, 'rgb.png')), sample['rgb.png'].cpu().numpy())
        alpha = _png(os.path.join(d, 'alpha.png'))
        alpha = alpha[..., 0] if alpha.ndim == 3 else alpha
        assert np.array_equal(alpha, sample['alpha.png'].cpu().numpy())
        assert set(np.unique(alpha)) - {0, 255} and (alpha == 255).any() and (alpha == 0).any()
        # partially covered pixels drop out of uv2cam, as in a Blender capture (data_gen/render.py:155)
        uv2cam = np.load(os.path.join(d, 'uv2cam.npy'))
        assert not uv2cam[alpha < 255].any() and uv2cam[alpha == 255].any()
        assert not rgb[alpha == 0].any()                                                 # black background
        seen.append(rgb)
    # L001 sits behind the cube as C000 sees it (a black image is right there); L000 and L002 light faces in view, differently
    assert seen[0].max() > 64 and seen[2].max() > 64 and not np.array_equal(seen[0], seen[2])


def test_a_bunny_capture_gives_a_train_step_something_to_learn(tmp_path):
    """The cube's six quads leave the texture-space maps nearly empty (only corner UVs are samples), so its train step below sees a
    black foreground.  The bunny fixture with one chart per face fills them: `write_capture` called directly, 2 cameras x 2 lights
    close to the mesh, then one train step whose ground truth is not black and whose loss is not zero."""
    from nlt_amd.data_gen import rig as RIG
    mesh = M.Mesh.load(R.BUNNY)
    root = str(tmp_path / 'bunny')
    cams, lights = RIG.light_stage(2, 2, 0.35, mesh.vertices.mean(0), hemisphere=True)
    index, info = CM.write_capture(mesh, R.grid_unwrap(948), root, cams, lights, imh=IMH, uvs=64, spp=SPP,
                                   material=SH.Material(vertex_rgb=np.random.default_rng(1).random((len(mesh.vertices), 3))))
    assert len(index) == 4 and all(e['complete'] for e in index.values()) and info['test'] == [] and info['material']['vertex_rgb']
    cfg = nlt_amd.make_config(data_root=root, bs=2, depth=32, uvh=64, uvw=64, imh=IMH, imw=IMW)
    train = D.Dataset(cfg, 'train')
    pm = get_model_class('nlt')(cfg)
    pm.build('cuda'); pm.register_trainable()
    batch = train.load_batch(sorted(train.files)[:2])
    loss, vis = trainvali.distributed_train_step(pm, batch, nlt_amd.optim.AdamAMSGrad(pm, 1e-3), 2)
    lit = int((vis['gt_camspc'] > 0).any(-1).sum())
    print("train step on %s: loss %.6e, %d pixels of gt_camspc are not black" % (batch[0], float(loss), lit))
    assert np.isfinite(float(loss)) and float(loss) > 0 and lit > 50


def test_the_capture_trains_and_tests(capture):
    root, _, _ = capture
    store = D.load_store(root, device='cuda')
    assert len(store['ids']) == 7 and all(store['complete'])
    kw = dict(depth=32, uvh=64, uvw=64, imh=IMH, imw=IMW)
    cfg = nlt_amd.make_config(data_root=root, bs=2, **kw)
    train = D.Dataset(cfg, 'train', store=store)
    assert len(train.files) == 6
    pm = get_model_class('nlt')(cfg)
    pm.build('cuda'); pm.register_trainable()
    batch = train.load_batch(sorted(train.files)[:2])
    assert float(batch[6].max()) > 0.25 and all(n.startswith('trainvali_') for n in batch[7])
    pred = pm.call(batch, 'train')[0]
    assert tuple(pred.shape) == (2, IMH, IMW, 3) and bool(torch.isfinite(pred).all())
    opt = nlt_amd.optim.AdamAMSGrad(pm, 1e-3)
    loss, vis = trainvali.distributed_train_step(pm, batch, opt, 2)
    # (a cube's six quads put only their corner UVs into the texture-space maps, so few texels carry colour at this size)
    print("train step on %s: loss %.6e, %d texels of rgb.png and %d pixels of gt_camspc are not black"
          % (batch[0], float(loss), int((batch[5] > 0).any(-1).sum()), int((vis['gt_camspc'] > 0).any(-1).sum())))
    assert np.isfinite(float(loss))
    test = D.Dataset(cfg, 'test', store=store)
    assert test.files == ['test_000000000_VC000_VL000']
    tb = test.load_batch(test.files)
    assert tb[7][0].startswith('trainvali_')
    out = pm.call(tb, 'test')[0]
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, IMH, IMW, 3) and bool(torch.isfinite(out).all())
