"""-m gpu: a capture from a bare .ply -- python -m nlt_amd.data_gen.capture_main --mesh <bunny> --uv_unwrap smart at the sizes of the
bunny capture of tests/test_gpu_capture_main.py (2 cameras x 2 lights close to the mesh, 24 x 32 pixels, a 64 x 64 texture, 4 samples
per pixel): the capture, <outroot>.uv.pickle and the `unwrap` record of <outroot>.capture.json; one train step on it; and
render_main with that pickle and with `smart` writing the same bytes.  One capture is written per module and shared."""
import json
import os

import numpy as np
import pytest

import nlt_amd
import raycast_ref as R
from nlt_amd import trainvali
from nlt_amd.data_gen import capture_main as CM
from nlt_amd.data_gen import mesh as M
from nlt_amd.data_gen import render_main as RM
from nlt_amd.data_gen import shade as SH
from nlt_amd.data_gen import unwrap as U
from nlt_amd.datasets import nlt as D
from nlt_amd.models import get_model_class

pytestmark = pytest.mark.gpu

IMH, IMW, UVS, SPP = 24, 32, 64, 4
SMART = ['--uv_unwrap', 'smart', '--angle_limit', '66', '--area_weight', '0']


@pytest.fixture(scope='module')
def capture(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('unwrap') / 'bunny')
    index, info = CM.main(['--mesh', R.BUNNY, '--outroot', root, '--n_cams', '2', '--n_lights', '2', '--n_test', '0', '--radius', '0.35',
                           '--hemisphere', '--imh', str(IMH), '--uvs', str(UVS), '--spp', str(SPP)] + SMART)
    return root, index, info


def test_the_capture_its_pickle_and_its_record(capture):
    root, index, info = capture
    assert len(index) == 4 and all(e['complete'] for e in index.values())
    with open(root + '.capture.json') as h:
        rec = json.load(h)
    assert rec == info and 'unwrap' in rec                            # (the file's keys are sorted: `dump_json`)
    un = rec['unwrap']
    assert un['method'] == 'smart' and (un['angle_limit'], un['area_weight'], un['margin']) == (66.0, 0.0, 0.002)
    assert set(un) == {'method', 'angle_limit', 'area_weight', 'margin', 'groups', 'islands', 'scale'}
    table = U.read_unwrap(root + '.uv.pickle')
    mesh = M.load_mesh(R.BUNNY)
    u = U.smart_unwrap(mesh, 66., 0.)
    assert (un['groups'], un['islands'], un['scale']) == (len(u.vectors), len(u.island_labels), u.scale)
    assert sorted(table) == list(range(len(mesh['faces']))) and all(np.array_equal(table[f], rows) for f, rows in u.table().items())


def test_capture_json_is_unchanged_without_smart(tmp_path):
    """`write_capture` with a given unwrap writes no `unwrap` entry: the record appears only when the unwrap was computed."""
    from nlt_amd.data_gen import rig as RIG
    mesh = M.Mesh.load(R.CUBE)
    cams, lights = RIG.light_stage(2, 2, 8.0, np.zeros(3))      # (two of each: everyone needs a neighbour)
    _, info = CM.write_capture(mesh, M.unwrap_from_obj(M.Mesh.load(R.CUBE, device=None)), str(tmp_path / 'cube'), cams, lights, imh=6, uvs=16, spp=1)   # (6 x 8 pixels: the rig's sensor is 32 x 24)
    assert 'unwrap' not in info and list(info)[-1] == 'light_size'
    with open(str(tmp_path / 'cube') + '.capture.json') as h:
        assert json.load(h) == info


def test_one_train_step_has_something_to_learn(capture):
    root, _, info = capture
    cfg = nlt_amd.make_config(data_root=root, bs=2, depth=32, uvh=UVS, uvw=UVS, imh=IMH, imw=IMW)
    train = D.Dataset(cfg, 'train')
    pm = get_model_class('nlt')(cfg)
    pm.build('cuda'); pm.register_trainable()
    batch = train.load_batch(sorted(train.files)[:2])
    loss, vis = trainvali.distributed_train_step(pm, batch, nlt_amd.optim.AdamAMSGrad(pm, 1e-3), 2)
    lit = int((vis['gt_camspc'] > 0).any(-1).sum())
    # the texture-space render under this unwrap and under the one-chart-per-face test helper, same camera, light and exposure
    mesh = M.Mesh.load(R.BUNNY)
    d = os.path.join(root, sorted(train.files)[0])
    cam, light = json.load(open(os.path.join(d, 'cam.json'))), json.load(open(os.path.join(d, 'light.json')))
    count = lambda unwrap: int((SH.render_view(mesh, unwrap, cam, light, IMH, UVS, SPP, SH.Material(), info['exposure'])['rgb.png'] > 0).any(-1).sum())
    smart, grid = count(U.smart_unwrap(mesh, 66., 0.).dense), count(M.dense_unwrap(R.grid_unwrap(948)))
    on_disk = int((D.read_png(os.path.join(d, 'rgb.png')) > 0).any(-1).sum())
    print("train step on %s: loss %.6e, %d pixels of gt_camspc are not black; non-black texels of rgb.png: %d with the smart unwrap, "
          "%d with grid_unwrap" % (batch[0], float(loss), lit, smart, grid))
    assert np.isfinite(float(loss)) and float(loss) > 0 and lit > 50 and on_disk == smart > 0


def test_render_main_with_the_pickle_and_with_smart_write_the_same_bytes(capture, tmp_path):
    root, index, _ = capture
    d = os.path.join(root, sorted(index)[0])
    nn = {}
    for kind, names in (('cam', ['C000', 'C001']), ('light', ['L000', 'L001'])):
        nn[kind] = str(tmp_path / (kind + '_nn.json'))
        with open(nn[kind], 'w') as h:
            json.dump({names[0]: names[1], names[1]: names[0]}, h)
    paths = {}
    for kind, name in (('cam', 'C000'), ('light', 'L000')):         # (a JSON path names its camera / light by its file name)
        paths[kind] = str(tmp_path / (name + '.json'))
        with open(os.path.join(d, kind + '.json')) as src, open(paths[kind], 'w') as dst:
            dst.write(src.read())
    common = ['--mesh', R.BUNNY, '--cam_json', paths['cam'], '--light_json', paths['light'], '--cam_nn_json',
              nn['cam'], '--light_nn_json', nn['light'], '--imh', str(IMH), '--uvs', str(UVS)]
    a, b = str(tmp_path / 'from_pickle'), str(tmp_path / 'from_smart')
    RM.main(common + ['--uv_unwrap', root + '.uv.pickle', '--outdir', a])
    RM.main(common + SMART + ['--outdir', b])
    files = sorted(os.listdir(a))
    assert files == sorted(os.listdir(b)) and 'cvis.png' in files and 'uv2cam.npy' in files
    for f in files:
        with open(os.path.join(a, f), 'rb') as ha, open(os.path.join(b, f), 'rb') as hb:
            assert ha.read() == hb.read(), f
