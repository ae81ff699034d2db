"""-m gpu: `trainvali.run` and `nlt_test.run` on the device, in deterministic mode, where a train step repeats bit for bit --
so everything the drivers compute is held to a hand-written loop over `load_batch` + `distributed_train_step` /
`distributed_vali_step` (or `extract_feat` + `infer`) byte for byte.  13 synthetic frames (64^2 UV, 32^2 camera), 2 held
out, bs 4: an epoch is batches of 4, 4 and 3 frames, the validation set one batch of 2."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from nlt_amd import ckpt, nlt_test, trainvali
from nlt_amd.datasets import nlt as D
from nlt_amd.datasets.synth import synthetic_store
from nlt_amd.models import nlt as M
from test_gpu_deterministic import CASES, _det_model
from trainloop_util import BS, CAM, N_FRAMES, UV, loop_config, tree

pytestmark = pytest.mark.gpu
SEED = 11
SHAPE = dict(uvh=UV, uvw=UV, imh=CAM, imw=CAM)
PLAIN = dict(SHAPE, depth=256, loss='l2')


@pytest.fixture(scope='module')
def store():
    return synthetic_store(N_FRAMES, UV, CAM)


def _cfg(outroot, model=PLAIN, **over):
    return loop_config(outroot, deterministic=True, **dict(model, **over))


def _mean(losses):
    return float(torch.stack(losses).cpu().mean())                             # one transfer, a float32 mean


def _epoch_batches(ds, epoch, seed=SEED):
    files = sorted(ds.files)
    ids = [files[i] for i in D.shuffle_order(len(files), 64, np.random.default_rng([seed, epoch]))]
    return [ids[i:i + BS] for i in range(0, len(ids), BS)]


def _by_hand(cfg, store, pm, epochs, step=None):
    """The loop written out.  Returns ({epoch: train loss}, {epoch: vali loss}, optimizer)."""
    opt = trainvali.make_optimizer(pm, cfg)
    train, vali = D.Dataset(cfg, 'train', store=store), D.Dataset(cfg, 'vali', store=store)
    vali_ids = sorted(vali.files)
    loss_train, loss_vali = {}, {}
    for e in range(epochs):
        id_lists = _epoch_batches(train, e)
        assert [len(x) for x in id_lists] == [4, 4, 3]
        losses = []
        for ids in id_lists:
            batch = train.load_batch(ids)
            loss, _ = step(batch) if (step is not None and len(ids) == BS) else trainvali.distributed_train_step(pm, batch, opt, BS)
            losses.append(loss)
        loss_train[e + 1] = _mean(losses)
        loss_vali[e + 1] = _mean([trainvali.distributed_vali_step(pm, vali.load_batch(vali_ids[i:i + BS]), BS)[0]
                                  for i in range(0, len(vali_ids), BS)])
    torch.cuda.synchronize()
    return loss_train, loss_vali, opt


def _same_floats(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.float32(got[k]).tobytes() == np.float32(want[k]).tobytes(), (k, got[k], want[k])
        assert np.isfinite(want[k]) and want[k] > 0


def _same_training_state(a_model, a_opt, b_model, b_opt):
    assert torch.equal(a_model.flat_params.detach(), b_model.flat_params.detach())
    assert a_opt.t == b_opt.t
    for slot in ('m', 'v', 'vhat'):
        assert torch.equal(getattr(a_opt, slot), getattr(b_opt, slot))


@pytest.fixture(scope='module')
def straight(store, tmp_path_factory):
    """Two epochs of `run`, eager: shared by the cases that compare against it."""
    rec = trainvali.run(_cfg(tmp_path_factory.mktemp('straight')), store=store, seed=SEED, model=_det_model(**PLAIN))
    torch.cuda.synchronize()
    return rec


def test_two_epochs_equal_the_manual_steps(store, straight, tmp_path):
    pm = _det_model(**PLAIN)
    loss_train, loss_vali, opt = _by_hand(_cfg(tmp_path), store, pm, 2)
    assert straight.step == 2 and opt.t == 6
    _same_training_state(straight.model, straight.optimizer, pm, opt)
    _same_floats(straight.loss_train, loss_train)
    _same_floats(straight.loss_vali, loss_vali)
    assert loss_train[1] != loss_train[2]


def test_resume_continues_bit_for_bit(store, straight, tmp_path):
    cfg = _cfg(tmp_path, epochs=1)
    first = trainvali.run(cfg, store=store, seed=SEED, model=_det_model(**PLAIN))
    assert first.step == 1
    cfg.set('DEFAULT', 'overwrite', 'False'); cfg.set('DEFAULT', 'epochs', '2')
    other = _det_model(**dict(PLAIN, seed=6))                                   # other weights: whatever it ends with was restored
    assert not torch.equal(other.flat_params.detach(), first.model.flat_params.detach())
    second = trainvali.run(cfg, store=store, seed=SEED, model=other)
    torch.cuda.synchronize()
    assert second.step == 2 and sorted(second.loss_train) == [2]
    _same_training_state(second.model, second.optimizer, straight.model, straight.optimizer)
    _same_floats(second.loss_train, {2: straight.loss_train[2]})
    _same_floats(second.loss_vali, {2: straight.loss_vali[2]})
    # a fresh model with the net alone restored from the last checkpoint renders what the straight run's model renders
    fresh = _det_model(**dict(PLAIN, seed=7))
    assert ckpt.restore_reference_checkpoint(fresh, os.path.join(second.outdir, 'checkpoints', 'ckpt-2')) == 2
    batch = D.Dataset(cfg, 'vali', store=store).load_batch(sorted(D.Dataset(cfg, 'vali', store=store).files))
    with torch.no_grad():
        got, want = fresh.call(batch, 'test'), straight.model.call(batch, 'test')
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[3]['pred'], want[3]['pred'])


def test_retention_and_artefacts(store, tmp_path):
    rec = trainvali.run(_cfg(tmp_path, keep_recent_epochs=1, vis_train_batches=1), store=store, seed=SEED, model=_det_model(**PLAIN))
    files = tree(rec.outdir)
    assert sorted(f for f in files if f.startswith('checkpoints/')) == [
        'checkpoints/checkpoint', 'checkpoints/ckpt-2.data-00000-of-00001', 'checkpoints/ckpt-2.index']
    for which, frames in (('train', 4), ('vali', 2)):
        root = os.path.join(rec.outdir, 'vis_' + which)
        assert os.listdir(root) == ['epoch%09d' % 2]
        epoch = os.path.join(root, 'epoch%09d' % 2)
        assert sorted(os.listdir(epoch)) == ['all.html', 'batch%09d' % 0, 'batch%09d_raw.pickle' % 0]
        metas = sorted(glob.glob(os.path.join(epoch, 'batch*', '*_metadata.json')))
        assert len(metas) == frames
        for path in metas:
            with open(path) as h:
                assert np.isfinite(json.load(h)['pred_psnr'])
        assert os.path.exists(os.path.join(epoch, 'batch%09d' % 0, '%d_pred.png' % (frames - 1)))


def test_graphs_replay_the_full_batches_and_leave_the_short_one_to_the_eager_step(store, straight, tmp_path, monkeypatch):
    eager_lens, graphed_calls = [], []
    real_step, real_call = trainvali.distributed_train_step, trainvali.GraphedTrainStep.__call__

    def step(model, batch, *a, **kw):
        eager_lens.append(len(batch[0]))
        return real_step(model, batch, *a, **kw)

    def call(self, batch):
        out = real_call(self, batch)
        graphed_calls.append((len(batch[0]), self.graph is not None))
        return out
    monkeypatch.setattr(trainvali, 'distributed_train_step', step)
    monkeypatch.setattr(trainvali.GraphedTrainStep, '__call__', call)
    rec = trainvali.run(_cfg(tmp_path), store=store, seed=SEED, graphs=True, model=_det_model(**PLAIN))
    torch.cuda.synchronize()
    assert rec.graphed is not None and rec.graphed.failed is None and rec.graphed.graph is not None
    assert [n for n, _ in graphed_calls] == [4] * 4 and eager_lens.count(3) == 2      # the graph saw full batches only
    assert sum(replayed for _, replayed in graphed_calls) >= 2, graphed_calls          # ... and replayed in both epochs
    print("graphed calls (frames, graph live after the call): %r" % graphed_calls)
    _same_training_state(rec.model, rec.optimizer, straight.model, straight.optimizer)
    _same_floats(rec.loss_train, straight.loss_train)
    _same_floats(rec.loss_vali, straight.loss_vali)


def test_a_layer_by_layer_config_equals_the_manual_steps(store, tmp_path):
    c = dict(CASES['layer_by_layer_kernel3'], **SHAPE)
    c.pop('cam'), c.pop('k')
    assert c['kernel'] == 3
    a = _det_model(**c)
    assert a.generic
    rec = trainvali.run(_cfg(tmp_path / 'run', model=c, epochs=1), store=store, seed=SEED, model=a)
    torch.cuda.synchronize()
    pm = _det_model(**c)
    loss_train, loss_vali, opt = _by_hand(_cfg(tmp_path / 'hand', model=c), store, pm, 1)
    _same_training_state(rec.model, rec.optimizer, pm, opt)
    _same_floats(rec.loss_train, loss_train)
    _same_floats(rec.loss_vali, loss_vali)


def _with_test_ids(store, n_test=2):
    ids, nn = list(store['ids']), dict(store['nn'])
    for i in range(len(ids) - n_test, len(ids)):
        new = ids[i].replace('trainvali', 'test')
        nn[new] = nn.pop(ids[i])
        ids[i] = new
    return dict(store, ids=ids, nn=nn)


def test_nlt_test_run_renders_what_extract_feat_and_infer_render_by_hand(store, tmp_path, monkeypatch):
    store = _with_test_ids(store)
    cfg = _cfg(tmp_path / 'out', epochs=1, holdout_cam='C009,C010', holdout_light='L009,L010')
    ini = tmp_path / 'run.ini'
    with open(ini, 'w') as h:
        cfg.write(h)
    rec = trainvali.run(cfg, config_ini=str(ini), store=store, seed=SEED, model=_det_model(**PLAIN))
    prefix = os.path.join(rec.outdir, 'checkpoints', 'ckpt-1')
    assert nlt_test.get_config_ini(prefix) == rec.outdir + '.ini' and os.path.exists(rec.outdir + '.ini')

    seen = []
    real = M.Model.vis_batch
    monkeypatch.setattr(M.Model, 'vis_batch', lambda self, to_vis, *a, **kw: (seen.append(to_vis['pred_camspc'].clone()), real(self, to_vis, *a, **kw))[1])
    model, outroot, view_at = nlt_test.run(prefix, store=store, seed=SEED)
    torch.cuda.synchronize()
    assert outroot == os.path.join(rec.outdir, 'vis_test', 'ckpt-1_pred')
    assert sorted(os.listdir(outroot)) == ['batch%09d' % 0]                    # 2 test frames at bs 4: one batch
    assert all(os.path.exists(os.path.join(outroot, 'batch%09d' % 0, '%d_pred.png' % i)) for i in range(2))
    assert os.path.exists(view_at) and view_at.startswith(outroot + '.') and os.path.exists(outroot + '.frames.json')

    hand = _det_model(**dict(PLAIN, seed=6))
    assert ckpt.restore_reference_checkpoint(hand, prefix) == 1
    assert torch.equal(hand.flat_params.detach(), model.flat_params.detach())
    train, test = D.Dataset(cfg, 'train', store=store), D.Dataset(cfg, 'test', store=store)
    test.bs = BS
    feat = nlt_test.extract_feat(hand, train.build_pipeline(seed=SEED), 1)
    want = nlt_test.infer(hand, test.build_pipeline(), feat)
    torch.cuda.synchronize()
    assert len(want) == len(seen) == 1 and want[0]['pred_camspc'].shape[0] == 2
    for got, w in zip(seen, want):
        assert torch.equal(got, w['pred_camspc'])

    # --batch_size_override acts on both pipelines, as the reference's: 2 -> one test batch of 2 still, observation batches
    # of 2 frames; 1 -> a batch directory per test frame
    lens = []
    real_feat = nlt_test.extract_feat
    monkeypatch.setattr(nlt_test, 'extract_feat', lambda m, pipe, n: real_feat(m, (lens.append(len(b[0])) or b for b in pipe), n))
    nlt_test.run(prefix, batch_size_override=2, store=store, seed=SEED)
    assert lens[0] == 2 and sorted(x for x in os.listdir(outroot)) == ['batch%09d' % 0]
    nlt_test.run(prefix, batch_size_override=1, store=store, seed=SEED)
    assert sorted(os.listdir(outroot)) == ['batch%09d' % 0, 'batch%09d' % 1]
    assert os.path.exists(os.path.join(outroot, 'batch%09d' % 1, '0_pred.png'))
