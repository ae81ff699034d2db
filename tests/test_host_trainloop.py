"""CPU: the config-driven drivers -- `Dataset.build_pipeline` / `shuffle_order` (nlt/datasets/base.py:89-117), `trainvali.run`
/ `main` (nlt/trainvali.py:48-251,328-332) and `nlt_test`'s flags and paths (nlt/nlt_test.py:33-48) -- with the device kernels
replaced by the TEST-ONLY C-ABI emulation (tests/fake_capi.py) where a model runs."""
import os
import warnings
from collections import deque

import numpy as np
import pytest
import torch

import nlt_amd
from nlt_amd import nlt_test, trainvali
from nlt_amd.datasets import nlt as D
from nlt_amd.datasets.synth import synthetic_store
import fake_capi
from test_dist_gloo import GLOBAL, _shard
from test_host_vis import fake_psnr
from trainloop_util import BS, CAM, N_FRAMES, UV, loop_config, scalars, tree


# ------------------------------------------------------------------------------------------------------ shuffle_order
@pytest.mark.parametrize('B', [1, 5, 64])
def test_shuffle_order_stays_inside_the_buffer_algorithms_support(B):
    n, orders = 40, set()
    for seed in range(200):
        order = D.shuffle_order(n, B, np.random.default_rng([seed, 0]))
        assert sorted(order) == list(range(n))                                  # a permutation
        for pos, i in enumerate(order):                                         # element i enters the buffer once i - B + 1
            assert pos >= i - B + 1, (seed, pos, i)                             # elements have left it
        orders.add(tuple(order))
    if B == 1:
        assert orders == {tuple(range(n))}
    else:
        assert len(orders) > 1
    if B >= n:                                                                  # every element can come first
        assert len({o[0] for o in orders}) > B // 4


def test_shuffle_order_is_a_function_of_seed_and_epoch():
    order = lambda seed, epoch: D.shuffle_order(40, 64, np.random.default_rng([seed, epoch]))
    assert order(3, 0) == order(3, 0) and order(3, 1) == order(3, 1)
    assert order(3, 0) != order(3, 1) and order(3, 0) != order(4, 0)


# ----------------------------------------------------------------------------------------------------------- batching
class _Loads(D.Dataset):
    """A Dataset whose `load_batch` returns the ids it was asked for (batching needs no texels)."""

    def load_batch(self, ids, resident=False):
        return list(ids)


def _store(n, test_ids=0):
    store = synthetic_store(n, 8, 8, device='cpu')
    for i in range(n - test_ids, n):
        new = store['ids'][i].replace('trainvali', 'test')
        store['nn'][new] = store['nn'].pop(store['ids'][i])
        store['ids'][i] = new
    return store


def _ds(n, mode='train', bs=4, holdout=(), cls=_Loads, **kw):
    cfg = nlt_amd.make_config(uvh=8, uvw=8, imh=8, imw=8, bs=bs, holdout_cam=','.join('C%03d' % i for i in holdout),
                              holdout_light=','.join('L%03d' % i for i in holdout))
    return cls(cfg, mode, store=kw.pop('store', None) or _store(n), device='cpu', **kw)


def test_batches_keep_the_short_last_one_and_no_batch_and_take():
    ds = _ds(11)
    pipe = ds.build_pipeline(seed=7)
    batches = list(pipe)
    assert [len(b) for b in batches] == [4, 4, 3] and len(pipe) == 3
    order = D.shuffle_order(11, 64, np.random.default_rng([7, 0]))
    assert [i for b in batches for i in b] == [sorted(ds.files)[i] for i in order]
    assert list(pipe) == batches                                                # the pipeline is fixed when it is built
    assert list(ds.build_pipeline(seed=7, epoch=1)) != batches
    assert list(ds.build_pipeline()) == list(ds.build_pipeline())              # seed=None: one draw per Dataset
    singles = list(ds.build_pipeline(seed=7, no_batch=True))
    assert [len(b) for b in singles] == [1] * 11 and [b[0] for b in singles] == [i for b in batches for i in b]
    assert list(pipe.take(2)) == batches[:2] and list(pipe.take(0)) == [] and list(pipe.take(-1)) == batches
    assert list(pipe.take(5)) == batches
    vali = _ds(11, mode='vali', holdout=range(11))                             # not shuffled: sorted files
    assert [i for b in vali.build_pipeline(seed=7) for i in b] == sorted(vali.files)
    assert _ds(11, shuffle_buffer_size=1).build_pipeline(seed=7).id_lists[0] == sorted(ds.files)[:4]


def test_vali_batches_counts_bs_batches_per_unit_as_the_reference_does(tmp_path, monkeypatch):
    """`take(vali_batches * bs)` on the batched pipeline: vali_batches = 1 at bs 4 takes up to 4 batches -- all 3 there are."""
    fake_capi.install(monkeypatch)
    fake_psnr(monkeypatch)
    store = synthetic_store(14, UV, CAM, device='cpu')
    held = range(3, 14)                                                         # 11 validation frames: 3 batches
    cfg = loop_config(tmp_path, epochs=1, vali_batches=1, holdout_cam=','.join('C%03d' % i for i in held),
                      holdout_light=','.join('L%03d' % i for i in held))
    seen = []
    real = trainvali.distributed_vali_step
    monkeypatch.setattr(trainvali, 'distributed_vali_step', lambda m, b, *a, **kw: (seen.append(list(b[0])), real(m, b, *a, **kw))[1])
    trainvali.run(cfg, store=store, device='cpu', seed=1)
    assert [len(x) for x in seen] == [4, 4, 3]


# ----------------------------------------------------------------------------------------------------------- sharding
def test_global_batches_are_cut_like_the_gloo_tests_shards():
    assert GLOBAL[4] == 7
    ds = _ds(7, bs=7)
    whole = ds.build_pipeline(seed=2).id_lists[0]
    for rank in range(4):
        (part,) = ds.build_pipeline(seed=2, rank=rank, world=4).id_lists
        assert part == whole[_shard(4, rank)]
        assert D.shard_slice(7, 4, rank) == _shard(4, rank)


def test_a_last_batch_shorter_than_the_world_is_dropped_everywhere_with_one_warning():
    ds = _ds(11)                                                                # 4, 4, 3 at world 4
    whole = ds.build_pipeline(seed=2).id_lists
    for rank in range(4):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            parts = ds.build_pipeline(seed=2, rank=rank, world=4).id_lists
        assert len(w) == 1 and 'dropped' in str(w[0].message)
        assert parts == [b[rank:rank + 1] for b in whole[:2]]
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert len(ds.build_pipeline(seed=2, rank=1, world=2).id_lists) == 3    # 3 frames over 2 ranks: kept


# ------------------------------------------------------------------------------------------------------------ helpers
def _touch_epochs(root, names):
    for n in names:
        os.makedirs(os.path.join(root, n))
    return [os.path.join(root, n) for n in names]


@pytest.mark.parametrize('keep,left', [(2, ['e2', 'e3']), (-1, ['e0', 'e1', 'e2', 'e3'])])
def test_maintain_epoch_queue(tmp_path, keep, left):
    queue = deque([], keep if keep > 0 else None)
    for i in range(4):
        (path,) = _touch_epochs(str(tmp_path), ['e%d' % i])
        trainvali.maintain_epoch_queue(queue, path)
    assert sorted(os.listdir(tmp_path)) == left
    # a fresh queue (a resumed run) forgets -- and removes -- what an earlier run left, as the reference's does
    (path,) = _touch_epochs(str(tmp_path), ['e4'])
    trainvali.maintain_epoch_queue(deque([], keep if keep > 0 else None), path)
    assert os.listdir(tmp_path) == ['e4']


def test_prepare_outdir_and_the_outdir_name(tmp_path):
    cfg = loop_config(tmp_path, lr=0.001)
    outdir = trainvali.outdir_of(cfg)
    assert outdir == os.path.join(str(tmp_path), 'loop_lr:0.001_depth:256')
    trainvali.prepare_outdir(outdir, overwrite=False)
    open(os.path.join(outdir, 'kept'), 'w').close()
    trainvali.prepare_outdir(outdir, overwrite=False)
    assert os.listdir(outdir) == ['kept']
    trainvali.prepare_outdir(outdir, overwrite=True)                            # wipes everything: checkpoints included
    assert os.listdir(outdir) == []


def test_flags_of_both_drivers(tmp_path, capsys):
    a = trainvali.parse_args([])
    assert (a.config, a.debug, a.device, a.seed, a.graphs) == ('config.ini', False, 'gpu', None, False)
    a = trainvali.parse_args(['--config', 'x.ini', '--debug', '--device', 'gpu', '--seed', '5', '--graphs'])
    assert (a.config, a.debug, a.device, a.seed, a.graphs) == ('x.ini', True, 'gpu', 5, True)
    with pytest.raises(SystemExit):
        trainvali.parse_args(['--device', 'cpu'])
    assert 'no CPU fallback exists' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        trainvali.main(['--config', str(tmp_path / 'x.ini'), '--device', 'cpu'])
    b = nlt_test.parse_args([])
    assert (b.ckpt, b.batch_size_override, b.n_obs_batches, b.fps) == ('/path/to/ckpt-100', None, 1, 24)
    b = nlt_test.parse_args(['--ckpt', '/o/x/checkpoints/ckpt-7', '--batch_size_override', '2', '--n_obs_batches', '3', '--fps', '12'])
    assert (b.ckpt, b.batch_size_override, b.n_obs_batches, b.fps) == ('/o/x/checkpoints/ckpt-7', 2, 3, 12)
    assert nlt_test.get_config_ini(b.ckpt) == '/o/x.ini'
    # --config: a path that exists, else a name inside config/ beside the module
    ini = tmp_path / 'here.ini'
    ini.write_text('[DEFAULT]\n')
    assert trainvali.resolve_config(str(ini)) == str(ini)
    assert trainvali.resolve_config('dragon_specular.ini') == os.path.join(os.path.dirname(trainvali.__file__), 'config', 'dragon_specular.ini')


# ---------------------------------------------------------------------------------------------------- neighbour cache
class _Counts(D.Dataset):
    scans = 0

    def _get_nn_id(self, nn):
        type(self).scans += 1
        return super()._get_nn_id(nn)


def test_neighbour_cache_gives_the_uncached_values_and_scans_once_per_sample(monkeypatch):
    fake_capi.install(monkeypatch)
    store = _store(11)
    gone = store['ids'][4]                                                      # sample 3's neighbour: frame 4 leaves the store's ids
    keep = [i for i in range(11) if i != 4]
    store['ids'] = [store['ids'][i] for i in keep]
    for k in ('diffuse', 'rgb', 'cvis', 'lvis', 'rgb_camspc', 'uv2cam'):
        store[k] = store[k][keep]
    store['complete'] = [True] * 10
    del store['nn'][gone]
    _Counts.scans = 0
    cached, plain = _ds(0, store=store, cls=_Counts), _ds(0, store=store, nn_cache=False)
    want = {i: plain._nn_indices(i) for i in plain.files}
    assert want[store['ids'][3]] == [-1] and sum(v == [-1] for v in want.values()) == 1
    for epoch in range(2):
        for ids in cached.build_pipeline(seed=1, epoch=epoch).id_lists:
            assert [cached._nn_indices(i) for i in ids] == [want[i] for i in ids]
    assert _Counts.scans == len(cached.files) == 10
    b = cached.load_batch(cached.files[2:5])                                    # through load_batch: the missing neighbour's name
    assert b[7][1] == 'incomplete-data' and _Counts.scans == 10


def test_a_duplicate_neighbour_match_still_raises_when_that_sample_is_loaded(monkeypatch):
    fake_capi.install(monkeypatch)
    store = _store(6)
    store['nn'][store['ids'][0]] = {'cam': 'C00.', 'light': 'L00.'}            # as a regex: matches every id
    ds = _ds(0, store=store, cls=D.Dataset)                                     # building the Dataset scans nothing
    ds.load_batch(store['ids'][1:3])
    for _ in range(2):
        with pytest.raises(ValueError, match='Found 6 matches'):
            ds.load_batch(store['ids'][0:2])


# ------------------------------------------------------------------------------------------------------ one small run
def test_run_two_epochs_then_resume_for_one_more(tmp_path, monkeypatch):
    fake_capi.install(monkeypatch)
    fake_psnr(monkeypatch)
    store = synthetic_store(N_FRAMES, UV, CAM, device='cpu')
    ini = tmp_path / 'small.ini'
    cfg = loop_config(tmp_path / 'out', vis_train_batches=1, overwrite=False)
    with open(ini, 'w') as h:
        cfg.write(h)
    steps = []
    real = trainvali.distributed_train_step
    monkeypatch.setattr(trainvali, 'distributed_train_step', lambda m, b, *a, **kw: (steps.append(list(b[0])), real(m, b, *a, **kw))[1])
    rec = trainvali.run(cfg, config_ini=str(ini), store=store, device='cpu', seed=3)
    outdir = os.path.join(str(tmp_path), 'out', 'loop_lr:0.001_depth:256')
    assert rec.outdir == outdir and rec.step == 2 and sorted(rec.loss_train) == sorted(rec.loss_vali) == [1, 2]
    assert [len(s) for s in steps] == [4, 4, 3] * 2 and sorted(steps[0] + steps[1] + steps[2]) == sorted(steps[3] + steps[4] + steps[5])
    assert steps[:3] != steps[3:]                                               # another epoch, another order
    assert open(outdir + '.ini').read() == open(ini).read()
    files = tree(outdir)
    ck = sorted(f for f in files if f.startswith('checkpoints/'))
    assert ck == ['checkpoints/checkpoint'] + ['checkpoints/ckpt-%d.%s' % (n, s) for n in (1, 2) for s in ('data-00000-of-00001', 'index')]
    for which, n_batches, n_last in (('train', 1, 4), ('vali', 1, 2)):
        for e in (1, 2):
            ep = 'vis_%s/epoch%09d/' % (which, e)
            assert ep + 'all.html' in files
            assert sorted({f[len(ep):].split('/')[0] for f in files if f.startswith(ep)}) == ['all.html', 'batch000000000', 'batch000000000_raw.pickle']
            assert ep + 'batch000000000/%d_pred.png' % (n_last - 1) in files and ep + 'batch000000000/%d_pred.png' % n_last not in files
            assert ep + 'batch000000000/0_metadata.json' in files
    train, vali = scalars(outdir, 'train'), scalars(outdir, 'vali')
    assert [(r['tag'], r['step']) for r in train] == [(t, e) for e in (1, 2) for t in ('loss_train', 'batch_time_train', 'vis_train')]
    assert [(r['tag'], r['step']) for r in vali] == [(t, e) for e in (1, 2) for t in ('loss_vali', 'vis_vali')]
    assert [r['value'] for r in train if r['tag'] == 'loss_train'] == [rec.loss_train[1], rec.loss_train[2]]
    assert [r['value'] for r in vali if r['tag'] == 'loss_vali'] == [rec.loss_vali[1], rec.loss_vali[2]]
    assert all(np.isfinite(v) and v > 0 for v in list(rec.loss_train.values()) + list(rec.loss_vali.values()))
    params = rec.model.flat_params.detach().clone()

    # overwrite = false, epochs = 3: exactly one more epoch, from the restored weights and optimizer
    del steps[:]
    cfg.set('DEFAULT', 'epochs', '3')
    rec2 = trainvali.run(cfg, config_ini=str(ini), store=store, device='cpu', seed=3)
    assert [len(s) for s in steps] == [4, 4, 3] and rec2.step == 3 and sorted(rec2.loss_train) == [3]
    assert rec2.optimizer.t == 9 and rec2.model is not rec.model
    assert not torch.equal(rec2.model.flat_params.detach(), params)
    assert [r['step'] for r in scalars(outdir, 'train') if r['tag'] == 'loss_train'] == [1, 2, 3]
    assert 'checkpoints/ckpt-3.index' in tree(outdir)
    # ... and with nothing left to do, a third call does nothing but restore
    del steps[:]
    rec3 = trainvali.run(cfg, store=store, device='cpu', seed=3)
    assert steps == [] and rec3.step == 3 and torch.equal(rec3.model.flat_params.detach(), rec2.model.flat_params.detach())


def test_debug_mode_takes_one_batch_per_epoch_and_a_norm_model_gets_native_checkpoints(tmp_path, monkeypatch):
    fake_capi.install(monkeypatch)
    fake_psnr(monkeypatch)
    store = synthetic_store(N_FRAMES, UV, CAM, device='cpu')
    cfg = loop_config(tmp_path, depth=32, norm='layer', epochs=2, keep_recent_epochs=1)
    steps = []
    real = trainvali.distributed_train_step
    monkeypatch.setattr(trainvali, 'distributed_train_step', lambda m, b, *a, **kw: (steps.append(list(b[0])), real(m, b, *a, **kw))[1])
    with pytest.warns(UserWarning, match='native format'):
        rec = trainvali.run(cfg, store=store, device='cpu', debug=True, seed=3)
    assert [len(s) for s in steps] == [4, 4]
    assert os.listdir(os.path.join(rec.outdir, 'checkpoints')) == ['ckpt-2.pt']
    assert os.listdir(os.path.join(rec.outdir, 'vis_train')) == ['epoch%09d' % 2]
    cfg.set('DEFAULT', 'overwrite', 'False'); cfg.set('DEFAULT', 'epochs', '3')
    with pytest.warns(UserWarning, match='native format'):
        rec2 = trainvali.run(cfg, store=store, device='cpu', debug=True, seed=3)
    assert rec2.step == 3 and rec2.optimizer.t == 3 and os.listdir(os.path.join(rec.outdir, 'checkpoints')) == ['ckpt-3.pt']
