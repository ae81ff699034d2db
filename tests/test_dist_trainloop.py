"""CPU, world_size 2 over gloo: one epoch of `trainvali.run` with the batches sharded by `Dataset.build_pipeline(rank=, world=)`.
Device kernels are replaced by the TEST-ONLY C-ABI emulation; the collectives, the files and the checkpoints are the real ones."""
import builtins
import os
import sys
import tempfile

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD, SEED = 2, 3


class _MP:                                      # minimal monkeypatch stand-in
    def setattr(self, obj, name, val):
        setattr(obj, name, val)


def _run(outroot, patch, steps, loaded):
    """One epoch on a model with the oracle's seed-1 weights; `steps` collects every train step's loss, `loaded` the ids of
    every batch `load_batch` assembled for the 'train' dataset."""
    from nlt_amd import trainvali
    from nlt_amd.datasets import nlt as D
    from nlt_amd.datasets.synth import synthetic_store
    import fake_capi
    from test_host_orchestration import make
    from test_host_vis import fake_psnr
    from trainloop_util import CAM, N_FRAMES, UV, loop_config
    fake_capi.install(patch)
    fake_psnr(patch)
    _, pm = make(256, UV, CAM, loss='l2')
    pm.build('cpu')
    real_step, real_load = trainvali.distributed_train_step, D.Dataset.load_batch

    def step(*a, **kw):
        loss, to_vis = real_step(*a, **kw)
        steps.append(float(loss))
        return loss, to_vis

    def load(self, ids, resident=False):
        if self.mode == 'train':
            loaded.append(list(ids))
        return real_load(self, ids, resident=resident)
    patch.setattr(trainvali, 'distributed_train_step', step)
    patch.setattr(D.Dataset, 'load_batch', load)
    cfg = loop_config(outroot, epochs=1, vis_train_batches=1)
    return trainvali.run(cfg, store=synthetic_store(N_FRAMES, UV, CAM, device='cpu'), device='cpu', seed=SEED, model=pm)


def _worker(rank, world, port, outroot, resdir):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
    os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    wrote = []
    real = {'open': builtins.open, 'makedirs': os.makedirs, 'replace': os.replace, 'remove': os.remove}

    def spy_open(path, mode='r', *a, **kw):
        if set(mode) & set('wax+'):
            wrote.append(('open', str(path)))
        return real['open'](path, mode, *a, **kw)

    def spy_makedirs(path, *a, **kw):
        if not os.path.isdir(path):
            wrote.append(('makedirs', str(path)))
        return real['makedirs'](path, *a, **kw)
    builtins.open, os.makedirs = spy_open, spy_makedirs
    os.replace = lambda *a, **kw: (wrote.append(('replace', str(a[0]))), real['replace'](*a, **kw))[1]
    os.remove = lambda *a, **kw: (wrote.append(('remove', str(a[0]))), real['remove'](*a, **kw))[1]
    steps, loaded = [], []
    try:
        rec = _run(outroot, _MP(), steps, loaded)
    finally:
        builtins.open, os.makedirs, os.replace, os.remove = real['open'], real['makedirs'], real['replace'], real['remove']
    torch.save({'steps': steps, 'loaded': loaded, 'wrote': wrote, 'params': rec.model.flat_params.detach().clone(),
                'loss_train': rec.loss_train, 'loss_vali': rec.loss_vali, 'step': rec.step}, os.path.join(resdir, 'r%d.pt' % rank))
    dist.destroy_process_group()


def test_one_epoch_on_two_ranks(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from trainloop_util import tree
    with tempfile.TemporaryDirectory() as td:
        out2, out1, res = (os.path.join(td, x) for x in ('world2', 'world1', 'res'))
        os.makedirs(res)
        port = 29500 + (os.getpid() * 7 + 31) % 2000
        mp.spawn(_worker, args=(WORLD, port, out2, res), nprocs=WORLD, join=True)
        r = [torch.load(os.path.join(res, 'r%d.pt' % i)) for i in range(WORLD)]
        files2 = tree(out2)
        steps1, loaded1 = [], []
        rec1 = _run(out1, monkeypatch, steps1, loaded1)
        files1 = tree(out1)
    # the ids each rank loaded, concatenated in rank order, are the single process's batches (11 frames at bs 4: 4, 4, 3)
    assert [len(b) for b in loaded1] == [4, 4, 3]
    assert [len(b) for b in r[0]['loaded']] == [2, 2, 2] and [len(b) for b in r[1]['loaded']] == [2, 2, 1]
    assert [a + b for a, b in zip(r[0]['loaded'], r[1]['loaded'])] == loaded1
    # every rank ends with bit-identical weights, and says the same about the run
    assert torch.equal(r[0]['params'], r[1]['params'])
    assert r[0]['steps'] == r[1]['steps'] and r[0]['loss_train'] == r[1]['loss_train'] and r[0]['loss_vali'] == r[1]['loss_vali']
    assert r[0]['step'] == r[1]['step'] == 1
    # only rank 0 wrote: the same files a single process leaves, the gathered visualisation of the FULL first batch included
    assert r[1]['wrote'] == [] and r[0]['wrote']
    assert files2 == files1 and any(f.endswith('vis_train/epoch000000001/batch000000000/3_pred.png') for f in files2)
    assert any(f.endswith('vis_vali/epoch000000001/batch000000000/1_pred.png') for f in files2)
    # the first step's loss against the single process on the full batch: the bar tests/test_dist_gloo.py holds its losses to
    np.testing.assert_allclose(r[0]['steps'][0], steps1[0], rtol=1e-5)
    assert rec1.step == 1
