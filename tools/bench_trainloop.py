"""What the config-driven loop costs over the bare steps: python tools/bench_trainloop.py [--uv 512] [--bs 4] [--steps 100]
[--losses l2 barron] [--repeats 3]

A synthetic capture at the released shape (512^2 UV and camera maps, bs 4), one model per loss, every leg in this one
process on that model, warmed first; a leg is one pass over the training set (`--steps` batches) timed on the host clock
from the first `load_batch` to a device synchronisation behind the last step, in ms per step:
  bare          `Dataset.load_batch` + `trainvali.distributed_train_step` in a plain for-loop over fixed batches (staging ring 2)
                -- nothing but what existed before `trainvali.run` did; `--repeats` times, to show the leg's own spread
  bare_nocache  the same with the neighbour cache off (`Dataset(nn_cache=False)`: the regex scan of every id of the store for
                every sample of every batch, which is what `load_batch` did before the cache)
  loop_epoch1   the first epoch of a two-epoch `trainvali.run` (shuffled batches, losses kept on the device, one transfer at
                the end), with checkpoints, visualisation and validation switched off by their periods; `--repeats` times.
                `run` makes its own Dataset, so this epoch fills the neighbour cache and the staging ring
  loop_epoch2   the second epoch of the same run: the cache is warm
Prints one line per leg and one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nlt_amd                                                    # noqa: E402
from nlt_amd import trainvali                                     # noqa: E402
from nlt_amd.datasets.nlt import Dataset                          # noqa: E402
from nlt_amd.datasets.synth import synthetic_store                # noqa: E402
from nlt_amd.models import get_model_class                        # noqa: E402

HELD = 4                                                          # validation frames (the Dataset wants some; never stepped)


def config(uv, bs, loss, n_frames, outroot):
    held = ','.join
    return nlt_amd.make_config(
        depth=256, uvh=uv, uvw=uv, imh=uv, imw=uv, loss=loss, bs=bs, dataset='nlt', no_batch=False, shuffle_buffer_size=256,
        epochs=2, ckpt_period=10 ** 9, vali_period=0, vis_train_batches=4, vali_batches=-1, keep_recent_epochs=-1,
        overwrite=True, outroot=outroot, xname='bench_{loss}',
        holdout_cam=held('C%03d' % i for i in range(n_frames - HELD, n_frames)),
        holdout_light=held('L%03d' % i for i in range(n_frames - HELD, n_frames)))


def bare(model, opt, ds, id_lists, bs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for ids in id_lists:
        trainvali.distributed_train_step(model, ds.load_batch(ids), opt, bs)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(id_lists)


def bench(uv, bs, steps, loss, repeats, store, outroot):
    n_frames = len(store['ids'])
    cfg = config(uv, bs, loss, n_frames, outroot)
    model = get_model_class('nlt')(cfg).build('cuda')
    model.register_trainable()
    opt = trainvali.make_optimizer(model, cfg)
    ds = Dataset(cfg, 'train', store=store, ring=2)
    ds_nocache = Dataset(cfg, 'train', store=store, ring=2, nn_cache=False)
    files = sorted(ds.files)
    id_lists = [files[i:i + bs] for i in range(0, len(files), bs)]
    assert len(id_lists) == steps and all(len(x) == bs for x in id_lists)
    bare(model, opt, ds, id_lists[:10], bs)                       # warm: plan-time trials, workspaces, the staging ring
    out = {'uv': uv, 'bs': bs, 'steps': steps, 'loss': loss, 'frames_in_store': n_frames, 'bare': [], 'bare_nocache': [], 'loop_epoch1': [], 'loop_epoch2': []}
    for r in range(repeats):                                      # alternated: no leg always runs first
        out['bare'].append(bare(model, opt, ds, id_lists, bs))
        rec = trainvali.run(cfg, store=store, seed=r, model=model)
        torch.cuda.synchronize()
        out['loop_epoch1'].append(rec.batch_time[1] * 1e3)
        out['loop_epoch2'].append(rec.batch_time[2] * 1e3)
        if r == 0:
            out['bare_nocache'].append(bare(model, opt, ds_nocache, id_lists, bs))
    for leg in ('bare', 'bare_nocache', 'loop_epoch1', 'loop_epoch2'):
        v = out[leg]
        print("trainloop %4d^2 bs %d %-7s %-13s %s ms / step  (min %.3f  max %.3f  over %d x %d steps)"
              % (uv, bs, loss, leg, ' '.join('%.3f' % x for x in v), min(v), max(v), len(v), steps))
    spread = max(out['bare']) - min(out['bare'])
    out['bare_spread'] = spread
    median = lambda v: sorted(v)[len(v) // 2]
    for leg in ('loop_epoch1', 'loop_epoch2'):
        out[leg + '_minus_bare_median'] = median(out[leg]) - median(out['bare'])
        out[leg + '_outside_bare_spread'] = not (min(out['bare']) - spread <= median(out[leg]) <= max(out['bare']) + spread)
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--uv', type=int, default=512)
    ap.add_argument('--bs', type=int, default=4)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--losses', nargs='+', default=['l2', 'barron'])
    ap.add_argument('--repeats', type=int, default=3)
    a = ap.parse_args()
    store = synthetic_store(a.steps * a.bs + HELD, a.uv, a.uv)
    with tempfile.TemporaryDirectory() as td:
        print(json.dumps([bench(a.uv, a.bs, a.steps, loss, a.repeats, store, td) for loss in a.losses]))
