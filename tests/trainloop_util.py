"""Shared by the train-loop tests (test_host_trainloop.py, test_dist_trainloop.py, test_gpu_trainloop.py): the config of a
small run -- 13 synthetic frames on a 64^2 UV / 32^2 camera map, 2 of them held out, bs 4, so that an epoch is batches of
4, 4 and 3 frames and the validation set one batch of 2 -- and readers for what `trainvali.run` leaves behind."""
import json
import os

import nlt_amd

N_FRAMES, UV, CAM, BS = 13, 64, 32, 4
HOLDOUT = (11, 12)                                  # synthetic_store ids carry cam C<i>, light L<i>


def loop_config(outroot, **over):
    d = dict(depth=256, uvh=UV, uvw=UV, imh=CAM, imw=CAM, loss='l2', bs=BS, dataset='nlt', no_batch=False,
             shuffle_buffer_size=64, epochs=2, ckpt_period=1, vali_period=1, vis_train_batches=4, vali_batches=-1,
             keep_recent_epochs=-1, overwrite=True, outroot=str(outroot), xname='loop_lr:{lr}_depth:{depth}',
             holdout_cam=','.join('C%03d' % i for i in HOLDOUT), holdout_light=','.join('L%03d' % i for i in HOLDOUT))
    d.update(over)
    return nlt_amd.make_config(**d)


def scalars(outdir, which):
    with open(os.path.join(outdir, 'summary_' + which, 'scalars.jsonl')) as h:
        return [json.loads(line) for line in h]


def tree(root):
    """Every file under root, relative, sorted."""
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)
