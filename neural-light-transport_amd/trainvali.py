"""Train / validation steps with the reference's semantics (nlt/trainvali.py:267-325), one process
per GPU: per-example loss -> sum / GLOBAL batch size -> backward -> ONE all-reduce(sum) of the flat
fp32 gradient bucket over RCCL/xGMI -> fused Adam-AMSGrad (bit-identical on every rank) -> scalar
loss all-reduce(sum).  MirroredStrategy's in-process replicas become torch.distributed ranks."""
import argparse
import json
import logging
import os
import re
import warnings
from collections import deque
from glob import glob
from os.path import dirname, exists, isdir, join
from shutil import copyfile, rmtree
from time import time
from types import SimpleNamespace

import torch
import torch.distributed as dist

from . import ckpt
from . import optim

logger = logging.getLogger('trainvali')


def make_optimizer(model, config):
    """nlt/trainvali.py:122-127: `Adam(lr, amsgrad=True, clipnorm=mgm)` when mgm > 0.

    What `clipnorm` DOES in the reference's loop is a property of the pinned TensorFlow 2.2.0 (environment.yml:14), not of
    the reference's code: the loop calls `tape.gradient` + `optimizer.apply_gradients` (trainvali.py:279-280), and
    OptimizerV2 2.2 clips only inside `get_gradients` / `_compute_gradients` (the `minimize` path); `apply_gradients` takes
    the gradients as given.  So, as far as can be established without a TF 2.2 install, mgm > 0 changes NOTHING in the
    reference's training.  Default here = that run-time behaviour (no clipping, one warning).  The per-variable
    `tf.clip_by_norm` a reader of the config would expect is built (nlt_clip_by_norm_slots) and OPT-IN: config key
    `mgm_apply = true` (not a reference key) or NLT_APPLY_CLIPNORM=1.  The released configs set mgm = -1 either way."""
    lr = config.getfloat('DEFAULT', 'lr')
    mgm = config.getfloat('DEFAULT', 'mgm')
    apply_clip = (config.getboolean('DEFAULT', 'mgm_apply', fallback=False)
                  or os.environ.get('NLT_APPLY_CLIPNORM', '0') == '1')
    if mgm > 0 and not apply_clip:
        import warnings
        warnings.warn("mgm = %g: TF 2.2's apply_gradients (the reference's train loop) does not apply clipnorm; not clipping. "
                      "Set mgm_apply = true (or NLT_APPLY_CLIPNORM=1) for per-variable tf.clip_by_norm." % mgm)
    return optim.AdamAMSGrad(model, lr, clipnorm=mgm if (mgm > 0 and apply_clip) else None)


CKPT_FORMAT = 'nlt_amd-ckpt-2'


def save_checkpoint(path, model, optimizer, step):
    """`tf.train.Checkpoint(step=, optimizer=, net=)` + `CheckpointManager.save` of the reference train loop
    (nlt/trainvali.py:134-141,197): weights, Adam-AMSGrad slots (m, v, vhat) and iteration count, global step -- enough to
    resume training bit for bit, and what `nlt_test`-style inference restores.  One torch.save file (tensors on CPU).
    Format 2 (r06): every kernel / bias and every optimizer slot is stored PER VARIABLE in canonical order; format 1 stored
    the raw flat bucket, whose slot order depends on the writer's `_flatten` (advisor r05: a file written under another
    NLT_GRAD_RANGES loaded without error and with permuted weights)."""
    cpu = lambda x: ([t.detach().cpu() for t in x] if isinstance(x, (list, tuple)) else (x.detach().cpu() if torch.is_tensor(x) else x))
    cpud = lambda d: {k: cpu(v) for k, v in d.items()}
    torch.save({'format': CKPT_FORMAT, 'step': int(step), 'net': cpud(model.state_dict()),
                'optimizer': cpud(optimizer.state_dict()) if optimizer is not None else None}, path)
    return path


def _convert_ckpt1(ck, model):
    """A format-1 file (raw flat buckets) -> format-2 dicts, cutting the buckets by THIS process's slot table."""
    net = ck['net']
    shapes = [(tuple(c.kernel.shape), tuple(c.bias.shape)) for c in model._conv_layers()]
    if [tuple(map(tuple, x)) for x in net['slots']] != shapes or net['flat_params'].numel() != model.flat_params.numel():
        raise ValueError("checkpoint was written by a different architecture (layer shapes differ)")
    cut = lambda flat: [flat.reshape(-1)[o:o + n].reshape(shp).clone() for o, n, shp in model.legacy_bucket_layout()]
    out = {'net': {'variables': cut(net['flat_params'])}, 'optimizer': None}
    if ck.get('optimizer') is not None:
        o = ck['optimizer']
        out['optimizer'] = {'t': o['t'], 'm': cut(o['m']), 'v': cut(o['v']), 'vhat': cut(o['vhat'])}
    return out


def restore_checkpoint(path, model, optimizer=None, legacy_layout=False):
    """Loads what `save_checkpoint` wrote into a built model (and optimizer); returns the global step.  The optimizer may be
    omitted (inference: nlt/nlt_test.py:92-97 restores the net alone).  A format-1 file (rounds 1-5: raw flat buckets) is
    refused unless `legacy_layout=True` states that it was written with the bucket layout this process uses (same code
    generation, same NLT_GRAD_RANGES) -- the file itself cannot tell."""
    ck = torch.load(path, map_location='cpu', weights_only=True)     # tensors, ints, strings, lists only: no pickle code runs
    fmt = ck.get('format')
    if fmt == 'nlt_amd-ckpt-1':
        if not legacy_layout:
            raise ValueError("%s is a format-1 checkpoint (raw flat parameter bucket): its slot order depends on the writer's "
                             "bucket layout and is not recorded in the file.  Pass legacy_layout=True if it was written by the "
                             "same code generation with the same NLT_GRAD_RANGES, then save it again (format 2)." % path)
        ck = dict(ck, **_convert_ckpt1(ck, model))
    elif fmt != CKPT_FORMAT:
        raise ValueError("%s is not an nlt_amd checkpoint" % path)
    model.load_state_dict(ck['net'])
    if optimizer is not None:
        if ck['optimizer'] is None:
            raise ValueError("%s holds no optimizer state" % path)
        optimizer.load_state_dict(ck['optimizer'])
    return ck['step']


def save_reference(manager, model, optimizer, step):
    """`ckptmanager.save()` of the reference's loop (nlt/trainvali.py:194) in the REFERENCE's own format: a TensorFlow tensor
    bundle `ckpt-N` under `manager` (a `ckpt.ReferenceCheckpointManager`), which the reference's `nlt_test.py --ckpt` and
    `trainvali.py` are meant to pick up (ckpt.py's STATUS says how far that has been checked).  Returns the prefix written."""
    return manager.save(model, optimizer, step)


def resume_reference(manager, model, optimizer):
    """`ioutil.restore(ckpt, ckptmanager)` (nlt/util/io.py:32-35): restores net + optimizer from the manager's latest
    checkpoint -- one a reference run left there included -- and returns its step; an empty directory changes nothing and
    returns 0 (`ckpt.step` keeps its initial value)."""
    latest = manager.latest_checkpoint
    if latest is None:
        return 0
    step = ckpt.restore_reference_checkpoint(model, latest, optimizer)
    return 0 if step is None else step


AUTOGRAD_STEP = os.environ.get('NLT_AUTOGRAD_STEP', '0') == '1'   # single-rank step through torch.autograd (the reference-shaped path)


def _world(group):
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


def distributed_train_step(model, batch, optimizer, global_bs, group=None, overlap=True, obs_weights=None):
    """batch = this rank's shard of the global batch.  Returns (loss summed over ranks, to_vis).
    obs_weights [N, k] (this rank's frames): `Model.call`'s per-frame, per-observation factors of the aggregate (nlt.py:162-163);
    such a step runs the layer-by-layer plan, forward and backward.

    One rank: per-example loss -> sum / global batch -> autograd backward -> fused Adam.
    Several ranks: the gradient sum is THREE all-reduces of fixed contiguous ranges of the flat bucket, cut in the order
    the backward pass finishes them (`Model.bucket_ranges`: expanding blocks | encoder levels D .. 3 | the rest), so every
    rank adds the same numbers in the same order: bit-identical weights.  The first two are issued from inside the backward
    plan as soon as their weight-gradient launches are queued (on their stream) and run over xGMI while the rest of the
    backward occupies the CUs; only the last (0.1 MB of 13.5) follows the backward.  overlap=False issues all three after
    the backward (same result)."""
    assert model.trainable_registered, "Register the trainable layers before using `trainable_variables`"
    world = _world(group)
    if world == 1 and not AUTOGRAD_STEP and not getattr(model, 'generic', False):     # (branch configs run layer by layer through autograd)
        # same arithmetic without a torch.autograd graph around the network (only the loss is differentiated): no AccumulateGrad
        # copy of the 13.5 MB bucket, no expand / fill launches for the sum and the division
        loss, to_vis = model.train_forward_backward(batch, global_bs, obs_weights=obs_weights)
        model.flat_params.grad = model.flat_grads
        optimizer.step(model.flat_grads)
        return loss.clone(), to_vis
    if world == 1:
        pred, gt, loss_kwargs, to_vis = model(batch, mode='train', obs_weights=obs_weights)
        loss_kwargs['keep_batch'] = True
        per_example_loss = model.compute_loss(pred, gt, **loss_kwargs)
        weighted_loss = per_example_loss.sum() / global_bs         # tf.nn.compute_average_loss
        model.flat_params.grad = None
        weighted_loss.backward()
        grad = model.flat_params.grad
        optimizer.step(grad)
        return weighted_loss.detach().clone(), to_vis
    if getattr(model, 'generic', False):
        # the layer-by-layer branch configs (elu / pixel, layer, batch norm / pooling): the same step, the network differentiated
        # through its hand-rolled tape (generic.py) into the same flat bucket, then ONE all-reduce of the whole bucket (no
        # backward plan to overlap with).  Batch norm needs no cross-replica statistics: the reference runs it in inference
        # mode (networks/elements.py ChannelNorm).
        pred, gt, loss_kwargs, to_vis = model(batch, mode='train', obs_weights=obs_weights)
        loss_kwargs['keep_batch'] = True
        loss = model.compute_loss(pred, gt, **loss_kwargs).sum() / global_bs
        model.flat_params.grad = None
        loss.backward()
        grad = model.flat_params.grad
        loss = loss.detach().clone()
        works = [dist.all_reduce(grad, op=dist.ReduceOp.SUM, group=group, async_op=True),
                 dist.all_reduce(loss, op=dist.ReduceOp.SUM, group=group, async_op=True)]
        for w in works:
            w.wait()
        optimizer.step(grad)
        return loss, to_vis
    grad, r = model.flat_grads, model.bucket_ranges
    works, sent = [], set()

    def reduce_range(i):
        if i not in sent and r[i + 1] > r[i]:
            works.append(dist.all_reduce(grad[r[i]:r[i + 1]], op=dist.ReduceOp.SUM, group=group, async_op=True))
        sent.add(i)
    if overlap:
        model.plan.grad_hook = reduce_range
    try:
        loss, to_vis = model.train_forward_backward(batch, global_bs, obs_weights=obs_weights)    # gradients land in the flat bucket (no autograd copy)
    finally:
        model.plan.grad_hook = None
    for i in range(len(r) - 1):                                         # whatever the backward did not send, in range order
        reduce_range(i)
    loss = loss.clone()
    works.append(dist.all_reduce(loss, op=dist.ReduceOp.SUM, group=group, async_op=True))
    for w in works:
        w.wait()                                                    # (CUDA: the current stream waits; the host does not block)
    model.flat_params.grad = grad
    optimizer.step(grad)
    return loss, to_vis


class GraphedTrainStep:
    """`distributed_train_step` with forward + loss + backward captured ONCE as a hipGraph and replayed: the step is
    ~170 small launches, and issuing them one by one from Python costs about as much wall time as the GPU needs to
    run them.  The gradient all-reduce (RCCL) and the Adam-AMSGrad launch (its bias-correction scalars change every
    step) stay eager, after the replay.

    The graph is tied to tensor ADDRESSES: the batch is copied into static buffers owned by this object (a no-op when
    the caller already passes them back), the shapes of the batches given to THIS object must not change, and the returned
    loss / to_vis tensors are the graph's static outputs -- consume them before the next call.  The first `warmup` calls
    run eagerly (plan-time autotune, workspace allocation); any failure to capture falls back to the eager step for good.

    Between two calls anything else may run: other calls on the model at any shape (a validation step on a short batch, a
    test render), other models in the process.  Such calls can hand memory the graph baked in back to the allocator -- the
    plan keeps one shape's buffers resident, cached scratch is replaced when a larger one is needed, a census retires packed
    fragments -- and `RenderPlan.replay_stamp` (three integers, compared before every replay) says so: after scratch or
    fragments moved the step is captured again at once; after the buffer set was replaced one step runs eagerly (the new set
    is allocated, and tuned, outside any capture) and the next one captures."""

    TENSORS = (1, 2, 3, 4, 5, 6, 8, 9, 10)       # tensor entries of the 11-tuple batch (nlt/models/nlt.py:91-92)

    def __init__(self, model, optimizer, global_bs, group=None, warmup=2):
        self.model, self.optimizer, self.global_bs, self.group = model, optimizer, global_bs, group
        self.warmup, self.seen = warmup, 0
        self.graph, self.static, self.out, self.failed = None, None, None, None
        self._table = self._stamp = None             # the registry's descriptor table the graph embeds, and `plan.replay_stamp` at the capture

    def static_batch(self):
        """The graph's own input tensors (None before the capture): a loader that fills THESE and passes them back
        skips the per-step device-to-device copies."""
        return tuple(self.static) if self.graph is not None else None

    def _body(self, batch):
        loss, to_vis = self.model.train_forward_backward(batch, self.global_bs)
        return loss.clone(), to_vis

    def _finish(self, loss):
        grad = self.model.flat_grads
        self.model.flat_params.grad = grad
        if _world(self.group) > 1:
            dist.all_reduce(grad, op=dist.ReduceOp.SUM, group=self.group)
            dist.all_reduce(loss, op=dist.ReduceOp.SUM, group=self.group)
        self.optimizer.step(grad)
        return loss

    def __call__(self, batch):
        dev_ok = isinstance(batch[1], torch.Tensor) and batch[1].is_cuda and self.model.plan.timer is None
        if self.failed is not None or not dev_ok or self.seen < self.warmup:
            self.seen += 1
            return distributed_train_step(self.model, batch, self.optimizer, self.global_bs, self.group)
        reg = getattr(self.model, 'pack_registry', None)
        stamp = self.model.plan.replay_stamp(reg)
        if self._stamp is not None and stamp != self._stamp:
            # Something the graph baked in was let go after the capture (`RenderPlan.replay_stamp`).  The SET of packed buffers
            # changed (a census retired some, a plan re-tuned: advisor r05): the captured repack launch would walk a descriptor
            # table the registry no longer maintains.  Cached scratch grew (another model, a larger shape): the graph points
            # into the old one.  Either way: capture again.  The plan's buffer set was replaced (a call on the model at another
            # shape): the graph's activations are back with the allocator -- this step runs eagerly, so that the new set is
            # allocated (and its plan-time trials run) outside any capture, and the next call captures.
            self.graph = self.out = None
            new_set, self._stamp = stamp[0] != self._stamp[0], None
            if new_set:
                return distributed_train_step(self.model, batch, self.optimizer, self.global_bs, self.group)
        if self.graph is None:
            try:
                self.static = list(batch)
                for i in self.TENSORS:
                    self.static[i] = batch[i].clone()
                reg = getattr(self.model, 'pack_registry', None)
                if reg is not None:                      # the refresh of the packed weights must be IN the graph, its
                    reg.prune()                          # (a running census of used fragment buffers ends here, not mid-capture)
                    reg.prepare()                        # descriptor upload must not
                    reg.state = None
                if self.model.plan._front_blob is not None:
                    self.model.plan._front_blob[0] = None    # ... and so must the folded front-kernel weights
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    self.out = self._body(tuple(self.static))
                self.graph = graph
                self._table = reg.table if reg is not None else None      # (keeps the captured table's tensors alive)
                self._stamp = self.model.plan.replay_stamp(reg)           # (after the capture: scratch it grew itself included)
            except Exception as e:                       # capture is an optimisation, never a requirement
                self.failed = repr(e)
                self.graph = None
                torch.cuda.synchronize()
                return distributed_train_step(self.model, batch, self.optimizer, self.global_bs, self.group)
        for i in self.TENSORS:
            if batch[i].data_ptr() != self.static[i].data_ptr():
                self.static[i].copy_(batch[i])
        self.graph.replay()
        loss, to_vis = self.out
        return self._finish(loss.clone()), to_vis


def distributed_vali_step(model, batch, global_bs, group=None):
    with torch.no_grad():
        pred, gt, loss_kwargs, to_vis = model(batch, mode='vali')
        loss_kwargs['keep_batch'] = True
        loss = model.compute_loss(pred, gt, **loss_kwargs).sum() / global_bs
        if _world(group) > 1:
            dist.all_reduce(loss, op=dist.ReduceOp.SUM, group=group)
    return loss, to_vis


# ---------------------------------------------------------------------------------------------------------------------
# The driver: nlt/trainvali.py:48-251,328-332 restated on the steps above.  The HOST schedules the batches
# (`Dataset.build_pipeline`); the loop has no arithmetic of its own beyond one float32 mean per epoch.
def read_config(path):
    """nlt/util/io.py:40-44."""
    from configparser import ConfigParser
    config = ConfigParser()
    with open(path, 'r') as h:
        config.read_file(h)
    return config


def config2dict(config):
    """nlt/util/config.py:15-22 (the .ini has only the default section)."""
    return dict(config.items('DEFAULT'))


def resolve_config(name):
    """nlt/trainvali.py:56-59: `name` as a path if it exists, else a file in the `config/` directory beside this module."""
    if not exists(name):
        return join(dirname(os.path.abspath(__file__)), 'config', name)
    return name


def outdir_of(config):
    """nlt/trainvali.py:62-65: <outroot>/<xname formatted with every key of the config>."""
    xname = config.get('DEFAULT', 'xname').format(**config2dict(config))
    return join(config.get('DEFAULT', 'outroot'), xname)


def prepare_outdir(outdir, overwrite=False):
    """nlt/util/io.py:47-60.  overwrite = True -- what both released configs set -- wipes the WHOLE directory, the
    checkpoints of an earlier run included: such a config never resumes."""
    if isdir(outdir):
        logger.info("Output directory already exisits:\n\t%s", outdir)
        if overwrite:
            rmtree(outdir)
            logger.warning("Output directory wiped:\n\t%s", outdir)
        else:
            logger.info("Overwrite is off, so doing nothing")
            return
    os.makedirs(outdir)


def maintain_epoch_queue(queue, new_epoch_dir):
    """nlt/trainvali.py:328-332: `queue` is a deque(maxlen = keep_recent_epochs or None); every sibling of the new epoch
    directory that is not in the queue is removed -- the directories of a run this one resumed from included, since the
    queue starts empty."""
    queue.appendleft(new_epoch_dir)
    for epoch_dir in glob(join(dirname(new_epoch_dir), '*')):
        if epoch_dir not in queue:      # already evicted from queue (FIFO)
            rmtree(epoch_dir)


class ScalarWriter:
    """Stands in for `tf.summary.create_file_writer(dir)` + `tf.summary.scalar / text`: one JSON object per line,
    {"tag", "step", "value"}, appended to `<dir>/scalars.jsonl`.  (TensorBoard event files are out of scope.)"""

    def __init__(self, directory):
        self.path = join(directory, 'scalars.jsonl')
        os.makedirs(directory, exist_ok=True)

    def write(self, tag, value, step):
        with open(self.path, 'a') as h:
            h.write(json.dumps({'tag': tag, 'step': int(step), 'value': value}) + '\n')

    scalar = text = write


class NativeCheckpointManager:
    """`ReferenceCheckpointManager`'s numbering and retention over `save_checkpoint` files `ckpt-N.pt`, for the models the
    reference format cannot hold (norm variables, upconv)."""

    def __init__(self, directory, max_to_keep=None):
        self.directory, self.max_to_keep = directory, max_to_keep
        os.makedirs(directory, exist_ok=True)

    @property
    def checkpoints(self):
        found = []
        for path in glob(join(self.directory, 'ckpt-*.pt')):
            m = re.search(r'ckpt-(\d+)\.pt$', path)
            if m:
                found.append((int(m.group(1)), path))
        return [p for _, p in sorted(found)]

    @property
    def latest_checkpoint(self):
        all_ = self.checkpoints
        return all_[-1] if all_ else None

    def save(self, model, optimizer, step):
        all_ = self.checkpoints
        n = int(re.search(r'ckpt-(\d+)\.pt$', all_[-1]).group(1)) + 1 if all_ else 1
        path = save_checkpoint(join(self.directory, 'ckpt-%d.pt' % n), model, optimizer, step)
        for old in ((all_ + [path])[:-self.max_to_keep] if self.max_to_keep else []):
            os.remove(old)
        return path

    def restore(self, model, optimizer):
        latest = self.latest_checkpoint
        return 0 if latest is None else restore_checkpoint(latest, model, optimizer)


def make_checkpoint_manager(config, model, directory, max_to_keep):
    """`ckpt_format = reference` (default; not a reference key): TensorFlow tensor bundles the reference's own tools read;
    `native`: `save_checkpoint` files.  A model the reference format refuses gets the native one, with one warning."""
    fmt = config.get('DEFAULT', 'ckpt_format', fallback='reference')
    if fmt not in ('reference', 'native'):
        raise ValueError("ckpt_format = %s (reference | native)" % fmt)
    if fmt == 'reference':
        try:
            ckpt._variable_prefixes(model)
        except NotImplementedError as e:
            warnings.warn("checkpoints are written in the native format (ckpt-N.pt): %s" % e)
            fmt = 'native'
    if fmt == 'native':
        return NativeCheckpointManager(directory, max_to_keep)
    return ckpt.ReferenceCheckpointManager(directory, max_to_keep=max_to_keep)


def _rank(group):
    return dist.get_rank(group) if dist.is_available() and dist.is_initialized() else 0


def mean_loss(losses):
    """`tf.reduce_mean(batch_loss)` (nlt/trainvali.py:199,236) of per-batch scalars still on the device: ONE transfer, then a
    float32 mean on the host."""
    return float(torch.stack([l.detach().reshape(()) for l in losses]).float().cpu().mean())


def _keep(to_vis):
    """A `to_vis` that outlives the step: the step may hand out views of buffers the next step (the loader's staging ring,
    a replayed graph's static outputs) writes again."""
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in to_vis.items()}


def gather_to_vis(to_vis, group=None):
    """`aggeregate_dstributed`'s concat (nlt/trainvali.py:319-323): every rank's partial `to_vis` back to the full batch, in
    rank order, on rank 0 (None elsewhere).  Shards differ in length, so the parts travel as host arrays."""
    world = _world(group)
    if world == 1:
        return to_vis
    host = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in to_vis.items()}
    lead = _rank(group) == 0
    parts = [None] * world if lead else None
    dist.gather_object(host, parts, dst=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    if not lead:
        return None
    import numpy as np
    out = {}
    for k in host:
        vals = [p[k] for p in parts]
        if vals[0] is None:
            out[k] = None
        elif isinstance(vals[0], np.ndarray):
            out[k] = np.concatenate(vals, 0)
        else:
            out[k] = [x for v in vals for x in v]
    return out


def _visualize(model, batch_vis, epoch_dir, mode, writer, step):
    """nlt/trainvali.py:203-215 / :237-249: every kept batch into `<epoch_dir>/batch<b>` (+ `batch<b>_raw.pickle`), then
    the compilation `<epoch_dir>/all.*`, whose address goes in as a text summary."""
    vis_dirs = []
    for batch_i, to_vis in enumerate(batch_vis):
        vis_dir = join(epoch_dir, 'batch{b:09d}'.format(b=batch_i))
        model.vis_batch(to_vis, vis_dir, mode=mode, dump_raw_to=vis_dir + '_raw.pickle')
        vis_dirs.append(vis_dir)
    view_at = model.compile_batch_vis(vis_dirs, join(epoch_dir, 'all'), mode=mode)
    if view_at is not None:
        writer.text('vis_' + mode, view_at, step)


def run(config, config_ini=None, store=None, device='cuda', group=None, debug=False, seed=None, graphs=False, model=None):
    """`main` of nlt/trainvali.py:61-251 for a parsed config: output directory, datasets, model, optimizer, resume, and the
    epoch loop with its checkpoints, summaries, visualisations and validation passes.
    store: the resident capture (None: `load_store(data_root)`); group: the process group of a several-rank run (rank 0
    alone writes, every rank restores); seed: the shuffle's seed (`Dataset.build_pipeline`); graphs: full batches through
    one `GraphedTrainStep`; model: a built model to train where the config's own, freshly initialised, is not wanted.
    Keys of ours, all optional: `k` (neighbours per sample, 1), `ckpt_format` (reference), `loader_ring` (2).  The
    reference's `cache`, `prefetch_buffer_size` and `n_map_parallel_calls` have nothing to steer here and are not read.
    Returns a record: outdir, step (the last epoch done), loss_train / loss_vali / batch_time ({epoch: float}), model,
    optimizer, graphed."""
    from .datasets import get_dataset_class
    from .models import get_model_class
    get = lambda k: config.get('DEFAULT', k)
    geti = lambda k: config.getint('DEFAULT', k)
    rank, world = _rank(group), _world(group)
    lead = rank == 0
    if debug:
        logger.warning("Debug mode: On")

    # Output directory
    outdir = outdir_of(config)
    overwrite = config.getboolean('DEFAULT', 'overwrite')
    if lead:
        prepare_outdir(outdir, overwrite=overwrite)
        logger.info("For results, see:\n\t%s", outdir)
        # Save a copy of the configuration file used
        ini_copy = outdir.rstrip('/') + '.ini'
        if config_ini is not None and not (exists(ini_copy) and os.path.samefile(config_ini, ini_copy)):
            copyfile(config_ini, ini_copy)
    if world > 1:
        dist.barrier(group)

    # Make training dataset
    Dataset = get_dataset_class(get('dataset'))
    k = config.getint('DEFAULT', 'k', fallback=1)
    shuffle_buffer_size = geti('shuffle_buffer_size')
    dataset_train = Dataset(config, 'train', store=store, k=k, device=device, shuffle_buffer_size=shuffle_buffer_size)
    store = dataset_train.store
    # The reference divides every batch's loss sum by `bs`: the short last batch's too, and with no_batch = True a
    # one-sample batch's as well (nlt/trainvali.py:87,176).
    global_bs_train = dataset_train.bs
    no_batch = config.getboolean('DEFAULT', 'no_batch')
    ring = config.getint('DEFAULT', 'loader_ring', fallback=2)

    # Make validation dataset
    dataset_vali = Dataset(config, 'vali', store=store, k=k, device=device, shuffle_buffer_size=shuffle_buffer_size)
    global_bs_vali = dataset_vali.bs
    # Sample validation batches, and just stick with them.  The reference calls `take(vali_batches * bs)` on the ALREADY
    # BATCHED pipeline (nlt/trainvali.py:106-111), so `vali_batches = n` keeps up to n * bs batches, not n; -1 keeps all.
    n_vali_batches = geti('vali_batches')
    n_elements = -1 if n_vali_batches == -1 else n_vali_batches * global_bs_vali
    vali_batches = list(dataset_vali.build_pipeline(no_batch=no_batch, rank=rank, world=world).take(n_elements))

    # Model
    if model is None:
        model = get_model_class(get('model'))(config)
        model.build(device)
    if not model.trainable_registered:
        model.register_trainable()

    # Optimizer
    optimizer = make_optimizer(model, config)

    # Resume from checkpoint, if any
    keep_recent_epochs = geti('keep_recent_epochs')
    if keep_recent_epochs <= 0:
        keep_recent_epochs = None       # keep all epochs
    if lead:                            # (the manager makes its directory; the other ranks open it once it is there)
        manager = make_checkpoint_manager(config, model, join(outdir, 'checkpoints'), keep_recent_epochs)
    if world > 1:
        dist.barrier(group)
    if not lead:
        manager = make_checkpoint_manager(config, model, join(outdir, 'checkpoints'), keep_recent_epochs)
    if isinstance(manager, NativeCheckpointManager):
        step = manager.restore(model, optimizer)
    else:
        step = resume_reference(manager, model, optimizer)
    logger.info("Resumed from step:\n\t%s", manager.latest_checkpoint) if step else logger.info("Started from scratch")

    # Summary directories
    writer_train = ScalarWriter(join(outdir, 'summary_train')) if lead else None
    writer_vali = ScalarWriter(join(outdir, 'summary_vali')) if lead else None
    train_vis_epoch_dir = join(outdir, 'vis_train', 'epoch{e:09d}')
    vali_vis_epoch_dir = join(outdir, 'vis_vali', 'epoch{e:09d}')
    train_vis_epoch_dir_deque = deque([], keep_recent_epochs)
    vali_vis_epoch_dir_deque = deque([], keep_recent_epochs)

    # ====== Training loop ======
    epochs = geti('epochs')
    vis_train_batches = geti('vis_train_batches')
    ckpt_period = geti('ckpt_period')
    vali_period = geti('vali_period')
    graphed = GraphedTrainStep(model, optimizer, global_bs_train, group, warmup=1) if graphs else None
    graphed_n = None                    # frames per batch of the shape the graph is captured at: the first batch's
    last_full = False                   # the last call on the model was a train step at that shape (its buffers are the plan's)
    record = SimpleNamespace(outdir=outdir, step=step, loss_train={}, loss_vali={}, batch_time={}, model=model,
                             optimizer=optimizer, graphed=graphed)
    for epoch in range(step, epochs):
        # ------ Train on all batches ------
        datapipe_train = dataset_train.build_pipeline(seed=seed, no_batch=no_batch, epoch=epoch, ring=ring, rank=rank,
                                                      world=world)
        will_vis = (epoch + 1) % ckpt_period == 0
        batch_loss, batch_vis, n_batches = [], [], 0
        t0 = time()
        for batch_i, batch in enumerate(datapipe_train):
            if graphed is not None and graphed_n is None:
                graphed_n = len(batch[0])
            full = graphed is not None and len(batch[0]) == graphed_n
            # A FIRST capture (no stamp to compare yet) right behind a call at another shape would allocate the plan's buffer
            # set inside the capture: that batch takes the eager step and the next one captures.  Once there is a graph,
            # `replay_stamp` sees to the way back from the short last batch and the validation pass by itself.
            if full and (graphed.graph is not None or graphed._stamp is not None or graphed.seen < graphed.warmup or last_full):
                loss, to_vis = graphed(batch)
            else:                       # (the short last batch too: the graph's shape is fixed)
                loss, to_vis = distributed_train_step(model, batch, optimizer, global_bs_train, group)
            last_full = full
            n_batches += 1
            batch_loss.append(loss)     # stays on the device: no per-step `.item()`
            if batch_i < vis_train_batches and will_vis:
                batch_vis.append(_keep(to_vis))
            if debug:
                logger.warning("Debug mode: Skipping the rest of this epoch")
                break
        assert n_batches, "Dataset is empty"
        loss_train = mean_loss(batch_loss)
        # (the steps are enqueued, not awaited, one by one: the epoch's wall time, loader included, over its batches)
        batch_time = (time() - t0) / n_batches

        # Record step
        step = epoch + 1
        record.step = step
        record.loss_train[step], record.batch_time[step] = loss_train, batch_time

        # Checkpoint and summarize/visualize training
        if step % ckpt_period == 0:
            batch_vis = [gather_to_vis(v, group) for v in batch_vis]
            if lead:
                saved_path = manager.save(model, optimizer, step)
                logger.info("Checkpointed step %s:\n\t%s", step, saved_path)
                writer_train.scalar('loss_train', loss_train, step)
                writer_train.scalar('batch_time_train', batch_time, step)
                epoch_dir = train_vis_epoch_dir.format(e=step)
                if batch_vis:
                    _visualize(model, batch_vis, epoch_dir, 'train', writer_train, step)
                else:
                    os.makedirs(epoch_dir, exist_ok=True)
                maintain_epoch_queue(train_vis_epoch_dir_deque, epoch_dir)
        del batch_vis

        # ------ Validation ------
        if vali_period > 0 and step % vali_period == 0:
            batch_loss, batch_vis = [], []
            for batch in vali_batches:
                loss, to_vis = distributed_vali_step(model, batch, global_bs_vali, group)
                last_full = False
                batch_loss.append(loss)
                batch_vis.append(gather_to_vis(_keep(to_vis), group))
            record.loss_vali[step] = loss_vali = mean_loss(batch_loss)
            if lead:
                writer_vali.scalar('loss_vali', loss_vali, step)
                epoch_dir = vali_vis_epoch_dir.format(e=step)
                _visualize(model, batch_vis, epoch_dir, 'vali', writer_vali, step)
                maintain_epoch_queue(vali_vis_epoch_dir_deque, epoch_dir)
            del batch_vis
    if world > 1:
        dist.barrier(group)             # (rank 0's files are there when any rank returns)
    return record


def parse_args(argv=None):
    """The reference's flags (nlt/trainvali.py:38-42) and two of ours: --seed (the shuffle's), --graphs."""
    p = argparse.ArgumentParser(prog='nlt_amd.trainvali', description="A general training and validation pipeline.")
    p.add_argument('--config', default='config.ini', help="a .ini file in `config/` or a full path")
    p.add_argument('--debug', action='store_true', help="debug mode switch")
    p.add_argument('--device', default='gpu', choices=['cpu', 'gpu'], help="running on what type of device(s)")
    p.add_argument('--seed', type=int, default=None, help="seed of the training shuffle (default: drawn once)")
    p.add_argument('--graphs', action='store_true', help="replay the train step of full batches as one hipGraph")
    args = p.parse_args(argv)
    if args.device == 'cpu':
        p.error("--device cpu: every layer of this package is a HIP kernel for the GPU and no CPU fallback exists")
    return args


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    group = None
    if int(os.environ.get('WORLD_SIZE', '1')) > 1 and 'RANK' in os.environ:      # under torchrun: one process per GPU
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
        dist.init_process_group('nccl')
    config_ini = resolve_config(args.config)
    try:
        return run(read_config(config_ini), config_ini=config_ini, device='cuda', group=group, debug=args.debug,
                   seed=args.seed, graphs=args.graphs)
    finally:
        if dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()


if __name__ == '__main__':             # python -m nlt_amd.trainvali: hand over to the package's own copy of this module
    from .trainvali import main as _main
    _main()
