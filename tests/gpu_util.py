"""Helpers shared by the -m gpu parity tests."""
import json
import os

import numpy as np
import torch

import nlt_amd
from nlt_amd.models import get_model_class
from oracle import nlt_oracle as O

DUMP = os.environ.get('NLT_PARITY_DUMP')


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def make_pair(depth=256, uv=64, im=64, loss='l2', seed=0, use_obs=True, skip_connect_base=True, act='leakyrelu', uvh=None, uvw=None,
              imh=None, imw=None, **product_only):
    """(oracle model, product model) sharing the same Keras-layout weights.  uv / im are the square shorthand; uvh, uvw, imh,
    imw (each defaulting to it) set the axes apart."""
    uvh, uvw, imh, imw = uvh or uv, uvw or uv, imh or im, imw or im
    om = O.OracleModel(depth=depth, uvh=uvh, uvw=uvw, imh=imh, imw=imw, loss=loss, seed=seed,
                       use_obs=use_obs, skip_connect_base=skip_connect_base, act=act)
    cfg = nlt_amd.make_config(depth=depth, uvh=uvh, uvw=uvw, imh=imh, imw=imw, loss=loss,
                              use_obs=use_obs, skip_connect_base=skip_connect_base, act=act, **product_only)
    pm = get_model_class('nlt')(cfg)
    pm.load_weights(om.numpy_weights())
    pm.register_trainable()
    return om, pm


def to_device_batch(batch, nn_list, device='cuda'):
    """Oracle batch (+ list of k neighbours) -> product batch with [N,k,H,W,3] neighbour tensors."""
    dev = lambda t: None if t is None else t.to(device).contiguous()
    b = list(batch)
    nn_base = torch.stack([x[0] for x in nn_list], 1)
    nn_rgb = torch.stack([x[1] for x in nn_list], 1)
    out = [dev(t) if torch.is_tensor(t) else t for t in b]
    out[8], out[9] = dev(nn_base), dev(nn_rgb)
    return tuple(out)


def hip_activation_masks(pm, dtype=torch.bool):
    """The branch every LeakyReLU of the LAST TRAIN FORWARD took on the HIP side, in OracleModel.act_masks' keys: read off
    the post-activation maps the plan keeps for its backward pass (y > 0 <=> pre-activation > 0 for alpha >= 0; the
    backward kernels test exactly `y > 0`).  Level l: qtmp[l] / fm[l][..., :C] (query), otmp[l][:, j] / obs[l][:, j]
    (observation j); expanding block j: dtmp[j] / dec[j]."""
    (b,) = pm.plan._bufs.values()
    D, U, cl = pm.plan.n_down, pm.plan.n_up, b['C']
    cpu = lambda t: (t > 0).cpu()
    masks = {}
    for l in range(1, D + 1):
        masks[('q', l)] = (cpu(b['qtmp'][l]), cpu(b['fm'][l][..., :cl[l]]))
        for j in range(b['obs'][l].shape[1]):
            masks[('o', l, j)] = (cpu(b['otmp'][l][:, j]), cpu(b['obs'][l][:, j]))
    for j in range(U):
        masks[('q', D + 1 + j)] = (cpu(b['dtmp'][j]), cpu(b['dec'][j]))
    return masks


def _dump(name, rec):
    """Measured numbers of a parity test, one JSON record per name in the file NLT_PARITY_DUMP names (if set)."""
    if DUMP:
        os.makedirs(os.path.dirname(DUMP) or '.', exist_ok=True)
        try:
            with open(DUMP) as f:
                d = json.load(f)
        except (OSError, ValueError):
            d = {}
        d[name] = rec
        with open(DUMP, 'w') as f:
            json.dump(d, f, indent=1)


def _set_alpha(om, pm, alpha):
    """Same negative slope on both sides (alpha = 1: LeakyReLU becomes the identity -- a kink-free network)."""
    from nlt_amd.networks.elements import Act, Sequential
    om.alpha = alpha
    for net in pm.net.values():
        for blk in net.layers:
            if isinstance(blk, Sequential):
                for l in blk.layers:
                    if isinstance(l, Act):
                        l.alpha = alpha


def _oracle_grads(loss, uv, cam, n, dtype, batch, nn, alpha=None, masks=None, depth=256, seed=41, uvh=None, uvw=None, imh=None,
                  imw=None, obs_weights=None, **model_kw):
    """(loss, every kernel / bias gradient) of one train step of a fresh OracleModel(depth, seed) in `dtype`; masks: the
    activation branches to take (OracleModel.act_masks, e.g. `hip_activation_masks`).  uv / cam: the square shorthand for
    uvh x uvw / imh x imw; obs_weights: `OracleModel.call`'s; model_kw: further OracleModel keywords (kernel = 3, pool, ...)."""
    om = O.OracleModel(depth=depth, uvh=uvh or uv, uvw=uvw or uv, imh=imh or cam, imw=imw or cam, loss=loss, seed=seed, dtype=dtype,
                       **model_kw)
    if alpha is not None:
        om.alpha = alpha
    om.act_masks = masks
    b = tuple(t.to(dtype) if torch.is_tensor(t) else t for t in batch)
    nnl = [(a.to(dtype), c.to(dtype)) for a, c in nn]
    po, go, _, _ = om.call(b, 'train', nn_list=nnl, obs_weights=None if obs_weights is None else obs_weights.to(dtype))
    lo = om.compute_loss(po, go, keep_batch=True).sum() / n
    grads = [g.double() for g in torch.autograd.grad(lo, om.parameters())]
    return float(lo.detach()), grads


def _per_tensor(pm, grads):
    """(rel-L2 of the whole flat bucket, the 8 worst (rel-L2, tensor name) pairs) of the product's gradients against `grads`."""
    it = iter(grads)
    names, errs = [], []
    num = den = 0.0
    for li, c in enumerate(pm._conv_layers()):
        for nm in ('dkernel', 'dbias'):
            g = next(it)
            got = getattr(c, nm).detach().cpu().double()
            d = float((got - g).norm())
            r = float(g.norm())
            num += d * d; den += r * r
            names.append('conv%d.%s%s' % (li, nm, tuple(g.shape)))
            errs.append(d / max(r, 1e-300))
    return (num / den) ** 0.5, sorted(zip(errs, names), reverse=True)[:8]


WGRAD_FNS = ('conv_backward_weights', 'conv_backward_weights_tiled', 'conv_backward_weights_narrow')


def _spy_backward(monkeypatch, plan):
    """Every weight-gradient and backward-data launch the plan issues outside its plan-time trials, as
    (function, mode, c0, c1, n, h, w, src0, src1, dw).  The engine looks `C.<fn>` up at call time."""
    from nlt_amd import capi as C
    calls = []
    for name in WGRAD_FNS + ('conv_backward_data',):
        real = getattr(C, name)

        def spy(*a, _name=name, _real=real, **kw):
            if not plan._tuning:
                if _name == 'conv_backward_data':
                    calls.append((_name, a[0], a[2], 0, a[4], a[5], a[6], None, None, None))
                else:
                    calls.append((_name, a[0], a[2], a[5], a[7], a[8], a[9], a[1], a[4], a[13]))
            return _real(*a, **kw)
        monkeypatch.setattr(C, name, spy)
    return calls


def _force(plan, kind, hint, labels):
    """Exactly one plan-time candidate on `labels`, every other launch on its default, no trials: stored the way
    `RenderPlan._autotune` stores a winner."""
    plan.clear_choices()
    for label in labels:
        plan.set_choice(label, kind, hint)
    plan.autotune = plan.tune_backward = False
    plan._drop_tapes()


def _sweep_candidates(plan, run):
    """Every (kind, hint) the plan-time trials recorded in `plan.tuned` (run the autotuned plan first), forced alone on every
    launch it ran on (`_force`), each through `run() -> (bad, record)`.  Returns (records by candidate, failures, the
    families covered: for the forward and for the backward-data launches)."""
    tuned = {label: sorted({(kind, hint) for _, kind, hint in res}) for label, res in plan.tuned.items()}
    cands = sorted({c for cs in tuned.values() for c in cs}, key=repr)
    ran_on = {c: sorted(label for label, cs in tuned.items() if c in cs) for c in cands}
    failures, recs = [], {}
    for kind, hint in cands:
        _force(plan, kind, hint, ran_on[(kind, hint)])
        bad, rec = run()
        recs[repr((kind, hint))] = dict(rec, launches=len(ran_on[(kind, hint)]))
        if bad:
            failures.append(((kind, hint), rec))

    bwd = lambda c: [label for label in ran_on[c] if 'dgrad' in label]
    fwd = lambda c: [label for label in ran_on[c] if not label.startswith('bwd.')]
    covered = {'fwd.c32': sorted({h for k, h in cands if k == 'c32' and fwd((k, h))}),
               'fwd.lds': sorted({h for k, h in cands if k == 'lds' and fwd((k, h))}),
               'fwd.wino': sorted({h for k, h in cands if k == 'wino' and fwd((k, h))}),
               'fwd.tile': sorted({h for k, h in cands if k == 'tile' and fwd((k, h))}),
               'fwd.splitk': sorted({h for k, h in cands if k == 'splitk' and fwd((k, h))}),
               'dgrad.splitk_one_launch': sorted({h for k, h in cands if k == 'splitk' and h[1] > 0 and bwd((k, h))}),
               'dgrad.splitk_two_launches': sorted({h for k, h in cands if k == 'splitk' and h[1] < 0 and bwd((k, h))}),
               'dgrad.lds': sorted({h for k, h in cands if k == 'lds' and bwd((k, h))}),
               'dgrad.wino': sorted({h for k, h in cands if k == 'wino' and bwd((k, h))})}
    return recs, failures, covered, len(tuned), len(cands)
