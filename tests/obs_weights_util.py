"""Inputs of the `obs_weights` tests (tests/test_gpu_obs_weights.py on the GPU, tests/test_obs_weights_inputs.py on the CPU) and the
conditions that make them able to tell a right implementation from a wrong one.

A weighted case proves something only if the weights matter at its bar: with n == k a swapped (frame, observation) index can
read the right element, with all-positive weights near 1 a dropped weight hides under the tolerance.  So every case has n != k
(k = 1 apart: there the frame axis is the only one), weights from `O.synth_obs_weights` (an exact 0, negative values, values
> 1, different per frame and per observation), and asserts on the ORACLE -- never on the code under test -- that its weighted
result is at least MARGIN x the bar it applies away from the result (a) without the weights, (b) with the frame axis of the
weights flipped, (c) with their observation axis flipped (k > 1)."""
import numpy as np
import torch

from oracle import nlt_oracle as O

MARGIN = 1000.0

# forward: (uvh, uvw, hc, wc, imh, imw, n, k).  Warp grid and camera image differ from the UV map and from each other; one
# non-square UV map.  (1, 1) is the smallest call there is: one weight, nothing to flip.
FORWARD = [(64, 64, 24, 40, 48, 32, 1, 1), (64, 64, 24, 40, 48, 32, 3, 2), (64, 192, 40, 24, 32, 48, 2, 3),
           (64, 64, 24, 40, 48, 32, 3, 4)]
# train step: (uvh, uvw, hc, wc, imh, imw, n, k, loss, alpha).  (2, 1): the case whose level-split fold the weights switch off
TRAIN = [(64, 64, 24, 40, 48, 32, 2, 1, 'l2', 0.3), (64, 64, 24, 40, 48, 32, 2, 3, 'barron', 1.0),
         (64, 192, 40, 24, 32, 48, 3, 2, 'l2', 1.0), (64, 64, 24, 40, 48, 32, 2, 3, 'l2', 0.3)]
case_id = lambda c: 'uv%dx%d-warp%dx%d-im%dx%d-n%d-k%d' % tuple(c[:8]) + ''.join('-%s' % x for x in c[8:])


def seeds(c):
    """(weights seed, batch seed) of a case: fixed by its sizes."""
    uvh, uvw, n, k = c[0], c[1], c[6], c[7]
    return 300 + 10 * n + k + uvw // 64, 400 + 10 * n + k + uvw // 64


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def check_weights(w, n, k):
    """The matrix itself: [n, k], n != k unless k == 1, every kind of factor that fits."""
    assert tuple(w.shape) == (n, k) and (n != k or n == k == 1)
    v = w.flatten().tolist()
    kinds = [any(x == 0 for x in v), any(x < 0 for x in v), any(x > 1 for x in v)]
    if k > 1:
        assert all(kinds), w
        assert len({tuple(r) for r in w.tolist()}) == n and len({tuple(r) for r in w.t().tolist()}) == k, w
    else:
        assert kinds[1] and (n == 1 or kinds[2]) and len(set(v)) == n, w       # one column: (-1, 3, .75) from the top


def variants(w):
    """{name: weights} of what the weighted result must be told from: None (no weights), the frame axis flipped, the
    observation axis flipped -- each only where it is another matrix."""
    out = {'unweighted': None}
    if w.shape[0] > 1:
        out['frames_flipped'] = w.flip(0).contiguous()
    if w.shape[1] > 1:
        out['observations_flipped'] = w.flip(1).contiguous()
    return out


def assert_sensitive(evaluate, w, bars, what=''):
    """evaluate(weights | None) -> {name: array}; bars: {name: the bar the case applies to that quantity}.  Asserts that every
    quantity under `w` is >= MARGIN x its bar (rel-L2) away from itself under each of `variants(w)`; returns (the result under
    w, the distances)."""
    ref = evaluate(w)
    dist = {}
    for vname, wv in variants(w).items():
        other = evaluate(wv)
        for q, bar in bars.items():
            d = dist['%s.%s' % (q, vname)] = rel(other[q], ref[q])
            assert d >= MARGIN * bar, "%s: %s under the weights is only %.3g from %s (needs >= %g)" % (what, q, d, vname, MARGIN * bar)
    return ref, dist


def forward_inputs(c):
    """(oracle model kwargs, batch, nn, weights) of a FORWARD / TRAIN case."""
    uvh, uvw, hc, wc, imh, imw, n, k = c[:8]
    wseed, bseed = seeds(c)
    batch, nn = O.synth_batch(n, uvh, uvw, hc, wc, imh, imw, k=k, seed=bseed)
    w = O.synth_obs_weights(n, k)
    check_weights(w, n, k)
    return dict(depth=256, uvh=uvh, uvw=uvw, imh=imh, imw=imw, seed=wseed), batch, nn, w


FORWARD_BARS = {'pred': 1e-4, 'pred_camspc': 1e-4, 'aggregates': 1e-5}


def oracle_forward(om, batch, nn, w, mode='test'):
    """What the forward cases hold the HIP output against, from the fp32 oracle: `call`'s outputs, every level's (weighted)
    aggregate (`feats`, in one vector under 'aggregates') and every level's per-observation features ('obs': [level][obs])."""
    obs = []
    with torch.no_grad():
        pred_c, gt_c, _, vis = om.call(batch, mode, nn_list=nn, obs_weights=w)
        y, feats = om._call(torch.cat((batch[1], batch[2], batch[3]), 3), [r - b for b, r in nn], obs_weights=w, return_feats=True,
                            obs_outputs=obs)
    return {'call_out': y.numpy(), 'pred': vis['pred'].numpy(), 'pred_camspc': pred_c.numpy(), 'gt_camspc': None if gt_c is None else gt_c.numpy(),
            'base_camspc': vis['base_camspc'].numpy(), 'warp_px': vis['warp_px'].numpy(), 'feats': [f.numpy() for f in feats],
            'aggregates': np.concatenate([f.numpy().ravel() for f in feats]), 'obs': [[y.numpy() for y in ys] for ys in obs]}


N_QUERY_TENSORS = 52        # depth 256: 26 query convs x (kernel, bias) come first in OracleModel.parameters(); then the obs path's L0 kernel
TRAIN_BARS = {'flat': 1e-5, 'obs_L0_kernel': 1e-5}


def oracle_train(c, w, masks=None, dtype=torch.float64):
    """(loss, gradients, {'flat', 'obs_L0_kernel'}) of one train step of a TRAIN case in float64 under weights w (None: without)."""
    from gpu_util import _oracle_grads
    uvh, uvw, hc, wc, imh, imw, n, k, loss, alpha = c
    kw, batch, nn, _ = forward_inputs(c)
    lo, g = _oracle_grads(loss, 0, 0, n, dtype, batch, nn, alpha, masks=masks, seed=kw['seed'], uvh=uvh, uvw=uvw, imh=imh, imw=imw,
                          obs_weights=w)
    assert tuple(g[N_QUERY_TENSORS].shape) == (1, 1, 3, 16)
    return lo, g, {'flat': torch.cat([x.flatten() for x in g]).numpy(), 'obs_L0_kernel': g[N_QUERY_TENSORS].numpy()}
