"""-m gpu: memory discipline of every entry point of csrc/lpips.hip with tests/guard_util.py, at the (1,31,31) and (2,47,64)
image shapes.  Every tensor argument is a guarded view under the three fills; the adapters' own allocations (outputs, the head's
and the chain's scratch, at exactly the queried size and starting as the fill) are guarded through `guard_util.guarded_allocs`.
Per case: bands and read-only operands (inputs, weights) intact, outputs fully written (no fill survives: finite), the same bits
under every fill -- so no scratch slot is read before it is written -- and bit for bit the result on plain tensors, which
tests/test_gpu_lpips.py holds to the float64 restatement.  One float less scratch is refused and nothing is touched."""
import numpy as np
import pytest
import torch

from nlt_amd import capi as C
from nlt_amd import lpips_weights
import guard_util as G
import lpips_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 31, 31), (2, 47, 64)]
W = R.random_weights(0)
t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _maps(shape):
    n, h, w = shape
    h1, w1 = (h - 7) // 4 + 1, (w - 7) // 4 + 1
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    return (h1, w1), (h2, w2), ((h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1)


def _rand(shape, seed, relu=False):
    a = np.random.RandomState(seed).standard_normal(shape).astype(np.float32)
    return t32(np.maximum(a + 0.3, 0) if relu else a)


@pytest.mark.parametrize('shape', SHAPES)
def test_conv1_pair(monkeypatch, shape):
    n, h, w = shape
    (h1, w1), _, _ = _maps(shape)
    ins = dict(x=t32(R.make_pair('far', n, h, w, seed=1)[0]), affine=t32(R.affine()), wk=t32(R.keras(W, 1)), b=t32(W['conv1_bias']))
    res, _, _ = G.bitwise_case(monkeypatch, lambda t: C.lpips_conv1_forward(t['x'], t['affine'], t['wk'], t['b']), ins)
    assert res[0]['ret'].shape == (n, h1, w1, 64)
    ins = dict(dpre=_rand((n, h1, w1, 64), 2), affine=ins['affine'], wk=ins['wk'])
    res, _, _ = G.bitwise_case(monkeypatch, lambda t: C.lpips_conv1_backward_data(t['dpre'], h, w, t['affine'], t['wk']), ins)
    assert res[0]['ret'].shape == (n, h, w, 3)


@pytest.mark.parametrize('shape', SHAPES)
def test_conv2_pair(monkeypatch, shape):
    n = shape[0]
    _, (h2, w2), _ = _maps(shape)
    ins = dict(x=_rand((n, h2, w2, 64), 3, relu=True), wk=t32(R.keras(W, 2)), b=t32(W['conv2_bias']))
    res, _, _ = G.bitwise_case(monkeypatch, lambda t: C.lpips_conv2_forward(t['x'], t['wk'], t['b']), ins)
    assert res[0]['ret'].shape == (n, h2, w2, 192)
    ins = dict(dpre=_rand((n, h2, w2, 192), 4), wk=ins['wk'])
    res, _, _ = G.bitwise_case(monkeypatch, lambda t: C.lpips_conv2_backward_data(t['dpre'], t['wk']), ins)
    assert res[0]['ret'].shape == (n, h2, w2, 64)


@pytest.mark.parametrize('shape', SHAPES)
def test_pool_pair(monkeypatch, shape):
    n = shape[0]
    (h1, w1), (h2, w2), (h3, w3) = _maps(shape)
    for (h, w, oh, ow, c) in ((h1, w1, h2, w2, 64), (h2, w2, h3, w3, 192)):
        ins = dict(x=_rand((n, h, w, c), 5, relu=True))
        G.bitwise_case(monkeypatch, lambda t: C.lpips_pool_forward(t['x']), ins)
        ins['dy'] = _rand((n, oh, ow, c), 6)
        G.bitwise_case(monkeypatch, lambda t: C.lpips_pool_backward(t['dy'], t['x']), ins)


@pytest.mark.parametrize('shape', SHAPES)
def test_head_pair(monkeypatch, shape):
    n = shape[0]
    for (h, w), c in zip(_maps(shape), (64, 192, 384)):
        ins = dict(fp=_rand((n, h, w, c), 7, relu=True), fg=_rand((n, h, w, c), 8, relu=True), lin=t32(W['lin%d' % {64: 1, 192: 2, 384: 3}[c]]))
        res, state, _ = G.bitwise_case(monkeypatch, lambda t: C.lpips_head_forward(t['fp'], t['fg'], t['lin']), ins)
        assert C.lib().nlt_lpips_head_workspace_floats(n, h * w) in [g.count for g in state['nan'][1].made]
        G.bitwise_case(monkeypatch, lambda t: C.lpips_head_backward(t['fp'], t['fg'], t['lin']), ins)
        ins['dup'] = _rand((n, h, w, c), 9)
        G.bitwise_case(monkeypatch, lambda t: C.lpips_head_backward(t['fp'], t['fg'], t['lin'], t['dup']), ins)


@pytest.mark.parametrize('shape', SHAPES)
def test_loss_chain_and_the_refusal_of_a_short_workspace(monkeypatch, shape):
    n, h, w = shape
    gt, pred = R.make_pair('far', n, h, w, seed=h)
    ins = dict(pred=t32(pred), gt=t32(gt), weights=t32(lpips_weights.blob(lpips_weights.validate(W))))
    for want_grad in (True, False):
        res, state, _ = G.bitwise_case(monkeypatch, lambda t: C.lpips_loss(t['pred'], t['gt'], t['weights'], want_grad), ins)
        assert C.lib().nlt_lpips_workspace_floats(n, h, w, 1 if want_grad else 0) in [g.count for g in state['nan'][1].made]
        assert res[0]['ret0'].shape == (n,) and (not want_grad or res[0]['ret1'].shape == (n, h, w, 3))
    real = C._size
    short = ('nlt_lpips_workspace_floats', 'nlt_lpips_head_workspace_floats')
    monkeypatch.setattr(C, '_size', lambda name, *a, **kw: real(name, *a, **kw) - (1 if name in short else 0))

    def refused(o):
        with pytest.raises(C.NLTError, match='bad argument'):
            C.lpips_loss(o['pred'].t, o['gt'].t, o['weights'].t, True)
    G.run_case(monkeypatch, refused, ins)
    (h1, w1), _, _ = _maps(shape)
    hins = dict(fp=_rand((n, h1, w1, 64), 7, relu=True), fg=_rand((n, h1, w1, 64), 8, relu=True), lin=t32(W['lin1']))

    def refused_head(o):
        with pytest.raises(C.NLTError, match='bad argument'):
            C.lpips_head_forward(o['fp'].t, o['fg'].t, o['lin'].t)
    G.run_case(monkeypatch, refused_head, hins)
