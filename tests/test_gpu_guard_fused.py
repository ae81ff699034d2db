"""-m gpu: memory discipline of the fused ends (csrc/fused.hip, front4.hip, front_ovr.hip, dec_block.hip, train_fused.hip,
train_back.hip) with tests/guard_util.py: every tensor argument -- float buffers, the uint8 capture stores and their int32 frame
ids, weight blobs, outputs, the backward launches' scratch -- is a guarded view under the three fills; the documented channel
slices (the query half of an interleaved level map: ldq / lds) have the other half as pad columns.

Per case: bands, pads and read-only operands intact; outputs bit-identical across the fills; values bit for bit what the same
adapter gives on plain dense tensors, at shapes its own oracle test holds to the reference ((1, 8, 8, k = 1), (2, 24, 40, k = 3),
h2 x w2 = 3 x 5: rows of tests/test_gpu_fused.py, test_gpu_front4.py, test_gpu_infer.py, test_gpu_dec_block.py,
test_gpu_train_fused.py); the two backward launches' scratch at exactly the queried size, nothing read before written.

Out of scope: the data-preparation kernels (cosine_map, albedo, diffuse_base, remap_*, uv_index_map, knn_indices, psnr_sums,
resize_cv_linear, gather_frames_u8, assemble_batch), the tape and event plumbing, and whole-model runs."""
import numpy as np
import pytest
import torch

from nlt_amd import capi as C
import guard_util as G

pytestmark = pytest.mark.gpu

ALPHA = 0.3
ORDER = ('wq0', 'bq0', 'wo0', 'bo0', 'wqa', 'bqa', 'wqb', 'bqb', 'woa', 'boa', 'wob', 'bob', 'wh', 'bh')
FRONT = [(1, 8, 8, 1), (2, 24, 40, 3)]              # (n, h, w, k)
BACK = [(1, 3, 5), (2, 12, 20)]                     # (n, h2, w2)


def _weights(rng):
    g = lambda *s: torch.from_numpy((rng.random(s, dtype=np.float32) - 0.5) * 0.8)
    P = dict(wq0=g(1, 1, 5, 16), bq0=g(16), wo0=g(1, 1, 3, 16), bo0=g(16), wqa=g(2, 2, 32, 16), bqa=g(16), wqb=g(2, 2, 16, 16),
             bqb=g(16), woa=g(2, 2, 16, 16), boa=g(16), wob=g(2, 2, 16, 16), bob=g(16), wh=g(1, 1, 36, 3), bh=g(3))
    L2 = dict(wq=g(2, 2, 32, 32), bq=g(32), wo=g(2, 2, 16, 32), bo=g(32))
    dev = lambda a: a.cuda().contiguous()
    blob = C.front_pack_weights(*[dev(P[k]) for k in ORDER])
    blob2 = C.front_pack_l2_weights(dev(L2['wq']), dev(L2['bq']), dev(L2['wo']), dev(L2['bo']))
    torch.cuda.synchronize()
    return P, blob, blob2


def _inputs(rng, n, h, w, k):
    U = lambda *s: torch.from_numpy(rng.random(s, dtype=np.float32))
    return dict(base=U(n, h, w, 3), cvis=U(n, h, w, 1), lvis=U(n, h, w, 1), nn_rgb=U(n, k, h, w, 3), nn_base=U(n, k, h, w, 3))


def _case(monkeypatch, call, ins, outs):
    res, state, _ = G.bitwise_case(monkeypatch, call, ins, outs)
    return res, state


E = lambda *shape, **kw: dict(shape=shape, **kw)


# ---------------------------------------------------------------- the front launches
@pytest.mark.parametrize('n,h,w,k', FRONT)
@pytest.mark.parametrize('add_base', [True, False])
def test_front_forward_and_front2(monkeypatch, n, h, w, k, add_base):
    rng = np.random.default_rng(h + k)
    P, blob, blob2 = _weights(rng)
    ins = dict(_inputs(rng, n, h, w, k), packed=blob, packed_l2=blob2)
    h2, w2 = h // 2, w // 2
    _case(monkeypatch, lambda t: C.front_forward(t['base'], t['cvis'], t['lvis'], t['nn_rgb'], t['nn_base'], n, k, h, w, t['packed'], add_base,
                                                 ALPHA, t['fm1'], t['obs1'], t['skip3']),
          {k_: v for k_, v in ins.items() if k_ != 'packed_l2'}, dict(fm1=E(n, h2, w2, 32), obs1=E(n, k, h2, w2, 16), skip3=E(n, h, w, 3)))
    _case(monkeypatch, lambda t: C.front2_forward(t['base'], t['cvis'], t['lvis'], t['nn_rgb'], t['nn_base'], n, k, h, w, t['packed'],
                                                  t['packed_l2'], add_base, ALPHA, t['fm1'], t['skip3'], t['qtmp2'], t['otmp2']),
          ins, dict(fm1=E(n, h2, w2, 32), skip3=E(n, h, w, 3), qtmp2=E(n, h // 4, w // 4, 32), otmp2=E(n, k, h // 4, w // 4, 32)))


@pytest.mark.parametrize('n,h,w,k', FRONT)
def test_front_forward_train(monkeypatch, n, h, w, k):
    rng = np.random.default_rng(h + k + 1)
    P, blob, _ = _weights(rng)
    h2, w2 = h // 2, w // 2
    _case(monkeypatch, lambda t: C.front_forward_train(t['base'], t['cvis'], t['lvis'], t['nn_rgb'], t['nn_base'], n, k, h, w, t['packed'], True,
                                                       ALPHA, t['fm1'], t['obs1'], t['skip3'], t['qtmp1'], t['otmp1']),
          dict(_inputs(rng, n, h, w, k), packed=blob),
          dict(fm1=E(n, h2, w2, 32), obs1=E(n, k, h2, w2, 16), skip3=E(n, h, w, 3), qtmp1=E(n, h2, w2, 16), otmp1=E(n, k, h2, w2, 16)))


@pytest.mark.parametrize('n,h,w,k', FRONT)
def test_front4_forward_and_train(monkeypatch, n, h, w, k):
    rng = np.random.default_rng(h + k + 2)
    P, blob, blob2 = _weights(rng)
    ins = dict(_inputs(rng, n, h, w, k), packed=blob, packed_l2=blob2)
    h2, w2 = h // 2, w // 2
    outs = dict(fm1=E(n, h2, w2, 32), skip3=E(n, h, w, 3), qtmp2=E(n, h // 4, w // 4, 32), otmp2=E(n, k, h // 4, w // 4, 32))
    args = lambda t: (t['base'], t['cvis'], t['lvis'], t['nn_rgb'], t['nn_base'], n, k, h, w, t['packed'], t['packed_l2'], True, ALPHA, t['fm1'],
                      t['skip3'], t['qtmp2'], t['otmp2'])
    _case(monkeypatch, lambda t: C.front4_forward(*args(t)), ins, outs)
    _case(monkeypatch, lambda t: C.front4_forward_train(*args(t), t['obs1'], t['qtmp1'], t['otmp1']), ins,
          dict(outs, obs1=E(n, k, h2, w2, 16), qtmp1=E(n, h2, w2, 16), otmp1=E(n, k, h2, w2, 16)))


def _stores(rng, F, h, w):
    R = lambda *s: torch.from_numpy(rng.integers(0, 256, s, dtype=np.uint8))
    return dict(diffuse=R(F, h, w, 3), rgb=R(F, h, w, 3), cvis=R(F, h, w), lvis=R(F, h, w))


@pytest.mark.parametrize('n,h,w,k', FRONT)
def test_front4_forward_u8(monkeypatch, n, h, w, k):
    """The uint8 capture stores and the int32 frame ids (one neighbour missing: -1) are guarded stores too; the first and the last
    frame of the store are among the ids."""
    rng = np.random.default_rng(h + k + 3)
    P, blob, blob2 = _weights(rng)
    F = 4
    ids = torch.tensor([F - 1, 0][:n], dtype=torch.int32)
    nn_ids = torch.from_numpy(rng.integers(0, F, (n, k)).astype(np.int32))
    nn_ids[0, 0] = F - 1
    nn_ids[n - 1, k - 1] = -1 if k > 1 else 0
    ins = dict(_stores(rng, F, h, w), ids=ids, nn_ids=nn_ids, packed=blob, packed_l2=blob2)
    _case(monkeypatch, lambda t: C.front4_forward_u8(t['diffuse'], t['rgb'], t['cvis'], t['lvis'], t['ids'], t['nn_ids'], n, k, h, w, t['packed'],
                                                     t['packed_l2'], True, ALPHA, t['fm1'], t['skip3'], t['qtmp2'], t['otmp2']),
          ins, dict(fm1=E(n, h // 2, w // 2, 32), skip3=E(n, h, w, 3), qtmp2=E(n, h // 4, w // 4, 32), otmp2=E(n, k, h // 4, w // 4, 32)))


@pytest.mark.parametrize('n,h,w', [(1, 8, 8), (2, 24, 40)])
@pytest.mark.parametrize('u8', [False, True])
def test_front_ovr_forward(monkeypatch, n, h, w, u8):
    """The query-only front of the inference mode: q1 is the query half (16 channels) of the interleaved level-1 map, ldq = 32 --
    the given half is pad columns here, which the launch must neither read nor write."""
    rng = np.random.default_rng(h + 4)
    P, blob, blob2 = _weights(rng)
    S = lambda *s: torch.from_numpy(rng.random(s, dtype=np.float32) - 0.5)
    maps = dict(p1=S(1, h // 2, w // 2, 16), s0=S(1, h, w, 4), p2=S(1, h // 4, w // 4, 32), packed=blob, packed_l2=blob2)
    outs = dict(q1=E(n, h // 2, w // 2, 16, ld=32), skip3=E(n, h, w, 3), qtmp2=E(n, h // 4, w // 4, 32))
    tail = lambda t: (n, h, w, t['packed'], t['packed_l2'], t['p1'], t['s0'], t['p2'], True, ALPHA, t['q1'], 32, t['skip3'], t['qtmp2'])
    if u8:
        F = 3
        st = _stores(rng, F, h, w)
        del st['rgb']
        ids = torch.tensor([F - 1, 0][:n], dtype=torch.int32)
        _case(monkeypatch, lambda t: C.front_ovr_forward_u8(t['diffuse'], t['cvis'], t['lvis'], t['ids'], *tail(t)), dict(st, ids=ids, **maps), outs)
    else:
        x = _inputs(rng, n, h, w, 1)
        _case(monkeypatch, lambda t: C.front_ovr_forward(t['base'], t['cvis'], t['lvis'], *tail(t)),
              dict(base=x['base'], cvis=x['cvis'], lvis=x['lvis'], **maps), outs)


# ---------------------------------------------------------------- expanding blocks and the back launches
@pytest.mark.parametrize('c,cx,cs', [(8, 16, 64), (16, 32, 128)])
def test_dec_block_forward_and_map(monkeypatch, c, cx, cs):
    n, h, w = 2, 3, 5
    rng = np.random.default_rng(c)
    S = lambda *s, sc=0.5: torch.from_numpy(((rng.random(s, dtype=np.float32) - 0.5) * 2 * sc).astype(np.float32))
    x, skip = S(n, h, w, cx), S(n, h, w, cs)
    w2, b2, w1, b1 = S(2, 2, c, cx + cs, sc=0.2), S(c, sc=0.1), S(2, 2, c, c, sc=0.3), S(c, sc=0.1)
    _case(monkeypatch, lambda t: C.dec_block_forward(t['x'], cx, t['skip'], cs, n, h, w, t['w_s2'], t['b_s2'], t['w_s1'], t['b_s1'], c, ALPHA,
                                                     t['out']),
          dict(x=x, skip=skip, w_s2=w2, b_s2=b2, w_s1=w1, b_s1=b1), dict(out=E(n, 2 * h, 2 * w, c)))
    # the inference mode's form: [x 2c | query half 4c of the interleaved map, lds = 8c] + a bias map shared by the frames
    _case(monkeypatch, lambda t: C.dec_block_forward_map(t['x'], t['skip'], 8 * c, n, h, w, t['w_s2q'], t['w_s1'], t['b_s1'], c, ALPHA, t['bmap'],
                                                         t['out']),
          dict(x=x, skip=dict(data=skip[..., :4 * c].contiguous(), ld=8 * c), w_s2q=w2[..., :6 * c].contiguous(), w_s1=w1, b_s1=b1,
               bmap=S(1, 2 * h, 2 * w, c)), dict(out=E(n, 2 * h, 2 * w, c)))


def _back_operands(rng, n, h2, w2):
    S = lambda *s: torch.from_numpy(rng.random(s, dtype=np.float32) - 0.5)
    return dict(x=S(n, h2, w2, 8), fm1=S(n, h2, w2, 32), skip3=S(n, 2 * h2, 2 * w2, 3), w_s2=S(2, 2, 4, 40), b_s2=S(4), w_s1=S(2, 2, 4, 4),
                b_s1=S(4), w_head=S(1, 1, 36, 3))


@pytest.mark.parametrize('n,h2,w2', BACK)
def test_back_forward_train_and_map(monkeypatch, n, h2, w2):
    rng = np.random.default_rng(h2)
    B = _back_operands(rng, n, h2, w2)
    H, W = 2 * h2, 2 * w2
    head = lambda t: (t['x'], t['fm1'], t['skip3'], n, h2, w2, t['w_s2'], t['b_s2'], t['w_s1'], t['b_s1'], t['w_head'], ALPHA, t['pred'])
    _case(monkeypatch, lambda t: C.back_forward(*head(t)), B, dict(pred=E(n, H, W, 3)))
    _case(monkeypatch, lambda t: C.back_forward_train(*head(t), t['u'], t['v']), B, dict(pred=E(n, H, W, 3), u=E(n, H, W, 4), v=E(n, H, W, 4)))
    S = lambda *s: torch.from_numpy(rng.random(s, dtype=np.float32) - 0.5)
    M = dict(x=B['x'], q1=dict(data=B['fm1'][..., :16].contiguous(), ld=32), skip3=B['skip3'], w_s2q=B['w_s2'][..., :24].contiguous(),
             w_s1=B['w_s1'], b_s1=B['b_s1'], w_head=B['w_head'], bmap=S(1, H, W, 4))
    _case(monkeypatch, lambda t: C.back_forward_map(t['x'], t['q1'], 32, t['skip3'], n, h2, w2, t['w_s2q'], t['w_s1'], t['b_s1'], t['w_head'], ALPHA,
                                                    t['bmap'], t['pred']), M, dict(pred=E(n, H, W, 3)))


# ---------------------------------------------------------------- the two fused backward launches (scratch without a capacity argument)
@pytest.mark.parametrize('n,h,w,k', FRONT)
def test_front_backward(monkeypatch, n, h, w, k):
    """nlt_front_backward accumulates nine gradients through scratch of nlt_front_backward_workspace_floats(n, h, w) floats: the
    guarded scratch is exactly that long and starts as the fill."""
    rng = np.random.default_rng(h * 5 + k)
    P, _, _ = _weights(rng)
    S = lambda *s: torch.from_numpy(rng.random(s, dtype=np.float32) - 0.5)
    names = ('wq0', 'bq0', 'wo0', 'bo0', 'wqa', 'woa', 'wh')
    gnames = ('wq0', 'bq0', 'wo0', 'bo0', 'wqa', 'bqa', 'woa', 'boa', 'wh')
    ins = dict(_inputs(rng, n, h, w, k), dy1q=S(n, h // 2, w // 2, 16), dy1o=S(n, k, h // 2, w // 2, 16), dpred=S(n, h, w, 3))
    ins.update({'w.' + k_: P[k_] for k_ in names})
    outs = {'g.' + k_: dict(data=torch.from_numpy(rng.random(tuple(P[k_].shape), dtype=np.float32))) for k_ in gnames}
    res, state = _case(monkeypatch, lambda t: C.front_backward(t['base'], t['cvis'], t['lvis'], t['nn_rgb'], t['nn_base'], n, k, h, w, t['dy1q'],
                                                               t['dy1o'], t['dpred'], tuple(t['w.' + k_] for k_ in names),
                                                               tuple(t['g.' + k_] for k_ in gnames)), ins, outs)
    (key, need, zero, ws), = state['nan'][0].requests
    assert need == C.lib().nlt_front_backward_workspace_floats(n, h, w) and not zero


@pytest.mark.parametrize('n,h2,w2', BACK)
def test_back_backward(monkeypatch, n, h2, w2):
    rng = np.random.default_rng(h2 * 11)
    B = _back_operands(rng, n, h2, w2)
    H, W = 2 * h2, 2 * w2
    d = lambda a: a.cuda().contiguous()
    pred, u, v = (torch.empty((n, H, W, c), device='cuda') for c in (3, 4, 4))
    C.back_forward_train(d(B['x']), d(B['fm1']), d(B['skip3']), n, h2, w2, d(B['w_s2']), d(B['b_s2']), d(B['w_s1']), d(B['b_s1']), d(B['w_head']),
                         ALPHA, pred, u, v)
    torch.cuda.synchronize()
    S = lambda *s: torch.from_numpy(rng.random(s, dtype=np.float32) - 0.5)
    ins = dict(x=B['x'], fm1=B['fm1'], u=u.cpu(), v=v.cpu(), dpred=S(n, H, W, 3), w_s2=B['w_s2'], w_s1=B['w_s1'], w_head=B['w_head'])
    acc = lambda *s: dict(data=torch.from_numpy(rng.random(s, dtype=np.float32)))
    outs = dict(dx=E(n, h2, w2, 8), dfm1=E(n, h2, w2, 32), dw_s2=acc(2, 2, 4, 40), db_s2=acc(4), dw_s1=acc(2, 2, 4, 4), db_s1=acc(4),
                dw_head=acc(1, 1, 36, 3), db_head=acc(3))
    res, state = _case(monkeypatch, lambda t: C.back_backward(t['x'], t['fm1'], t['u'], t['v'], t['dpred'], n, h2, w2, t['w_s2'], t['w_s1'],
                                                              t['w_head'], ALPHA, t['dx'], t['dfm1'], t['dw_s2'], t['db_s2'], t['dw_s1'],
                                                              t['db_s1'], t['dw_head'], t['db_head']), ins, outs)
    (key, need, zero, ws), = state['nan'][0].requests
    assert need == C.lib().nlt_back_backward_workspace_floats(n, h2, w2) and not zero
