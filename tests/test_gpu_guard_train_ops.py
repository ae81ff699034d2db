"""-m gpu: memory discipline of the pointwise ops, warps, losses, norms and optimizer kernels of the render path and the train
step (csrc/pointwise.hip, train_ops.hip, warp.hip, deterministic.hip, barron.hip, ssim.hip, branches.hip, norms.hip) with
tests/guard_util.py.  Every tensor argument is a guarded view under the three fills; what an adapter allocates itself (its result,
the Barron and SSIM scratch) is guarded through `guard_util.guarded_allocs`, its cached scratch through `guarded_workspace`, both
at exactly the queried size and starting as the fill.

Per case: bands, pads and read-only operands intact.  Kernels without float atomics (and the `_det` / `_gather` forms under
`capi.deterministic_scope(True)`): the same bits under every fill, and bit for bit the adapter's result on plain dense tensors, at a
shape its own oracle test holds to the reference (tests/test_gpu_pointwise.py, test_gpu_train_ops.py, test_gpu_branches.py,
test_gpu_ssim.py); the exact ops (mul, sub, finish_pred) against torch.  The atomic forms (stem / head / warp / resize backward,
the L2 sums, Barron): finite under every fill and within the bar their own test states against float64.  Entry points with a
capacity argument refuse `need - 1` and touch nothing.

Out of scope: the data-preparation kernels (cosine_map, albedo, diffuse_base, remap_*, uv_index_map, knn_indices, psnr_sums,
resize_cv_linear, gather_frames_u8, assemble_batch), the tape and event plumbing, and whole-model runs."""
import math

import numpy as np
import pytest
import torch

from nlt_amd import capi as C
from oracle import barron as B
from oracle import nlt_oracle as O
from oracle import tf_ops as T
import guard_util as G
import ssim_ref as R
from test_gpu_pointwise import _warp_case

pytestmark = pytest.mark.gpu

PAD = 4
E = lambda *shape, **kw: dict(shape=shape, **kw)
t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _sl(data, pad=PAD):
    return dict(data=data, ld=data.shape[-1] + pad)


def _refused(monkeypatch, call, ins, outs):
    """One float less scratch than the query asks for: NLT_ERR_BAD_ARG, every operand and band as it was."""
    def refused(o):
        with pytest.raises(C.NLTError, match='bad argument'):
            call({k: (None if g is None else g.t) for k, g in o.items()})
    ops = dict(ins)
    ops.update(outs)
    G.run_case(monkeypatch, refused, ops, outputs=(), short=1)


# ---------------------------------------------------------------- stem, observation mean, head
@pytest.mark.parametrize('k,weights', [(3, False), (4, True)])
def test_stem_forward(monkeypatch, k, weights):
    rng = np.random.default_rng(k)
    n, h, w, c = 2, 5, 7, 16
    U = lambda *s: t32(rng.random(s, dtype=np.float32))
    N = lambda *s: t32(rng.standard_normal(s))
    ins = dict(base=U(n, h, w, 3), cvis=U(n, h, w, 1), lvis=U(n, h, w, 1), nn_rgb=U(n, k, h, w, 3), nn_base=U(n, k, h, w, 3),
               ow=U(n, k) if weights else None, wq=N(1, 1, 5, c), bq=N(c), wo=N(1, 1, 3, c), bo=N(c))
    G.bitwise_case(monkeypatch, lambda t: C.stem_forward(t['base'], t['cvis'], t['lvis'], t['nn_rgb'], t['nn_base'], t['ow'], n, k, h, w, c,
                                                         t['wq'], t['bq'], t['wo'], t['bo'], t['fm0'], t['obs0']),
                   ins, dict(fm0=E(n, h, w, 2 * c), obs0=E(n, k, h, w, c)))


def _stem_backward_case():
    rng = np.random.default_rng(3)
    n, k, h, w, c = 2, 3, 9, 7, 16
    U = lambda *s: rng.random(s, dtype=np.float32)
    base, cvis, lvis, nn_rgb, nn_base, ow = U(n, h, w, 3), U(n, h, w, 1), U(n, h, w, 1), U(n, k, h, w, 3), U(n, k, h, w, 3), U(n, k)
    dfm0 = rng.standard_normal((n, h, w, 2 * c)).astype(np.float32)
    dobs0 = rng.standard_normal((n, k, h, w, c)).astype(np.float32)
    x = np.concatenate((base, cvis, lvis), -1).reshape(-1, 5).astype(np.float64)
    gq = dfm0[..., :c].reshape(-1, c).astype(np.float64)
    g = np.broadcast_to(dfm0[:, None, ..., c:] / k, (n, k, h, w, c)).astype(np.float64) * ow[:, :, None, None, None] + dobs0
    dd = (nn_rgb - nn_base).reshape(-1, 3).astype(np.float64)
    ref = dict(dwq=x.T @ gq, dbq=gq.sum(0), dwo=dd.T @ g.reshape(-1, c), dbo=g.reshape(-1, c).sum(0))
    ins = dict(base=t32(base), cvis=t32(cvis), lvis=t32(lvis), nn_rgb=t32(nn_rgb), nn_base=t32(nn_base), ow=t32(ow), dfm0=t32(dfm0),
               dobs0=t32(dobs0))
    Z = lambda *s: dict(data=torch.zeros(s))
    outs = dict(dwq=Z(1, 1, 5, c), dbq=Z(c), dwo=Z(1, 1, 3, c), dbo=Z(c))
    call = lambda t: C.stem_backward(t['base'], t['cvis'], t['lvis'], t['nn_rgb'], t['nn_base'], t['ow'], n, k, h, w, c, t['dfm0'], t['dobs0'],
                                     t['dwq'], t['dbq'], t['dwo'], t['dbo'])
    return call, ins, outs, ref


def _det(call):
    def wrapped(t):
        with C.deterministic_scope(True):
            return call(t)
    return wrapped


@pytest.mark.parametrize('det', [False, True], ids=['atomic', 'det'])
def test_stem_backward(monkeypatch, det):
    """tests/test_gpu_train_ops.py's bar: 2e-4 absolute from the float64 sums."""
    call, ins, outs, ref = _stem_backward_case()
    res, state, _ = G.bitwise_case(monkeypatch, _det(call) if det else call, ins, outs, det=det)
    for r in res:
        for name, want in ref.items():
            np.testing.assert_allclose(r[name].numpy().reshape(want.shape), want, atol=2e-4)
    if det:
        (key, need, zero, ws), = state['nan'][0].requests
        assert need == C.lib().nlt_stem_backward_det_workspace_floats(2, 9, 7, 16)
        _refused(monkeypatch, _det(call), ins, outs)


@pytest.mark.parametrize('k,weights', [(1, False), (3, True)])
def test_obs_mean_forward_into_the_upper_half(monkeypatch, k, weights):
    rng = np.random.default_rng(10 + k)
    n, hw, c = 2, 33, 32
    obs = t32(rng.standard_normal((n, k, hw, c)))
    old = t32(rng.standard_normal((n, hw, 2 * c)))
    res, _, _ = G.bitwise_case(monkeypatch, lambda t: C.obs_mean_forward(t['obs'], t['ow'], n, k, hw, c, t['fm'].view(-1)[c:], 2 * c),
                               dict(obs=obs, ow=t32(rng.random((n, k), dtype=np.float32)) if weights else None), dict(fm=dict(data=old)))
    assert torch.equal(res[0]['fm'][..., :c], old[..., :c])


def test_lrelu_and_obs_mean_backward_and_level_split(monkeypatch):
    rng = np.random.default_rng(0)
    n, k, hw, c = 2, 3, 35, 16
    N = lambda *s: t32(rng.standard_normal(s))
    g, y = N(n * hw, 2 * c), N(n * hw, 2 * c)
    # in place on the first half of a 2c-wide map (the other half: pad columns), and out of place between three strides
    G.bitwise_case(monkeypatch, lambda t: C.lrelu_backward(t['g'], 2 * c, t['y'], 2 * c, c, n * hw, 0.3, t['g'], 2 * c),
                   dict(y=dict(data=y[:, :c].contiguous(), ld=2 * c)), dict(g=dict(data=g[:, :c].contiguous(), ld=2 * c)))
    G.bitwise_case(monkeypatch, lambda t: C.lrelu_backward(t['g'], c + 4, t['y'], c + 8, c, n * hw, 0.3, t['out'], c + 12),
                   dict(g=_sl(g[:, :c].contiguous(), 4), y=_sl(y[:, :c].contiguous(), 8)), dict(out=E(n * hw, c, ld=c + 12)))
    dmean, obs_y, part, ow = N(n, hw, c), N(n, k, hw, c), N(n, k, hw, c), t32(rng.random((n, k), dtype=np.float32))
    for use_w, use_p, use_y in ((True, True, True), (False, False, True), (False, True, False)):
        G.bitwise_case(monkeypatch, lambda t: C.obs_mean_backward(t['dmean'], 2 * c, t['obs_y'], t['ow'], t['pd'] if use_p else None, n, k, hw, c,
                                                                  0.3, t['pd']),
                       dict(dmean=dict(data=dmean, ld=2 * c), obs_y=obs_y if use_y else None, ow=ow if use_w else None),
                       dict(pd=dict(data=part) if use_p else E(n, k, hw, c)))
    # one launch for both: the query half of dfm in place, the observation half read (never written), dobs finished in place
    dfm, fm_y = N(n, hw, 2 * c), N(n, hw, 2 * c)
    res, _, _ = G.bitwise_case(monkeypatch, lambda t: C.level_split_backward(t['dfm'], t['fm_y'], 2 * c, t['obs_y'], t['ow'], t['pd'], n, k, hw, c,
                                                                             0.3, 0.2, t['pd']),
                               dict(fm_y=dict(data=fm_y[..., :c].contiguous(), ld=2 * c), obs_y=obs_y, ow=ow), dict(dfm=dict(data=dfm), pd=dict(data=part)))
    assert torch.equal(res[0]['dfm'][..., c:], dfm[..., c:])


def _head_case():
    rng = np.random.default_rng(1)
    n, h, w, cd, cs = 2, 7, 9, 4, 32
    N = lambda *s: rng.standard_normal(s).astype(np.float32)
    dec, skip, wk, dpred = N(n, h, w, cd), N(n, h, w, cs), N(1, 1, cd + cs, 3), N(n, h, w, 3)
    return n, h, w, cd, cs, dec, skip, wk, dpred


@pytest.mark.parametrize('with_base', [True, False])
def test_head_forward(monkeypatch, with_base):
    rng = np.random.default_rng(3)
    n, h, w, cd, cs = 2, 6, 5, 4, 32
    N = lambda *s: t32(rng.standard_normal(s))
    ins = dict(dec=_sl(N(n, h, w, cd)), skip=_sl(N(n, h, w, cs)), wk=N(1, 1, cd + cs, 3), b=N(3),
               base=t32(rng.random((n, h, w, 3), dtype=np.float32)) if with_base else None)
    res, _, _ = G.bitwise_case(monkeypatch, lambda t: C.head_forward(t['dec'], cd + PAD, cd, t['skip'], cs + PAD, cs, t['wk'], t['b'], t['base'],
                                                                     n, h, w, t['pred']), ins, dict(pred=E(n, h, w, 3)))
    assert not res[0]['pred'][:, 0, 0].any()


@pytest.mark.parametrize('det', [False, True], ids=['atomic', 'det'])
def test_head_backward(monkeypatch, det):
    """d_dec / d_skip into channel slices; dw / db accumulated.  Bars of tests/test_gpu_train_ops.py (1e-5 / 2e-4 absolute)."""
    n, h, w, cd, cs, dec, skip, wk, dpred = _head_case()
    ins = dict(dec=_sl(t32(dec)), skip=_sl(t32(skip)), wk=t32(wk), dpred=t32(dpred))
    outs = dict(d_dec=E(n, h, w, cd, ld=cd + PAD), d_skip=E(n, h, w, cs, ld=cs + PAD), dw=dict(data=torch.zeros(1, 1, cd + cs, 3)),
                db=dict(data=torch.zeros(3)))
    call = lambda t: C.head_backward(t['dec'], cd + PAD, cd, t['skip'], cs + PAD, cs, t['wk'], t['dpred'], n, h, w, t['d_dec'], cd + PAD,
                                     t['d_skip'], cs + PAD, t['dw'], t['db'])
    res, state, _ = G.bitwise_case(monkeypatch, _det(call) if det else call, ins, outs, det=det)
    g = dpred.copy(); g[:, 0, 0, :] = 0
    dx = g @ wk[0, 0].T
    x = np.concatenate((dec, skip), -1).reshape(-1, cd + cs).astype(np.float64)
    for r in res:
        np.testing.assert_allclose(r['d_dec'].numpy(), dx[..., :cd], atol=1e-5)
        np.testing.assert_allclose(r['d_skip'].numpy(), dx[..., cd:], atol=1e-5)
        np.testing.assert_allclose(r['dw'].numpy()[0, 0], x.T @ g.reshape(-1, 3), atol=2e-4)
        np.testing.assert_allclose(r['db'].numpy(), g.reshape(-1, 3).sum(0), atol=2e-4)
    if det:
        (key, need, zero, ws), = state['nan'][0].requests
        assert need == C.lib().nlt_head_backward_det_workspace_floats(n, h, w, cd, cs)
        _refused(monkeypatch, _det(call), ins, outs)


# ---------------------------------------------------------------- warps and resizes
def _warp_inputs():
    """tests/test_gpu_pointwise.py's map: samples on the last row and column, just outside the map on both sides, zeros."""
    n, uvh, uvw, hc, wc = 2, 32, 48, 16, 24
    pred, base, warp = _warp_case(n, uvh, uvw, hc, wc, 0)
    warp[1, hc - 1, wc - 1] = (np.float32(uvw - 1) / uvw, np.float32(uvh - 1) / uvh)       # the last pixel of the last frame -> the last texel
    warp[1, hc - 1, wc - 2] = (1.0, 1.0)
    return n, uvh, uvw, hc, wc, pred, base, warp


def test_warp_forward_and_from_the_stores(monkeypatch):
    n, uvh, uvw, hc, wc, pred, base, warp = _warp_inputs()
    outs = dict(pc=E(n, hc, wc, 3), bc=E(n, hc, wc, 3), fc=E(n, hc, wc, 3), idx=E(n, hc, wc, 4, dtype=torch.int32))
    G.bitwise_case(monkeypatch, lambda t: C.warp_forward(t['pred'], t['base'], t['warp'], n, uvh, uvw, hc, wc, t['pc'], t['bc'], t['fc'], t['idx']),
                   dict(pred=t32(pred), base=t32(base), warp=t32(warp)), outs)
    F = 3
    rng = np.random.default_rng(11)
    diffuse = torch.from_numpy(rng.integers(0, 256, (F, uvh, uvw, 3), dtype=np.uint8))
    maps = torch.from_numpy(rng.random((F, hc, wc, 2), dtype=np.float32)).half()
    ids = torch.tensor([F - 1, 0], dtype=torch.int32)
    maps[ids.long()] = torch.from_numpy(warp).half()
    G.bitwise_case(monkeypatch, lambda t: C.warp_forward_store(t['pred'], t['diffuse'], t['maps'], t['ids'], n, uvh, uvw, hc, wc, t['pc'], t['bc'],
                                                               t['fc'], t['idx']), dict(pred=t32(pred), diffuse=diffuse, maps=maps, ids=ids), outs)


@pytest.mark.parametrize('det', [False, True], ids=['atomic', 'det'])
def test_warp_backward(monkeypatch, det):
    """The scatter (float atomics) and the ordered form (scratch sized in bytes); 1e-5 absolute from autograd through the oracle's
    resampler (tests/test_gpu_train_ops.py)."""
    n, uvh, uvw, hc, wc, _, _, warp = _warp_inputs()
    warp = warp.astype(np.float16).astype(np.float32)
    dcam = t32(np.random.default_rng(2).standard_normal((n, hc, wc, 3)))
    data = torch.zeros(n, uvh, uvw, 3, requires_grad=True)
    out = T.resampler(T.set_left_top_corner(data, 0), torch.tensor(warp) * torch.tensor([uvw, uvh], dtype=torch.float32))
    (ref,) = torch.autograd.grad(out, data, dcam)
    call = lambda t: C.warp_backward(t['dcam'], t['warp'], n, uvh, uvw, hc, wc, t['dpred'])
    res, state, _ = G.bitwise_case(monkeypatch, _det(call) if det else call, dict(dcam=dcam, warp=t32(warp)), dict(dpred=E(n, uvh, uvw, 3)), det=det)
    for r in res:
        np.testing.assert_allclose(r['dpred'].numpy(), ref.numpy(), atol=1e-5)
    if det:
        (key, need, zero, ws), = state['nan'][0].requests
        assert need == (C.lib().nlt_warp_backward_det_workspace_bytes(n, uvh, uvw, hc, wc) + 3) // 4


def test_resample_forward(monkeypatch):
    n, h, w, hc, wc, c = 2, 24, 40, 16, 24, 4
    _, _, warp = _warp_case(n, h, w, hc, wc, 5)
    warp[1, hc - 1, wc - 1] = (np.float32(w - 1) / w, np.float32(h - 1) / h)
    warp[1, hc - 1, wc - 2] = (1.0, 1.0)
    data = t32(np.random.default_rng(c).random((n, h, w, c), dtype=np.float32))
    wpx = t32(warp * np.float32([w, h]))
    G.bitwise_case(monkeypatch, lambda t: C.resample_forward(t['data'], t['wpx']), dict(data=data, wpx=wpx))


@pytest.mark.parametrize('oh,ow', [(5, 7), (32, 24)])
def test_resize_bilinear_forward(monkeypatch, oh, ow):
    x = t32(np.random.default_rng(oh).random((2, 16, 16, 3), dtype=np.float32))
    G.bitwise_case(monkeypatch, lambda t: C.resize_bilinear_forward(t['x'], oh, ow), dict(x=x))


@pytest.mark.parametrize('gather', [False, True], ids=['atomic', 'gather'])
def test_resize_bilinear_backward(monkeypatch, gather):
    """1e-5 absolute from autograd through the oracle's resize (tests/test_gpu_train_ops.py), up and down."""
    for (h, w), (oh, ow) in (((12, 10), (20, 14)), ((17, 29), (5, 7))):
        dout = t32(np.random.default_rng(h).standard_normal((2, oh, ow, 3)))
        x = torch.zeros(2, h, w, 3, requires_grad=True)
        (ref,) = torch.autograd.grad(T.resize_bilinear(x, oh, ow), x, dout)
        call = lambda t: C.resize_bilinear_backward(t['dout'], h, w)
        res, _, _ = G.bitwise_case(monkeypatch, _det(call) if gather else call, dict(dout=dout), det=gather)
        for r in res:
            np.testing.assert_allclose(r['ret'].numpy(), ref.numpy(), atol=1e-5)


# ---------------------------------------------------------------- losses
def _l2_inputs():
    rng = np.random.default_rng(3)
    U = lambda *s: t32(rng.random(s, dtype=np.float32))
    return U(3, 17, 19, 3), U(3, 17, 19, 3), U(3), U(3, 17, 19), rng


@pytest.mark.parametrize('det', [False, True], ids=['atomic', 'det'])
def test_l2_losses(monkeypatch, det):
    """3 x 17 x 19 texels: no multiple of a workgroup's share.  Sums: rtol 2e-6 against the oracle's (tests/test_gpu_train_ops.py);
    the three `_det` sums share one scratch query and each refuses one float less."""
    pred, gt, gl, wt, rng = _l2_inputs()
    fg = t32((rng.random((3, 17, 19, 1)) > 0.3).astype(np.float32).repeat(3, -1))
    wrap = _det if det else (lambda f: f)
    fwd = wrap(lambda t: C.l2_loss_forward(t['pred'], t['gt']))
    res, _, _ = G.bitwise_case(monkeypatch, fwd, dict(pred=pred, gt=gt), det=det)
    ref = O.l2_loss(gt.double(), pred.double(), keep_batch=True).numpy()
    for r in res:
        np.testing.assert_allclose(r['ret'].numpy(), ref, rtol=2e-6)
    wfwd = wrap(lambda t: C.l2_loss_weighted_forward(t['pred'], t['gt'], t['wt']))
    res, _, _ = G.bitwise_case(monkeypatch, wfwd, dict(pred=pred, gt=gt, wt=wt), det=det)
    refw = O.l2_loss(gt.double(), pred.double(), keep_batch=True, weights=wt.double()).numpy()
    for r in res:
        np.testing.assert_allclose(r['ret'].numpy(), refw, rtol=2e-6)
    train = wrap(lambda t: C.l2_train_loss(t['pred'], t['rgb'], t['fg'], 8))
    res, _, _ = G.bitwise_case(monkeypatch, train, dict(pred=pred, rgb=gt, fg=fg), det=det)
    gtm = gt * fg
    for r in res:
        np.testing.assert_allclose(float(r['ret0']), float(O.l2_loss(gtm.double(), pred.double(), keep_batch=True).sum()) / 8, rtol=2e-6)
        assert torch.equal(r['ret1'], gtm)
        np.testing.assert_allclose(r['ret2'].numpy(), (2 * (pred - gtm) / (17 * 19 * 3) / 8).numpy(), atol=1e-7)
    if det:
        for call, ins in ((fwd, dict(pred=pred, gt=gt)), (wfwd, dict(pred=pred, gt=gt, wt=wt)), (train, dict(pred=pred, rgb=gt, fg=fg))):
            def refused(o, call=call):
                with pytest.raises(C.NLTError, match='bad argument'):
                    call({k: g.t for k, g in o.items()})
            G.run_case(monkeypatch, refused, ins, short=1)


def test_l2_backward_and_scale_rows(monkeypatch):
    pred, gt, gl, wt, _ = _l2_inputs()
    G.bitwise_case(monkeypatch, lambda t: C.l2_loss_backward(t['pred'], t['gt'], t['gl']), dict(pred=pred, gt=gt, gl=gl))
    G.bitwise_case(monkeypatch, lambda t: C.l2_loss_weighted_backward(t['pred'], t['gt'], t['wt'], t['gl']), dict(pred=pred, gt=gt, wt=wt, gl=gl))
    G.bitwise_case(monkeypatch, lambda t: C.scale_rows(t['x'], t['s']), dict(x=pred, s=gl))


@pytest.mark.parametrize('det', [False, True], ids=['atomic', 'det'])
def test_barron_loss(monkeypatch, det):
    """17 x 17: the adapter's own scratch (nlt_barron_workspace_floats) and the `_det` form's slots at exactly their queried sizes.
    rtol 2e-5 on the loss, 1e-4 rel-L2 on the gradient (tests/test_gpu_train_ops.py)."""
    rng = np.random.default_rng(17)
    pred = torch.tensor(rng.random((2, 17, 17, 3), dtype=np.float32), requires_grad=True)
    gt = torch.tensor(rng.random((2, 17, 17, 3), dtype=np.float32))
    ref = B.barron_loss(gt.double(), pred.double(), keep_batch=True)
    (gref,) = torch.autograd.grad(ref.sum(), pred)
    for want_grad in (True, False):
        call = lambda t: C.barron_loss(t['pred'], t['gt'], want_grad)
        res, state, _ = G.bitwise_case(monkeypatch, _det(call) if det else call, dict(pred=pred.detach(), gt=gt), det=det)
        sizes = [g.count for g in state['nan'][1].made]
        assert C.lib().nlt_barron_workspace_floats(2, 17, 17) in sizes
        for r in res:
            np.testing.assert_allclose(r['ret0'].numpy(), ref.detach().numpy(), rtol=2e-5)
            if want_grad:
                assert float((r['ret1'] - gref).norm() / gref.norm()) < 1e-4


@pytest.mark.parametrize('shape,c', [((1, 11, 11), 3), ((3, 37, 53), 3), ((3, 37, 53), 1)])
def test_ssim_loss_and_values(monkeypatch, shape, c):
    """11 x 11 (one window) and 37 x 53 (27 x 43 windows: one past a 16 x 32 tile in each axis); the scratch is the adapter's own
    allocation of nlt_ssim_workspace_floats floats, guarded and starting as the fill; one float less is refused."""
    n, h, w = shape
    x, y = R.make_pair('noise', n, h, w, c, seed=h * 100 + w)
    ins = dict(pred=torch.from_numpy(y), gt=torch.from_numpy(x))
    for want_grad in (True, False):
        res, state, _ = G.bitwise_case(monkeypatch, lambda t: C.ssim_loss(t['pred'], t['gt'], 1.0, want_grad), ins)
        assert C.lib().nlt_ssim_workspace_floats(n, h, w, c, 1 if want_grad else 0) in [g.count for g in state['nan'][1].made]
    G.bitwise_case(monkeypatch, lambda t: C.ssim_values(t['pred'], t['gt'], 1.0), ins)
    real = C._size
    monkeypatch.setattr(C, '_size', lambda name, *a, **kw: real(name, *a, **kw) - (1 if name == 'nlt_ssim_workspace_floats' else 0))
    for call in (lambda t: C.ssim_loss(t['pred'], t['gt'], 1.0, True), lambda t: C.ssim_values(t['pred'], t['gt'], 1.0)):
        def refused(o, call=call):
            with pytest.raises(C.NLTError, match='bad argument'):
                call({k: g.t for k, g in o.items()})
        G.run_case(monkeypatch, refused, ins)


# ---------------------------------------------------------------- pointwise, activations, norms, pools, optimizer
def test_mul_sub_finish_pred(monkeypatch):
    rng = np.random.default_rng(0)
    a, b = t32(rng.random(1003, dtype=np.float32)), t32(rng.random(1003, dtype=np.float32))
    res, _, _ = G.bitwise_case(monkeypatch, lambda t: C.mul_forward(t['a'], t['b']), dict(a=a, b=b))
    assert torch.equal(res[0]['ret'], a * b)
    res, _, _ = G.bitwise_case(monkeypatch, lambda t: C.sub_forward(t['a'], t['b']), dict(a=a, b=b))
    assert torch.equal(res[0]['ret'], a - b)
    y, base = t32(rng.standard_normal((3, 17, 19, 3))), t32(rng.random((3, 17, 19, 3), dtype=np.float32))
    for with_base in (True, False):
        res, _, _ = G.bitwise_case(monkeypatch, lambda t: C.finish_pred(t['y'], t['base'], t['pred']), dict(y=y, base=base if with_base else None),
                                   dict(pred=E(3, 17, 19, 3)))
        want = (y + base) if with_base else y.clone()
        want[:, 0, 0, :] = 0
        assert torch.equal(res[0]['pred'], want)


@pytest.mark.parametrize('kind,alpha', [(C.ACT_LRELU, 0.3), (C.ACT_LRELU, 0.0), (C.ACT_ELU, 1.0)])
def test_activations(monkeypatch, kind, alpha):
    gen = torch.Generator().manual_seed(kind + 1)
    x, g = torch.randn(3, 9, 7, 10, generator=gen), torch.randn(3, 9, 7, 10, generator=gen)
    res, _, _ = G.bitwise_case(monkeypatch, lambda t: C.act_forward(t['x'], kind, alpha), dict(x=x))
    G.bitwise_case(monkeypatch, lambda t: C.act_backward(t['g'], t['y'], kind, alpha), dict(g=g, y=res[0]['ret']))


@pytest.mark.parametrize('c', [3, 16, 40])
def test_pixelnorm(monkeypatch, c):
    gen = torch.Generator().manual_seed(c)
    x, g = torch.randn(2, 6, 5, c, generator=gen), torch.randn(2, 6, 5, c, generator=gen)
    G.bitwise_case(monkeypatch, lambda t: C.pixelnorm_forward(t['x']), dict(x=x))
    G.bitwise_case(monkeypatch, lambda t: C.pixelnorm_backward(t['g'], t['x']), dict(g=g, x=x))


@pytest.mark.parametrize('kind', [C.NORM_LAYER, C.NORM_BATCH], ids=['layer', 'batch'])
@pytest.mark.parametrize('shape', [(2, 6, 5, 3), (3, 4, 4, 40), (1, 2, 3, 1024)])
def test_norms(monkeypatch, kind, shape):
    """c = 3, 40 and 1024 (the widest the kernel takes); dgamma / dbeta accumulated through scratch of nlt_norm_workspace_floats
    floats -- an entry without a capacity argument: the guarded scratch is exactly that long."""
    gen = torch.Generator().manual_seed(sum(shape) + kind)
    c = shape[-1]
    x, g = torch.randn(shape, generator=gen) * 2 + 0.5, torch.randn(shape, generator=gen)
    gamma, beta = torch.rand(c, generator=gen) + 0.5, torch.rand(c, generator=gen) - 0.5
    mean, var = torch.randn(c, generator=gen) * 0.1, torch.rand(c, generator=gen) + 0.5
    G.bitwise_case(monkeypatch, lambda t: C.norm_forward(kind, t['x'], t['gamma'], t['beta'], t['mean'], t['var'], O.NORM_EPS),
                   dict(x=x, gamma=gamma, beta=beta, mean=mean, var=var))
    res, state, _ = G.bitwise_case(monkeypatch, lambda t: C.norm_backward(kind, t['g'], t['x'], t['gamma'], t['mean'], t['var'], O.NORM_EPS,
                                                                          t['dgamma'], t['dbeta']),
                                   dict(g=g, x=x, gamma=gamma, mean=mean, var=var),
                                   dict(dgamma=dict(data=torch.full((c,), 2.0)), dbeta=dict(data=torch.full((c,), -1.0))))
    (key, need, zero, ws), = state['nan'][0].requests
    assert need == C.lib().nlt_norm_workspace_floats(math.prod(shape[:-1]), c)


@pytest.mark.parametrize('kind', [C.POOL_MAX, C.POOL_AVG], ids=['max', 'avg'])
def test_pools(monkeypatch, kind):
    gen = torch.Generator().manual_seed(kind + 5)
    x, g = torch.randn(2, 8, 12, 5, generator=gen), torch.randn(2, 4, 6, 5, generator=gen)
    G.bitwise_case(monkeypatch, lambda t: C.pool2x2_forward(t['x'], kind), dict(x=x))
    G.bitwise_case(monkeypatch, lambda t: C.pool2x2_backward(t['g'], t['x'], kind), dict(g=g, x=x))


def test_clip_by_norm_slots(monkeypatch):
    """In place on a flat bucket; the int64 slot table is a guarded store.  The padding between slots is not written; values at the
    bar of tests/test_gpu_train_ops.py (2e-6 of the largest entry) against the oracle's clip_by_norm."""
    gen = torch.Generator().manual_seed(5)
    sizes = [16, 5 * 16, 2 * 2 * 32 * 16, 3, 4099, 64, 8]
    offs, off = [], 0
    for n in sizes:
        offs.append((off, n)); off += (n + 3) // 4 * 4
    flat = torch.randn(off, generator=gen) * 1e-3
    flat[offs[5][0]:offs[5][0] + 64] = 0
    flat[offs[2][0]:offs[2][0] + sizes[2]] *= 50
    clip = 0.02
    ref = flat.clone()
    for o, n in offs:
        ref[o:o + n] = O.clip_by_norm(ref[o:o + n].clone(), clip)
    res, _ = G.run_case(monkeypatch, lambda o: C.clip_by_norm_slots(o['grad'].t, o['slots'].t, clip),
                        dict(grad=flat, slots=torch.tensor(offs, dtype=torch.int64)), outputs=('grad',))
    got = res[0]['grad']
    assert float((got - ref).abs().max()) <= 2e-6 * float(ref.abs().max())
    pad = torch.ones(off, dtype=torch.bool)
    for o, n in offs:
        pad[o:o + n] = False
    assert torch.equal(got[pad], flat[pad])


def test_adam_amsgrad_step(monkeypatch):
    """One step on 1001 parameters (no multiple of four), all five buffers guarded; 2e-6 absolute from the Keras form
    (tests/test_gpu_train_ops.py)."""
    rng = np.random.default_rng(4)
    p0, g = rng.standard_normal(1001).astype(np.float32), rng.standard_normal(1001).astype(np.float32)
    p = torch.tensor(p0.copy(), requires_grad=True)
    O.KerasAdamAMSGrad([p], 1e-2).step([torch.tensor(g)])
    lr_t = 1e-2 * math.sqrt(1 - 0.999) / (1 - 0.9)
    Z = lambda: dict(data=torch.zeros(1001))
    res, _ = G.run_case(monkeypatch, lambda o: C.adam_amsgrad_step(o['p'].t, o['g'].t, o['m'].t, o['v'].t, o['vh'].t, lr_t, 0.9, 0.999, 1e-7),
                        dict(p=t32(p0), g=t32(g), m=Z(), v=Z(), vh=Z()), outputs=('p', 'm', 'v', 'vh'))
    np.testing.assert_allclose(res[0]['p'].numpy(), p.detach().numpy(), atol=2e-6)


# ---------------------------------------------------------------- the helper itself, on the device
def test_the_helper_detects_on_the_device():
    """The wrong "kernels" of tests/test_host_guard_util.py as torch ops on device buffers: the checks above are live on 'cuda'."""
    import test_host_guard_util as H
    for kernel, ld, pattern in ((H._past_end, None, r"^out: guard band after the payload was overwritten: first at element offset 0, 1 element"),
                                (H._before, None, r"^out: guard band before the payload was overwritten: first at element offset -1, 1 element"),
                                (H._pad, 7, r"^out: pad columns was overwritten: first at \(texel, pad column\) \(2, 0\), 1 element"),
                                (H._modifies_input, 7, r"^x: read-only payload was modified: first at \(texel, column\) \(3, 1\), 1 element")):
        with pytest.raises(AssertionError, match=pattern):
            G.run_guarded(kernel, H._ops(ld=ld), outputs=('out',), device='cuda')
    G.assert_same_across_fills(G.run_guarded(H._good, H._ops(ld=7), outputs=('out',), device='cuda'))
