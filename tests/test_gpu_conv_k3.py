"""-m gpu: kernel = 3 on csrc/conv_k3.hip.  Each 3x3 layer form (Conv2D / Conv2DTranspose, stride 1 / 2) through the layer
object and the layer-by-layer path's backward closure -- forward, dx, dkernel, dbias -- against float64 from
tests/conv_k3_ref.py, at the bound tests/test_gpu_conv.py holds k2 to (max abs error <= 2e-5 x the reference's max abs);
first at narrow channel counts, then at the default depth-256 config's widths (up to 1024 -> 128) with the channel counts and grids
that reach every instantiation and ragged block of the kernels (WIDE_CASES) and on every 3x3 layer a depth-256 model holds;
then whole kernel = 3 models against oracle.OracleModel, whose transposed conv is replaced by conv_k3_ref's (the oracle's
own crops the wrong ring at k3 s1: tests/test_conv_k3_ref.py)."""
import functools

import numpy as np
import pytest
import torch

import nlt_amd
from nlt_amd import capi as C
from nlt_amd import generic, trainvali
from nlt_amd.models import get_model_class
from nlt_amd.networks.elements import Act, Conv2D
from oracle import nlt_oracle as O
from oracle import tf_ops as T
import conv_k3_ref as R
from gpu_util import rel_l2, to_device_batch, _dump, _set_alpha, _oracle_grads
from test_gpu_train_step import flat_oracle_grads, per_tensor_worst, FLAT_TOL, TENSOR_TOL

pytestmark = pytest.mark.gpu

FORMS = [(1, False), (2, False), (1, True), (2, True)]
SHAPES = [(6, 10), (2, 2), (34, 18), (5, 7)]
CHANNELS = [(16, 16), (32, 16), (80, 8), (128, 16), (8, 4), (3, 16), (5, 3), (6, 10)]
CASES = [(s, tr, hw, ch) for (s, tr) in FORMS for hw in SHAPES for ch in CHANNELS if not (s == 2 and hw == (5, 7))]
ALPHA = 0.3


def _make_reference(stride, transpose, hw, ch, n=2):
    """Inputs (fp32) and the float64 pre-activation output with the gradients of <y, g>; shared by the act on / off cases."""
    (h, w), (cin, cout) = hw, ch
    gen = torch.Generator().manual_seed(1000 * stride + 100 * transpose + 7 * h + cin)
    x = torch.randn(n, h, w, cin, generator=gen)
    wk = torch.randn((3, 3, cout, cin) if transpose else (3, 3, cin, cout), generator=gen) * 0.2
    b = torch.randn(cout, generator=gen)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, wk, b))
    y = R.layer_f64(xd, wd, bd, stride, transpose)
    g = torch.randn(y.shape, generator=gen)
    return x, wk, b, g, y.detach(), xd, wd, bd, y


_reference = functools.lru_cache(maxsize=None)(_make_reference)
_recent_reference = functools.lru_cache(maxsize=8)(_make_reference)    # the wide-layer matrix: 1024-channel kernels are not kept for the session


def _close(got, ref, what):
    err, scale = float((got.double().cpu() - ref).abs().max()), float(ref.abs().max())
    print('%s: max abs error %.3e, reference max abs %.3e (bound %.3e)' % (what, err, scale, 2e-5 * scale))
    assert err <= 2e-5 * scale, (what, err, scale)


def _run_layer(ref, stride, transpose, act):
    """The layer object + generic.conv's backward closure on the device, twice into pre-filled dkernel / dbias (bit-identical
    runs asserted).  Returns {name: (device result, float64 reference)} and the float64 gradient w.r.t. the pre-activation."""
    x, wk, b, g, ypre, xd, wd, bd, ygraph = ref
    cout = b.numel()
    layer = Conv2D(cout, 3, stride, transpose)
    layer.set_weights(wk, b)
    a = Act(ALPHA) if act else None
    tape = generic.Tape(True)
    xin = tape.add(x.cuda(), (tape.leaf(x.cuda()),), lambda gr: (None,))         # not a network input: dx is wanted
    outs = []
    for _ in range(2):                                                            # twice into pre-filled destinations
        layer.dkernel = torch.full(tuple(wk.shape), 0.5, device='cuda')
        layer.dbias = torch.full((cout,), -2.0, device='cuda')
        node = generic.conv(tape, layer, xin, act=a)
        (dx,) = node.back(g.cuda())
        torch.cuda.synchronize()
        outs.append((node.value.cpu(), dx.cpu(), layer.dkernel.cpu(), layer.dbias.cpu()))
    assert all(torch.equal(p, q) for p, q in zip(*outs)), "two runs are bit-identical"
    y, dx, dk, db = outs[0]
    yref = T.leaky_relu(ypre, ALPHA) if act else ypre
    assert tuple(y.shape) == tuple(yref.shape)
    gpre = g.double() * torch.where(y.double() > 0, 1.0, ALPHA) if act else g.double()   # the mask the device path takes from its own y
    rdx, rdw, rdb = torch.autograd.grad(ygraph, (xd, wd, bd), gpre, retain_graph=True)
    return {'forward': (y, yref), 'dx': (dx, rdx), 'dkernel (accumulated on 0.5)': (dk - 0.5, rdw),
            'dbias (accumulated on -2)': (db + 2.0, rdb)}, gpre


def _check_layer(ref, stride, transpose, act):
    res, _ = _run_layer(ref, stride, transpose, act)
    for what, (got, want) in res.items():
        _close(got, want, what)
    return res


@pytest.mark.parametrize('act', [False, True], ids=['linear', 'lrelu'])
@pytest.mark.parametrize('stride,transpose,hw,ch', CASES,
                         ids=['%s_s%d_%dx%d_%dto%d' % ('deconv' if tr else 'conv', s, hw[0], hw[1], ch[0], ch[1]) for s, tr, hw, ch in CASES])
def test_layer_forward_and_backward(stride, transpose, hw, ch, act):
    _check_layer(_reference(stride, transpose, hw, ch), stride, transpose, act)


@pytest.mark.parametrize('stride,transpose', FORMS)
def test_direct_kernel_on_mfma_shapes_and_bad_arguments(stride, transpose):
    """The any-channel kernel on a shape the fast path would take; the stride-2 CONV on an odd size is an error status, the
    stride-2 TRANSPOSED conv takes it (5 x 7 -> 10 x 14) and is held to float64."""
    x, wk, b, g, ypre, *_ = _reference(stride, transpose, (6, 10), (16, 16))
    mode = Conv2D(16, 3, stride, transpose).mode
    out = torch.empty(tuple(ypre.shape), device='cuda')
    C.conv_k3_forward(mode, x.cuda(), wk.cuda(), b.cuda(), 16, out, act=False, algo=C.ALGO_DIRECT)
    _close(out, ypre, 'direct forward')
    with pytest.raises(C.NLTError):
        C.conv_k3_forward(mode, torch.zeros(1, 6, 10, 6, device='cuda'), torch.zeros(3, 3, 6, 6, device='cuda'), torch.zeros(6, device='cuda'),
                          6, torch.empty(1, 6, 10, 6, device='cuda'), algo=C.ALGO_MFMA)                 # 6 channels: no fast path
    if stride == 2 and not transpose:
        x57 = torch.zeros(2, 5, 7, 16, device='cuda')
        with pytest.raises(C.NLTError):
            Conv2D(16, 3, 2, transpose)(x57)
        with pytest.raises(C.NLTError):
            C.conv_k3_backward_weights(mode, x57, torch.zeros(2, 10, 14, 16, device='cuda'), 16,
                                       torch.zeros(3, 3, 16, 16, device='cuda'), torch.zeros(16, device='cuda'))
    if stride == 2 and transpose:
        x, wk, b, g, ypre, xd, wd, bd, ygraph = _reference(2, True, (5, 7), (16, 16))
        layer = Conv2D(16, 3, 2, True)
        layer.set_weights(wk, b)
        y = layer(x.cuda())
        assert tuple(y.shape) == (2, 10, 14, 16)
        _close(y, ypre, 'forward 5 x 7')
        dw, db = torch.zeros(3, 3, 16, 16, device='cuda'), torch.zeros(16, device='cuda')
        C.conv_k3_backward_weights(mode, x.cuda(), g.cuda(), 16, dw, db)
        rdw, rdb = torch.autograd.grad(ygraph, (wd, bd), g.double(), retain_graph=True)
        _close(dw, rdw, 'dkernel 5 x 7')
        _close(db, rdb, 'dbias 5 x 7')


# ---------------------------------------------------------------- wide layers: the default config's widths, odd and thin grids
def _name(stride, transpose):
    return '%s_s%d' % ('deconv' if transpose else 'conv', stride)


# (cin, cout) -> the path it is here for (csrc/conv_k3.hip):
#   (40, 24)    k3_mfma_kernel<2>, 24 of 32 outputs live; K = two slices + half a slice; weight gradient: 3 cin blocks, the last ragged, nbv = 2 ragged
#   (32, 48)    <4> with a fully masked fourth block; nbv = 3
#   (48, 64)    <4> full, three K slices; nbv = 4
#   (20, 72)    a second blockIdx.y with 8 of 64 live; ogroups = 2, the second ragged; the bias kernel's o0 loop runs twice
#   (144, 136)  nine K slices, three output groups
# input sizes per form: one texel, one row, one column, exactly one 8 x 8 tile of the row grid, one texel past it on both axes
# (the stride-2 conv's grid is half its input; the stride-2 transposed conv also takes odd inputs).
_S1 = {(40, 24): [(1, 1), (1, 9), (9, 1), (8, 8), (9, 17)], (32, 48): [(8, 8), (9, 17)], (48, 64): [(1, 1), (9, 17)],
       (20, 72): [(1, 9), (9, 17)], (144, 136): [(9, 1), (9, 17)]}
_PICK = {(1, False): _S1, (1, True): _S1,
         (2, False): {(40, 24): [(2, 2), (16, 16), (18, 34)], (32, 48): [(16, 16), (18, 34)], (48, 64): [(2, 2), (18, 34)],
                      (20, 72): [(2, 2), (18, 34)], (144, 136): [(16, 16), (18, 34)]},
         (2, True): {(40, 24): [(1, 1), (2, 1), (5, 7), (8, 8), (9, 17)], (32, 48): [(8, 8), (9, 17)], (48, 64): [(1, 1), (9, 17)],
                     (20, 72): [(2, 1), (5, 7), (9, 17)], (144, 136): [(5, 7), (9, 17)]}}
# the default config's (depth 256) deepest layers, on ROW GRIDS of 1 x 1, 2 x 2 and 4 x 6
DEEP = [(1024, 128), (512, 256), (256, 256)]
_DEEP_SIZES = {(1, False): [(1, 1), (2, 2), (4, 6)], (1, True): [(1, 1), (2, 2), (4, 6)], (2, False): [(4, 4), (8, 12)],
               (2, True): [(1, 1), (2, 2), (4, 6)]}
WIDE_CASES = [(s, tr, hw, ch, 2) for (s, tr) in FORMS for ch, sizes in _PICK[(s, tr)].items() for hw in sizes]
WIDE_CASES += [(s, tr, hw, ch, 2) for (s, tr) in FORMS for ch in DEEP for hw in _DEEP_SIZES[(s, tr)]]
# more frames than parity classes, and a last weight-gradient row slice that is no multiple of 4
WIDE_CASES += [(s, tr, (18, 34) if (s, tr) == (2, False) else (9, 17), (40, 24), n) for (s, tr) in FORMS for n in (3, 5)]
WORST = {}                                # form -> (worst layer error / reference max, where): printed by the last test of the matrix


def _f32_cpu(ref, stride, transpose, act, gpre):
    """The same layer and gradients in float32 with torch on the CPU: the plain float32 evaluation a device kernel is measured by
    where K is beyond the 2048 the 2e-5 bar is stated for (the rule of tests/test_gpu_ssim.py)."""
    x, wk, b = (t.clone().requires_grad_(True) for t in ref[:3])
    ypre = R.layer_f64(x, wk, b, stride, transpose)
    dx, dw, db = torch.autograd.grad(ypre, (x, wk, b), gpre.float())
    y = T.leaky_relu(ypre.detach(), ALPHA) if act else ypre.detach()
    return dict(zip(('forward', 'dx', 'dkernel (accumulated on 0.5)', 'dbias (accumulated on -2)'), (y, dx, dw, db)))


def _check_wide_layer(ref, stride, transpose, act, tag):
    """_close on every result; a layer with K > 2048 (9 x 256 channels and up) that misses it is allowed 4 x the distance of the
    float32 CPU evaluation from float64 instead, both numbers printed.  Returns the worst error / reference max."""
    cin, cout = ref[0].shape[3], ref[2].numel()
    res, gpre = _run_layer(ref, stride, transpose, act)
    f32, worst = None, 0.0
    for what, (got, want) in res.items():
        err, scale = float((got.double().cpu() - want).abs().max()), float(want.abs().max())
        worst = max(worst, err / scale)
        if err > 2e-5 * scale and 9 * max(cin, cout) > 2048:
            f32 = f32 or _f32_cpu(ref, stride, transpose, act, gpre)
            dist = float((f32[what].double() - want).abs().max())
            print('%s %s: max abs error %.3e over the 2e-5 bar (%.3e); float32 on the CPU is %.3e from float64, bound 4 x that = %.3e'
                  % (tag, what, err, 2e-5 * scale, dist, 4 * dist))
            assert err <= 4 * dist, (tag, what, err, dist, scale)
        else:
            _close(got, want, tag + ' ' + what)
    key = _name(stride, transpose)
    if worst > WORST.get(key, (0.0, ''))[0]:
        WORST[key] = (worst, tag)
    return worst


@pytest.mark.parametrize('stride,transpose,hw,ch,n', WIDE_CASES,
                         ids=['%s_%dx%d_%dto%d_n%d' % (_name(s, tr), hw[0], hw[1], ch[0], ch[1], n) for s, tr, hw, ch, n in WIDE_CASES])
def test_wide_layer_forward_and_backward(stride, transpose, hw, ch, n):
    """Forward with bias (linear and LeakyReLU), dx, dkernel and dbias of the layers the default depth-256 config runs, and of
    the channel counts that reach the other instantiations and ragged blocks of the kernels, against float64."""
    ref = _recent_reference(stride, transpose, hw, ch, n)
    for act in (False, True):
        _check_wide_layer(ref, stride, transpose, act, '%s %dx%d %d->%d n=%d %s' % (_name(stride, transpose), hw[0], hw[1], ch[0], ch[1], n,
                                                                                 'lrelu' if act else 'linear'))


def test_wide_layer_worst_errors_per_form():
    """Record: the worst layer error / reference max of the matrix above, per form (empty when run alone)."""
    for key, (worst, tag) in sorted(WORST.items()):
        print('worst of %s: %.3e of the reference max (bar 2e-5) at %s' % (key, worst, tag))
    _dump('kernel3_wide_layers_worst', {k: {'rel_max': v[0], 'case': v[1]} for k, v in WORST.items()})


@pytest.mark.parametrize('stride,transpose', FORMS)
def test_unaligned_input_takes_the_direct_kernel(stride, transpose):
    """A contiguous x that starts 4 bytes into its allocation cannot be read with 16-byte loads: ALGO_AUTO must fall back to the
    any-channel kernel and give the float64 result, ALGO_MFMA must refuse."""
    x, wk, b, g, ypre, *_ = _reference(stride, transpose, (6, 10), (16, 16))
    mode = Conv2D(16, 3, stride, transpose).mode
    xo = torch.empty(x.numel() + 1, device='cuda')[1:].view(x.shape)
    xo.copy_(x)
    assert xo.is_contiguous() and xo.data_ptr() % 16 == 4
    out = torch.full(tuple(ypre.shape), float('nan'), device='cuda')
    C.conv_k3_forward(mode, xo, wk.cuda(), b.cuda(), 16, out, act=False, algo=C.ALGO_AUTO)
    _close(out, ypre, 'unaligned x, ALGO_AUTO')
    with pytest.raises(C.NLTError):
        C.conv_k3_forward(mode, xo, wk.cuda(), b.cuda(), 16, torch.empty_like(out), act=False, algo=C.ALGO_MFMA)


def test_every_3x3_layer_of_the_depth256_models(monkeypatch):
    """Every distinct (mode, cin, cout) among the 3 x 3 layers of the depth-256 kernel = 3 model, with and without the
    observation path, on the row grid the layer has at UV 64 x 64 (capped at 8 x 8), as in the matrix above.  The list comes
    off the models: `_conv_layers()` for the channels, the models' own launches for the grids."""
    layers = {}
    for kw in (dict(), dict(use_obs=False)):
        om, pm = _pair(monkeypatch, depth=256, uvh=64, uvw=64, imh=32, imw=32, **kw)
        pm.build('cuda')
        seen, real = {}, C.conv_k3_forward

        def spy(mode, x, w_keras, bias, cout, out, **k):
            seen.setdefault((mode, x.shape[3], cout), tuple(x.shape[1:3]))
            return real(mode, x, w_keras, bias, cout, out, **k)
        monkeypatch.setattr(C, 'conv_k3_forward', spy)
        batch, nn = O.synth_batch(2, 64, 64, 32, 32, 32, 32, k=2, seed=5)
        pm.call(to_device_batch(batch, nn), 'vali')
        torch.cuda.synchronize()
        monkeypatch.setattr(C, 'conv_k3_forward', real)
        mine = {(c.mode, c.cin, c.n_ch_out): c for c in pm._conv_layers() if c.kernel_size == 3}
        assert set(mine) == set(seen), (sorted(set(mine) ^ set(seen)))
        for key, c in mine.items():
            layers.setdefault(key, (c.stride, c.transpose, seen[key]))
    assert (C.DECONV_K3S2, 1024, 128) in layers and (C.CONV_K3S2, 512, 256) in layers, sorted(layers)
    worst = {}
    for (mode, cin, cout), (stride, transpose, (h, w)) in sorted(layers.items()):
        cap = 16 if mode == C.CONV_K3S2 else 8                     # (the stride-2 conv's row grid is half its input)
        hw = (min(h, cap), min(w, cap))
        ref = _recent_reference(stride, transpose, hw, (cin, cout))
        for act in (False, True):
            tag = '%s %dx%d %d->%d %s' % (_name(stride, transpose), hw[0], hw[1], cin, cout, 'lrelu' if act else 'linear')
            e = _check_wide_layer(ref, stride, transpose, act, tag)
            worst[_name(stride, transpose)] = max(worst.get(_name(stride, transpose), (0.0, '')), (e, tag))
    for key, (e, tag) in sorted(worst.items()):
        print('worst of %s over %d model layers: %.3e of the reference max at %s' % (key, len(layers), e, tag))
    _dump('kernel3_depth256_model_layers_worst', {k: {'rel_max': v[0], 'case': v[1]} for k, v in worst.items()})


def test_k2_entry_points_refuse_the_new_modes():
    x = torch.zeros(1, 4, 4, 16, device='cuda')
    w = torch.zeros(3, 3, 16, 16, device='cuda')
    b = torch.zeros(16, device='cuda')
    for mode in (C.CONV_K3S1, C.CONV_K3S2, C.DECONV_K3S1, C.DECONV_K3S2):
        assert C.packed_weight_floats(mode, 16, 0, 16) <= 0
        assert not C.conv_tile_supported(mode, 16, 32, 32) and not C.conv_wino_supported(mode, 16, 32, 32)
        assert not C.conv_c32_supported(mode, 16, 32) and not C.wgrad_narrow_supported(mode, 16, 0, 1, 4, 4, 16)
        with pytest.raises(C.NLTError):
            C.conv_forward(mode, x, 16, 16, None, 0, 0, 1, 4, 4, w, None, b, 16, torch.empty_like(x), 16, algo=C.ALGO_DIRECT)
        with pytest.raises((C.NLTError, NotImplementedError)):
            C.conv_backward_weights(mode, x, 16, 16, None, 0, 0, 1, 4, 4, x, 16, 16, torch.zeros_like(w), torch.zeros_like(b))
        with pytest.raises(C.NLTError):
            C.conv_backward_weights_tiled(mode, x, 16, 16, None, 0, 0, 1, 4, 4, x, 16, 16, torch.zeros_like(w), torch.zeros_like(b))
        with pytest.raises(C.NLTError):
            C.pack_conv_weights(mode, w, 16, 0, 16)


# ---------------------------------------------------------------- whole models
def _pair(monkeypatch, depth=32, uvh=128, uvw=128, imh=64, imw=64, **kw):
    monkeypatch.setattr(T, 'conv2d_transpose_same', R.conv2d_transpose_same)
    om = O.OracleModel(depth=depth, kernel=3, uvh=uvh, uvw=uvw, imh=imh, imw=imw, seed=2, **kw)
    pm = get_model_class('nlt')(nlt_amd.make_config(depth=depth, kernel=3, uvh=uvh, uvw=uvw, imh=imh, imw=imw, **kw))
    pm.load_weights(om.numpy_weights())
    pm.register_trainable()
    return om, pm


MODELS = [dict(), dict(pool='avg', act='elu'), dict(use_obs=False), dict(norm='layer', pool='max')]


@pytest.mark.parametrize('kw', MODELS, ids=lambda kw: '+'.join('%s=%s' % x for x in kw.items()) or 'plain')
def test_kernel3_model_forward_and_train_step_vs_oracle(monkeypatch, kw):
    om, pm = _pair(monkeypatch, loss='l2', **kw)
    assert pm.generic
    pm.build('cuda')
    batch, nn = O.synth_batch(2, 128, 128, 64, 64, 64, 64, k=2, seed=9)
    db = to_device_batch(batch, nn)
    with torch.no_grad():
        ref = om.call(batch, 'vali', nn_list=nn)
    got = pm.call(db, 'vali', want_indices=True)
    torch.cuda.synchronize()
    e1, e2 = rel_l2(got[3]['pred'].cpu(), ref[3]['pred']), rel_l2(got[0].cpu(), ref[0])
    print('pred rel-L2 %.3e, pred_camspc rel-L2 %.3e (bound 1e-4)' % (e1, e2))
    assert e1 <= 1e-4 and e2 <= 1e-4
    po, go, _, _ = om.call(batch, 'train', nn_list=nn)
    lo = om.compute_loss(po, go, keep_batch=True).sum() / 2
    grads = torch.autograd.grad(lo, om.parameters(), allow_unused=True)   # (use_obs = False: the observation net is unused)
    pred, gt, _, _ = pm(db, mode='train')
    lp = pm.compute_loss(pred, gt, keep_batch=True).sum() / 2
    pm.flat_params.grad = None
    lp.backward()
    torch.cuda.synchronize()
    print('loss %.9e vs %.9e' % (float(lp.detach()), float(lo.detach())))
    assert abs(float(lp.detach()) - float(lo.detach())) <= 1e-5 * abs(float(lo.detach()))
    it = iter(grads)
    worst = 0.0
    for c in pm._conv_layers():
        for name in ('dkernel', 'dbias'):
            g = next(it)
            if g is None:
                assert not kw.get('use_obs', True) and not getattr(c, name).any()
                continue
            worst = max(worst, float((getattr(c, name).cpu() - g).norm() / (g.norm() + 1e-30)))
    print('worst per-tensor gradient rel-L2 %.3e (bound 5e-3)' % worst)
    assert worst <= 5e-3, worst
    opt = nlt_amd.optim.AdamAMSGrad(pm, 1e-3)
    loss, _ = trainvali.distributed_train_step(pm, db, opt, 2)
    assert np.isfinite(float(loss))


def test_kernel3_depth256_forward(monkeypatch):
    """The deepest level is 2 x 2 texels with 512 -> 256 channels: tiles larger than the image."""
    om, pm = _pair(monkeypatch, depth=256)
    pm.build('cuda')
    batch, nn = O.synth_batch(2, 128, 128, 64, 64, 64, 64, k=2, seed=5)
    with torch.no_grad():
        ref = om.call(batch, 'vali', nn_list=nn)
    got = pm.call(to_device_batch(batch, nn), 'vali')
    torch.cuda.synchronize()
    e1, e2 = rel_l2(got[3]['pred'].cpu(), ref[3]['pred']), rel_l2(got[0].cpu(), ref[0])
    print('pred rel-L2 %.3e, pred_camspc rel-L2 %.3e (bound 1e-4)' % (e1, e2))
    assert e1 <= 1e-4 and e2 <= 1e-4


@pytest.mark.parametrize('uvh,uvw', [(64, 64), (128, 64)])
def test_kernel3_depth256_forward_with_an_odd_deepest_level(monkeypatch, uvh, uvw):
    """Six stride-2 levels: the deepest map is 1 x 1 at 64 x 64 and 2 x 1 at 128 x 64, so the bottleneck's stride-2 transposed
    conv (1024 -> 128) runs on an odd input."""
    imh, imw = uvh // 2, uvw // 2
    om, pm = _pair(monkeypatch, depth=256, uvh=uvh, uvw=uvw, imh=imh, imw=imw)
    pm.build('cuda')
    batch, nn = O.synth_batch(2, uvh, uvw, imh, imw, imh, imw, k=2, seed=5)
    with torch.no_grad():
        ref = om.call(batch, 'vali', nn_list=nn)
    got = pm.call(to_device_batch(batch, nn), 'vali')
    torch.cuda.synchronize()
    e1, e2 = rel_l2(got[3]['pred'].cpu(), ref[3]['pred']), rel_l2(got[0].cpu(), ref[0])
    print('%d x %d: pred rel-L2 %.3e, pred_camspc rel-L2 %.3e (bound 1e-4)' % (uvh, uvw, e1, e2))
    _dump('kernel3_depth256_forward_%dx%d' % (uvh, uvw), {'rel_l2_pred_uv': e1, 'rel_l2_pred_camspc': e2})
    assert e1 <= 1e-4 and e2 <= 1e-4


def test_kernel3_depth256_train_step_vs_float64(monkeypatch):
    """Loss and EVERY kernel / bias gradient of one depth-256 kernel = 3 train step (64 x 64, n = 2, k = 2, l2) against the
    float64 oracle, kink-free (alpha = 1 on both sides), at the bars of tests/test_gpu_depth1024_train.py: loss 1e-5 relative,
    flat bucket and every tensor 1e-5 rel-L2.  The weight gradients here are the default config's: 64, 128 and 256 output
    channels, up to 1024 input channels.  A tensor over its bar is allowed 4 x the distance of the float32 CPU oracle from
    float64 for that tensor instead (measured here, printed)."""
    uv, cam, n = 64, 32, 2
    om, pm = _pair(monkeypatch, depth=256, uvh=uv, uvw=uv, imh=cam, imw=cam, loss='l2')
    _set_alpha(om, pm, 1.0)
    pm.build('cuda')
    assert pm.generic
    batch, nn = O.synth_batch(n, uv, uv, cam, cam, cam, cam, k=2, seed=11)
    args = ('l2', uv, cam, n)
    lo, grads = _oracle_grads(*args, torch.float64, batch, nn, 1.0, depth=256, seed=2, kernel=3)
    pred, gt, _, _ = pm(to_device_batch(batch, nn), mode='train')
    lp = pm.compute_loss(pred, gt, keep_batch=True).sum() / n
    pm.flat_params.grad = None
    lp.backward()
    torch.cuda.synchronize()
    lp = float(lp.detach())
    convs = pm._conv_layers()
    assert max(c.n_ch_out for c in convs if c.kernel_size == 3) == 256 and max(c.cin for c in convs if c.kernel_size == 3) == 1024
    names = ['conv%d.%s%s' % (li, nm, tuple(getattr(c, nm).shape)) for li, c in enumerate(convs) for nm in ('dkernel', 'dbias')]
    got = [getattr(c, nm).detach().cpu().double() for c in convs for nm in ('dkernel', 'dbias')]
    num = [float((a - g).norm()) for a, g in zip(got, grads)]
    den = [float(g.norm()) for g in grads]
    errs = [a / max(b, 1e-300) for a, b in zip(num, den)]
    flat = (sum(a * a for a in num) / sum(b * b for b in den)) ** 0.5
    order = sorted(range(len(errs)), key=lambda i: -errs[i])
    print('loss %.9e vs float64 %.9e (rel %.3e, bound 1e-5); flat bucket rel-L2 %.3e (bound 1e-5)' % (lp, lo, abs(lp - lo) / abs(lo), flat))
    for i in order[:8]:
        print('  %-40s rel-L2 %.3e (bound 1e-5)' % (names[i], errs[i]))
    rec = {'loss_hip': lp, 'loss_oracle_f64': lo, 'flat_rel': flat, 'worst': [(errs[i], names[i]) for i in order[:8]]}
    over = [i for i in order if errs[i] > 1e-5]
    if over:
        _, g32 = _oracle_grads(*args, torch.float32, batch, nn, 1.0, depth=256, seed=2, kernel=3)
        dist = {i: float((g32[i] - grads[i]).norm()) / max(den[i], 1e-300) for i in over}
        for i in over:
            print('  %-40s over 1e-5: float32 CPU oracle is %.3e from float64, bound 4 x that = %.3e' % (names[i], dist[i], 4 * dist[i]))
        rec['over_1e-5'] = [(names[i], errs[i], dist[i]) for i in over]
    _dump('kernel3_depth256_train_64_n2_l2_alpha1', rec)
    assert abs(lp - lo) <= 1e-5 * abs(lo), (lp, lo)
    assert flat <= 1e-5, flat
    for i in over:
        assert errs[i] <= 4 * dist[i], (names[i], errs[i], dist[i])


def test_kernel3_three_adam_steps_match_oracle(monkeypatch):
    """Three `distributed_train_step`s of the depth-32 kernel = 3 model (alpha = 0.3) against `O.train_step` + KerasAdamAMSGrad,
    with the structure and bars of test_depth1024_adam_and_clipnorm_steps_match_oracle."""
    n = 2
    om, pm = _pair(monkeypatch, loss='l2')
    pm.build('cuda')
    batch, nn = O.synth_batch(n, 128, 128, 64, 64, 64, 64, k=2, seed=13)
    db = to_device_batch(batch, nn)
    opt_o = O.KerasAdamAMSGrad(om.parameters(), 1e-3)
    opt_p = nlt_amd.optim.AdamAMSGrad(pm, 1e-3)
    recs = []
    for step in range(3):
        lo, go = O.train_step(om, opt_o, batch, global_bs=n, nn_list=nn)
        lp, _ = trainvali.distributed_train_step(pm, db, opt_p, global_bs=n)
        torch.cuda.synchronize()
        ref = flat_oracle_grads(pm, go)
        rel = float((pm.flat_params.grad - ref).norm() / ref.norm())
        worst = per_tensor_worst(pm, go)
        print('step %d: loss %.9e vs %.9e; flat bucket rel-L2 %.3e (bound %g); worst tensor %.3e at %s (bound %g)'
              % (step, float(lp), float(lo), rel, FLAT_TOL, worst[0], worst[1], TENSOR_TOL))
        recs.append({'step': step, 'loss_hip': float(lp), 'loss_oracle': float(lo), 'flat_rel': rel, 'worst_tensor': worst})
        assert abs(float(lp) - float(lo)) <= 2e-5 * max(1.0, abs(float(lo))), (step, float(lp), float(lo))
        assert rel < FLAT_TOL, (step, rel)
        assert worst[0] < TENSOR_TOL, (step, worst)
    wdiff = max(float((po.detach() - c.kernel.cpu()).abs().max()) for po, c in zip(om.parameters()[::2], pm._conv_layers()))
    print('weights after three steps: max abs difference %.3e (bound 2e-4)' % wdiff)
    _dump('kernel3_depth32_three_adam_steps', {'steps': recs, 'weights_max_abs_diff': wdiff})
    assert wdiff < 2e-4, wdiff


def test_kernel3_test_mode_with_obs_override(monkeypatch):
    om, pm = _pair(monkeypatch)
    pm.build('cuda')
    n = 2
    batch, nn = O.synth_batch(n, 128, 128, 64, 64, 64, 64, k=2, seed=4)
    with torch.no_grad():
        x = torch.cat((batch[1], batch[2], batch[3]), 3)
        _, feats = om._call(x, [r - b for b, r in nn], return_feats=True)
        agg = [f.mean(0, keepdim=True) for f in feats]
        ref = om.call(batch, 'test', obs_override=[a.expand(n, -1, -1, -1) for a in agg], nn_list=nn)
    got = pm.call(to_device_batch(batch, nn), 'test', obs_override=[a.cuda() for a in agg])
    torch.cuda.synchronize()
    e1, e2 = rel_l2(got[3]['pred'].cpu(), ref[3]['pred']), rel_l2(got[0].cpu(), ref[0])
    print('obs_override: pred rel-L2 %.3e, pred_camspc rel-L2 %.3e (bound 1e-4)' % (e1, e2))
    assert e1 <= 1e-4 and e2 <= 1e-4


def test_kernel3_checkpoint_round_trip(monkeypatch, tmp_path):
    _, pm = _pair(monkeypatch, loss='l2')
    pm.build('cuda')
    batch, nn = O.synth_batch(2, 128, 128, 64, 64, 64, 64, k=2, seed=6)
    db = to_device_batch(batch, nn)
    opt = nlt_amd.optim.AdamAMSGrad(pm, 1e-3)
    trainvali.distributed_train_step(pm, db, opt, 2)
    want = pm.call(db, 'vali')[0].clone()
    path = trainvali.save_checkpoint(str(tmp_path / 'ckpt-1.pt'), pm, opt, step=1)
    pm2 = get_model_class('nlt')(nlt_amd.make_config(depth=32, kernel=3, uvh=128, uvw=128, imh=64, imw=64, loss='l2'))
    pm2.build('cuda'); pm2.register_trainable()
    assert trainvali.restore_checkpoint(path, pm2, nlt_amd.optim.AdamAMSGrad(pm2, 1e-3)) == 1
    got = pm2.call(db, 'vali')[0]
    torch.cuda.synchronize()
    assert torch.equal(got, want)
