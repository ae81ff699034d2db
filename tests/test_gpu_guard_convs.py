"""-m gpu: memory discipline of the conv families (tests/guard_util.py).  Every tensor argument -- sources, Keras arrays, packed
fragments, biases, masks, outputs, scratch -- is a guarded view (256 KiB bands before and after, pad columns on every channel
slice), run under the three fills.  Per case: bands and pads intact and read-only operands bitwise unchanged; outputs bit-identical
across the fills (the first-generation atomic weight gradient: finite, within its bar); values against float64 `oracle.tf_ops`
(or autograd through it) at the bar the kernel's own test already uses; scratch handed out at exactly the queried size, with
nothing read before it is written, and a refusal at capacity `need - 1`.

Shapes are the smallest with an edge in each indexing scheme: 2-3 frames of 6 x 10 / 5 x 7 (row counts that are no multiple of
16) for the layerwise kernels, one 8 x 16 tile plus one texel on both axes (and a grid smaller than a tile) for the tiled ones.

Out of scope here (and in the two sibling files): the data-preparation kernels (cosine_map, albedo, diffuse_base, remap_*,
uv_index_map, knn_indices, psnr_sums, resize_cv_linear, gather_frames_u8, assemble_batch), the tape and event plumbing, and
whole-model runs."""
import functools

import numpy as np
import pytest
import torch

from nlt_amd import capi as C
from oracle import nlt_oracle as O
from oracle import tf_ops as T
import conv_k3_ref as R3
import guard_util as G
from gpu_util import rel_l2

pytestmark = pytest.mark.gpu

PAD = 4
ALPHA = 0.3
MODES = {C.CONV1X1: (1, 1, False), C.CONV_K2S2: (2, 2, False), C.CONV_K2S1: (2, 1, False),
         C.DECONV_K2S2: (2, 2, True), C.DECONV_K2S1: (2, 1, True)}
ADJOINT = {C.CONV_K2S2: C.DECONV_K2S2, C.CONV_K2S1: C.DECONV_K2S1, C.DECONV_K2S2: C.CONV_K2S2, C.DECONV_K2S1: C.CONV_K2S1}
NAME = {C.CONV1X1: 'c1x1', C.CONV_K2S2: 'c2s2', C.CONV_K2S1: 'c2s1', C.DECONV_K2S2: 'd2s2', C.DECONV_K2S1: 'd2s1'}
SPLITK_COUNTERS = 16384         # include/nlt_hip.h, nlt_conv_forward_splitk: the words of the scratch that are zero between launches


def _hw(mode):
    return (6, 10) if mode == C.CONV_K2S2 else (5, 7)


def _r(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def _conv64(mode, x, wk, b):
    k, s, tr = MODES[mode]
    return (T.conv2d_transpose_same if tr else T.conv2d_same)(x.double(), wk.double(), b.double(), s)


@functools.lru_cache(maxsize=None)
def _layer(mode, n, h, w, c0, c1, cout, seed=0):
    """Inputs of one k2 / 1x1 layer and its float64 pre-activation output: computed once, shared, never written."""
    rng = np.random.default_rng(seed + 17 * mode + c0 + cout)
    k, s, tr = MODES[mode]
    cin = c0 + c1
    x0, x1 = _r(rng, n, h, w, c0), (_r(rng, n, h, w, c1) if c1 else None)
    wk = _r(rng, *((k, k, cout, cin) if tr else (k, k, cin, cout)), scale=1.0 / np.sqrt(k * k * cin))
    b = _r(rng, cout)
    x = x0 if not c1 else torch.cat((x0, x1), -1)
    with torch.no_grad():
        pre = _conv64(mode, x, wk, b)
    return dict(x0=x0, x1=x1, x=x, wk=wk, b=b, pre=pre, oh=pre.shape[1], ow=pre.shape[2])


def _sl(data, pad=PAD):
    return None if data is None else dict(data=data, ld=data.shape[-1] + pad)


def _close(got, ref, bar=2e-5, what=''):
    """The bar of tests/test_gpu_conv.py: max abs error <= 2e-5 x the output scale."""
    scale = max(float(ref.abs().max()), 1.0)
    err = float((got.double() - ref.double()).abs().max())
    assert err <= bar * scale, (what, err, scale)


def _lrelu(y, alpha=ALPHA):
    return torch.where(y > 0, y, alpha * y)


# ---------------------------------------------------------------- nlt_conv_forward
FWD = [(m, a, 16, 8, 12) for m in MODES for a in (C.ALGO_DIRECT, C.ALGO_MFMA)]
FWD += [(C.DECONV_K2S2, C.ALGO_MFMA, 8, 32, 4), (C.CONV1X1, C.ALGO_MFMA, 4, 32, 12), (C.DECONV_K2S1, C.ALGO_MFMA, 4, 0, 4),
        (C.CONV_K2S1, C.ALGO_DIRECT, 3, 2, 7)]


@pytest.mark.parametrize('mode,algo,c0,c1,cout', FWD, ids=['%s-%s-%d+%d-%d' % (NAME[m], 'mfma' if a == C.ALGO_MFMA else 'direct', c0, c1, co)
                                                           for m, a, c0, c1, co in FWD])
def test_conv_forward(monkeypatch, mode, algo, c0, c1, cout):
    n, (h, w) = 3, _hw(mode)
    L = _layer(mode, n, h, w, c0, c1, cout)
    pad = PAD if algo == C.ALGO_MFMA else 3             # (the direct path takes any stride)
    packed = C.pack_conv_weights(mode, L['wk'].cuda(), c0, c1, cout) if algo == C.ALGO_MFMA else None
    ops = {'src0': _sl(L['x0'], pad), 'src1': _sl(L['x1'], pad), 'w_keras': L['wk'], 'w_packed': packed, 'bias': L['b'],
           'out': dict(shape=(n, L['oh'], L['ow'], cout), ld=cout + pad)}

    def call(o):
        C.conv_forward(mode, o['src0'].t, c0, c0 + pad, o['src1'].t if c1 else None, c1, c1 + pad if c1 else 0, n, h, w, o['w_keras'].t,
                       o['w_packed'].t if packed is not None else None, o['bias'].t, cout, o['out'].t, cout + pad, act=True, alpha=ALPHA,
                       algo=algo)
    res, _ = G.run_case(monkeypatch, call, ops, outputs=('out',))
    _close(res[0]['out'], _lrelu(L['pre']))


@pytest.mark.parametrize('tile', [0x12, 0x21, 0x24, 0x44])
@pytest.mark.parametrize('mode', [C.CONV_K2S2, C.CONV_K2S1, C.DECONV_K2S2], ids=lambda m: NAME[m])
def test_conv_forward_mfma_wave_tiles(monkeypatch, mode, tile):
    """Wave tiles of 1 - 4 row blocks x 1 - 4 column blocks on 45 / 105 GEMM rows: every one has a ragged last row block."""
    n, (h, w), c0, cout = 3, _hw(mode), 32, 64
    L = _layer(mode, n, h, w, c0, 0, cout)
    packed = C.pack_conv_weights(mode, L['wk'].cuda(), c0, 0, cout)
    ops = {'src0': _sl(L['x0']), 'w_keras': L['wk'], 'w_packed': packed, 'bias': L['b'], 'out': dict(shape=(n, L['oh'], L['ow'], cout), ld=cout + PAD)}

    def call(o):
        C.conv_forward(mode, o['src0'].t, c0, c0 + PAD, None, 0, 0, n, h, w, o['w_keras'].t, o['w_packed'].t, o['bias'].t, cout, o['out'].t,
                       cout + PAD, act=True, alpha=ALPHA, algo=C.ALGO_MFMA, tile_hint=tile)
    res, _ = G.run_case(monkeypatch, call, ops, outputs=('out',))
    _close(res[0]['out'], _lrelu(L['pre']))


@pytest.mark.parametrize('algo', [C.ALGO_DIRECT, C.ALGO_MFMA])
def test_conv_forward_mask_and_accumulate(monkeypatch, algo):
    """out = (old + conv(x)) * lrelu'(mask): the target is read and written, the mask is a channel slice."""
    mode, n, h, w, c0, c1, cout = C.CONV_K2S1, 3, 5, 7, 16, 8, 12
    L = _layer(mode, n, h, w, c0, c1, cout)
    rng = np.random.default_rng(5)
    old, mask = _r(rng, n, h, w, cout), _r(rng, n, h, w, cout)
    packed = C.pack_conv_weights(mode, L['wk'].cuda(), c0, c1, cout)
    ops = {'src0': _sl(L['x0']), 'src1': _sl(L['x1']), 'w_keras': L['wk'], 'w_packed': packed, 'bias': L['b'], 'mask': _sl(mask),
           'out': _sl(old)}

    def call(o):
        C.conv_forward(mode, o['src0'].t, c0, c0 + PAD, o['src1'].t, c1, c1 + PAD, n, h, w, o['w_keras'].t, o['w_packed'].t, o['bias'].t,
                       cout, o['out'].t, cout + PAD, act=False, alpha=ALPHA, algo=algo, mask_src=o['mask'].t, ldm=cout + PAD, accumulate=True)
    res, _ = G.run_case(monkeypatch, call, ops, outputs=('out',))
    _close(res[0]['out'], (old.double() + L['pre']) * torch.where(mask > 0, 1.0, ALPHA).double())


# ---------------------------------------------------------------- split-K, the bias-map form, backward-data
@pytest.mark.parametrize('ksplit', [3, 8, -3])
@pytest.mark.parametrize('mode', list(MODES), ids=lambda m: NAME[m])
def test_conv_forward_splitk(monkeypatch, mode, ksplit):
    """One group of slices (the scratch is the ticket counters alone: all of it zero on exit), two groups meeting through the
    scratch, and the two-launch form.  The counters are zero on entry and on exit; the partial tiles behind them start as the fill."""
    n, h, w, c0, c1, cout = 2, 6, 10, 48, 16, 32
    L = _layer(mode, n, h, w, c0, c1, cout)
    packed = C.pack_conv_weights(mode, L['wk'].cuda(), c0, c1, cout)
    ops = {'src0': _sl(L['x0']), 'src1': _sl(L['x1']), 'w_packed': packed, 'bias': L['b'],
           'out': dict(shape=(n, L['oh'], L['ow'], cout), ld=cout + PAD)}

    def call(o):
        C.conv_forward_splitk(mode, ksplit, o['src0'].t, c0, c0 + PAD, o['src1'].t, c1, c1 + PAD, n, h, w, o['w_packed'].t, o['bias'].t,
                              cout, o['out'].t, cout + PAD, act=True, alpha=ALPHA, tile_hint=0x11)
    res, state = G.run_case(monkeypatch, call, ops, outputs=('out',), zero_words=SPLITK_COUNTERS)
    (key, need, zero, g), = state['nan'][0].requests
    assert zero and need == C.lib().nlt_conv_splitk_workspace_floats(mode, n, h, w, cout, ksplit) and need >= SPLITK_COUNTERS
    _close(res[0]['out'], _lrelu(L['pre']))


@pytest.mark.parametrize('mode,ksplit,map_frames', [(C.CONV_K2S1, 1, 1), (C.DECONV_K2S2, 8, 1), (C.CONV_K2S2, -3, 2), (C.CONV1X1, 8, 2)],
                         ids=str)
def test_conv_forward_map(monkeypatch, mode, ksplit, map_frames):
    """out = act(conv + bias + bias_map), the map shared by the frames (1) or one per frame (n)."""
    n, h, w, c0, c1, cout = 2, 6, 10, 48, 16, 32
    L = _layer(mode, n, h, w, c0, c1, cout)
    bmap = _r(np.random.default_rng(9), map_frames, L['oh'], L['ow'], cout)
    packed = C.pack_conv_weights(mode, L['wk'].cuda(), c0, c1, cout)
    ops = {'src0': _sl(L['x0']), 'src1': _sl(L['x1']), 'w_packed': packed, 'bias': L['b'], 'bias_map': bmap,
           'out': dict(shape=(n, L['oh'], L['ow'], cout), ld=cout + PAD)}

    def call(o):
        C.conv_forward_map(mode, ksplit, o['src0'].t, c0, c0 + PAD, o['src1'].t, c1, c1 + PAD, n, h, w, o['w_packed'].t, o['bias'].t, cout,
                           o['out'].t, cout + PAD, o['bias_map'].t, act=True, alpha=ALPHA, tile_hint=0x11)
    res, _ = G.run_case(monkeypatch, call, ops, outputs=('out',), zero_words=SPLITK_COUNTERS)
    _close(res[0]['out'], _lrelu(L['pre'] + bmap.double()))


def _dgrad_reference(mode, n, h, w, cin, cout, seed):
    """A layer `mode` cin -> cout on [n,h,w,cin]: Keras array, dpre, and the float64 gradient w.r.t. its input."""
    rng = np.random.default_rng(seed)
    k, s, tr = MODES[mode]
    wk = _r(rng, *((2, 2, cout, cin) if tr else (2, 2, cin, cout)), scale=0.1)
    x = torch.zeros(n, h, w, cin, dtype=torch.float64, requires_grad=True)
    y = (T.conv2d_transpose_same if tr else T.conv2d_same)(x, wk.double(), torch.zeros(cout, dtype=torch.float64), s)
    dp = _r(rng, *y.shape)
    (gx,) = torch.autograd.grad(y, x, dp.double())
    return rng, wk, dp, gx, y.shape[1], y.shape[2]


@pytest.mark.parametrize('mode,ksplit,split,partial', [(C.CONV_K2S1, 1, False, False), (C.DECONV_K2S1, 4, False, False),
                                                       (C.DECONV_K2S2, 8, False, False), (C.CONV_K2S2, 1, True, True),
                                                       (C.CONV_K2S2, 8, True, False), (C.DECONV_K2S2, -3, True, True)],
                         ids=str)
def test_conv_backward_data(monkeypatch, mode, ksplit, split, partial):
    """nlt_conv_backward_data (the adjoint family on the layer's own array) accumulated onto the target with the producer's
    LeakyReLU', without and with the level-split epilogue; the bar of tests/test_gpu_train_ops.py: 3e-5 x max |total|."""
    c, cout, n = 16, 48, 2
    cin = 2 * c
    h, w = (6, 10) if mode in (C.CONV_K2S2, C.DECONV_K2S2) else (5, 7)
    rng, wk, dp, gx, oh, ow = _dgrad_reference(mode, n, h, w, cin, cout, 40 + mode)
    adj = ADJOINT[mode]
    packed = C.pack_conv_weights(adj, wk.cuda(), cout, 0, cin)
    old, fm_y, obs_y, dobs0 = _r(rng, n, h, w, cin), _r(rng, n, h, w, cin), _r(rng, n, h, w, c), _r(rng, n, h, w, c)
    aq, ao = 0.3, 0.2
    ldo = cin if split else cin + PAD            # (with the split the target is the whole dfm[l] map)
    ops = {'dpre': _sl(dp), 'w_packed': packed, 'zero_bias': torch.zeros(cin), 'mask': dict(data=fm_y, ld=ldo),
           'out': dict(data=old, ld=ldo), 'split_y': obs_y if split else None, 'split_d': dobs0 if split else None}

    def call(o):
        C.conv_backward_data(adj, o['dpre'].t, cout, cout + PAD, n, oh, ow, o['w_packed'].t, o['zero_bias'].t, cin, o['out'].t, ldo,
                             mask_src=o['mask'].t, ldm=ldo, mask_alpha=aq, accumulate=True, tile_hint=0x11, ksplit=ksplit,
                             split=(c, o['split_y'].t, o['split_d'].t, ao, partial) if split else None)
    res, _ = G.run_case(monkeypatch, call, ops, outputs=('out', 'split_d') if split else ('out',), zero_words=SPLITK_COUNTERS)
    tot = gx + old.double()
    tol = 3e-5 * float(tot.abs().max())
    nq = c if split else cin
    ref_q = tot[..., :nq] * torch.where(fm_y[..., :nq] > 0, 1.0, aq).double()
    assert float((res[0]['out'][..., :nq].double() - ref_q).abs().max()) <= tol
    if split:
        ref_o = (tot[..., c:] + (dobs0.double() if partial else 0)) * torch.where(obs_y > 0, 1.0, ao).double()
        assert float((res[0]['split_d'].double() - ref_o).abs().max()) <= tol
        assert torch.equal(res[0]['out'][..., c:], old[..., c:])             # the observation half of dfm[l] is not rewritten


# ---------------------------------------------------------------- the tiled families (8 x 16 output tiles)
def _tiled_ref(mode, cin, cout, frames, kobs, h, w):
    L = _layer(mode, frames * kobs, h, w, cin, 0, cout, seed=3)
    return L, L['pre'].reshape(frames, kobs, L['oh'], L['ow'], cout)


@functools.lru_cache(maxsize=None)
def _native_tile_error(mode, cin, cout, tn, frames, kobs, h, w):
    """rel-L2 of the native fp32 LDS-tiled kernel from float64 on the same inputs: the yardstick of the bf16-split kernels' bars
    (tests/test_gpu_tile.py).  Plain dense tensors."""
    L, _ = _tiled_ref(mode, cin, cout, frames, kobs, h, w)
    out = torch.empty((frames * kobs, L['oh'], L['ow'], cout), device='cuda')
    C.conv_tile_forward(mode, L['x0'].cuda(), cin, cin, frames * kobs, 1, h, w, C.pack_conv_tile_weights(mode, L['wk'].cuda(), cin, cout, tn),
                        L['b'].cuda(), cout, tn, out, cout, None, 0, act=True, alpha=ALPHA)
    torch.cuda.synchronize()
    return rel_l2(out.cpu(), _lrelu(L['pre']))


def _tiled_case(monkeypatch, family, mode, cin, cout, tn, h, w, kobs, **kw):
    frames = 2
    L, pre = _tiled_ref(mode, cin, cout, frames, kobs, h, w)
    oh, ow = L['oh'], L['ow']
    wk = L['wk'].cuda()
    fn = {'tile': C.conv_tile_forward, 'c32': C.conv_c32_forward, 'wino': C.conv_wino_forward, 'tile3': C.conv_tile3_forward,
          'tile3r': C.conv_tile3r_forward}[family]
    if family in ('tile', 'c32'):
        packed = C.pack_conv_tile_weights(mode, wk, cin, cout, tn)
    elif family == 'wino':
        packed = C.pack_conv_wino_weights(mode, wk, cin, cout, tn)
    else:
        packed = C.pack_conv_tile3_weights(mode, wk, cin, cout, tn)
    torch.cuda.synchronize()
    old_mean = _r(np.random.default_rng(2), frames, oh, ow, 2 * cout)
    ops = {'src': _sl(L['x0']), 'packed': packed, 'bias': L['b'], 'out': dict(shape=(frames * kobs, oh, ow, cout), ld=cout + PAD),
           'mean': old_mean if kobs > 1 else None}
    tn_arg = () if family == 'c32' else (tn,)

    def call(o):
        mean = o['mean'].t.view(-1)[cout:] if kobs > 1 else None              # the upper half of a 2 cout map
        fn(mode, o['src'].t, cin + PAD, cin, frames, kobs, h, w, o['packed'].t, o['bias'].t, cout, *tn_arg, o['out'].t, cout + PAD,
           mean, 2 * cout if kobs > 1 else 0, act=True, alpha=ALPHA, **kw)
    res, _ = G.run_case(monkeypatch, call, ops, outputs=('out', 'mean') if kobs > 1 else ('out',))
    ref = _lrelu(L['pre'])
    e_out = rel_l2(res[0]['out'], ref)
    e_mean = None
    if kobs > 1:
        assert torch.equal(res[0]['mean'][..., :cout], old_mean[..., :cout]), "the lower half of the mean map was written"
        e_mean = rel_l2(res[0]['mean'][..., cout:], _lrelu(pre).mean(1))
    return e_out, e_mean


TILE_GRIDS = {C.CONV_K2S1: [(9, 17), (3, 5)], C.DECONV_K2S1: [(9, 17), (3, 5)], C.CONV_K2S2: [(18, 34), (6, 10)]}
_tiled_ids = str


@pytest.mark.parametrize('kobs', [1, 3])
@pytest.mark.parametrize('tn', [32, 64])
@pytest.mark.parametrize('mode,grid', [(m, g) for m in (C.CONV_K2S1, C.CONV_K2S2) for g in TILE_GRIDS[m]], ids=_tiled_ids)
def test_conv_tile_forward(monkeypatch, mode, grid, tn, kobs):
    e_out, e_mean = _tiled_case(monkeypatch, 'tile', mode, 16, tn, tn, grid[0], grid[1], kobs)
    assert e_out <= 1e-5 and (e_mean is None or e_mean <= 1e-5)               # tests/test_gpu_tile.py


@pytest.mark.parametrize('kobs', [1, 3])
@pytest.mark.parametrize('cin', [16, 32])
@pytest.mark.parametrize('grid', TILE_GRIDS[C.CONV_K2S1], ids=_tiled_ids)
def test_conv_c32_forward(monkeypatch, grid, cin, kobs):
    e_out, e_mean = _tiled_case(monkeypatch, 'c32', C.CONV_K2S1, cin, 32, 32, grid[0], grid[1], kobs)
    assert e_out <= 1e-5 and (e_mean is None or e_mean <= 1e-5)               # tests/test_gpu_tile.py


@pytest.mark.parametrize('mode,tn,kobs', [(C.CONV_K2S1, 32, 1), (C.CONV_K2S1, 32, 3), (C.CONV_K2S1, 64, 1), (C.DECONV_K2S1, 32, 1)], ids=_tiled_ids)
@pytest.mark.parametrize('grid', TILE_GRIDS[C.CONV_K2S1], ids=_tiled_ids)
def test_conv_wino_forward(monkeypatch, grid, mode, tn, kobs):
    e_out, e_mean = _tiled_case(monkeypatch, 'wino', mode, 8, tn, tn, grid[0], grid[1], kobs)
    assert e_out <= 2e-6 and (e_mean is None or e_mean <= 2e-6)               # tests/test_gpu_wino.py


@pytest.mark.parametrize('nprod', [6, 9])
@pytest.mark.parametrize('kobs', [1, 3])
@pytest.mark.parametrize('family,mode,tn,max_wg', [('tile3', C.CONV_K2S1, 32, None), ('tile3', C.CONV_K2S2, 32, None),
                                                   ('tile3r', C.CONV_K2S1, 32, 0), ('tile3r', C.CONV_K2S1, 32, 1),
                                                   ('tile3r', C.CONV_K2S2, 32, 0), ('tile3r', C.CONV_K2S2, 32, 1),
                                                   ('tile3r', C.CONV_K2S1, 64, 0), ('tile3r', C.CONV_K2S1, 64, 1)], ids=_tiled_ids)
def test_conv_tile3_forward_streaming_and_resident(monkeypatch, family, mode, tn, max_wg, kobs, nprod):
    """csrc/conv_tile3.hip, both forms (the resident one with its grid from the device and with one workgroup walking every item);
    the bar of tests/test_gpu_tile.py: as close to float64 as the native fp32 kernel x 1.5 (+ 3e-8 with six products, 1e-9 with
    nine; the mean + 1e-7)."""
    for h, w in TILE_GRIDS[mode]:
        kw = dict(nprod=nprod) if max_wg is None else dict(nprod=nprod, max_workgroups=max_wg)
        e_out, e_mean = _tiled_case(monkeypatch, family, mode, 16, tn, tn, h, w, kobs, **kw)
        e1 = _native_tile_error(mode, 16, tn, tn, 2, kobs, h, w)
        print("%s %s %dx%d kobs %d nprod %d: rel-L2 %.2e (native fp32 kernel %.2e)" % (family, NAME[mode], h, w, kobs, nprod, e_out, e1))
        assert e_out <= 1.5 * e1 + (1e-9 if nprod == 9 else 3e-8), (e_out, e1)
        assert e_mean is None or e_mean <= 1.5 * e1 + 1e-7, (e_mean, e1)


TILE_BWD = [(C.CONV_K2S1, 32, 16, 9, 17), (C.CONV_K2S1, 32, 16, 3, 5), (C.DECONV_K2S1, 32, 16, 9, 17), (C.DECONV_K2S2, 32, 16, 9, 17),
            (C.DECONV_K2S2, 32, 16, 3, 5), (C.CONV_K2S2, 32, 32, 18, 34), (C.CONV_K2S2, 32, 32, 6, 10)]


@pytest.mark.parametrize('mode,cin,cout,h,w', TILE_BWD, ids=['%s-%d-%d-%dx%d' % ((NAME[c[0]],) + c[1:]) for c in TILE_BWD])
def test_conv_tile_backward_data(monkeypatch, mode, cin, cout, h, w):
    """nlt_conv_tile_backward_data on every adjoint family, accumulated, with the producer's LeakyReLU'; the transposed k2s2
    family (a Conv2D k2s2 layer) with the level-split epilogue.  Bars of tests/test_gpu_train_ops.py."""
    n, tn = 2, 32
    rng, wk, dp, gx, oh, ow = _dgrad_reference(mode, n, h, w, cin, cout, 60 + mode + h)
    adj = ADJOINT[mode]
    split = adj == C.DECONV_K2S2
    c = cin // 2
    packed = C.pack_conv_tile_weights_adjoint(adj, wk.cuda(), cout, cin, tn, cin, 0)
    torch.cuda.synchronize()
    old, ymask, obs_y, dobs0 = _r(rng, n, h, w, cin), _r(rng, n, h, w, cin), _r(rng, n, h, w, c), _r(rng, n, h, w, c)
    ldo = cin if split else cin + PAD
    ops = {'dpre': _sl(dp), 'packed': packed, 'mask': dict(data=ymask, ld=ldo), 'out': dict(data=old, ld=ldo),
           'split_y': obs_y if split else None, 'split_d': dobs0 if split else None}

    def call(o):
        C.conv_tile_backward_data(adj, o['dpre'].t, cout, cout + PAD, n, oh, ow, o['packed'].t, cin, tn, o['out'].t, ldo,
                                  mask_src=o['mask'].t, ldm=ldo, mask_alpha=0.3, accumulate=True,
                                  split=(c, o['split_y'].t, o['split_d'].t, 0.2, True) if split else None)
    res, _ = G.run_case(monkeypatch, call, ops, outputs=('out', 'split_d') if split else ('out',))
    tot = gx + old.double()
    nq = c if split else cin
    tol = (3e-5 if split else 2 * 3e-5) * float((tot if split else gx).abs().max())
    assert float((res[0]['out'][..., :nq].double() - tot[..., :nq] * torch.where(ymask[..., :nq] > 0, 1.0, 0.3).double()).abs().max()) <= tol
    if split:
        ref_o = (tot[..., c:] + dobs0.double()) * torch.where(obs_y > 0, 1.0, 0.2).double()
        assert float((res[0]['split_d'].double() - ref_o).abs().max()) <= tol
        assert torch.equal(res[0]['out'][..., c:], old[..., c:])


@pytest.mark.parametrize('h,w', [(9, 17), (3, 5)])
@pytest.mark.parametrize('transpose_fwd', [False, True])
def test_conv_wino_backward_data(monkeypatch, transpose_fwd, h, w):
    """Gradient w.r.t. input channels [lo, hi) of a stride-1 layer, read in place from the layer's own array: += target,
    x LeakyReLU'(mask); rel-L2 <= 2e-6 against float64 autograd (tests/test_gpu_wino.py)."""
    mode = C.DECONV_K2S1 if transpose_fwd else C.CONV_K2S1
    n, cin_f, cout_f, lo, hi, tn = 2, 40, 16, 8, 40, 32
    rng, wk, dp, gx, oh, ow = _dgrad_reference(mode, n, h, w, cin_f, cout_f, 80 + h)
    adj = ADJOINT[mode]
    packed = C.pack_conv_wino_weights(adj, wk.cuda(), cout_f, hi - lo, tn, full=cin_f, lo=lo)
    torch.cuda.synchronize()
    prev, mask = _r(rng, n, h, w, hi - lo), _r(rng, n, h, w, hi - lo)
    ops = {'dpre': _sl(dp), 'packed': packed, 'mask': _sl(mask), 'out': _sl(prev)}

    def call(o):
        C.conv_wino_backward_data(adj, o['dpre'].t, cout_f, cout_f + PAD, n, h, w, o['packed'].t, hi - lo, tn, o['out'].t, hi - lo + PAD,
                                  mask_src=o['mask'].t, ldm=hi - lo + PAD, mask_alpha=0.3, accumulate=True)
    res, _ = G.run_case(monkeypatch, call, ops, outputs=('out',))
    ref = (prev.double() + gx[..., lo:hi]) * torch.where(mask > 0, 1.0, 0.3).double()
    assert rel_l2(res[0]['out'], ref) <= 2e-6


# ---------------------------------------------------------------- bf16 middle
@pytest.mark.parametrize('mode,c0,c1,cout,f32_in,f32_out', [(C.CONV_K2S2, 32, 0, 64, True, False), (C.CONV_K2S1, 64, 0, 64, False, False),
                                                            (C.DECONV_K2S2, 32, 128, 16, False, False), (C.DECONV_K2S1, 16, 0, 16, False, True),
                                                            (C.CONV1X1, 64, 0, 64, False, True)], ids=str)
def test_conv_bf16_forward(monkeypatch, mode, c0, c1, cout, f32_in, f32_out):
    """csrc/conv_bf16.hip on bf16 / fp32 stored maps (16-byte row pieces: pad 8); tests/test_gpu_bf16.py's oracle and bars."""
    n, (h, w) = 3, _hw(mode)
    rng = np.random.default_rng(mode * 1000 + c0)
    rb, bf = O.round_bf16, torch.bfloat16
    k, s, tr = MODES[mode]
    cin = c0 + c1
    x0, x1 = _r(rng, n, h, w, c0), (_r(rng, n, h, w, c1) if c1 else None)
    wk = torch.from_numpy(T.glorot_uniform(rng, (k, k, cout, cin) if tr else (k, k, cin, cout)))
    bias = torch.from_numpy(rng.uniform(-0.1, 0.1, cout).astype(np.float32))
    xin = rb(torch.cat((x0, x1), 3) if c1 else x0)
    ref = T.leaky_relu((T.conv2d_transpose_same if tr else T.conv2d_same)(xin, rb(wk), bias, s), 0.3)
    ref = ref if f32_out else rb(ref)
    packed = C.conv_bf16_pack(mode, wk.cuda(), c0, c1, cout)
    torch.cuda.synchronize()
    ops = {'src0': dict(data=x0 if f32_in else x0.to(bf), ld=c0 + 8), 'src1': dict(data=x1.to(bf), ld=c1 + 8) if c1 else None,
           'packed': packed, 'bias': bias,
           'out': dict(shape=tuple(ref.shape), dtype=torch.float32 if f32_out else bf, ld=cout + 8)}

    def call(o):
        C.conv_bf16_forward(mode, o['src0'].t, c0, c0 + 8, o['src1'].t if c1 else None, c1, c1 + 8 if c1 else 0, n, h, w, o['packed'].t,
                            o['bias'].t, cout, o['out'].t, cout + 8, act=True, alpha=0.3)
    res, _ = G.run_case(monkeypatch, call, ops, outputs=('out',))
    got = res[0]['out'].float()
    assert rel_l2(got, ref) <= (2e-6 if f32_out else 5e-3)
    if not f32_out:
        bad = got != ref
        assert float(((got - ref).abs() / ref.abs().clamp_min(1e-20))[bad].max() if bad.any() else 0.0) <= 2 ** -7


def test_obs_mean_bf16(monkeypatch):
    n, k, hw, c = 2, 3, 35, 8
    x = torch.randn(n, k, hw, c, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    old = torch.randn(n, hw, 2 * c, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)

    def call(o):
        C.obs_mean_bf16(o['obs'].t, n, k, hw, c, o['fm'].t.view(-1)[c:], 2 * c)
    res, _ = G.run_case(monkeypatch, call, {'obs': x, 'fm': old}, outputs=('fm',))
    assert torch.equal(res[0]['fm'][..., c:].float(), O.round_bf16(x.float().sum(1) * (1.0 / k)))
    assert torch.equal(res[0]['fm'][..., :c], old[..., :c])


@pytest.mark.parametrize('cin,cout,shape', [(64, 32, (1, 5, 3)), (32, 32, (3, 17, 19))])
def test_chmix_bf16_forward(monkeypatch, cin, cout, shape):
    """Bit for bit the adapter's result on plain dense tensors, at shapes tests/test_gpu_chmix.py holds to the oracle."""
    g = torch.Generator().manual_seed(cin + cout + shape[1])
    x = (torch.randn(shape + (cin,), generator=g) * 1.5).to(torch.bfloat16)
    w = torch.randn((1, 1, cin, cout), generator=g) * (cin ** -0.5)
    b = torch.randn(cout, generator=g) * 0.1
    packed = C.chmix_bf16_pack(w.cuda())
    want = C.chmix_bf16_forward(x.cuda(), packed, b.cuda(), cout, act=True).cpu()
    res, _ = G.run_case(monkeypatch, lambda o: C.chmix_bf16_forward(o['x'].t, o['packed'].t, o['bias'].t, cout, act=True),
                        {'x': x, 'packed': packed, 'bias': b})
    assert torch.equal(res[0]['ret'].view(torch.int16), want.view(torch.int16))


# ---------------------------------------------------------------- kernel = 3
K3_MODES = {(1, False): C.CONV_K3S1, (2, False): C.CONV_K3S2, (1, True): C.DECONV_K3S1, (2, True): C.DECONV_K3S2}
K3_GRIDS = {(1, False): [(1, 1), (1, 9), (9, 17)], (1, True): [(1, 1), (1, 9), (9, 17)], (2, False): [(2, 2), (2, 18), (18, 34)],
            (2, True): [(1, 1), (2, 1), (9, 17)]}
K3 = [(s, tr, hw, ch, algo) for (s, tr), grids in K3_GRIDS.items() for hw in grids
      for ch, algo in (((8, 4), C.ALGO_MFMA), ((8, 4), C.ALGO_DIRECT), ((5, 3), C.ALGO_DIRECT))]


@functools.lru_cache(maxsize=None)
def _k3_reference(stride, transpose, hw, ch, n=2):
    (h, w), (cin, cout) = hw, ch
    gen = torch.Generator().manual_seed(1000 * stride + 100 * transpose + 7 * h + cin)
    x = torch.randn(n, h, w, cin, generator=gen)
    wk = torch.randn((3, 3, cout, cin) if transpose else (3, 3, cin, cout), generator=gen) * 0.2
    b = torch.randn(cout, generator=gen)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, wk, b))
    y = R3.layer_f64(xd, wd, bd, stride, transpose)
    g = torch.randn(y.shape, generator=gen)
    rdx, rdw, rdb = torch.autograd.grad(y, (xd, wd, bd), g.double())
    return x, wk, b, g, y.detach(), rdx, rdw, rdb


def _k3_close(got, ref, what):
    """tests/test_gpu_conv_k3.py: max abs error <= 2e-5 x the reference's max abs."""
    err, scale = float((got.double() - ref).abs().max()), float(ref.abs().max())
    assert err <= 2e-5 * scale, (what, err, scale)


@pytest.mark.parametrize('stride,transpose,hw,ch,algo', K3,
                         ids=['%s_s%d_%dx%d_%dto%d_%s' % ('deconv' if tr else 'conv', s, hw[0], hw[1], ch[0], ch[1],
                                                          'mfma' if a == C.ALGO_MFMA else 'direct') for s, tr, hw, ch, a in K3])
def test_conv_k3(monkeypatch, stride, transpose, hw, ch, algo):
    """nlt_conv_k3_forward / _backward_data (each algorithm) and _backward_weights (accumulating, two passes through scratch of
    exactly the queried size) on the one-texel, one-row and tile-plus-one grids."""
    x, wk, b, g, ypre, rdx, rdw, rdb = _k3_reference(stride, transpose, hw, ch)
    mode = K3_MODES[(stride, transpose)]
    n, h, w, cin = x.shape
    cout = b.numel()
    res, _ = G.run_case(monkeypatch, lambda o: C.conv_k3_forward(mode, o['x'].t, o['w'].t, o['b'].t, cout, o['y'].t, act=True, alpha=ALPHA, algo=algo),
                        {'x': x, 'w': wk, 'b': b, 'y': dict(shape=tuple(ypre.shape))}, outputs=('y',))
    _k3_close(res[0]['y'], _lrelu(ypre), 'forward')
    res, _ = G.run_case(monkeypatch, lambda o: C.conv_k3_backward_data(mode, o['g'].t, o['w'].t, n, h, w, cin, cout, o['dx'].t, algo=algo),
                        {'g': g, 'w': wk, 'dx': dict(shape=tuple(x.shape))}, outputs=('dx',))
    _k3_close(res[0]['dx'], rdx, 'dx')
    if algo == C.ALGO_DIRECT and ch == (8, 4):  # (the weight gradient has one form: once per channel pair)
        return
    dw0, db0 = torch.full(tuple(wk.shape), 0.5), torch.full((cout,), -2.0)
    res, state = G.run_case(monkeypatch, lambda o: C.conv_k3_backward_weights(mode, o['x'].t, o['g'].t, cout, o['dw'].t, o['db'].t),
                            {'x': x, 'g': g, 'dw': dw0, 'db': db0}, outputs=('dw', 'db'))
    (key, need, zero, ws), = state['nan'][0].requests
    assert need == C.lib().nlt_conv_k3_wgrad_workspace_floats(mode, n, h, w, cin, cout)
    _k3_close(res[0]['dw'] - 0.5, rdw, 'dkernel')
    _k3_close(res[0]['db'] + 2.0, rdb, 'dbias')


def test_conv_k3_backward_weights_refuses_a_short_workspace(monkeypatch):
    x, wk, b, g, *_ = _k3_reference(1, False, (9, 17), (8, 4))
    _untouched(monkeypatch, lambda o: C.conv_k3_backward_weights(C.CONV_K3S1, o['x'].t, o['g'].t, 4, o['dw'].t, o['db'].t),
               {'x': x, 'g': g, 'dw': torch.zeros(tuple(wk.shape)), 'db': torch.zeros(4)})


def _untouched(monkeypatch, call, ops):
    """A refusal case: with one float less scratch than the query asks for the entry point returns NLT_ERR_BAD_ARG, and every
    operand -- the outputs included -- and every band is as it was."""
    def refused(o):
        with pytest.raises(C.NLTError, match='bad argument'):
            call(o)
    G.run_case(monkeypatch, refused, ops, outputs=(), short=1)


# ---------------------------------------------------------------- weight gradients
def _wgrad_reference(mode, n, h, w, c0, c1, cout, seed):
    L = _layer(mode, n, h, w, c0, c1, cout, seed)
    k, s, tr = MODES[mode]
    wz = torch.zeros(tuple(L['wk'].shape), dtype=torch.float64, requires_grad=True)
    bz = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    y = (T.conv2d_transpose_same if tr else T.conv2d_same)(L['x'].double(), wz, bz, s)
    dp = _r(np.random.default_rng(seed + 1), *y.shape)
    gw, gb = torch.autograd.grad(y, (wz, bz), dp.double())
    return L, dp, gw, gb


WGRAD = [(m, a, 16, 8, 12) for m in MODES for a in ('direct', 'mfma', 'det', 'tiled')]
WGRAD += [(m, 'narrow', 16, 8, 12) for m in (C.CONV_K2S2, C.CONV_K2S1, C.DECONV_K2S1)]         # (<= 32 columns, K <= 128)
WGRAD += [(C.DECONV_K2S2, a, 8, 32, 4) for a in ('mfma', 'det', 'tiled', 'narrow')] + [(C.CONV_K2S1, 'direct', 3, 2, 7)]
# the narrow kernel's LDS-tiled form (16 / 32-channel stride-1 layers: one clipped tile here) and a 32-column stride-2 layer
WGRAD += [(C.CONV_K2S1, 'narrow', 16, 0, 16), (C.DECONV_K2S1, 'narrow', 32, 0, 32), (C.CONV_K2S2, 'narrow', 32, 0, 32)]


def _wgrad_call(algo, mode, c0, c1, cout, n, h, w):
    def call(o):
        args = (mode, o['src0'].t, c0, c0 + PAD, o['src1'].t if c1 else None, c1, c1 + PAD if c1 else 0, n, h, w, o['dpre'].t, cout + PAD, cout,
                o['dw'].t, o['db'].t)
        if algo == 'tiled':
            C.conv_backward_weights_tiled(*args)
        elif algo == 'narrow':
            C.conv_backward_weights_narrow(*args)
        elif algo == 'det':
            with C.deterministic_scope(True):
                C.conv_backward_weights(*args, algo=C.ALGO_MFMA)
        else:
            C.conv_backward_weights(*args, algo=C.ALGO_MFMA if algo == 'mfma' else C.ALGO_DIRECT)
    return call


def _wgrad_ops(L, dp, c1, w0=0.0):
    return {'src0': _sl(L['x0']), 'src1': _sl(L['x1']) if c1 else None, 'dpre': _sl(dp),
            'dw': torch.full(tuple(L['wk'].shape), w0), 'db': torch.full((L['b'].numel(),), w0)}


@pytest.mark.parametrize('mode,algo,c0,c1,cout', WGRAD, ids=['%s-%s-%d+%d-%d' % (NAME[m], a, c0, c1, co) for m, a, c0, c1, co in WGRAD])
def test_conv_backward_weights(monkeypatch, mode, algo, c0, c1, cout):
    """Every weight-gradient kernel, accumulating onto 0.5; sources and dP as channel slices.  The atomic first generation
    (direct, mfma): finite under every fill and within the bar; its `_det` form, the tiled and the narrow kernels: the same bits
    under every fill.  Bar of tests/test_gpu_train_ops.py: 3e-5 x max(|g|, 1)."""
    n = 3
    h, w = 6, 10                                 # (the tiled / narrow kernels want >= 4 texels per GEMM grid row)
    L, dp, gw, gb = _wgrad_reference(mode, n, h, w, c0, c1, cout, 7)
    res, _ = G.run_case(monkeypatch, _wgrad_call(algo, mode, c0, c1, cout, n, h, w), _wgrad_ops(L, dp, c1, 0.5), outputs=('dw', 'db'),
                        det=algo not in ('direct', 'mfma'))
    for r in res:
        sw, sb = max(float(gw.abs().max()), 1.0), max(float(gb.abs().max()), 1.0)
        assert float((r['dw'].double() - 0.5 - gw).abs().max()) <= 3e-5 * sw
        assert float((r['db'].double() - 0.5 - gb).abs().max()) <= 3e-5 * sb


@pytest.mark.parametrize('algo', ['det', 'tiled', 'narrow'])
def test_conv_backward_weights_refuses_a_short_workspace(monkeypatch, algo):
    mode, n, h, w, c0, c1, cout = C.CONV_K2S1, 3, 6, 10, 16, 8, 12
    L, dp, gw, gb = _wgrad_reference(mode, n, h, w, c0, c1, cout, 7)
    _untouched(monkeypatch, _wgrad_call(algo, mode, c0, c1, cout, n, h, w), _wgrad_ops(L, dp, c1))


# ---------------------------------------------------------------- one-launch refresh of packed weights
def test_repack_weights(monkeypatch):
    """nlt_repack_weights: sources, destinations and the descriptor table itself (a uint8 store) guarded; bit for bit the per-layer
    pack launches (tests/test_gpu_repack.py)."""
    rng = np.random.default_rng(0)
    rows = [(C.REPACK_MFMA, C.CONV1X1, (1, 1, 36, 3), 4, 32, 3, 0), (C.REPACK_MFMA, C.DECONV_K2S2, (2, 2, 4, 40), 8, 32, 4, 0),
            (C.REPACK_MFMA, C.CONV_K2S1, (2, 2, 24, 40), 24, 0, 40, 0), (C.REPACK_TILE, C.CONV_K2S2, (2, 2, 16, 32), 16, 0, 32, 32)]
    srcs = [_r(rng, *r[2]) for r in rows]
    refs = []
    for (kind, mode, shape, c0, c1, cout, tn), s in zip(rows, srcs):
        refs.append((C.pack_conv_weights(mode, s.cuda(), c0, c1, cout) if kind == C.REPACK_MFMA
                     else C.pack_conv_tile_weights(mode, s.cuda(), c0, cout, tn)).cpu())
    ops = {'src%d' % i: s for i, s in enumerate(srcs)}
    ops.update({'dst%d' % i: dict(shape=tuple(r.shape)) for i, r in enumerate(refs)})
    keep = []

    def call(o):
        entries = [dict(src=o['src%d' % i].t, dst=o['dst%d' % i].t, kind=r[0], mode=r[1], c0=r[3], c1=r[4], cout=r[5], tn=r[6], lo=0, full=r[5])
                   for i, r in enumerate(rows)]
        table, n_desc, blocks = C.repack_table(entries, 'cuda')
        tab = G.Guarded('repack table', tuple(table.shape), torch.uint8, o['src0'].fill, 'cuda', data=table)
        keep.append(tab)
        C.repack_weights(tab.t, n_desc, blocks)
    res, _ = G.run_case(monkeypatch, call, ops, outputs=tuple('dst%d' % i for i in range(len(rows))))
    for tab in keep:
        tab.check_intact(); tab.check_unchanged()
    for i, r in enumerate(refs):
        assert torch.equal(res[0]['dst%d' % i], r), i
