"""CPU: lane-level NumPy emulation of csrc/conv_k3.hip -- the fast forward kernel (k3_mfma_kernel: block decode, the staged
input tile with its halo, the live-tap weight slice in both Keras layouts, the 16-byte fragment reads with their shared
permutation of k, the parity classes of the stride-2 transposed conv, the epilogue addresses) and the weight gradient's two
stages (k3_wgrad_partial_kernel / k3_wgrad_reduce_kernel: row slices, operand addresses, partial layout).  The same tile,
halo, tap and parity functions are restated here and run over every lane of every workgroup; each global or LDS access is
range-checked, every output must be written exactly once, and the result must equal the float64 loops of conv_k3_ref.
(v_mfma_f32_16x16x4_f32 layout as in tests/test_mfma_index_math.py.)"""
import numpy as np
import pytest

import conv_k3_ref as R

CONV_S1, CONV_S2, DECONV_S1, DECONV_S2 = 5, 6, 7, 8
T_, KC, XS = 8, 16, 20
LANE = np.arange(64); KG, LI = LANE >> 4, LANE & 15


def ntaps(mode, par): return (1 if par else 2) if mode == DECONV_S2 else 3
def tap(mode, par, t): return (1 if par else 2 * t) if mode == DECONV_S2 else t


def dy_of(mode, a):
    if mode == DECONV_S2:
        return 0 if a == 2 else 1
    return 2 - a if mode == DECONV_S1 else a


def geom(mode, n, h, w, cin, cout):
    p = dict(mode=mode, deconv=mode in (DECONV_S1, DECONV_S2), n=n, h=h, w=w, cin=cin, cout=cout,
             gh=h, gw=w, oh=h, ow=w, S=1, OFF=-1, US=1)
    dmax = 2
    if mode == CONV_S2:
        assert h % 2 == 0 and w % 2 == 0
        p.update(gh=h // 2, gw=w // 2, oh=h // 2, ow=w // 2, S=2, OFF=0)
    elif mode == DECONV_S2:
        p.update(oh=2 * h, ow=2 * w, US=2)
        dmax = 1
    p['it'] = (T_ - 1) * p['S'] + dmax + 1
    p['tiles_y'], p['tiles_x'] = -(-p['gh'] // T_), -(-p['gw'] // T_)
    return p


class Checked:
    """A flat buffer whose every access is range-checked (NumPy would wrap a negative index silently)."""

    def __init__(self, size, data=None):
        self.a = np.zeros(size, np.float32) if data is None else np.ascontiguousarray(data, np.float32).reshape(-1)

    def ld(self, idx):
        idx = np.asarray(idx)
        assert idx.size == 0 or (idx.min() >= 0 and idx.max() < self.a.size), (idx.min(), idx.max(), self.a.size)
        return self.a[idx]

    def st(self, idx, v):
        idx = np.asarray(idx)
        assert idx.size == 0 or (idx.min() >= 0 and idx.max() < self.a.size), (idx.min(), idx.max(), self.a.size)
        self.a[idx] = v


def mfma(a, b, acc):
    """acc [64, 4] += A B with A[i = lane & 15][k = lane >> 4] = a, B[k = lane >> 4][j = lane & 15] = b;
    D row = 4 (lane >> 4) + r, column = lane & 15."""
    A = np.zeros((16, 4), np.float32); B = np.zeros((4, 16), np.float32)
    A[LI, KG] = a; B[KG, LI] = b
    D = A @ B
    for r in range(4):
        acc[:, r] += D[4 * KG + r, LI]


def emulate_forward(mode, x, wk, bias, cout):
    n, h, w, cin = x.shape
    p = geom(mode, n, h, w, cin, cout)
    NB = 4 if cout > 32 else 2 if cout > 16 else 1
    TN, it = 16 * NB, p['it']
    X, W = Checked(0, x), Checked(0, wk)
    Y = Checked(n * p['oh'] * p['ow'] * cout)
    written = np.zeros(Y.a.size, np.int32)
    lds_floats = it * it * XS + 9 * 4 * TN * 4
    assert 4 * lds_floats <= 64 * 1024 and (4 * it * it * XS) % 16 == 0
    ncls = 4 if mode == DECONV_S2 else 1
    tid = np.arange(256)
    for bx in range(n * ncls * p['tiles_y'] * p['tiles_x']):
        t = bx
        tx = t % p['tiles_x']; t //= p['tiles_x']
        ty = t % p['tiles_y']; t //= p['tiles_y']
        cls = (t & 3) if mode == DECONV_S2 else 0
        f = (t >> 2) if mode == DECONV_S2 else t
        pm, pn = cls >> 1, cls & 1
        nty, ntx = ntaps(mode, pm), ntaps(mode, pn)
        gy0, gx0 = ty * T_, tx * T_
        iy0, ix0 = gy0 * p['S'] + p['OFF'], gx0 * p['S'] + p['OFF']
        for by in range(-(-cout // TN)):
            o0 = by * TN
            acc = np.zeros((4, NB, 64, 4), np.float32)           # [wave][nb][lane][r]
            for c0 in range(0, cin, KC):
                lds = Checked(lds_floats)
                lds.a[:] = np.nan                                # a read of an unstaged word poisons the result
                idx = np.arange(it * it * 4)                     # (the kernel strides this range by 256 threads)
                tex, q = idx >> 2, idx & 3
                iy, ix, c = iy0 + tex // it, ix0 + tex % it, c0 + 4 * q
                ok = (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w) & (c < cin)
                for e in range(4):
                    v = np.zeros(idx.size, np.float32)
                    v[ok] = X.ld((((f * h + iy[ok]) * w + ix[ok]) * cin + c[ok] + e))
                    lds.st(tex * XS + 4 * q + e, v)
                wbase = it * it * XS
                idx = np.arange(nty * ntx * 4 * TN)
                if p['deconv']:
                    c4, ol, tapi = idx & 3, (idx >> 2) % TN, idx // (4 * TN)
                    tp = np.array([tap(mode, pm, ti // ntx) * 3 + tap(mode, pn, ti % ntx) for ti in tapi])
                    c, o = c0 + 4 * c4, o0 + ol
                    ok = (c < cin) & (o < cout)
                    for e in range(4):
                        v = np.zeros(idx.size, np.float32)
                        v[ok] = W.ld((tp[ok] * cout + o[ok]) * cin + c[ok] + e)
                        lds.st(wbase + ((tapi * 4 + c4) * TN + ol) * 4 + e, v)
                else:
                    o4, cl, tapi = idx % (TN // 4), (idx // (TN // 4)) & 15, idx // (4 * TN)
                    tp = np.array([tap(mode, pm, ti // ntx) * 3 + tap(mode, pn, ti % ntx) for ti in tapi])
                    c, o = c0 + cl, o0 + 4 * o4
                    ok = (c < cin) & (o < cout)
                    for e in range(4):
                        v = np.zeros(idx.size, np.float32)
                        v[ok] = W.ld((tp[ok] * cin + c[ok]) * cout + o[ok] + e)
                        lds.st(wbase + ((tapi * 4 + (cl >> 2)) * TN + 4 * o4 + e) * 4 + (cl & 3), v)
                for wave in range(4):
                    lr, lc = 2 * wave + (LI >> 3), LI & 7
                    for ity in range(nty):
                        dy = dy_of(mode, tap(mode, pm, ity))
                        for itx in range(ntx):
                            dx = dy_of(mode, tap(mode, pn, itx))
                            texl = (lr * p['S'] + dy) * it + lc * p['S'] + dx
                            assert texl.max() < it * it
                            for nb in range(NB):
                                wt = wbase + (((ity * ntx + itx) * 4 + KG) * TN + LI) * 4 + nb * 64
                                for r in range(4):
                                    mfma(lds.ld(texl * XS + 4 * KG + r), lds.ld(wt + r), acc[wave, nb])
            for wave in range(4):
                for nb in range(NB):
                    o = o0 + nb * 16 + LI
                    for r in range(4):
                        row = 4 * KG + r
                        gy, gx = gy0 + 2 * wave + (row >> 3), gx0 + (row & 7)
                        ok = (o < cout) & (gy < p['gh']) & (gx < p['gw'])
                        dst = ((f * p['oh'] + gy * p['US'] + pm) * p['ow'] + gx * p['US'] + pn) * cout + o
                        Y.st(dst[ok], acc[wave, nb][ok, r] + bias[o[ok]])
                        np.add.at(written, dst[ok], 1)
    assert (written == 1).all(), "every output exactly once"
    return Y.a.reshape(n, p['oh'], p['ow'], cout)


def slices_of(p):
    rows = p['n'] * p['gh'] * p['gw']
    cblocks, ogroups = -(-p['cin'] // 16), -(-(-(-p['cout'] // 16)) // 4)
    tiles = 9 * cblocks * ogroups
    want = max(1, min(-(-4096 // tiles), -(-rows // 64)))
    chunk = (-(-rows // want) + 3) // 4 * 4
    return rows, chunk, -(-rows // chunk), cblocks, ogroups


def emulate_wgrad(mode, x, g, cout, dw0):
    n, h, w, cin = x.shape
    p = geom(mode, n, h, w, cin, cout)
    rows, chunk, nsl, cblocks, ogroups = slices_of(p)
    X, G = Checked(0, x), Checked(0, g)
    per = 9 * cin * cout
    ws = Checked(nsl * per)
    ws.a[:] = np.nan
    oblocks = -(-cout // 16)
    for sl in range(nsl):
        r_begin, r_end = sl * chunk, min(rows, sl * chunk + chunk)
        assert r_begin < rows
        for bx in range(9 * cblocks * ogroups):
            og = bx % ogroups; cb = (bx // ogroups) % cblocks; tp = bx // (ogroups * cblocks)
            a, b = tp // 3, tp % 3
            dy, dx = dy_of(mode, a), dy_of(mode, b)
            pm, pn = ((a & 1), (b & 1)) if p['US'] == 2 else (0, 0)
            c = cb * 16 + LI
            nbv = min(4, oblocks - og * 4)
            acc = np.zeros((4, 64, 4), np.float32)
            for r0 in range(r_begin, r_end, 4):
                r = r0 + KG
                live = r < r_end
                gx, gy, f = r % p['gw'], (r // p['gw']) % p['gh'], r // (p['gw'] * p['gh'])
                iy, ix = gy * p['S'] + p['OFF'] + dy, gx * p['S'] + p['OFF'] + dx
                ok = live & (c < cin) & (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)
                av = np.zeros(64, np.float32)
                av[ok] = X.ld((((f * h + iy) * w + ix) * cin + c)[ok])
                gp = ((f * p['oh'] + gy * p['US'] + pm) * p['ow'] + gx * p['US'] + pn) * cout
                for nb in range(nbv):
                    o = (og * 4 + nb) * 16 + LI
                    okb = live & (o < cout)
                    bv = np.zeros(64, np.float32)
                    bv[okb] = G.ld((gp + o)[okb])
                    mfma(av, bv, acc[nb])
            for nb in range(nbv):
                o = (og * 4 + nb) * 16 + LI
                for r in range(4):
                    cc = cb * 16 + 4 * KG + r
                    ok = (o < cout) & (cc < cin)
                    dst = (sl * 9 + tp) * cin * cout + cc * cout + o
                    assert np.isnan(ws.ld(dst[ok])).all(), "a partial written twice"
                    ws.st(dst[ok], acc[nb][ok, r])
    assert not np.isnan(ws.a).any(), "a partial never written"
    dw = dw0.copy().reshape(-1)
    for e in range(per):
        s = np.float32(0)
        for i in range(nsl):
            s = np.float32(s + ws.a[i * per + e])
        dst = e
        if p['deconv']:
            o, c, tp = e % cout, (e // cout) % cin, e // (cin * cout)
            dst = (tp * cout + o) * cin + c
        dw[dst] += s
    return dw.reshape(dw0.shape)


def _case(mode, h, w, cin, cout, seed, n=1):
    rng = np.random.default_rng(seed)
    tr = mode in (DECONV_S1, DECONV_S2)
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    wk = rng.standard_normal((3, 3, cout, cin) if tr else (3, 3, cin, cout)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    stride = 2 if mode in (CONV_S2, DECONV_S2) else 1
    ref = (R.deconv3_naive if tr else R.conv3_naive)(x, wk, b, stride)
    return x, wk, b, stride, tr, ref


SHAPES = [(6, 10), (5, 7), (2, 2), (34, 18)]
CHANNELS = [(4, 4), (16, 32), (80, 8), (128, 16)]
CASES = [(m, h, w, ci, co) for m in (CONV_S1, CONV_S2, DECONV_S1, DECONV_S2) for (h, w) in SHAPES for (ci, co) in CHANNELS
         if not (m == CONV_S2 and (h, w) == (5, 7))]                 # (only the stride-2 CONV needs an even input)
# Shapes the device suite (tests/test_gpu_conv_k3.py) holds to float64: NB = 2 with 24 of 32 outputs live and a ragged third K
# slice, NB = 4 with a fully masked fourth block, a second ragged blockIdx.y; grids one texel wide or high; the stride-2
# transposed conv on odd inputs.  (h, w) is the GRID the case is about: CONV_S2 runs it on the 2h x 2w input.
WIDE = [(9, 17, 40, 24), (9, 17, 32, 48), (9, 17, 20, 72)]
THIN = [(1, 1, 8, 16), (1, 9, 20, 8), (9, 1, 8, 24), (2, 1, 16, 16)]
CASES += [(m, (2 * h if m == CONV_S2 else h), (2 * w if m == CONV_S2 else w), ci, co)
          for m in (CONV_S1, CONV_S2, DECONV_S1, DECONV_S2) for (h, w, ci, co) in WIDE + THIN]


@pytest.mark.parametrize('mode,h,w,cin,cout', CASES)
def test_forward_kernel_index_math(mode, h, w, cin, cout):
    x, wk, b, stride, tr, ref = _case(mode, h, w, cin, cout, mode * 1000 + h * 10 + cin)
    got = emulate_forward(mode, x, wk, b, cout)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max()


def test_forward_kernel_wide_output_tile_and_channel_tail():
    """cout = 72: NB = 4 with a second, ragged output-channel tile (72 = 64 + 8)."""
    for mode in (CONV_S1, DECONV_S2):
        x, wk, b, stride, tr, ref = _case(mode, 6, 10, 8, 72, mode)
        assert np.abs(emulate_forward(mode, x, wk, b, 72) - ref).max() <= 2e-5 * np.abs(ref).max()


@pytest.mark.parametrize('mode', [CONV_S1, DECONV_S2])
def test_forward_kernel_frame_and_class_decode_with_three_frames(mode):
    """blockIdx.x -> (frame, parity class, tile) with more frames than classes and an odd tile count (5 x 9: 1 x 2 tiles)."""
    x, wk, b, stride, tr, ref = _case(mode, 5, 9, 8, 16, mode, n=3)
    assert np.abs(emulate_forward(mode, x, wk, b, 16) - ref).max() <= 2e-5 * np.abs(ref).max()


def _wgrad_case(mode, h, w, cin, cout, n):
    import torch
    rng = np.random.default_rng(mode + h)
    tr, stride = mode in (DECONV_S1, DECONV_S2), 2 if mode in (CONV_S2, DECONV_S2) else 1
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    oh, ow = (h * stride, w * stride) if tr else (h // stride, w // stride)
    g = rng.standard_normal((n, oh, ow, cout)).astype(np.float32)
    dw0 = rng.standard_normal((3, 3, cout, cin) if tr else (3, 3, cin, cout)).astype(np.float32)
    got = emulate_wgrad(mode, x, g, cout, dw0)
    wz = torch.zeros(dw0.shape, dtype=torch.float64, requires_grad=True)
    y = R.layer_f64(torch.from_numpy(x).double(), wz, None, stride, tr)
    (ref,) = torch.autograd.grad(y, wz, torch.from_numpy(g).double())
    assert np.abs(got - dw0 - ref.numpy()).max() <= 2e-5 * np.abs(ref.numpy()).max()


@pytest.mark.parametrize('mode', [CONV_S1, CONV_S2, DECONV_S1, DECONV_S2])
@pytest.mark.parametrize('h,w,cin,cout', [(6, 10, 5, 3), (2, 2, 16, 32), (6, 10, 20, 72), (18, 10, 4, 4)])
def test_weight_gradient_index_math(mode, h, w, cin, cout):
    _wgrad_case(mode, h, w, cin, cout, 2)


@pytest.mark.parametrize('mode', [CONV_S1, CONV_S2, DECONV_S1, DECONV_S2])
@pytest.mark.parametrize('h,w,cin,cout,n', [(9, 17, 40, 24, 3), (9, 17, 32, 48, 2), (9, 17, 20, 72, 2), (1, 1, 8, 16, 2),
                                            (1, 9, 20, 8, 5), (9, 1, 8, 24, 2), (2, 1, 16, 16, 2), (5, 7, 4, 4, 2)])
def test_weight_gradient_index_math_wide_thin_and_odd(mode, h, w, cin, cout, n):
    """The shapes tests/test_gpu_conv_k3.py runs on the device.  (h, w) is the row grid: the stride-2 conv gets the 2h x 2w
    input that has it.  n = 3 at 9 x 17: 459 rows, a last slice whose length is no multiple of 4."""
    _wgrad_case(mode, *((2 * h, 2 * w) if mode == CONV_S2 else (h, w)), cin, cout, n)
