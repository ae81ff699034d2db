"""-m gpu: the texels-direct form of the three-term split stride-2 conv (csrc/conv_tile3.hip, conv_tile3d_kernel: a lane's B
operand loaded straight from global memory into registers and split there, no LDS texel stage) against the streaming form
(nlt_conv_tile3_forward, NLT_CONV_K2S2) on the same packed weights.  Per output element the two add the same terms in the same
order, so the whole `out` buffer -- its guard bands and the gaps of ldo > cout included -- has to be the same BITS; against float64
at the bar tests/test_gpu_tile3w_s2.py applies to its stride-2 output (the incumbent's own error on the same inputs, x 2); and
what the form does not take is refused with its status code and nothing written."""
import numpy as np
import pytest
import torch

from nlt_amd import capi as C
from oracle import tf_ops as T
from gpu_util import rel_l2

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
PAD = 64                                                                  # floats of guard band on either side of `out`
# (h, w, frames, kobs): one output texel; less than one 8 x 16 tile both ways; exactly one tile; one tile + a one-row, one-column
# rim of partial tiles; frame index arithmetic (observation pairs share a weight slab).  And the other two weight-sharing depths:
# kobs = 4 (four frames per slab at 32 channels per workgroup) and kobs = 3 (none: three passes over the weights per tile)
SHAPES = [(2, 2, 1, 1), (4, 16, 1, 1), (16, 32, 1, 1), (18, 34, 1, 1), (6, 24, 3, 2), (6, 24, 2, 4), (4, 16, 1, 3)]
# (cin, cout, tn): cin 16 / 64 / 128; cout 32 at tn 32, 64, 128 (two groups), 256 (four groups); two groups at tn 32
CHANNELS = [(16, 32, 32), (64, 64, 64), (128, 128, 64), (64, 256, 64), (16, 64, 32), (128, 32, 32)]
_cache = {}


def operands(h, w, frames, kobs, cin, cout):
    """Inputs (ld = cin + 16) and weights, once per case on the CPU; the float64 pre-activation conv on demand."""
    key = (h, w, frames, kobs, cin, cout)
    if key not in _cache:
        rng = np.random.default_rng(h * 131 + w * 7 + frames * 3 + kobs + cin * 17 + cout)
        R = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
        _cache[key] = dict(src=R(frames * kobs, h, w, cin + 16), wk=R(2, 2, cin, cout) * (1.0 / np.sqrt(4 * cin)), bias=R(cout) * 0.1)
    return _cache[key]


def run(fn, o, h, w, frames, kobs, cin, cout, tn, nprod, act):
    """`out` (ldo = cout + 8) in the middle of a sentinel-filled buffer; returns the whole buffer and the view."""
    ldo, n = cout + 8, frames * kobs * (h // 2) * (w // 2)
    buf = torch.full((PAD + n * ldo + PAD,), SENTINEL, device='cuda')
    out = buf[PAD:PAD + n * ldo].view(frames * kobs, h // 2, w // 2, ldo)
    packed = C.pack_conv_tile3_weights(C.CONV_K2S2, o['wk'].cuda(), cin, cout, tn)
    fn(C.CONV_K2S2, o['src'].cuda(), cin + 16, cin, frames, kobs, h, w, packed, o['bias'].cuda(), cout, tn, out, ldo, None, 0,
       act=act, alpha=0.3, nprod=nprod)
    torch.cuda.synchronize()
    return buf, out


@pytest.mark.parametrize('nprod', [6, 9])
@pytest.mark.parametrize('cin,cout,tn', CHANNELS)
@pytest.mark.parametrize('h,w,frames,kobs', SHAPES)
def test_direct_form_gives_the_streaming_forms_bits(h, w, frames, kobs, cin, cout, tn, nprod):
    o = operands(h, w, frames, kobs, cin, cout)
    for act in (True, False):
        want, want_out = run(C.conv_tile3_forward, o, h, w, frames, kobs, cin, cout, tn, nprod, act)
        got, got_out = run(C.conv_tile3d_forward, o, h, w, frames, kobs, cin, cout, tn, nprod, act)
        assert not (want_out[..., :cout] == SENTINEL).any()
        assert (got[:PAD] == SENTINEL).all() and (got[-PAD:] == SENTINEL).all() and (got_out[..., cout:] == SENTINEL).all()
        assert torch.equal(got, want), (act, int((got != want).sum()))


@pytest.mark.parametrize('nprod', [6, 9])
@pytest.mark.parametrize('h,w,frames,kobs,cin,cout,tn', [(18, 34, 1, 1, 64, 64, 64), (6, 24, 3, 2, 128, 128, 64), (16, 32, 1, 1, 16, 32, 32)])
def test_direct_form_vs_float64(h, w, frames, kobs, cin, cout, tn, nprod):
    """Max-abs and rel-L2 distance to the conv evaluated in float64, with the streaming kernel's own distances on the same inputs
    as the yardstick, x 2 (every term product is exact in both)."""
    o = operands(h, w, frames, kobs, cin, cout)
    with torch.no_grad():
        ref = T.leaky_relu(T.conv2d_same(o['src'][..., :cin].double().contiguous(), o['wk'].double(), o['bias'].double(), 2), 0.3)
    errs = lambda t: (float((t[..., :cout].cpu().double() - ref).abs().max()), rel_l2(t[..., :cout].cpu(), ref))
    ma_s, rl_s = errs(run(C.conv_tile3_forward, o, h, w, frames, kobs, cin, cout, tn, nprod, True)[1])
    ma_d, rl_d = errs(run(C.conv_tile3d_forward, o, h, w, frames, kobs, cin, cout, tn, nprod, True)[1])
    print("tile3d %dx%d frames %d k %d %d->%d nprod %d: max-abs %.3e rel-L2 %.3e (streaming %.3e %.3e)"
          % (h, w, frames, kobs, cin, cout, nprod, ma_d, rl_d, ma_s, rl_s))
    assert rl_s < 1e-5                                                       # (the yardstick itself is a conv of these inputs)
    assert ma_d <= 2 * ma_s and rl_d <= 2 * rl_s, (ma_d, ma_s, rl_d, rl_s)


def test_refusals_return_their_status_and_launch_nothing():
    """NLT_ERR_UNSUPPORTED (-2): the stride-1 conv, an odd h, an odd w, a mean_out request, nprod = 3.  NLT_ERR_BAD_ARG (-1): a
    source pointer that is not 16-byte aligned.  Every output untouched."""
    cin, cout, tn, h, w = 16, 32, 32, 4, 16
    src = torch.zeros(1 * (h + 1) * (w + 1) * cin + 4, device='cuda')
    packed = C.pack_conv_tile3_weights(C.CONV_K2S2, torch.ones(2, 2, cin, cout, device='cuda'), cin, cout, tn)
    packed1 = C.pack_conv_tile3_weights(C.CONV_K2S1, torch.ones(2, 2, cin, cout, device='cuda'), cin, cout, tn)
    bias = torch.ones(cout, device='cuda')
    out = torch.full((1, h, w, cout), SENTINEL, device='cuda')                # (room for the stride-1 conv's map too)
    mean = torch.full((1, h, w, cout), SENTINEL, device='cuda')

    def call(mode=C.CONV_K2S2, s=src, hh=h, ww=w, pk=packed, mean_out=None, nprod=9):
        C.conv_tile3d_forward(mode, s, cin, cin, 1, 1, hh, ww, pk, bias, cout, tn, out, cout, mean_out, cout if mean_out is not None else 0,
                              nprod=nprod)
    for kw in (dict(mode=C.CONV_K2S1, pk=packed1), dict(hh=h + 1), dict(ww=w + 1), dict(mean_out=mean), dict(nprod=3)):
        with pytest.raises(C.NLTError, match=r'unsupported.*\(-2\)'):
            call(**kw)
    with pytest.raises(C.NLTError, match=r'bad argument.*\(-1\)'):
        call(s=src[1:])
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (mean == SENTINEL).all()
    call()                                                                    # (the same arguments without a fault are taken)
    torch.cuda.synchronize()
    n = (h // 2) * (w // 2) * cout
    assert not (out.view(-1)[:n] == SENTINEL).any() and (out.view(-1)[n:] == SENTINEL).all() and (mean == SENTINEL).all()
