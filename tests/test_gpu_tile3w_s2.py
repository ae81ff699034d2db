"""-m gpu: csrc/conv_tile3.hip, conv_tile3w_s2_kernel -- the wave-private stride-1 conv (32 -> 32) of a level and the next level's
stride-2 conv (32 -> 64) per observation in one launch, the stride-1 results handed over in registers.

  * the observation-mean slice is the BITS nlt_conv_tile3r_forward's wave-private form writes (interleaved ldm);
  * the stride-2 output against a float64 evaluation of both convs, with the unfused sequence (wave-private stride-1, then the
    resident stride-2 launch with the same number of term products) as the yardstick: its own max-abs and rel-L2 error on the same
    inputs, measured here, times 2 (every product is exact in both; only the fp32 summation order differs);
  * two runs agree bit for bit; what the kernel does not take is refused with nothing written;
  * the permuted stride-2 pack is refreshed by the one-launch repack like every other derived buffer.
"""
import numpy as np
import pytest
import torch

from nlt_amd import capi as C
from nlt_amd.networks.elements import Conv2D, PackRegistry
from oracle import tf_ops as T
from gpu_util import rel_l2

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
CIN, C1, C2, LD = 32, 32, 64, 40
# (h, w, frames, kobs, max_workgroups of the second run): one 4 x 16 tile; a partial tile in x and y; more items (48) than the 16
# waves of two workgroups; fewer items (6) than waves, four workgroups cut mid-run
SHAPES = [(4, 16, 1, 1, 1), (6, 24, 2, 3, 1), (32, 48, 2, 4, 2), (10, 18, 1, 4, 4)]
_cache = {}


def operands(h, w, frames, kobs):
    """Inputs, weights and the float64 evaluation of both convs, once per shape."""
    key = (h, w, frames, kobs)
    if key not in _cache:
        rng = np.random.default_rng(h * 131 + w * 7 + frames + kobs)
        R = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
        src = R(frames * kobs, h, w, LD)
        w1, b1 = R(2, 2, CIN, C1) * (1.0 / np.sqrt(4 * CIN)), R(C1) * 0.1
        w2, b2 = R(2, 2, C1, C2) * (1.0 / np.sqrt(4 * C1)), R(C2) * 0.1
        with torch.no_grad():
            y1 = T.leaky_relu(T.conv2d_same(src[..., :CIN].double().contiguous(), w1.double(), b1.double(), 1), 0.3)
            y2 = T.leaky_relu(T.conv2d_same(y1, w2.double(), b2.double(), 2), 0.3)
        _cache[key] = dict(src=src, w1=w1, b1=b1, w2=w2, b2=b2, mean64=y1.reshape(frames, kobs, h, w, C1).mean(1), y2=y2)
    return _cache[key]


def fused(o, h, w, frames, kobs, nprod, max_wg=0, **kw):
    dev = lambda t: t.cuda()
    mean = torch.full((frames, h, w, 2 * C1), SENTINEL, device='cuda')
    out2 = torch.full((frames * kobs, h // 2, w // 2, C2 + 4), SENTINEL, device='cuda')
    C.conv_tile3w_s2_forward(dev(o['src']), LD, CIN, frames, kobs, h, w,
                             C.pack_conv_tile3_weights(C.CONV_K2S1, dev(o['w1']), CIN, C1, 32), dev(o['b1']), C1,
                             mean.view(-1)[C1:], 2 * C1, C.pack_conv_tile3w_s2_weights(dev(o['w2']), C1, C2), dev(o['b2']), C2,
                             out2, C2 + 4, nprod=nprod, max_workgroups=max_wg, **kw)
    torch.cuda.synchronize()
    return mean, out2


def unfused(o, h, w, frames, kobs, nprod):
    dev = lambda t: t.cuda()
    mean = torch.full((frames, h, w, 2 * C1), SENTINEL, device='cuda')
    y1 = torch.empty((frames * kobs, h, w, C1), device='cuda')
    out2 = torch.full((frames * kobs, h // 2, w // 2, C2 + 4), SENTINEL, device='cuda')
    assert C.conv_tile3r_plan(C.CONV_K2S1, CIN, 32)[3] == 4                 # the wave-private form, 4-row tiles
    C.conv_tile3r_forward(C.CONV_K2S1, dev(o['src']), LD, CIN, frames, kobs, h, w,
                          C.pack_conv_tile3_weights(C.CONV_K2S1, dev(o['w1']), CIN, C1, 32), dev(o['b1']), C1, 32, y1, C1,
                          mean.view(-1)[C1:], 2 * C1, nprod=nprod)
    C.conv_tile3r_forward(C.CONV_K2S2, y1, C1, C1, frames * kobs, 1, h, w,
                          C.pack_conv_tile3_weights(C.CONV_K2S2, dev(o['w2']), C1, C2, 64), dev(o['b2']), C2, 64, out2, C2 + 4,
                          None, 0, nprod=nprod)
    torch.cuda.synchronize()
    return mean, out2


@pytest.mark.parametrize('nprod', [6, 9])
@pytest.mark.parametrize('h,w,frames,kobs,max_wg', SHAPES)
def test_mean_bits_stride2_error_and_repeatability(h, w, frames, kobs, max_wg, nprod):
    o = operands(h, w, frames, kobs)
    mean_u, out_u = unfused(o, h, w, frames, kobs, nprod)
    ref = o['y2']
    errs = lambda t: (float((t[..., :C2].cpu().double() - ref).abs().max()), rel_l2(t[..., :C2].cpu(), ref))
    ma_u, rl_u = errs(out_u)
    assert not (mean_u[..., C1:] == SENTINEL).any() and rel_l2(mean_u[..., C1:].cpu(), o['mean64']) < 1e-5
    for wg in (0, max_wg):
        mean_f, out_f = fused(o, h, w, frames, kobs, nprod, wg)
        assert torch.equal(mean_f, mean_u), (wg, int((mean_f != mean_u).sum()))      # (whole map: the query half stays untouched)
        assert (out_f[..., C2:] == SENTINEL).all() and not (out_f[..., :C2] == SENTINEL).any()
        ma_f, rl_f = errs(out_f)
        print("tile3w_s2 %dx%d frames %d k %d nprod %d max_wg %d: max-abs %.3e rel-L2 %.3e (unfused %.3e %.3e)"
              % (h, w, frames, kobs, nprod, wg, ma_f, rl_f, ma_u, rl_u))
        assert ma_f <= 2 * ma_u and rl_f <= 2 * rl_u, (ma_f, ma_u, rl_f, rl_u)
        mean_g, out_g = fused(o, h, w, frames, kobs, nprod, wg)
        assert torch.equal(mean_g, mean_f) and torch.equal(out_g, out_f)


def test_refusals_launch_nothing():
    """cin = 64, an odd h, and a caller that wants the stride-1 map: NLT_ERR_UNSUPPORTED, every output untouched."""
    h, w = 4, 16
    o = operands(h, w, 1, 1)
    dev = lambda t: t.cuda()
    p1 = C.pack_conv_tile3_weights(C.CONV_K2S1, dev(o['w1']), CIN, C1, 32)
    p2 = C.pack_conv_tile3w_s2_weights(dev(o['w2']), C1, C2)
    mean = torch.full((1, h, w, C1), SENTINEL, device='cuda')
    out2 = torch.full((1, h // 2, w // 2, C2), SENTINEL, device='cuda')
    y1 = torch.full((1, h, w, C1), SENTINEL, device='cuda')
    src = torch.zeros((1, h + 1, w, 64), device='cuda')
    args = lambda **kw: dict(dict(src=src, ld=64, cin=CIN, h=h, out=None), **kw)
    for kw in (args(cin=64), args(h=h + 1), args(out=y1)):
        with pytest.raises(C.NLTError, match='unsupported'):
            C.conv_tile3w_s2_forward(kw['src'], kw['ld'], kw['cin'], 1, 1, kw['h'], w, p1, dev(o['b1']), C1, mean, C1, p2, dev(o['b2']), C2,
                                     out2, C2, nprod=9, out=kw['out'], ldo=C1)
    with pytest.raises(C.NLTError, match='unsupported'):
        C.pack_conv_tile3w_s2_weights(torch.zeros(2, 2, 64, 64, device='cuda'), 64, 64)
    assert C.conv_tile3w_s2_plan(64, 32, 64) is None and C.conv_tile3w_s2_plan(32, 32, 128) is None
    assert C.conv_tile3w_s2_plan(32, 32, 64) <= 160 * 1024
    torch.cuda.synchronize()
    assert (mean == SENTINEL).all() and (out2 == SENTINEL).all() and (y1 == SENTINEL).all()


def test_registry_refreshes_the_permuted_pack_after_the_kernel_changes():
    """In the manner of tests/test_gpu_repack.py: an in-place weight change, then the one-launch refresh -- the same buffer, the
    bits of a fresh pack; unused under a census it goes inactive and comes back fresh when asked for."""
    conv = Conv2D(C2, 2, 2)
    conv.build(C1, 'cuda', seed=3)
    reg = conv._registry = PackRegistry()
    a, s = conv.packed(C1, 0), conv.packed_tile3s2()
    assert s.dtype == torch.int16 and s.numel() == 12 * C1 * C2
    assert torch.equal(s, C.pack_conv_tile3w_s2_weights(conv.kernel.detach(), C1, C2))
    ptr = s.data_ptr()
    with torch.no_grad():
        conv.kernel.mul_(-2.0)                                            # an "optimizer step"
    conv.packed(C1, 0)                                                    # first stale access: ONE launch refreshes both
    s2 = conv.packed_tile3s2()
    torch.cuda.synchronize()
    assert s2.data_ptr() == ptr and torch.equal(s2, C.pack_conv_tile3w_s2_weights(conv.kernel.detach(), C1, C2))
    reg.begin_census(passes=1)
    reg.tick(); conv.packed(C1, 0); reg.tick()                            # a pass that never asks for the permuted pack
    assert reg.is_inactive(conv, ('tile3s2',)) and not reg.is_inactive(conv, (C1, 0))
    with torch.no_grad():
        conv.kernel.add_(0.5)
    reg.refresh()                                                         # skips the inactive buffer
    s3 = conv.packed_tile3s2()                                            # asked for again: re-activated, re-packed in place
    torch.cuda.synchronize()
    assert s3.data_ptr() == ptr and not reg.is_inactive(conv, ('tile3s2',))
    assert torch.equal(s3, C.pack_conv_tile3w_s2_weights(conv.kernel.detach(), C1, C2)) and a.data_ptr() == conv.packed(C1, 0).data_ptr()
