"""-m gpu: nlt_conv_bf16_forward_map (csrc/conv_bf16.hip) -- the bf16-region conv with a per-output-texel fp32 map added in
its epilogue, the per-frame half of a conv over concat(query, GIVEN observation map) under `precision = bf16`
(nlt/nlt_test.py:78-94, nlt/models/nlt.py:172-174).

Two references.  (a) The kernel's own unfused sequence: with an fp32 output, act((acc + bias) + map) must be BIT-EQUAL to
nlt_conv_bf16_forward(act = 0, fp32 out) followed by "+ map" and LeakyReLU in torch on the device (same kernel, same
accumulation order, the add order is fixed).  (b) The operand oracle: round_bf16(leaky(conv(round_bf16([x | given]),
round_bf16(W_full), bias))) with the map = the given channels' share + bias in fp32 -- tests/test_gpu_bf16.py's bars: rel-L2
<= 5e-3, fewer than 2 % of the elements off, each by at most one bf16 ulp (2^-7 relative); a float64-accumulating emulation of
the split sits at <= 0.033 % / 0.0066."""
import numpy as np
import pytest
import torch

from nlt_amd import capi as C
from oracle import nlt_oracle as O
from oracle import tf_ops as T
from gpu_util import rel_l2

pytestmark = pytest.mark.gpu
ALPHA = 0.3
GIVEN = 32                                                   # channels of the given map behind the per-frame sources
BF = torch.bfloat16

# mode, c0, c1, cout, n, h, w, src0 fp32?, ld0, ld1, both sources the same tensor?
CASES = [
    pytest.param(C.CONV_K2S2, 32, 0, 64, 2, 8, 12, True, 64, 0, False, id='level3-f32src-ld64'),
    pytest.param(C.CONV_K2S2, 64, 0, 128, 3, 4, 6, False, 64, 0, False, id='c2s2-64-128'),
    pytest.param(C.DECONV_K2S2, 128, 128, 64, 2, 3, 5, False, 128, 128, True, id='bottleneck-same-tensor-twice'),
    pytest.param(C.DECONV_K2S2, 32, 64, 16, 1, 8, 12, False, 32, 128, False, id='d2s2-32+64-ld128'),
    pytest.param(C.DECONV_K2S2, 256, 0, 128, 3, 2, 2, False, 256, 0, False, id='d2s2-fewer-rows-than-a-tile'),
]
HINTS = (17, 18, 33, 34, 36, 66, 68)                         # 16 * RT + CT of every wave tile launch_mode instantiates


def _leaky(v):
    return torch.where(v > 0, v, ALPHA * v)


def _rows(wk, tr, lo, hi):
    return (wk[..., lo:hi] if tr else wk[:, :, lo:hi, :]).contiguous()


class Case:
    """Inputs of one row of CASES on the device, and its operand-oracle result for `frames` given maps."""

    def __init__(self, mode, c0, c1, cout, n, h, w, f32_in, ld0, ld1, same, frames):
        self.mode, self.c0, self.c1, self.cout, self.n, self.h, self.w = mode, c0, c1, cout, n, h, w
        self.ld0, self.ld1 = ld0, ld1
        rng = np.random.default_rng(c0 + h)
        rb = O.round_bf16
        tr = self.tr = mode == C.DECONV_K2S2
        R = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32))
        x0 = R(n, h, w, ld0)                                 # (channels past c0: never part of the conv)
        x1 = x0 if same else (R(n, h, w, ld1) if c1 else None)
        given = R(frames, h, w, GIVEN)
        cq = c0 + c1
        cin = cq + GIVEN
        self.wk = torch.from_numpy(T.glorot_uniform(rng, (2, 2, cout, cin) if tr else (2, 2, cin, cout)))
        self.bias = torch.from_numpy(rng.uniform(-0.1, 0.1, cout).astype(np.float32))
        conv = T.conv2d_transpose_same if tr else T.conv2d_same
        xq = torch.cat((x0[..., :c0], x1[..., :c1]), 3) if c1 else x0[..., :c0]
        full = rb(torch.cat((xq, given.expand(n, -1, -1, -1)), 3))
        self.ref = rb(_leaky(conv(full, rb(self.wk), self.bias, 2)))
        # the given channels' share + bias, fp32: what the plan hands the kernel as its map
        self.map = conv(rb(given), rb(_rows(self.wk, tr, cq, cin)), self.bias, 2).contiguous().cuda()
        self.oh, self.ow = self.ref.shape[1:3]
        self.src0 = (x0 if f32_in else x0.to(BF)).cuda().contiguous()
        self.src1 = self.src0 if same else (x1.to(BF).cuda().contiguous() if c1 else None)
        self.packed = C.conv_bf16_pack(mode, _rows(self.wk, tr, 0, cq).cuda(), c0, c1, cout)
        self.zero = torch.zeros(cout, device='cuda')

    def srcs(self):
        return (self.src0, self.c0, self.ld0, self.src1, self.c1, self.ld1, self.n, self.h, self.w)

    def out(self, dtype):
        return torch.full((self.n, self.oh, self.ow, self.cout), float('nan'), device='cuda', dtype=dtype)


@pytest.mark.parametrize('per_frame', [False, True], ids=['map_frames=1', 'map_frames=n'])
@pytest.mark.parametrize('mode,c0,c1,cout,n,h,w,f32_in,ld0,ld1,same', CASES)
def test_fp32_out_is_bit_equal_to_the_unfused_sequence(mode, c0, c1, cout, n, h, w, f32_in, ld0, ld1, same, per_frame):
    k = Case(mode, c0, c1, cout, n, h, w, f32_in, ld0, ld1, same, n if per_frame else 1)
    bias = k.bias.cuda()
    pre = k.out(torch.float32)
    C.conv_bf16_forward(mode, *k.srcs(), k.packed, bias, cout, pre, cout, act=False)
    want = _leaky(pre + k.map)                               # (acc + bias) + map, then LeakyReLU
    got = k.out(torch.float32)
    C.conv_bf16_forward_map(mode, *k.srcs(), k.packed, bias, cout, got, cout, k.map, act=True, alpha=ALPHA)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(got, want)
    lin = k.out(torch.float32)                               # act = 0: the sum itself
    C.conv_bf16_forward_map(mode, *k.srcs(), k.packed, bias, cout, lin, cout, k.map, act=False)
    torch.cuda.synchronize()
    assert torch.equal(lin, pre + k.map)


@pytest.mark.parametrize('per_frame', [False, True], ids=['map_frames=1', 'map_frames=n'])
@pytest.mark.parametrize('mode,c0,c1,cout,n,h,w,f32_in,ld0,ld1,same', CASES)
def test_bf16_out_matches_the_bf16_operand_oracle_of_the_full_concat(mode, c0, c1, cout, n, h, w, f32_in, ld0, ld1, same, per_frame):
    k = Case(mode, c0, c1, cout, n, h, w, f32_in, ld0, ld1, same, n if per_frame else 1)
    out = k.out(BF)
    C.conv_bf16_forward_map(mode, *k.srcs(), k.packed, k.zero, cout, out, cout, k.map, act=True, alpha=ALPHA)
    torch.cuda.synchronize()
    got = out.float().cpu()
    bad = got != k.ref
    e, share = rel_l2(got, k.ref), float(bad.float().mean())
    worst = float(((got - k.ref).abs() / k.ref.abs().clamp_min(1e-20))[bad].max() if bad.any() else 0.0)
    print("conv_bf16_forward_map vs operand oracle: rel-L2 %.2e, %.4f %% of the elements off, worst %.4f relative" % (e, 100 * share, worst))
    assert e <= 5e-3 and share < 0.02 and worst <= 2 ** -7


@pytest.mark.parametrize('mode,c0,c1,cout,n,h,w,f32_in,ld0,ld1,same', [CASES[0], CASES[2], CASES[3]])
def test_every_wave_tile_gives_the_same_bits(mode, c0, c1, cout, n, h, w, f32_in, ld0, ld1, same):
    """fp32-out form under every wave-tile hint the launcher accepts for this many 16-column tiles; M is no multiple of
    16 * RT here, so the clamped tail rows run."""
    k = Case(mode, c0, c1, cout, n, h, w, f32_in, ld0, ld1, same, n)
    bias = k.bias.cuda()
    ntiles = ((4 if k.tr else 1) * cout + 15) // 16
    M = n * (h * w // 4 if mode == C.CONV_K2S2 else h * w)
    hints = [t for t in HINTS if ntiles % (t & 15) == 0]
    assert len(hints) == len(HINTS) and any(M % (16 * (t >> 4)) for t in hints)
    first = None
    for hint in (0,) + tuple(hints):
        got = k.out(torch.float32)
        C.conv_bf16_forward_map(mode, *k.srcs(), k.packed, bias, cout, got, cout, k.map, act=True, alpha=ALPHA, tile_hint=hint)
        torch.cuda.synchronize()
        first = got if first is None else first
        assert torch.isfinite(got).all() and torch.equal(got, first), hint
    with pytest.raises(C.NLTError):                          # a CT that does not divide the column tiles is refused, not run
        C.conv_bf16_forward_map(mode, *k.srcs(), k.packed, bias, cout, k.out(torch.float32), cout, k.map, tile_hint=16 + 3)


@pytest.mark.parametrize('mode,c,cout,h,w,twice', [(C.CONV_K2S2, 32, 64, 8, 12, False), (C.DECONV_K2S2, 64, 32, 3, 5, True),
                                                   (C.DECONV_K2S2, 128, 64, 6, 10, False)])
def test_the_map_builders_form_fp32_source_no_activation_fp32_out(mode, c, cout, h, w, twice):
    """conv_bf16_forward with act = 0 and an fp32 output on an fp32 source (one [1,h,w,c] map; `twice`: as both sources of a
    two-group conv, the bottleneck's form) -- how the override maps of the bf16 region are made: fp32 summation order only."""
    rng = np.random.default_rng(c + h)
    rb = O.round_bf16
    tr = mode == C.DECONV_K2S2
    cin = 2 * c if twice else c
    x = torch.from_numpy(rng.standard_normal((1, h, w, c), dtype=np.float32))
    wk = torch.from_numpy(T.glorot_uniform(rng, (2, 2, cout, cin) if tr else (2, 2, cin, cout)))
    bias = torch.from_numpy(rng.uniform(-0.1, 0.1, cout).astype(np.float32))
    ref = (T.conv2d_transpose_same if tr else T.conv2d_same)(rb(torch.cat((x, x), 3) if twice else x), rb(wk), bias, 2)
    out = torch.full(tuple(ref.shape), float('nan'), device='cuda')
    xd = x.cuda()
    c1 = c if twice else 0
    C.conv_bf16_forward(mode, xd, c, c, xd if twice else None, c1, c1, 1, h, w, C.conv_bf16_pack(mode, wk.cuda(), c, c1, cout),
                        bias.cuda(), cout, out, cout, act=False, alpha=0.0)
    torch.cuda.synchronize()
    assert rel_l2(out.cpu(), ref) <= 2e-6
