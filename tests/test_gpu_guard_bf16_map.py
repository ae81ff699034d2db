"""-m gpu: nlt_conv_bf16_forward_map between guard bands (tests/guard_util.py), like test_gpu_guard_convs.py's
test_conv_bf16_forward: sources and output as channel slices of wider texels (ld + 8: 16-byte row pieces), the map a dense
read-only operand under guard, all three fills -- only the described elements are read or written, and the result is held
to the operand oracle of the full conv over [sources | given] (tests/test_gpu_bf16_map.py)."""
import numpy as np
import pytest
import torch

from nlt_amd import capi as C
from oracle import nlt_oracle as O
from oracle import tf_ops as T
import guard_util as G
from gpu_util import rel_l2

pytestmark = pytest.mark.gpu
GIVEN = 32


@pytest.mark.parametrize('mode,c0,c1,cout,f32_in,hw,frames', [(C.CONV_K2S2, 32, 0, 64, True, (6, 10), 1),
                                                              (C.DECONV_K2S2, 32, 128, 16, False, (5, 7), 3)], ids=str)
def test_conv_bf16_forward_map(monkeypatch, mode, c0, c1, cout, f32_in, hw, frames):
    n, (h, w) = 3, hw
    rng = np.random.default_rng(mode * 1000 + c0)
    rb, bf = O.round_bf16, torch.bfloat16
    tr = mode == C.DECONV_K2S2
    R = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32))
    x0, x1, given = R(n, h, w, c0), (R(n, h, w, c1) if c1 else None), R(frames, h, w, GIVEN)
    cq = c0 + c1
    cin = cq + GIVEN
    wk = torch.from_numpy(T.glorot_uniform(rng, (2, 2, cout, cin) if tr else (2, 2, cin, cout)))
    bias = torch.from_numpy(rng.uniform(-0.1, 0.1, cout).astype(np.float32))
    conv = T.conv2d_transpose_same if tr else T.conv2d_same
    rows = lambda lo, hi: (wk[..., lo:hi] if tr else wk[:, :, lo:hi, :]).contiguous()
    full = rb(torch.cat(((torch.cat((x0, x1), 3) if c1 else x0), given.expand(n, -1, -1, -1)), 3))
    ref = rb(T.leaky_relu(conv(full, rb(wk), bias, 2), 0.3))
    bmap = conv(rb(given), rb(rows(cq, cin)), bias, 2).contiguous()
    packed = C.conv_bf16_pack(mode, rows(0, cq).cuda(), c0, c1, cout)
    torch.cuda.synchronize()
    ops = {'src0': dict(data=x0 if f32_in else x0.to(bf), ld=c0 + 8), 'src1': dict(data=x1.to(bf), ld=c1 + 8) if c1 else None,
           'packed': packed, 'bias': torch.zeros(cout), 'map': bmap,
           'out': dict(shape=tuple(ref.shape), dtype=bf, ld=cout + 8)}

    def call(o):
        C.conv_bf16_forward_map(mode, o['src0'].t, c0, c0 + 8, o['src1'].t if c1 else None, c1, c1 + 8 if c1 else 0, n, h, w,
                                o['packed'].t, o['bias'].t, cout, o['out'].t, cout + 8, o['map'].t, act=True, alpha=0.3)
    res, _ = G.run_case(monkeypatch, call, ops, outputs=('out',))
    got = res[0]['out'].float()
    bad = got != ref
    assert rel_l2(got, ref) <= 5e-3 and float(bad.float().mean()) < 0.02
    assert float(((got - ref).abs() / ref.abs().clamp_min(1e-20))[bad].max() if bad.any() else 0.0) <= 2 ** -7
