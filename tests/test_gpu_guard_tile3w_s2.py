"""-m gpu: guard bands (tests/guard_util.py) around every buffer of the level hand-off launch, C.conv_tile3w_s2_forward
(csrc/conv_tile3.hip, conv_tile3w_s2_kernel), and its pack C.pack_conv_tile3w_s2_weights: the texel source as a channel slice of
wider rows, both packed weight sets, both biases, the observation mean into the upper half of an interleaved map and the
stride-2 output in padded rows -- one case per shape of tests/test_gpu_tile3w_s2.py, under the three fills.  Nothing outside the
payloads may change, no fill value may reach a result, and the results are the bits of the run on plain tensors."""
import numpy as np
import pytest
import torch

from nlt_amd import capi as C
import guard_util as G
from gpu_util import rel_l2
from test_gpu_tile3w_s2 import operands, SHAPES, CIN, C1, C2

pytestmark = pytest.mark.gpu
PAD = 8


@pytest.mark.parametrize('h,w,frames,kobs,max_wg', SHAPES)
def test_conv_tile3w_s2_forward(monkeypatch, h, w, frames, kobs, max_wg):
    o = operands(h, w, frames, kobs)
    p1 = C.pack_conv_tile3_weights(C.CONV_K2S1, o['w1'].cuda(), CIN, C1, 32)
    p2 = C.pack_conv_tile3w_s2_weights(o['w2'].cuda(), C1, C2)
    torch.cuda.synchronize()
    old_mean = torch.from_numpy(np.random.default_rng(5).standard_normal((frames, h, w, 2 * C1)).astype(np.float32))
    ins = {'src': dict(data=o['src'][..., :CIN], ld=CIN + PAD), 'p1': p1.cpu(), 'p2': p2.cpu(), 'b1': o['b1'], 'b2': o['b2']}
    outs = {'mean': old_mean, 'out2': dict(shape=(frames * kobs, h // 2, w // 2, C2), ld=C2 + PAD)}

    def call(t):
        C.conv_tile3w_s2_forward(t['src'], CIN + PAD, CIN, frames, kobs, h, w, t['p1'], t['b1'], C1, t['mean'].view(-1)[C1:], 2 * C1,
                                 t['p2'], t['b2'], C2, t['out2'], C2 + PAD, nprod=9, max_workgroups=max_wg)
    res, _, want = G.bitwise_case(monkeypatch, call, ins, outs)
    assert torch.equal(res[0]['mean'][..., :C1], old_mean[..., :C1]), "the query half of the interleaved map was written"
    assert rel_l2(res[0]['mean'][..., C1:], o['mean64']) < 1e-5 and rel_l2(res[0]['out2'], o['y2']) < 1e-5


def test_pack_conv_tile3w_s2_weights(monkeypatch):
    """The pack launch writes exactly its nlt_conv_tile3w_s2_packed_elems() elements, the same under every fill."""
    o = operands(4, 16, 1, 1)
    res, _, want = G.bitwise_case(monkeypatch, lambda t: C.pack_conv_tile3w_s2_weights(t['w'], C1, C2), {'w': o['w2']})
    assert want['ret'].numel() == 12 * C1 * C2 and want['ret'].dtype == torch.int16
