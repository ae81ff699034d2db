"""TEST-ONLY: tests/fake_capi.py plus CPU emulations of the bf16 region's adapters (csrc/conv_bf16.hip), so the host
orchestration of `precision = bf16` can be verified without a GPU.  Operands are rounded to bf16 (oracle.nlt_oracle.round_bf16:
inputs as stored, weights as packed), the convs are the oracle's fp32 tf_ops, the store is bf16 or fp32 as the output tensor
is -- the arithmetic OracleModel.set_precision('bf16') states, launch by launch.  Never used by the product."""
import torch

from nlt_amd import _capi as C
from oracle import tf_ops as T
from oracle import nlt_oracle as O
import fake_capi
from fake_capi import _MODES, _view


def conv_bf16_pack(mode, w_keras, c0, c1, cout):
    assert c0 > 0 and c0 % 8 == 0 and c1 % 8 == 0 and cout % 4 == 0, (c0, c1, cout)
    tr = _MODES[mode][1]
    assert (w_keras.shape[3] if tr else w_keras.shape[2]) == c0 + c1
    return O.round_bf16(w_keras.detach())                   # "packed" = the rounded Keras kernel itself


def _source(t, n, h, w, c, ld):
    assert t.dtype in (torch.float32, torch.bfloat16) and ld >= c and ld % 8 == 0
    return O.round_bf16(_view(t, n, h, w, c, ld).float())


def _conv(mode, src0, c0, ld0, src1, c1, ld1, n, h, w, w_packed, bias, cout, out, ldo, bias_map, act, alpha):
    x = _source(src0, n, h, w, c0, ld0)
    if c1:
        x = torch.cat((x, _source(src1, n, h, w, c1, ld1)), -1)
    s, tr = _MODES[mode]
    y = (T.conv2d_transpose_same if tr else T.conv2d_same)(x, w_packed, bias[:cout], s)
    if bias_map is not None:
        assert bias_map.dtype == torch.float32 and bias_map.is_contiguous()
        assert tuple(bias_map.shape[1:]) == tuple(y.shape[1:]) and bias_map.shape[0] in (1, n)
        y = y + bias_map                                    # (acc + bias) + map
    if act:
        y = T.leaky_relu(y, alpha)
    assert out.dtype in (torch.float32, torch.bfloat16) and ldo >= cout and ldo % 4 == 0
    _view(out, n, y.shape[1], y.shape[2], cout, ldo).copy_(y)       # (a bf16 destination rounds to nearest even)


def conv_bf16_forward(mode, src0, c0, ld0, src1, c1, ld1, n, h, w, w_packed, bias, cout, out, ldo, act=True, alpha=0.3, tile_hint=0):
    _conv(mode, src0, c0, ld0, src1, c1, ld1, n, h, w, w_packed, bias, cout, out, ldo, None, act, alpha)


def conv_bf16_forward_map(mode, src0, c0, ld0, src1, c1, ld1, n, h, w, w_packed, bias, cout, out, ldo, bias_map,
                          act=True, alpha=0.3, tile_hint=0):
    _conv(mode, src0, c0, ld0, src1, c1, ld1, n, h, w, w_packed, bias, cout, out, ldo, bias_map, act, alpha)


def obs_mean_bf16(obs, n, k, hw, c, out, ldo):
    assert obs.dtype == torch.bfloat16 and out.dtype == torch.bfloat16
    m = obs.float().reshape(n, k, hw, c).sum(1) * (1.0 / k)
    torch.as_strided(out, (n, hw, c), (hw * ldo, ldo, 1)).copy_(m)


_BF16 = ('conv_bf16_pack', 'conv_bf16_forward', 'conv_bf16_forward_map', 'obs_mean_bf16')


def install(monkeypatch):
    """fake_capi.install, then the bf16 region's adapters."""
    fake_capi.install(monkeypatch)
    for name in _BF16:
        monkeypatch.setattr(C, name, globals()[name])
