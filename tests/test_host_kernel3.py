"""CPU: the host side of kernel = 3 -- the layer factory accepts the four 3x3 forms and names their modes, the resolution
bookkeeping, the reference's layer list, the route of a kernel = 3 model (layer by layer, never the fused plan), and what
still refuses."""
import pytest

import nlt_amd
from nlt_amd import capi as C
from nlt_amd.models import get_model_class
from nlt_amd.networks import convnet
from nlt_amd.networks.elements import Act, Conv2D, Identity, Sequential, conv, deconv
from oracle import nlt_oracle as O


@pytest.mark.parametrize('stride,transpose,mode', [(1, False, 'CONV_K3S1'), (2, False, 'CONV_K3S2'),
                                                   (1, True, 'DECONV_K3S1'), (2, True, 'DECONV_K3S2')])
def test_conv2d_constructs_the_four_3x3_forms(stride, transpose, mode):
    l = Conv2D(16, 3, stride, transpose)
    assert l.mode == getattr(C, mode) and l.kernel_size == 3 and not l.is_plain()
    want = (6, 10) if stride == 1 else ((12, 20) if transpose else (3, 5))
    assert l.out_hw(6, 10) == want
    adj = Conv2D.ADJOINT[l.mode]
    assert Conv2D.ADJOINT[adj] == l.mode and adj != l.mode
    assert Conv2D(16, 3, stride, not transpose).mode == adj
    l.build(8, 'cpu')
    assert tuple(l.kernel.shape) == ((3, 3, 16, 8) if transpose else (3, 3, 8, 16)) and tuple(l.bias.shape) == (16,)


def test_new_modes_do_not_renumber_the_old_ones():
    assert (C.CONV1X1, C.CONV_K2S2, C.CONV_K2S1, C.DECONV_K2S2, C.DECONV_K2S1) == (0, 1, 2, 3, 4)
    assert sorted((C.CONV_K3S1, C.CONV_K3S2, C.DECONV_K3S1, C.DECONV_K3S2)) == [5, 6, 7, 8]
    assert Conv2D(16, 2, 1).is_plain() and Conv2D(16, 1, 1).is_plain()


def test_network_has_the_references_layer_list():
    net = convnet.Network(16, 32, 3, 2)
    layers, is_c, changes = O.build_layers(16, 32, 3, 2)
    assert net.is_contracting == is_c and [float(c) for c in net.spatsize_changes] == [float(c) for c in changes]
    assert len(net.layers) == len(layers)
    for got, want in zip(net.layers, layers):
        if want['kind'] == 'conv1x1':
            assert isinstance(got, Conv2D) and (got.kernel_size, got.stride, got.n_ch_out) == (1, 1, want['n'])
            continue
        assert isinstance(got, Sequential) and not got.is_plain()
        convs = [l for l in got.layers if isinstance(l, Conv2D)]
        assert [(c.kernel_size, c.stride, c.n_ch_out, c.transpose) for c in convs] == \
            [(3, want['s'], want['n'], want['kind'] == 'up'), (3, 1, want['n'], want['kind'] == 'up')]
        assert all(isinstance(l, (Conv2D, Identity, Act)) for l in got.layers)
        assert [(c, a is not None) for c, a in got.convs()] == [(convs[0], True), (convs[1], True)]     # LeakyReLU still fuses


def test_kernel3_model_runs_layer_by_layer():
    pm = get_model_class('nlt')(nlt_amd.make_config(kernel=3, depth=32, uvh=64, uvw=64, imh=32, imw=32))
    assert pm.generic
    assert not get_model_class('nlt')(nlt_amd.make_config(kernel=2, depth=32, uvh=64, uvw=64, imh=32, imw=32)).generic


@pytest.mark.parametrize('precision', ['bf16', 'f32x3', 'f32x3_9'])
def test_kernel3_refuses_other_precisions(precision):
    with pytest.raises(NotImplementedError, match='precision = %s' % precision):
        get_model_class('nlt')(nlt_amd.make_config(kernel=3, depth=32, uvh=64, uvw=64, imh=32, imw=32, precision=precision))


def test_what_still_raises():
    for args in ((16, 4, 1), (16, 4, 2), (16, 5, 1), (16, 1, 2), (16, 3, 3)):
        with pytest.raises(NotImplementedError):
            Conv2D(*args)
    with pytest.raises(NotImplementedError):
        Conv2D(16, 1, 1, transpose=True)
    with pytest.raises(NotImplementedError):
        get_model_class('nlt')(nlt_amd.make_config(kernel=4, depth=32, uvh=64, uvw=64, imh=32, imw=32))
    assert conv(3, 5).mode == C.CONV_K3S1 and deconv(3, 5, stride=2).mode == C.DECONV_K3S2
