"""CPU: the reference the 3x3 kernels are held to (tests/conv_k3_ref.py).  The adjoint-defined transposed conv equals the
float64 index-formula loops for k3 s1 / s2 and equals oracle.tf_ops.conv2d_transpose_same for k2 (there the definition IS
that function); at k3 s1 it differs from the oracle's, which crops the wrong ring.  The conv form equals the oracle's loops."""
import numpy as np
import pytest
import torch

from oracle import tf_ops as T
import conv_k3_ref as R


def _data(n, h, w, cin, cout, k, transpose, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, cin, generator=g, dtype=torch.float64)
    wk = torch.randn((k, k, cout, cin) if transpose else (k, k, cin, cout), generator=g, dtype=torch.float64)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    return x, wk, b


@pytest.mark.parametrize('stride,h,w', [(1, 5, 7), (1, 2, 2), (2, 3, 5), (2, 1, 1), (2, 4, 2)])
def test_adjoint_transposed_conv_equals_naive_k3(stride, h, w):
    x, wk, b = _data(2, h, w, 3, 4, 3, True, 10 * stride + h)
    got = R.conv2d_transpose_same(x, wk, b, stride).detach().numpy()
    ref = R.deconv3_naive(x.numpy(), wk.numpy(), b.numpy(), stride)
    assert got.shape == ref.shape == (2, h * stride, w * stride, 4)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize('stride', [1, 2])
def test_adjoint_transposed_conv_equals_oracle_k2(stride):
    x, wk, b = _data(2, 4, 6, 3, 5, 2, True, stride)
    got = R.conv2d_transpose_same(x, wk, b, stride).detach()
    ref = T.conv2d_transpose_same(x, wk, b, stride)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert np.abs(got.numpy() - T.conv2d_transpose_same_naive(x.numpy(), wk.numpy(), b.numpy(), stride)).max() <= 1e-12 * float(ref.abs().max())


def test_oracle_transposed_conv_is_wrong_at_k3_s1_and_right_at_k3_s2():
    x, wk, b = _data(1, 6, 6, 4, 4, 3, True, 7)
    mine = R.conv2d_transpose_same(x, wk, b, 1).detach()
    assert float((mine - T.conv2d_transpose_same(x, wk, b, 1)).abs().max()) > 0.1 * float(mine.abs().max())
    mine2 = R.conv2d_transpose_same(x, wk, b, 2).detach()
    assert float((mine2 - T.conv2d_transpose_same(x, wk, b, 2)).abs().max()) <= 1e-12 * float(mine2.abs().max())


@pytest.mark.parametrize('stride,h,w', [(1, 5, 7), (1, 2, 2), (2, 6, 10), (2, 2, 2)])
def test_conv_form_equals_oracle_naive_and_formula(stride, h, w):
    x, wk, b = _data(2, h, w, 3, 4, 3, False, 3 * stride + w)
    got = R.conv2d_same(x, wk, b, stride).numpy()
    ref = T.conv2d_same_naive(x.numpy(), wk.numpy(), b.numpy(), stride)
    mine = R.conv3_naive(x.numpy(), wk.numpy(), b.numpy(), stride)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max() and np.abs(mine - ref).max() <= 1e-12 * np.abs(ref).max()


def test_adjoint_form_is_differentiable_in_all_arguments():
    x, wk, b = _data(1, 3, 4, 2, 3, 3, True, 5)
    x.requires_grad_(True); wk.requires_grad_(True); b.requires_grad_(True)
    g = torch.randn(1, 3, 4, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    dx, dw, db = torch.autograd.grad(R.conv2d_transpose_same(x, wk, b, 1), (x, wk, b), g)
    # backward-data of the transposed conv is the conv of the same stride on the same array
    assert float((dx - T.conv2d_same(g, wk.detach(), None, 1)).abs().max()) <= 1e-12 * float(dx.abs().max())
    assert float((db - g.sum((0, 1, 2))).abs().max()) <= 1e-12 and dw.shape == wk.shape
