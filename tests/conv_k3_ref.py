"""Reference for the 3x3 layers (kernel = 3), TF 'SAME' semantics, Keras layouts.

`oracle.tf_ops.conv2d_transpose_same` crops the full transposed conv to its first h*s rows / columns.  That is the
transpose of the SAME-padded conv for k2 (pad before = 0) and for k3 s2 on even sizes (pad before = 0), and NOT for k3 s1,
whose forward conv pads one row / column BEFORE the image: its transpose crops one at the top / left and one at the bottom /
right.  Here the transposed conv is therefore DEFINED by adjointness to `oracle.tf_ops.conv2d_same`, which is what
Conv2DTranspose(padding='same') is in TF (conv2d_backprop_input of the SAME conv); the float64 loops below restate both
families from their index formulas and cross-check that definition (tests/test_conv_k3_ref.py).
"""
import numpy as np
import torch

from oracle import tf_ops as T


def conv2d_transpose_same(x, w_hwoi, b, stride):
    """x [N,h,w,Cin]; w_hwoi [kh,kw,Cout,Cin] -> [N,h*s,w*s,Cout]: the gradient of conv2d_same(z, w_hwoi, None, s) w.r.t. z
    (z of the output's shape; the array read as a conv kernel maps Cout -> Cin) contracted with x, plus the bias.
    Differentiable in x, w_hwoi and b."""
    n, h, w, _ = x.shape
    cout = w_hwoi.shape[2]
    with torch.enable_grad():
        z = torch.zeros((n, h * stride, w * stride, cout), dtype=x.dtype, requires_grad=True)
        (y,) = torch.autograd.grad(T.conv2d_same(z, w_hwoi, None, stride), z, x, create_graph=True)
    return y if b is None else y + b


def conv2d_same(x, w_hwio, b, stride):
    return T.conv2d_same(x, w_hwio, b, stride)


def conv3_naive(x, w, b, stride):
    """Conv2D k3 from the index formula: s1  y[i,j] = sum x[i+a-1, j+b-1] W[a,b];  s2 (even sizes)  y[i,j] = sum x[2i+a, 2j+b] W[a,b]."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, h, wd, _ = x.shape
    assert w.shape[:2] == (3, 3) and (stride == 1 or (h % 2 == 0 and wd % 2 == 0))
    oh, ow, off = h // stride, wd // stride, (-1 if stride == 1 else 0)
    y = np.zeros((n, oh, ow, w.shape[3]))
    for i in range(oh):
        for j in range(ow):
            for a in range(3):
                for bb in range(3):
                    yi, xi = stride * i + a + off, stride * j + bb + off
                    if 0 <= yi < h and 0 <= xi < wd:
                        y[:, i, j, :] += x[:, yi, xi, :] @ w[a, bb]
    return y + np.asarray(b, np.float64)


def deconv3_naive(x, w, b, stride):
    """Conv2DTranspose k3 from the index formula: s1  y[i,j] = sum x[i+1-a, j+1-b] W[a,b]^T;
    s2  y[m,n] = sum over the taps with (m-a), (n-b) even of x[(m-a)/2, (n-b)/2] W[a,b]^T."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, h, wd, _ = x.shape
    assert w.shape[:2] == (3, 3)
    oh, ow = h * stride, wd * stride
    y = np.zeros((n, oh, ow, w.shape[2]))
    for m in range(oh):
        for nn in range(ow):
            for a in range(3):
                for bb in range(3):
                    if stride == 1:
                        yi, xi = m + 1 - a, nn + 1 - bb
                    else:
                        if (m - a) % 2 or (nn - bb) % 2:
                            continue
                        yi, xi = (m - a) // 2, (nn - bb) // 2
                    if 0 <= yi < h and 0 <= xi < wd:
                        y[:, m, nn, :] += x[:, yi, xi, :] @ w[a, bb].T
    return y + np.asarray(b, np.float64)


def layer_f64(x, w, b, stride, transpose):
    """float64 forward of one layer on torch tensors (differentiable): the reference the device kernels are held to."""
    f = conv2d_transpose_same if transpose else T.conv2d_same
    return f(x, w, b, stride)
