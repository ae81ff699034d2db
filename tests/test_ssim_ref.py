"""CPU: the test-side SSIM restatement (tests/ssim_ref.py) against an independent 2-D correlation, its own symmetries and
central differences -- the reference the GPU tests of csrc/ssim.hip stand on."""
import numpy as np
import pytest
import torch

import ssim_ref as R


def test_window_is_the_softmax_of_the_squared_distances():
    g = R.window()
    i = np.arange(11) - 5
    e = np.exp(-(i * i) * 0.5 / 1.5 ** 2)
    np.testing.assert_allclose(g, e / e.sum(), rtol=1e-15)
    # TF builds the 2-D window as a softmax over the 121 sums: the same thing as the outer product
    s = -(i[:, None] ** 2 + i[None, :] ** 2) * 0.5 / 1.5 ** 2
    w2 = np.exp(s) / np.exp(s).sum()
    np.testing.assert_allclose(np.outer(g, g), w2, rtol=1e-14)
    assert R.window(np.float32).dtype == np.float32


def test_separable_filter_equals_scipy_correlate2d():
    from scipy.signal import correlate2d
    rng = np.random.RandomState(0)
    a = rng.uniform(0, 1, (2, 17, 23, 3))
    g = R.window()
    got = R.filter_valid(a, g)
    assert got.shape == (2, 7, 13, 3)
    for f in range(2):
        for c in range(3):
            want = correlate2d(a[f, :, :, c], np.outer(g, g), 'valid')
            assert np.abs(got[f, :, :, c] - want).max() <= 1e-14


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_identical_images_give_exactly_one(dtype):
    x, _ = R.make_pair('near', 2, 14, 19, 3)
    s = R.ssim_np(x, x, 1.0, dtype)
    assert s.dtype == dtype and (s == 1).all()
    assert R.metric_ssim_np(x[0], x[0], 1.0) == 1.0


@pytest.mark.parametrize('kind', R.KINDS)
def test_symmetric_in_its_arguments(kind):
    x, y = R.make_pair(kind, 2, 13, 16, 3)
    a, b = R.ssim_np(x, y, 1.0), R.ssim_np(y, x, 1.0)
    assert np.abs(a - b).max() <= 1e-15
    assert not np.allclose(a[0], a[1])                  # the examples of a batch are different images


def test_torch_version_equals_the_numpy_one_and_small_images_are_refused():
    for kind in R.KINDS:
        x, y = R.make_pair(kind, 2, 12, 15, 3)
        t = R.ssim_torch(torch.from_numpy(x), torch.from_numpy(y), 1.0).numpy()
        assert np.abs(t - R.ssim_np(x, y, 1.0)).max() <= 1e-12
    with pytest.raises(ValueError):
        R.ssim_np(np.zeros((10, 11, 1)), np.zeros((10, 11, 1)), 1.0)
    with pytest.raises(ValueError):
        R.ssim_torch(torch.zeros(1, 11, 10, 1), torch.zeros(1, 11, 10, 1), 1.0)


def test_metric_goes_to_luma_first_and_scales_with_the_dynamic_range():
    x, y = R.make_pair('near', 1, 12, 12, 3)
    def lum(a):
        a = a.astype(np.float64)
        return (0.2126 * a[..., 0] + 0.7152 * a[..., 1] + 0.0722 * a[..., 2]).astype(np.float32)[..., None]
    assert R.metric_ssim_np(x[0], y[0], 1.0) == float(R.ssim_np(lum(x[0]), lum(y[0]), 1.0))
    assert R.metric_ssim_np(x[0, ..., 0], y[0, ..., 0], 1.0) == R.metric_ssim_np(x[0, ..., :1], y[0, ..., :1], 1.0)
    # c1, c2 scale with max_val^2: SSIM of (255 x, 255 y) at max_val 255 is SSIM of (x, y) at max_val 1
    a = R.metric_ssim_np(x[0].astype(np.float64) * 255, y[0].astype(np.float64) * 255, 255.0)
    assert abs(a - R.metric_ssim_np(x[0], y[0], 1.0)) <= 1e-6


def test_torch_gradient_agrees_with_central_differences():
    x, y = R.make_pair('near', 1, 13, 12, 3, seed=3)
    per, d = R.loss_and_unit_grad(x, y, 1.0)
    assert per.shape == (1,) and d.shape == (1, 13, 12, 3)
    y64 = y.astype(np.float64)
    eps = 1e-6
    rng = np.random.RandomState(1)
    idx = [(0, 0, 0, 0), (0, 12, 11, 2), (0, 6, 6, 1)] + [(0, rng.randint(13), rng.randint(12), rng.randint(3)) for _ in range(12)]
    for i in idx:
        yp, ym = y64.copy(), y64.copy()
        yp[i] += eps; ym[i] -= eps
        fd = ((1 - R.ssim_np(x, yp, 1.0)) / 2 - (1 - R.ssim_np(x, ym, 1.0)) / 2)[0] / (2 * eps)
        assert abs(fd - d[i]) <= 1e-7 * np.abs(d).max() + 1e-9, (i, fd, d[i])
