"""CPU: tests/lpips_ref.py holds itself to account -- its float64 gradient against central differences, and the properties the
GPU tests lean on (no all-zero texel, kinks agreeing between float32 and float64) at the shapes they use."""
import numpy as np
import pytest
import torch

import lpips_ref as R

W = R.random_weights(0)


def test_map_sizes_at_the_minimum_image():
    gt, _ = R.make_pair('far', 1, 31, 31, seed=1)
    assert [tuple(f.shape[1:]) for f in R.features(gt, W, torch.float64)] == [(64, 7, 7), (192, 3, 3), (384, 1, 1), (256, 1, 1), (256, 1, 1)]
    with pytest.raises(RuntimeError):
        R.features(gt[:, :30], W, torch.float64)              # 30 rows: pool2 has no window left


def test_float64_gradient_against_central_differences():
    """One pixel channel at a time, step h = 1e-6 in float64.  Error budget: roundoff 2 eps64 |L| / (2 h) ~ 2e-10 |L|, truncation
    h^2 / 6 |L'''| -- both far below 1e-5 of the largest gradient entry unless a ReLU / pool kink lies within h of the input, which
    the fixed seed does not hit (a kink would show as an error of the order of the entry itself)."""
    gt, pred = R.make_pair('far', 1, 31, 31, seed=3)
    l64, g64 = R.loss_and_unit_grad(gt, pred, W, torch.float64, check_zero=True)
    assert np.isfinite(g64).all() and np.abs(g64).max() > 0
    rng = np.random.RandomState(0)
    h = 1e-6
    big = np.abs(g64).max()
    p64 = pred.astype(np.float64)
    g = torch.as_tensor(gt, dtype=torch.float64)
    for _ in range(24):
        i, j, c = rng.randint(31), rng.randint(31), rng.randint(3)
        up, dn = p64.copy(), p64.copy()
        up[0, i, j, c] += h
        dn[0, i, j, c] -= h
        fd = (float(R.distance(g, torch.from_numpy(up), W, torch.float64)) - float(R.distance(g, torch.from_numpy(dn), W, torch.float64))) / (2 * h)
        assert abs(fd - g64[0, i, j, c]) <= 1e-5 * big, (i, j, c, fd, g64[0, i, j, c])


@pytest.mark.parametrize('shape', [(1, 31, 31), (2, 32, 35), (2, 47, 64)])
@pytest.mark.parametrize('kind', R.KINDS)
def test_chosen_inputs_have_no_zero_texel_and_no_flipped_kink(kind, shape):
    n, h, w = shape
    gt, pred = R.make_pair(kind, n, h, w, seed=h * 100 + w)
    l64, g64, l32, g32 = R.checked(gt, pred, W)
    e_loss = np.abs(l32 - l64) / np.abs(l64)
    e_grad = max(np.abs(g32[f] - g64[f]).max() / np.abs(g64[f]).max() for f in range(n))
    print("lpips_ref %s %s: loss %s  float32 loss error %s  gradient error %.2e" % (kind, shape, l64, e_loss, e_grad))
    assert (l64 > 0).all() and e_loss.max() < 1e-5 and e_grad < 1e-4     # float32 is float32, not something else
    if n > 1:
        assert len(set(np.round(l64, 9))) == n


def test_identical_images_give_zero():
    gt, _ = R.make_pair('far', 1, 31, 31, seed=4)
    l, g = R.loss_and_unit_grad(gt, gt, W, torch.float64)
    assert (l == 0).all() and (g == 0).all()
