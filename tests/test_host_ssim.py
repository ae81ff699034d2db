"""CPU: the host side of the SSIM loss and metric (loss-string parsing, refusals, dynamic-range rules, the autograd glue, the
argument checks of the C entry points) with C.ssim_loss / C.ssim_values replaced by the NumPy restatement of tests/ssim_ref.py,
the way tests/test_host_vis.py replaces psnr_sums."""
import numpy as np
import pytest
import torch

import nlt_amd
from nlt_amd import capi as C
from nlt_amd import losses, metric
from nlt_amd.models import get_model_class
import fake_capi
import ssim_ref as R


def fake_ssim(monkeypatch):
    calls = []

    def ssim_loss(pred, gt, max_val, want_grad):
        calls.append(('loss', tuple(pred.shape), float(max_val), bool(want_grad)))
        per, d = R.loss_and_unit_grad(gt.numpy(), pred.numpy(), max_val)
        return torch.from_numpy(per.astype(np.float32)), (torch.from_numpy(d.astype(np.float32)) if want_grad else None)

    def ssim_values(im1, im2, max_val):
        calls.append(('values', tuple(im1.shape), float(max_val)))
        return torch.tensor([R.metric_ssim_np(a, b, max_val) for a, b in zip(im1.numpy(), im2.numpy())], dtype=torch.float64)
    monkeypatch.setattr(C, 'ssim_loss', ssim_loss)
    monkeypatch.setattr(C, 'ssim_values', ssim_values)
    monkeypatch.setattr(metric, 'DEVICE', 'cpu')
    return calls


def _model(loss):
    return get_model_class('nlt')(nlt_amd.make_config(depth=256, uvh=64, uvw=64, imh=32, imw=32, loss=loss))


def test_loss_string_with_an_ssim_term_parses_to_weights_and_classes():
    pm = _model('0.5ssim,l2')
    assert [(w, type(f)) for w, f in pm.wloss] == [(0.5, losses.SSIM), (1.0, losses.L2)]
    assert pm.wloss[0][1].dynamic_range == 1.0
    pm = _model('l2,0.2ssim,1e-1barron')
    assert [(w, type(f)) for w, f in pm.wloss] == [(1.0, losses.L2), (0.2, losses.SSIM), (0.1, losses.Barron)]
    assert [(w, type(f)) for w, f in _model('ssim').wloss] == [(1.0, losses.SSIM)]


@pytest.mark.parametrize('loss', ['l1', 'lpips', 'l2,0.1l1', '0.5ssim,lpips'])
def test_l1_and_lpips_stay_refused(loss):
    with pytest.raises(NotImplementedError):
        _model(loss)


def test_metric_ssim_dynamic_range_rules_are_psnr_s():
    for dt in (np.float32, np.float64, 'float16', 'uint8', np.uint16):
        assert metric.SSIM(dt).drange == metric.PSNR(dt).drange
    assert metric.SSIM('uint8').drange == 255.0 and metric.SSIM(np.uint16).drange == 65535.0 and metric.SSIM(np.float32).drange == 1.0
    for dt in (np.int32, np.int8, bool):
        with pytest.raises(NotImplementedError):
            metric.SSIM(dt)
        with pytest.raises(NotImplementedError):
            metric.PSNR(dt)


def test_metric_ssim_input_handling(monkeypatch):
    calls = fake_ssim(monkeypatch)
    x, y = R.make_pair('near', 2, 12, 14, 3)
    m = metric.SSIM(np.float32)
    v = m(x[0], y[0])
    assert isinstance(v, float) and v == R.metric_ssim_np(x[0], y[0], 1.0)
    assert m(torch.from_numpy(x[0]), torch.from_numpy(y[0])) == v
    assert m(x[0, ..., 0], y[0, ..., 0]) == m(x[0, ..., :1], y[0, ..., :1]) == R.metric_ssim_np(x[0, ..., 0], y[0, ..., 0], 1.0)
    assert [c[1] for c in calls[-2:]] == [(1, 12, 14, 1)] * 2
    assert m.batch(x, y) == [m(x[0], y[0]), m(x[1], y[1])]
    u = metric.SSIM('uint8')
    xu, yu = (x[0] * 255).astype(np.uint8), (y[0].clip(0, 1) * 255).astype(np.uint8)
    assert u(xu, yu) == R.metric_ssim_np(xu, yu, 255.0) and calls[-1][2] == 255.0
    with pytest.raises(AssertionError):
        m(x[0], y[0][:, :13])
    with pytest.raises(NotImplementedError):
        m(np.zeros((12, 12, 4), np.float32), np.zeros((12, 12, 4), np.float32))
    with pytest.raises(ValueError):
        m(x, y)                                          # a batch goes through .batch


def test_losses_ssim_glue(monkeypatch):
    fake_capi.install(monkeypatch)
    calls = fake_ssim(monkeypatch)
    x, y = R.make_pair('near', 2, 12, 13, 3)
    gt, pred = torch.from_numpy(x), torch.from_numpy(y).requires_grad_(True)
    f = losses.SSIM(1 - 0)
    per = f(gt, pred, keep_batch=True)
    assert per.shape == (2,) and calls[-1] == ('loss', (2, 12, 13, 3), 1.0, True)
    assert float(f(gt, pred.detach())) == float(per.detach().mean()) and calls[-1][3] is False
    (per * torch.tensor([2.0, -1.0])).sum().backward()
    _, d = R.loss_and_unit_grad(x, y, 1.0)
    want = d.astype(np.float32) * np.array([2.0, -1.0], np.float32)[:, None, None, None]
    assert np.array_equal(pred.grad.numpy(), want) and gt.grad is None
    # weights: gt and pred alpha-blended against zeros, the gradient comes back through the blend
    wt = torch.rand(2, 12, 13, 1)
    p = torch.from_numpy(y).requires_grad_(True)
    got = f(gt, p, keep_batch=True, weights=wt)
    a = wt.expand(2, 12, 13, 3).numpy()
    lw, dw = R.loss_and_unit_grad(x * a, y * a, 1.0)
    np.testing.assert_allclose(got.detach().numpy(), lw, rtol=1e-6)
    got.sum().backward()
    np.testing.assert_allclose(p.grad.numpy(), dw * a, rtol=1e-5, atol=1e-9)


def test_bad_arguments_return_status_codes_without_a_gpu():
    """Sizes below 11, a channel count other than 1 or 3 and a short workspace are refused before any launch."""
    L = C.lib()
    assert L.nlt_ssim_workspace_floats(1, 10, 32, 3, 1) == -1 and L.nlt_ssim_workspace_floats(1, 32, 10, 1, 0) == -1
    assert L.nlt_ssim_workspace_floats(1, 32, 32, 2, 0) == -1 and L.nlt_ssim_workspace_floats(1, 32, 32, 4, 1) == -1
    assert L.nlt_ssim_workspace_floats(0, 32, 32, 3, 1) == -1
    # float64 partials (2 floats per workgroup) + 3 coefficient maps per channel over the valid grid when a gradient is wanted
    assert L.nlt_ssim_workspace_floats(2, 11, 11, 3, 0) == 2 * 2 * 1
    assert L.nlt_ssim_workspace_floats(2, 11, 11, 3, 1) == 2 * 2 * 1 + 3 * 2 * 3
    assert L.nlt_ssim_workspace_floats(1, 10 + 33, 10 + 65, 1, 1) == 2 * 3 * 3 + 3 * 33 * 65
    P = 4096                                             # a non-null aligned fake pointer: checked, never dereferenced here
    n = None
    assert L.nlt_ssim_loss(n, n, 1, 16, 16, 3, 1.0, n, 0, n, n, n) == -1
    assert L.nlt_ssim_loss(P, P, 1, 10, 16, 3, 1.0, P, 1 << 20, P, P, n) == -2
    assert L.nlt_ssim_loss(P, P, 1, 16, 16, 4, 1.0, P, 1 << 20, P, P, n) == -2
    need = L.nlt_ssim_workspace_floats(1, 16, 16, 3, 1)
    assert L.nlt_ssim_loss(P, P, 1, 16, 16, 3, 1.0, P, need - 1, P, P, n) == -1
    assert L.nlt_ssim_loss(P, P, 1, 16, 16, 3, 1.0, P + 4, need, P, P, n) == -1          # float64 partials: 8-byte aligned
    assert L.nlt_ssim_loss(P, P, 1, 16, 16, 3, 0.0, P, need, P, P, n) == -1
    assert L.nlt_ssim_values(P, P, 1, 16, 16, 3, 1.0, P, 1 << 20, n, n) == -1
    assert L.nlt_ssim_values(P, P, 1, 16, 10, 1, 1.0, P, 1 << 20, P, n) == -2
    assert L.nlt_ssim_values(P, P, 1, 16, 16, 1, 1.0, P, 1, P, n) == -1
