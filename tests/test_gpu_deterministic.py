"""-m gpu: deterministic mode (`deterministic = true` / NLT_DETERMINISTIC=1 / model.deterministic): the atomic-free siblings of
the train step's float-atomic kernels repeat bit for bit, agree with float64 as well as the kernels they stand in for, and a
whole train step -- loss scalar, flat gradient bucket, updated parameters -- is identical between two models, between the launch
tape and the adapters, and between two fresh processes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import nlt_amd
from nlt_amd import capi as C
from nlt_amd import trainvali
from nlt_amd.models import get_model_class
from oracle import nlt_oracle as O
from oracle import tf_ops as T
from gpu_util import rel_l2, make_pair, to_device_batch, _oracle_grads, _per_tensor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPEATS = 5


def _five_times(fn):
    outs = [fn() for _ in range(REPEATS)]
    torch.cuda.synchronize()
    first = outs[0] if isinstance(outs[0], tuple) else (outs[0],)
    for o in outs[1:]:
        o = o if isinstance(o, tuple) else (o,)
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(first, o))
    return outs[0]


# ------------------------------------------------------------------------------------------------------ kernel tests
def _warp_maps(kind, n, hc, wc, uvh, uvw, rng):
    F = np.float32
    if kind == 'chart':
        jj, ii = np.meshgrid(np.arange(wc, dtype=F), np.arange(hc, dtype=F))
        w = np.stack(((jj + F(0.37)) / F(wc) * F(0.9) + F(0.03), (ii + F(0.61)) / F(hc) * F(0.8) + F(0.1)), -1)[None].repeat(n, 0)
    elif kind == 'random':
        w = rng.random((n, hc, wc, 2), dtype=F)
    elif kind == 'many_to_one':
        w = np.zeros((n, hc, wc, 2), F)
        w[..., 0] = F(5.25) / F(uvw); w[..., 1] = F(7.5) / F(uvh)
    else:
        w = rng.random((n, hc, wc, 2), dtype=F)
        e = w.reshape(-1, 2)
        e[0::7, 0] = F(-0.5) / F(uvw); e[1::7, 1] = F(-0.25) / F(uvh)
        e[2::7, 0] = (F(uvw) - F(0.5)) / F(uvw); e[3::7, 1] = (F(uvh) - F(0.75)) / F(uvh)
        e[4::7, 0] = F(3) / F(uvw); e[5::7, 1] = F(6) / F(uvh)
        e[6::7] = 0
    return np.ascontiguousarray(w.astype(F))


@pytest.mark.parametrize('kind,n,hc,wc,uvh,uvw', [('chart', 2, 96, 160, 128, 80), ('random', 2, 96, 160, 128, 80),
                                                  ('many_to_one', 1, 64, 64, 48, 32), ('borders_and_integers', 2, 40, 72, 24, 56),
                                                  ('chart', 1, 128, 128, 64, 64)])
def test_warp_backward_det_repeats_and_is_as_close_to_float64_as_the_scatter(kind, n, hc, wc, uvh, uvw):
    """Bit-repeatable over 5 runs; rel-L2 distance from the float64 resampler gradient (oracle/tf_ops.py) at most 2x what the
    float-atomic nlt_warp_backward measures on the same input (both are fp32 sums of identical terms in different orders)."""
    rng = np.random.default_rng(5)
    warp = _warp_maps(kind, n, hc, wc, uvh, uvw, rng)
    g = rng.standard_normal((n, hc, wc, 3)).astype(np.float32)
    # float64 reference: autograd of the oracle's resampler at the float32 pixel coordinates the kernels form
    px = torch.from_numpy(warp * np.array([uvw, uvh], np.float32)).double()
    data = torch.zeros((n, uvh, uvw, 3), dtype=torch.float64, requires_grad=True)
    (ref,) = torch.autograd.grad(T.resampler(data, px), data, torch.from_numpy(g).double())
    ref[:, 0, 0] = 0                                                           # texel (0,0) of each frame is skipped
    dw, dg = torch.from_numpy(warp).cuda(), torch.from_numpy(g).cuda()

    def det():
        out = torch.full((n, uvh, uvw, 3), float('nan'), device='cuda')        # fully written: no zero-fill by the caller
        C.warp_backward_det(dg, dw, n, uvh, uvw, hc, wc, out)
        return out
    got = _five_times(det)
    old = torch.empty_like(got)
    C.warp_backward(dg, dw, n, uvh, uvw, hc, wc, old)
    e_det, e_old = rel_l2(got.cpu(), ref), rel_l2(old.cpu(), ref)
    print("warp_backward %s: rel-L2 vs float64  det %.3e  atomic %.3e" % (kind, e_det, e_old))
    assert torch.isfinite(got).all()
    assert e_det <= 2 * e_old, (kind, e_det, e_old)
    with C.deterministic_scope(True):                                          # the adapter takes the sibling in the mode
        via = torch.empty_like(got)
        C.warp_backward(dg, dw, n, uvh, uvw, hc, wc, via)
    assert torch.equal(via, got)


@pytest.mark.parametrize('n,h,w,c,oh,ow', [(2, 24, 40, 3, 48, 80), (2, 32, 48, 3, 24, 36), (1, 17, 29, 8, 40, 23), (2, 40, 23, 3, 17, 29),
                                           (1, 16, 16, 32, 32, 32)])
def test_resize_backward_gather_repeats_and_matches_float64_and_the_scatter(n, h, w, c, oh, ow):
    rng = np.random.default_rng(6)
    g = torch.from_numpy(rng.standard_normal((n, oh, ow, c)).astype(np.float32))
    x = torch.zeros((n, c, h, w), dtype=torch.float64, requires_grad=True)
    y = Fn.interpolate(x, size=(oh, ow), mode='bilinear', align_corners=False)
    (ref,) = torch.autograd.grad(y, x, g.double().permute(0, 3, 1, 2))
    ref = ref.permute(0, 2, 3, 1)
    dg = g.cuda()
    with C.deterministic_scope(True):
        got = _five_times(lambda: C.resize_bilinear_backward(dg, h, w))
    old = C.resize_bilinear_backward(dg, h, w)
    e_det, e_old = rel_l2(got.cpu(), ref), rel_l2(old.cpu(), ref)
    print("resize_backward %s -> %s: rel-L2 vs float64  gather %.3e  atomic %.3e" % ((h, w), (oh, ow), e_det, e_old))
    assert e_det <= 2 * e_old, (e_det, e_old)
    assert rel_l2(got.cpu(), old.cpu()) <= 1e-6


@pytest.mark.parametrize('n,h,w', [(2, 48, 80), (3, 33, 57)])
def test_deterministic_l2_sums_repeat_and_match_the_atomic_entry_points(n, h, w):
    rng = np.random.default_rng(7)
    R = lambda *s: torch.from_numpy(rng.random(s, dtype=np.float32)).cuda()
    pred, rgb, fg, wt = R(n, h, w, 3), R(n, h, w, 3), R(n, h, w, 3), R(n, h, w)
    gt = C.mul_forward(rgb, fg)
    ref = (C.l2_loss_forward(pred, gt), C.l2_loss_weighted_forward(pred, gt, wt)) + C.l2_train_loss(pred, rgb, fg, 4)
    with C.deterministic_scope(True):
        got = _five_times(lambda: (C.l2_loss_forward(pred, gt), C.l2_loss_weighted_forward(pred, gt, wt)) + C.l2_train_loss(pred, rgb, fg, 4))
    for a, b in zip(got[:3], ref[:3]):                                         # the three sums
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-6)
    assert torch.equal(got[3], ref[3]) and torch.equal(got[4], ref[4])         # gt and dpred: no atomics on either side


@pytest.mark.parametrize('n,h,w', [(2, 128, 192), (2, 72, 40), (1, 512, 512)])
def test_deterministic_barron_repeats_and_matches_the_atomic_entry_point(n, h, w):
    """(72, 40): the last level is 5 x 3 (72 -> 36 -> 18 -> 9 -> 5, 40 -> 20 -> 10 -> 5 -> 3), axes shorter than 6 -- the
    brute-force gather adjoint; there the atomic entry point's gradient is itself not bit-stable.  The other two sizes keep
    every axis >= 6, so the gradient passes are the same kernels on both sides."""
    rng = np.random.default_rng(8)
    R = lambda *s: torch.from_numpy(rng.random(s, dtype=np.float32)).cuda()
    pred, gt = R(n, h, w, 3), R(n, h, w, 3)
    ref_loss, ref_grad = C.barron_loss(pred, gt, True)
    with C.deterministic_scope(True):
        loss, grad = _five_times(lambda: C.barron_loss(pred, gt, True))
        only = C.barron_loss(pred, gt, False)[0]
    assert torch.equal(only, loss)
    np.testing.assert_allclose(loss.cpu().numpy(), ref_loss.cpu().numpy(), rtol=1e-6)
    sizes, a, b = [], h, w
    for _ in range(5):
        sizes.append((a, b)); a, b = (a - 1) // 2 + 1, (b - 1) // 2 + 1
    if min(min(s) for s in sizes) < 6:
        assert (h, w) == (72, 40)
        assert rel_l2(grad.cpu(), ref_grad.cpu()) <= 1e-5
    else:
        assert torch.equal(grad, ref_grad)


def test_deterministic_weight_gradient_siblings_repeat_and_match():
    """nlt_stem_backward_det / nlt_head_backward_det / nlt_conv_backward_weights_det (MFMA and direct forms) against their
    float-atomic siblings: bit-repeatable, and the same sums to fp32 accumulation error."""
    rng = np.random.default_rng(9)
    R = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    n, k, h, w, c = 2, 2, 24, 40, 16
    stem_in = (R(n, h, w, 3), R(n, h, w, 1), R(n, h, w, 1), R(n, k, h, w, 3), R(n, k, h, w, 3), None, n, k, h, w, c, R(n, h, w, 2 * c), R(n, k, h, w, c))
    cd, cs = 16, 32
    head_in = (R(n, h, w, cd), cd, cd, R(n, h, w, cs), cs, cs, R(cd + cs, 3), R(n, h, w, 3), n, h, w)

    def stem():
        out = [torch.zeros(5, c, device='cuda'), torch.zeros(c, device='cuda'), torch.zeros(3, c, device='cuda'), torch.zeros(c, device='cuda')]
        C.stem_backward(*stem_in, *out)
        return tuple(out)

    def head():
        d_dec, d_skip = torch.empty(n, h, w, cd, device='cuda'), torch.empty(n, h, w, cs, device='cuda')
        dw, db = torch.zeros(cd + cs, 3, device='cuda'), torch.zeros(3, device='cuda')
        C.head_backward(*head_in, d_dec, cd, d_skip, cs, dw, db)
        return d_dec, d_skip, dw, db

    def wgrad(mode, cin, cout, hh, ww):
        x = R(n, hh, ww, cin)
        oh, ow = {C.CONV_K2S2: (hh // 2, ww // 2), C.DECONV_K2S2: (2 * hh, 2 * ww)}.get(mode, (hh, ww))
        g = R(n, oh, ow, cout)
        shape = {C.CONV1X1: (1, 1, cin, cout), C.CONV_K2S2: (2, 2, cin, cout), C.CONV_K2S1: (2, 2, cin, cout),
                 C.DECONV_K2S2: (2, 2, cout, cin), C.DECONV_K2S1: (2, 2, cout, cin)}[mode]

        def run():
            dw, db = torch.zeros(shape, device='cuda'), torch.zeros(cout, device='cuda')
            C.conv_backward_weights(mode, x, cin, cin, None, 0, 0, n, hh, ww, g, cout, cout, dw, db)
            return dw, db
        return run
    cases = [stem, head] + [wgrad(m, ci, co, hh, ww) for m, ci, co, hh, ww in (
        (C.CONV1X1, 5, 16, 24, 40), (C.CONV1X1, 3, 16, 24, 40), (C.CONV_K2S2, 32, 64, 2, 6), (C.CONV_K2S1, 64, 64, 1, 3),
        (C.DECONV_K2S2, 64, 32, 1, 3), (C.DECONV_K2S1, 32, 32, 2, 6), (C.CONV_K2S1, 16, 32, 24, 40), (C.DECONV_K2S2, 16, 8, 12, 20))]
    for i, fn in enumerate(cases):
        ref = fn()
        with C.deterministic_scope(True):
            got = _five_times(fn)
        for a, b in zip(got, ref):
            assert rel_l2(a.cpu(), b.cpu()) <= 1e-5, (i, rel_l2(a.cpu(), b.cpu()))


# ---------------------------------------------------------------------------------------------------- end to end
def _det_model(depth=256, uvh=64, uvw=64, imh=32, imw=32, loss='l2', seed=5, tape=True, fused=True, **branch):
    om = O.OracleModel(depth=depth, uvh=uvh, uvw=uvw, imh=imh, imw=imw, loss=loss, seed=seed, **branch)
    pm = get_model_class('nlt')(nlt_amd.make_config(depth=depth, uvh=uvh, uvw=uvw, imh=imh, imw=imw, loss=loss,
                                                    deterministic=True, **branch))
    pm.load_weights(om.numpy_weights())
    pm.register_trainable()
    assert pm.deterministic and not pm.plan.autotune
    pm.plan.use_tape = tape
    pm.plan.fuse_train = fused
    pm.build('cuda')
    return pm


def _steps(pm, batches, gbs):
    opt = nlt_amd.optim.AdamAMSGrad(pm, 1e-3)
    out = []
    for b in batches:
        loss, _ = trainvali.distributed_train_step(pm, b, opt, gbs)
        torch.cuda.synchronize()
        out.append((loss.clone(), pm.flat_grads.clone(), pm.flat_params.detach().clone()))
    return out


def _same(a, b):
    for (la, ga, pa), (lb, gb, pb) in zip(a, b):
        assert la.cpu().numpy().tobytes() == lb.cpu().numpy().tobytes(), (float(la), float(lb))
        assert torch.equal(ga, gb) and torch.equal(pa, pb)
        assert torch.isfinite(ga).all() and float(ga.abs().sum()) > 0


CASES = {
    'l2_cam_eq_im': dict(loss='l2', uvh=64, uvw=128, imh=32, imw=64, cam=(32, 64), k=1),
    'l2_cam_ne_im': dict(loss='l2', uvh=64, uvw=128, imh=32, imw=64, cam=(40, 56), k=2),
    'barron_cam_eq_im': dict(loss='barron', uvh=64, uvw=128, imh=32, imw=64, cam=(32, 64), k=2),
    'barron_cam_ne_im': dict(loss='barron', uvh=128, uvw=64, imh=64, imw=32, cam=(36, 52), k=1),
    'depth1024_small_uv': dict(loss='l2', depth=1024, uvh=256, uvw=256, imh=64, imw=64, cam=(64, 64), k=1),
    'layer_by_layer_pool_upconv': dict(loss='l2', depth=32, uvh=128, uvw=64, imh=64, imw=32, cam=(48, 40), k=2, pool='avg'),
    'layer_by_layer_kernel3': dict(loss='l2', depth=32, uvh=128, uvw=64, imh=64, imw=32, cam=(48, 40), k=2, kernel=3),
    'layer_by_layer_norm': dict(loss='barron', depth=32, uvh=64, uvw=128, imh=32, imw=64, cam=(32, 64), k=1, norm='layer'),
    'unfused_train_plan': dict(loss='l2', uvh=64, uvw=128, imh=32, imw=64, cam=(40, 56), k=2, fused=False),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_two_models_same_seed_three_steps_are_bit_identical(name):
    c = dict(CASES[name])
    cam, k, fused = c.pop('cam'), c.pop('k'), c.pop('fused', True)
    n = 2
    batches = [to_device_batch(*O.synth_batch(n, c['uvh'], c['uvw'], cam[0], cam[1], c['imh'], c['imw'], k=k, seed=80 + i)) for i in range(3)]
    a = _det_model(fused=fused, **c)
    if name == 'unfused_train_plan':
        assert not a.plan.fuse_train                                  # set by attribute, not by environment
    if name.startswith('layer_by_layer'):
        assert a.generic
    ra = _steps(a, batches, n)
    rb = _steps(_det_model(fused=fused, **c), batches, n)
    _same(ra, rb)


@pytest.mark.parametrize('loss', ['l2', 'barron'])
def test_tape_on_and_tape_off_are_bit_identical_in_deterministic_mode(loss):
    """The bound tests/test_gpu_tape.py has to leave at 1e-4 because of the float atomics."""
    batch = to_device_batch(*O.synth_batch(2, 64, 64, 40, 24, 32, 32, k=2, seed=72))
    res = []
    for tape in (True, False):
        pm = _det_model(loss=loss, seed=6, tape=tape)
        res.append(_steps(pm, [batch] * 6, 2))
        assert (pm.plan.tape_replays >= 4) if tape else (pm.plan.tape_replays == 0)
    _same(res[0], res[1])


def test_autograd_route_is_bit_identical_too():
    """call(batch, 'train') + compute_loss + .backward() in the mode: same bits twice, and the bits of train_forward_backward."""
    batch = to_device_batch(*O.synth_batch(2, 64, 128, 40, 56, 32, 64, k=1, seed=90))
    outs = []
    for _ in range(2):
        pm = _det_model(loss='barron', uvh=64, uvw=128, imh=32, imw=64)
        pred, gt, kw, _ = pm(batch, mode='train')
        lp = pm.compute_loss(pred, gt, keep_batch=True).sum() / 2
        pm.flat_params.grad = None
        lp.backward()
        torch.cuda.synchronize()
        outs.append((lp.detach().clone(), pm.flat_grads.clone()))
    assert outs[0][0].cpu().numpy().tobytes() == outs[1][0].cpu().numpy().tobytes() and torch.equal(outs[0][1], outs[1][1])
    pm = _det_model(loss='barron', uvh=64, uvw=128, imh=32, imw=64)
    pm.train_forward_backward(batch, 2)
    torch.cuda.synchronize()
    assert torch.equal(pm.flat_grads, outs[0][1])


CHILD = r'''
import hashlib, sys, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import nlt_amd
from nlt_amd import trainvali
from oracle import nlt_oracle as O
from gpu_util import make_pair, to_device_batch
_, pm = make_pair(depth=256, uvh=64, uvw=128, imh=32, imw=64, loss=%(loss)r, seed=5)
assert pm.deterministic                     # NLT_DETERMINISTIC=1 in the environment
pm.build('cuda')
opt = nlt_amd.optim.AdamAMSGrad(pm, 1e-3)
for i in range(2):
    b = to_device_batch(*O.synth_batch(2, 64, 128, 40, 56, 32, 64, k=2, seed=60 + i))
    loss, _ = trainvali.distributed_train_step(pm, b, opt, 2)
torch.cuda.synchronize()
print("RESULT", loss.cpu().numpy().tobytes().hex(), hashlib.sha256(pm.flat_params.detach().cpu().numpy().tobytes()).hexdigest())
'''


@pytest.mark.parametrize('loss', ['l2', 'barron'])
def test_two_fresh_processes_write_the_same_bytes(loss, tmp_path):
    script = tmp_path / 'child.py'
    script.write_text(CHILD % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'), loss=loss))
    env = dict(os.environ, NLT_DETERMINISTIC='1')
    lines = []
    for _ in range(2):                                                 # one after the other, each a fresh process under its own time limit
        r = subprocess.run([sys.executable, '-s', str(script)], env=env, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append([l for l in r.stdout.splitlines() if l.startswith('RESULT')][-1])
    assert lines[0] == lines[1], lines


def test_accuracy_is_unchanged_at_one_frame_of_the_config4_shape():
    """tests/test_gpu_baseline_sizes.py's bars against the float64 oracle, in deterministic mode: loss <= 1e-5, flat bucket <= 1e-5."""
    torch.set_num_threads(min(os.cpu_count() or 1, 64))
    uv, cam, n = 1024, 512, 1
    _, pm = make_pair(depth=256, uv=uv, im=cam, loss='l2', seed=41, deterministic=True)
    assert pm.deterministic
    pm.build('cuda')
    batch, nn = O.synth_batch(n, uv, uv, cam, cam, cam, cam, k=1, seed=141)
    lo, grads = _oracle_grads('l2', uv, cam, n, torch.float64, batch, nn, 0.3)
    db = to_device_batch(batch, nn)
    for _ in range(2):
        pred, gt, kw, _ = pm(db, mode='train')
        lp = pm.compute_loss(pred, gt, keep_batch=True).sum() / n
        pm.flat_params.grad = None
        lp.backward()
        torch.cuda.synchronize()
        flat, _ = _per_tensor(pm, grads)
        print("deterministic config-4 frame: loss rel %.3e  flat bucket rel-L2 %.3e" % (abs(float(lp.detach()) - lo) / abs(lo), flat))
        assert abs(float(lp.detach()) - lo) <= 1e-5 * abs(lo)
        assert flat <= 1e-5


def test_the_default_mode_launches_what_it_launched_before(monkeypatch):
    """Mode off: the adapters hand their arguments to the same entry points as ever (no `_det` / `_gather` symbol is resolved)
    and the plan keeps its plan-time trials; mode on: none of the float-atomic entry points is called."""
    _, pm = make_pair(depth=256, uv=64, im=32, loss='barron', seed=5)
    assert not pm.deterministic and pm.plan.autotune == (os.environ.get('NLT_AUTOTUNE', '1') != '0')
    pm.plan.use_tape = False                                              # (the spy below stands between the adapters and the tape)
    pm.build('cuda')
    real = C.lib()
    seen = []

    class Spy:
        def __getattr__(self, name):
            seen.append(name)
            return getattr(real, name)
    monkeypatch.setattr(C, 'lib', lambda: Spy())
    batch = to_device_batch(*O.synth_batch(2, 64, 64, 40, 24, 32, 32, k=1, seed=91))
    opt = nlt_amd.optim.AdamAMSGrad(pm, 1e-3)
    trainvali.distributed_train_step(pm, batch, opt, 2)
    torch.cuda.synchronize()
    assert 'nlt_warp_backward' in seen and 'nlt_barron_loss' in seen and 'nlt_resize_bilinear_backward' in seen
    assert not [s for s in seen if s.endswith('_det') or s.endswith('_gather') or '_det_' in s], seen
    pm.deterministic = True
    assert not pm.plan.autotune
    del seen[:]
    trainvali.distributed_train_step(pm, batch, opt, 2)
    torch.cuda.synchronize()
    assert 'nlt_warp_backward_det' in seen and 'nlt_barron_loss_det' in seen and 'nlt_resize_bilinear_backward_gather' in seen
    assert not {'nlt_warp_backward', 'nlt_barron_loss', 'nlt_resize_bilinear_backward', 'nlt_l2_train_loss', 'nlt_stem_backward',
                'nlt_head_backward', 'nlt_conv_backward_weights'} & set(seen)
