"""-m gpu: csrc/relight.hip and nlt_amd.relight against the float64 restatements of tests/relight_ref.py.

Weights: every weight is a float64 sum rounded once to float32, so |err| <= 2^-23 |ref| + 1e-12 -- provided the kernel's float32
dot products pick the light the float64 ones pick.  A float32 dot product of unit vectors is off by about 3 * 2^-24 ~ 2e-7, so
each case first asserts, on its INPUTS and in float64, that every pixel's margin between the best and the second-best light is
>= 1e-5 (seeds chosen on the CPU so that this holds at every listed shape; a bad seed fails there, loudly, instead of flaking).
Accumulate / finish: the project's rendered-texel bar, rel-L2 <= 1e-4 per rotation (README); measured ~1e-7.
End to end on the smallest config the model builds, a capture of one camera x 6 lights written by the capture writer."""
import os

import numpy as np
import pytest
import torch

import nlt_amd
from nlt_amd import capi as C
from nlt_amd import relight as RL
from nlt_amd import relight_main, trainvali
from nlt_amd.models import get_model_class
from oracle import nlt_oracle as O
import capture_ref
import relight_ref as R
from gpu_util import rel_l2

pytestmark = pytest.mark.gpu

_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
_bits = lambda t: t.detach().cpu().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------- weights
PROBES = [(4, 8), (16, 32)]
N_LIGHTS = [1, 5, 37, 300]
N_ROT = [1, 3]
SEED_SHIFT = {(16, 32, 300, 3): 26}            # the first shift (searched on the CPU) at which the float64 margins reach 1e-5
MIN_MARGIN = 1e-5
_REF = {}


def _weights_case(he, we, n_lights, n_rot):
    """Inputs and the float64 reference of a case, computed once and left alone."""
    key = (he, we, n_lights, n_rot)
    if key not in _REF:
        s = SEED_SHIFT.get(key, 0)
        dirs, rot = R.random_directions(n_lights, 1000 * n_lights + s), R.random_rotations(n_rot, 77 + s)
        probe = (np.random.default_rng(he * we + n_lights).random((he, we, 3)) + 0.05).astype(np.float32)
        idx, margin = R.nearest_lights(he, we, dirs, rot)
        _REF[key] = dict(dirs=dirs, rot=rot, probe=probe, idx=idx, margin=margin, ref=R.envmap_light_weights(probe, dirs, rot))
    return _REF[key]


@pytest.mark.parametrize('n_rot', N_ROT)
@pytest.mark.parametrize('n_lights', N_LIGHTS)
@pytest.mark.parametrize('he,we', PROBES)
def test_weights_against_float64(he, we, n_lights, n_rot):
    c = _weights_case(he, we, n_lights, n_rot)
    assert c['margin'].min() >= MIN_MARGIN, "near-tie in the INPUTS (margin %.3g): pick another seed" % c['margin'].min()
    assert np.array_equal(c['rot'][0], np.eye(3, dtype=np.float32))                 # the identity is among the rotations
    args = (_dev(c['probe']), _dev(c['dirs']), _dev(c['rot']))
    got = C.envmap_light_weights(*args)
    again = C.envmap_light_weights(*args)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (n_rot, n_lights, 3) and torch.equal(_bits(got), _bits(again))     # two runs: the same bits
    g, ref = got.cpu().numpy().astype(np.float64), c['ref']
    err = np.abs(g - ref)
    bound = 2.0 ** -23 * np.abs(ref) + 1e-12
    print("weights %dx%d L=%d R=%d: max err / bound %.3f" % (he, we, n_lights, n_rot, float((err / bound).max())))
    assert (err <= bound).all()
    energy = (c['probe'].astype(np.float64) * R.solid_angles(he, we)[:, None, None]).sum((0, 1))      # sum_p E dO, per channel
    for r in range(n_rot):
        assert (np.abs(g[r].sum(0) - energy) <= n_lights * (2.0 ** -23 * np.abs(energy) + 1e-12)).all()


@pytest.mark.parametrize('he,we', PROBES)
def test_a_single_hot_pixel_lights_exactly_one_light_per_rotation(he, we):
    c = _weights_case(he, we, 37, 3)
    assert c['margin'].min() >= MIN_MARGIN
    probe = np.zeros((he, we, 3), np.float32)
    i, j = he // 3, (2 * we) // 3
    probe[i, j] = (3.0, 700.0, 0.25)
    got = C.envmap_light_weights(_dev(probe), _dev(c['dirs']), _dev(c['rot'])).cpu().numpy().astype(np.float64)
    ref = R.envmap_light_weights(probe, c['dirs'], c['rot'])
    for r in range(3):
        lit = np.nonzero(got[r].any(1))[0]
        assert lit.tolist() == [int(c['idx'][r, i, j])]
        assert (np.abs(got[r] - ref[r]) <= 2.0 ** -23 * np.abs(ref[r]) + 1e-12).all()


def test_weights_argument_checks():
    L = C.lib()
    P = 4096                                   # a non-null fake pointer: checked, never dereferenced
    q = L.nlt_envmap_light_weights_workspace_floats
    assert q(4, 8, 5, 3) == 3 * 2 * 4 * 5 * 3 and q(4, 8, 1025, 1) == -1 and q(0, 8, 5, 1) == -1
    assert L.nlt_envmap_light_weights(None, 4, 8, P, 5, P, 1, P, 10 ** 6, P, None) == -1
    assert L.nlt_envmap_light_weights(P, 4, 8, P, 5, P, 0, P, 10 ** 6, P, None) == -1
    assert L.nlt_envmap_light_weights(P, 4, 8, P, 5, P, 1, P, q(4, 8, 5, 1) - 1, P, None) == -1
    assert L.nlt_envmap_light_weights(P, 4, 8, P, 1025, P, 1, P, 10 ** 9, P, None) == -2
    assert L.nlt_relight_accumulate(P, 3, 5, P, 1, 7, 5, 1, P, None) == -1              # l0 + Lc > L
    assert L.nlt_relight_accumulate(P, 3, 0, P, 1, 7, 0, 1, P, None) == -1
    assert L.nlt_relight_accumulate(P, 3, 5, None, 1, 7, 0, 1, P, None) == -1
    assert L.nlt_relight_accumulate(P, 3, 2 ** 29, P, 1, 7, 0, 1, P, None) == -2        # 3 x 2^29 x 3 elements
    assert L.nlt_relight_finish(P, 0, 5, 1.0, 1, P, None) == -1 and L.nlt_relight_finish(P, 2, 2 ** 29, 1.0, 1, P, None) == -2


# ---------------------------------------------------------------------------------------------------- accumulate / finish
TEXELS = [1, 5, 63, 257]
N_ACC_LIGHTS = 7
CHUNKINGS = [(7,), (3, 3, 1), (1,) * 7]
BAR = 1e-4


def _acc_inputs(texels, n_rot):
    rng = np.random.default_rng(texels * 10 + n_rot)
    pred = (rng.random((N_ACC_LIGHTS, texels, 3)) * 1.5 - 0.25).astype(np.float32)      # below 0 and above 1: the clip is live
    pred[0, 0, 0], pred[-1, -1, -1] = -0.5, 1.75
    if texels > 1:
        pred[1, 1] = (0.02, 0.04045, 0.05)                                              # both branches of the decode
    weights = (rng.random((n_rot, N_ACC_LIGHTS, 3)) * 0.4).astype(np.float32)
    acc0 = (rng.random((n_rot, texels, 3)) * 0.1).astype(np.float32)                    # accumulation starts from what is stored
    return pred, weights, acc0


def _accumulate(pred, weights, acc0, chunks, is_linear):
    acc, l0 = _dev(acc0), 0
    w = _dev(weights)
    for n in chunks:
        C.relight_accumulate(_dev(pred[l0:l0 + n]), w, l0, acc, is_linear)
        l0 += n
    torch.cuda.synchronize()
    return acc


@pytest.mark.parametrize('is_linear', [True, False])
@pytest.mark.parametrize('n_rot', [1, 3, 9])
@pytest.mark.parametrize('texels', TEXELS)
def test_accumulate_and_finish_against_float64(texels, n_rot, is_linear):
    pred, weights, acc0 = _acc_inputs(texels, n_rot)
    assert (pred < 0).any() and (pred > 1).any()
    runs = [_accumulate(pred, weights, acc0, ch, is_linear) for ch in CHUNKINGS]
    for other in runs[1:]:
        assert torch.equal(_bits(runs[0]), _bits(other))                               # the cut into chunks changes no bit
    ref = R.relight_accumulate(acc0, pred, weights, 0, is_linear)
    got = runs[0].cpu().numpy()
    errs = [rel_l2(got[r], ref[r]) for r in range(n_rot)]
    print("accumulate texels=%d R=%d linear=%s: rel-L2 %.3e" % (texels, n_rot, is_linear, max(errs)))
    assert max(errs) <= BAR
    for to_srgb in (True, False):
        exposure = 1.7                                                                   # some of it clips
        out = C.relight_finish(runs[0], exposure, to_srgb)
        torch.cuda.synchronize()
        want = R.relight_finish(got, exposure, to_srgb)                                  # of the device's own sums: finish alone
        assert out.shape == runs[0].shape and (texels < 63 or (exposure * got.astype(np.float64) > 1.0).any())
        errs = [rel_l2(out[r].cpu().numpy(), want[r]) for r in range(n_rot)]
        print("finish texels=%d R=%d srgb=%s: rel-L2 %.3e" % (texels, n_rot, to_srgb, max(errs)))
        assert max(errs) <= BAR


def test_accumulate_takes_the_vector_path_and_the_tail_path_to_the_same_bits():
    """texels % 4 == 0 on aligned arrays runs the 16-byte form; the same data one float off alignment runs the other: same bits."""
    texels, n_rot = 64, 3
    pred, weights, acc0 = _acc_inputs(texels, n_rot)
    aligned = _accumulate(pred, weights, acc0, (7,), False)
    shifted_pred = torch.zeros(pred.size + 1, device='cuda')[1:].view(pred.shape).copy_(_dev(pred))
    shifted_acc = torch.zeros(acc0.size + 1, device='cuda')[1:].view(acc0.shape).copy_(_dev(acc0))
    assert shifted_pred.data_ptr() % 16 == 4 and shifted_acc.data_ptr() % 16 == 4
    C.relight_accumulate(shifted_pred, _dev(weights), 0, shifted_acc, False)
    torch.cuda.synchronize()
    assert torch.equal(_bits(aligned), _bits(shifted_acc))


# ---------------------------------------------------------------------------------------------------- end to end
UVS, IM, N_CAP_LIGHTS, CAM = 64, 32, 6, 'C01'
CAM_POS = [2.0, -1.0, 3.0]
LIGHT_POS = {'L%02d' % i: [3.0 * np.cos(i), 3.0 * np.sin(i), 1.0 + 0.5 * i] for i in range(N_CAP_LIGHTS)}
KW = dict(depth=32, uvh=UVS, uvw=UVS, imh=IM, imw=IM)


def _sample_inputs(n, faces=24):
    """What the renderer hands over for sample n at IM x IM (tests/capture_ref.py:sample_inputs at this size)."""
    rng = np.random.default_rng(500 + n)
    p = IM * IM
    valid = (rng.random(p) > 0.2).astype(np.uint8)
    locs, normals = rng.random((p, 3)) * 2 - 1, rng.random((p, 3)) * 2 - 1
    face_i = np.where(valid > 0, rng.integers(0, faces, p), -1).astype(np.int64)
    occluded = (rng.random(p) < 0.3).astype(np.uint8)
    alpha = np.where(valid.reshape(IM, IM) > 0, 255, 0).astype(np.uint8)
    rgba = np.dstack((rng.integers(0, 256, (IM, IM, 3), dtype=np.uint8), alpha))
    return dict(locs=locs, normals=normals, valid=valid, face_i=face_i, occluded=occluded), rgba, alpha


@pytest.fixture(scope='module')
def capture(tmp_path_factory):
    """One camera x 6 lights through data_gen.render.write_sample + postproc.postprocess, read back by load_store."""
    from nlt_amd.data_gen import postproc, render
    from nlt_amd.datasets import nlt as D
    root = str(tmp_path_factory.mktemp('relight') / 'capture')
    table = capture_ref.unwrap_table()
    names = sorted(LIGHT_POS)
    light_nn = {n: names[(i + 1) % len(names)] for i, n in enumerate(names)}
    # ids in an order that is NOT the lights' order: view_samples has to sort
    for n, name in enumerate(reversed(names)):
        inter, rgba, alpha = _sample_inputs(n)
        dense = {k: (v if k == 'face_i' else torch.from_numpy(v).cuda()) for k, v in inter.items()}
        cam, light = dict(name=CAM, position=CAM_POS), dict(name=name, position=LIGHT_POS[name])
        sample = render.render_sample(dense, table, cam, light, UVS, rgb_camspc=rgba, alpha=alpha)
        render.write_sample(os.path.join(root, 'trainvali_%09d_%s_%s' % (n, CAM, name)), sample, cam, light, ({CAM: CAM}, light_nn))
    postproc.postprocess(root)
    store = D.load_store(root, device='cuda')
    assert len(store['ids']) == N_CAP_LIGHTS and all(store['complete'])
    return root, store


def _models(linear_space, root):
    om = O.OracleModel(seed=3, **KW)
    cfg = nlt_amd.make_config(linear_space=linear_space, bs=4, data_root=root, dataset='nlt', no_batch=False, **KW)
    pm = get_model_class('nlt')(cfg)
    pm.load_weights(om.numpy_weights())
    pm.register_trainable()
    return om, pm, cfg


def _probe_weights(root, store):
    lights = RL.load_lights(root)
    samples = RL.view_samples(store, CAM)
    assert [n for _, n in samples] == sorted(LIGHT_POS) and lights == {k: tuple(float(x) for x in v) for k, v in LIGHT_POS.items()}
    dirs = RL.light_directions([lights[n] for _, n in samples])
    probe = (np.random.default_rng(8).random((8, 16, 3)) + 0.05).astype(np.float32)
    return samples, probe, RL.envmap_weights(probe, dirs, rotations=[0.0, 1.3])


def _combine(preds, weights, is_linear):
    """Float64 combination of per-light predictions [L,imh,imw,3] -> [R,imh,imw,3]."""
    n = preds.shape[0]
    acc = R.relight_accumulate(np.zeros((weights.shape[0], IM * IM, 3)), preds.reshape(n, -1, 3), weights, 0, is_linear)
    return acc.reshape(weights.shape[0], IM, IM, 3)


@pytest.mark.parametrize('linear_space', [False, True])
def test_relight_end_to_end(capture, monkeypatch, linear_space):
    from nlt_amd.datasets import nlt as D
    root, store = capture
    om, pm, cfg = _models(linear_space, root)
    ds = D.Dataset(cfg, 'train', store=store)
    samples, probe, weights = _probe_weights(root, store)
    assert tuple(weights.shape) == (2, N_CAP_LIGHTS, 3)
    w64 = weights.cpu().numpy().astype(np.float64)

    # the references: per-light predictions of separate Model.calls (existing code), and of the oracle
    own, orc = [], []
    for id_, _ in samples:
        b = ds.load_batch([id_])
        own.append(pm.call(b, 'test')[0].cpu().numpy()[0])
        cb = tuple(t.cpu() if torch.is_tensor(t) else t for t in b)
        with torch.no_grad():                                       # (load_batch stacks the k = 1 neighbours: [n,1,h,w,3])
            orc.append(om.call(cb, 'test', nn_list=[(cb[8][:, 0], cb[9][:, 0])])[0].numpy()[0])
    before = pm.call(ds.load_batch([samples[0][0]]), 'test')[0].clone()
    want_own, want_orc = _combine(np.stack(own), w64, linear_space), _combine(np.stack(orc), w64, linear_space)

    out4 = RL.relight(pm, ds, CAM, weights)                        # chunk = bs = 4: 4 + 2
    out1 = RL.relight(pm, ds, CAM, weights, chunk=1)
    torch.cuda.synchronize()
    assert tuple(out4['linear'].shape) == tuple(out4['image'].shape) == (2, IM, IM, 3)
    for k in ('linear', 'image'):
        assert torch.equal(_bits(out4[k]), _bits(out1[k])), k
    lin = out4['linear'].cpu().numpy()
    e_own = max(rel_l2(lin[r], want_own[r]) for r in range(2))
    e_orc = max(rel_l2(lin[r], want_orc[r]) for r in range(2))
    print("relight linear_space=%s: rel-L2 vs own renders %.3e, vs the oracle %.3e" % (linear_space, e_own, e_orc))
    assert e_own <= 1e-4
    assert e_orc <= (1e-4 if linear_space else 2.3e-4)              # 1e-4 render bar x the sRGB decode's largest slope, 2.4 / 1.055
    want_img = R.relight_finish(lin, 1.0, not linear_space)
    assert max(rel_l2(out4['image'][r].cpu().numpy(), want_img[r]) for r in range(2)) <= 1e-4

    # with feat_agg: the fused override plan is the route (its front kernel ran once per chunk), against the override renders
    feat_agg = nlt_amd.nlt_test.extract_feat(pm, ds.build_pipeline(seed=0), 1)
    ovr = np.stack([pm.call(ds.load_batch([i]), 'test', obs_override=feat_agg)[0].cpu().numpy()[0] for i, _ in samples])
    calls = []
    for name in [x for x in dir(C) if x.startswith('front') and 'forward' in x and callable(getattr(C, x))]:
        real = getattr(C, name)
        monkeypatch.setattr(C, name, lambda *a, _n=name, _r=real, **kw: (calls.append(_n), _r(*a, **kw))[1])
    got = RL.relight(pm, ds, CAM, weights, feat_agg=feat_agg)
    torch.cuda.synchronize()
    assert len(calls) >= 2 and set(calls) <= {'front_ovr_forward', 'front_ovr_forward_u8'}, calls      # (4 + 2; plan-time trials add to it)
    assert pm.plan._ovr is not None
    want_ovr = _combine(ovr, w64, linear_space)
    assert max(rel_l2(got['linear'][r].cpu().numpy(), want_ovr[r]) for r in range(2)) <= 1e-4
    monkeypatch.undo()

    # no plan state was disturbed: the ordinary call gives the bits it gave before
    after = pm.call(ds.load_batch([samples[0][0]]), 'test')[0]
    torch.cuda.synchronize()
    assert torch.equal(_bits(before), _bits(after))

    with pytest.raises(ValueError, match='6 lights'):
        RL.relight(pm, ds, CAM, weights[:, :5].contiguous())


def test_relight_main_writes_the_frames(capture, tmp_path):
    from nlt_amd.datasets import nlt as D
    from nlt_amd.util import vis as V
    root, store = capture
    _, pm, cfg = _models(False, root)
    pm.build('cuda')
    run_dir = tmp_path / 'out' / 'tiny'
    os.makedirs(run_dir / 'checkpoints')
    with open(str(run_dir) + '.ini', 'w') as h:
        cfg.write(h)
    ckpt = str(run_dir / 'checkpoints' / 'ckpt-3.pt')
    trainvali.save_checkpoint(ckpt, pm, None, 3)
    probe = (np.random.default_rng(9).random((8, 16, 3)) + 0.05).astype(np.float32)
    with open(str(tmp_path / 'sky.hdr'), 'wb') as h:
        h.write(R.hdr_bytes(R.encode_rgbe(probe), True))
    outdir, out = relight_main.main(['--ckpt', ckpt, '--cam', CAM, '--envmap', str(tmp_path / 'sky.hdr'), '--turns', '2', '--exposure', '0.8'])
    torch.cuda.synchronize()
    assert outdir == str(run_dir / 'vis_relight' / 'ckpt-3' / CAM / 'sky')
    assert sorted(os.listdir(outdir)) == ['frame_000.png', 'frame_001.png', 'linear.npy', 'turn.apng']
    assert np.array_equal(np.load(os.path.join(outdir, 'linear.npy')), out['linear'].cpu().numpy())
    V.write_arr(out['image'][0].cpu().numpy(), str(tmp_path / 'want.png'))
    with open(os.path.join(outdir, 'frame_000.png'), 'rb') as a, open(str(tmp_path / 'want.png'), 'rb') as b:
        assert a.read() == b.read()
    assert not torch.equal(out['image'][0], out['image'][1])                              # the probe turned
