"""-m gpu: reference-format checkpoints (nlt_amd.ckpt.ReferenceCheckpointManager, trainvali.save_reference / resume_reference)
on the device.  In deterministic mode a train step repeats bit for bit, so both properties are bit equality: (11) a fresh
model + optimizer resumed from the files continues exactly where the run that wrote them would have gone, and (12) saving
between two replays of a graphed train step leaves every version counter, the replay stamp and the next step's results as
they are without the save."""
import pytest
import torch

import nlt_amd
from nlt_amd import ckpt, trainvali
from oracle import nlt_oracle as O
from gpu_util import to_device_batch
from test_gpu_deterministic import CASES, _det_model

pytestmark = pytest.mark.gpu
N = 2


def _case(name):
    c = dict(CASES[name])
    cam, k = c.pop('cam'), c.pop('k')
    batches = [to_device_batch(*O.synth_batch(N, c['uvh'], c['uvw'], cam[0], cam[1], c['imh'], c['imw'], k=k, seed=180 + i)) for i in range(4)]
    return c, batches


def _train(pm, opt, batches):
    out = None
    for b in batches:
        loss, _ = trainvali.distributed_train_step(pm, b, opt, N)
        torch.cuda.synchronize()
        out = (loss.clone(), pm.flat_grads.clone(), pm.flat_params.detach().clone())
    return out


def _render(pm, batch):
    with torch.no_grad():
        out = pm.call(batch, 'test')
    torch.cuda.synchronize()
    return out[3]['pred'].clone(), out[0].clone()


def _same_step(a, b):
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes(), (float(a[0]), float(b[0]))
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert torch.isfinite(a[1]).all() and float(a[1].abs().sum()) > 0


@pytest.mark.parametrize('name', ['l2_cam_eq_im', 'layer_by_layer_kernel3'])
def test_resume_from_reference_checkpoint_is_bit_exact(name, tmp_path):
    """(11) A: three deterministic steps.  B: two steps, then ReferenceCheckpointManager.save.  C: a fresh model from another seed
    and a fresh optimizer, resume_reference, then step three: loss bytes, flat_grads, flat_params and a 'test' render equal A's."""
    c, batches = _case(name)
    a = _det_model(**c)
    want = _train(a, nlt_amd.optim.AdamAMSGrad(a, 1e-3), batches[:3])
    want_render = _render(a, batches[3])

    b = _det_model(**c)
    opt_b = nlt_amd.optim.AdamAMSGrad(b, 1e-3)
    _train(b, opt_b, batches[:2])
    prefix = trainvali.save_reference(ckpt.ReferenceCheckpointManager(str(tmp_path), max_to_keep=1), b, opt_b, 2)
    assert prefix == str(tmp_path / 'ckpt-1')

    c_model = _det_model(**dict(c, seed=6))
    assert not torch.equal(c_model.flat_params.detach(), b.flat_params.detach())
    opt_c = nlt_amd.optim.AdamAMSGrad(c_model, 1e-3)
    assert trainvali.resume_reference(ckpt.ReferenceCheckpointManager(str(tmp_path)), c_model, opt_c) == 2 and opt_c.t == 2
    for x, y in zip(c_model.bucket_to_variables(c_model.flat_params), b.bucket_to_variables(b.flat_params)):
        assert torch.equal(x, y)
    got = _train(c_model, opt_c, batches[2:3])
    _same_step(got, want)
    for x, y in zip(_render(c_model, batches[3]), want_render):
        assert torch.equal(x, y)


def _graphed_leg(save_dir):
    c, batches = _case('l2_cam_eq_im')
    pm = _det_model(**c)
    opt = nlt_amd.optim.AdamAMSGrad(pm, 1e-3)
    step = trainvali.GraphedTrainStep(pm, opt, N, warmup=1)
    for i in range(3):                                                        # eager, capture + replay, replay
        step(batches[i % 2])
    torch.cuda.synchronize()
    assert step.failed is None and step.graph is not None
    graph = step.graph
    if save_dir is not None:
        before = (pm.flat_params._version, pm._epoch[0], pm.plan.replay_stamp(pm.pack_registry), pm.flat_params.data_ptr())
        params = pm.flat_params.detach().clone()
        prefix = ckpt.ReferenceCheckpointManager(save_dir).save(pm, opt, 3)
        assert (pm.flat_params._version, pm._epoch[0], pm.plan.replay_stamp(pm.pack_registry), pm.flat_params.data_ptr()) == before
        assert torch.equal(pm.flat_params.detach(), params)
        saved = ckpt.read_bundle(prefix)                                      # ... and the file holds the weights of that moment
        assert saved['optimizer/iter/.ATTRIBUTES/VARIABLE_VALUE'] == 3
        k = pm.net['query'].layers[0].kernel
        assert saved['net/net_query_layer0/kernel/.ATTRIBUTES/VARIABLE_VALUE'].tobytes() == k.detach().cpu().numpy().tobytes()
    loss, _ = step(batches[1])
    torch.cuda.synchronize()
    assert step.graph is graph and step.failed is None                        # replayed, not captured again
    return loss.clone(), pm.flat_grads.clone(), pm.flat_params.detach().clone()


def test_saving_between_two_replays_disturbs_nothing(tmp_path):
    """(12) a GraphedTrainStep in its replaying state; a save between two replays changes neither `flat_params._version`,
    `model._epoch[0]` nor `plan.replay_stamp(pack_registry)`, and the next replay gives what a twin that did not save gives."""
    _same_step(_graphed_leg(str(tmp_path)), _graphed_leg(None))
