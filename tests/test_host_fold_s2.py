"""CPU: the plan side of the level hand-off launch (engine.FOLD_HINT: level l's stride-1 observation conv + level l + 1's stride-2
one in one launch) under the SCRIPTED timer and the stand-in adapters of tests/test_host_autotune.py.

The kernel exists on the GPU only, so here the plan is told it exists (`_fold_trial`, `_fold_ok`) and the launch is computed by
the two convs it stands for.  What is checked is host logic: which launches the trial makes, that the candidate is held against
the SUM of the two launches it replaces, that the choice travels through export / import, that a training forward and a plan
without the choice launch the two convs, and that the rendered texels do not depend on the choice."""
import pytest
import torch

from nlt_amd import _capi as C
from nlt_amd import engine
import fake_capi
import test_host_autotune as HA
from test_host_orchestration import make, cpu_batch
from oracle import nlt_oracle as O

LABEL, PARTNER = 'L2.o.s1', 'L3.o.s2'


def conv_tile3w_s2_forward(src, ld, cin, frames, kobs, h, w, packed, bias, cout, mean_out, ldm, packed2, bias2, cout2, out2, ldo2,
                           act=True, alpha=0.3, act2=True, alpha2=0.3, nprod=6, max_workgroups=0, out=None, ldo=0):
    assert out is None and (cin, cout, cout2) == (32, 32, 64) and nprod in (6, 9)
    y1 = torch.empty(frames * kobs, h, w, cout)
    fake_capi.conv_tile_forward(C.CONV_K2S1, src, ld, cin, frames, kobs, h, w, packed, bias, cout, 32, y1, cout, mean_out, ldm, act, alpha)
    fake_capi.conv_tile_forward(C.CONV_K2S2, y1, cout, cout, frames * kobs, 1, h, w, packed2, bias2, cout2, 64, out2, ldo2, None, 0,
                                act2, alpha2)


def _plan(monkeypatch, price):
    """The f32x3_9 fused inference case of test_host_autotune (depth 256, 64 x 64, k = 3, 2 frames) with the hand-off on offer
    and priced at `price` (16 = par) by the script."""
    HA.install(monkeypatch)
    monkeypatch.setenv('NLT_SPLITK', 'off')
    monkeypatch.setattr(C, 'conv_tile3w_s2_forward', conv_tile3w_s2_forward)
    monkeypatch.setattr(C, 'pack_conv_tile3w_s2_weights', lambda w, cin2, cout2: w)
    monkeypatch.setitem(HA.BIAS, 'conv_tile3w_s2_forward', price)
    plan, run, _ = HA._forward_case(True, 'f32x3_9')
    plan._fold_trial = lambda: True
    plan._fold_ok = lambda layer, cin, nxt: (cin, layer.n_ch_out, nxt.n_ch_out) == (32, 32, 64)
    return plan, run


def _best(res, fold):
    return min(t for t, kind, hint in res if (kind == 'lds' and hint == engine.FOLD_HINT) == fold)


@pytest.mark.parametrize('price,chosen', [(1, True), (64, False)])
def test_the_candidate_is_held_against_the_sum_of_the_two_launches(monkeypatch, price, chosen):
    plan, run = _plan(monkeypatch, price)
    HA.Scripted.log = [[]]
    HA._spy_launches(plan)
    plan._autotune(run)
    res, res2 = plan.tuned[LABEL], plan.tuned[PARTNER]
    t_fold, t_two = _best(res, True), _best(res, False) + min(res2)[0]
    assert (t_fold < t_two) == chosen                                   # (the script's prices put the two cases on either side)
    assert (plan.lds_hints.get(LABEL) == engine.FOLD_HINT) == chosen
    assert not any(kind == 'lds' and hint == engine.FOLD_HINT for _, kind, hint in res2)
    # the trial's launches: the hand-off under the stride-1 label, no launch under the partner's, every other label as without it
    seg = [s for s in HA.Scripted.log if any(fn == 'conv_tile3w_s2_forward' for _, fn, _ in s)]
    assert len(seg) == 2                                                # the trial's untimed run closes one segment, its two timed runs are the next
    starts = [i for i, (l, _, _) in enumerate(seg[1]) if l == 'F.front']     # (the next trial's untimed run follows in the same segment)
    timed = seg[1][:starts[2]] if len(starts) > 2 else seg[1]
    labels = [l for l, _, _ in timed]
    assert LABEL in labels and PARTNER not in labels and [fn for l, fn, _ in timed if l == LABEL] == ['conv_tile3w_s2_forward'] * 2
    assert sum(fn == 'conv_tile3w_s2_forward' for s in HA.Scripted.log for _, fn, _ in s) == 3
    # the partner keeps a choice of its own for the plans that still launch it
    assert any(PARTNER in getattr(plan, a) for a in engine.HINT_DICTS) or min(res2)[1] == 'tile'


def test_the_choice_travels_and_only_inference_plans_use_it(monkeypatch):
    plan, run = _plan(monkeypatch, 1)
    plan._autotune(run)
    assert plan.lds_hints[LABEL] == engine.FOLD_HINT
    tuning = plan.export_tuning()
    # a second plan over other weights imports the choice and launches the same kernels
    _, pm = make(256, 64, 32)
    pm.plan.fuse_ends, pm.plan.precision = True, 'f32x3_9'
    pm.plan._fold_trial, pm.plan._fold_ok = plan._fold_trial, plan._fold_ok
    pm.plan.import_tuning(tuning)
    assert pm.plan.export_tuning() == tuning and pm.plan.autotune is False
    batch, nn = O.synth_batch(2, 64, 64, 32, 32, 32, 32, k=3, seed=2)
    cb = cpu_batch(batch, nn)
    HA.Scripted.log = [[]]
    HA._spy_launches(pm.plan)
    folded = pm.call(cb, 'test')[3]['pred'].clone()
    names = {l: fn for l, fn, _ in HA.Scripted.log[-1]}
    assert names[LABEL] == 'conv_tile3w_s2_forward' and PARTNER not in names
    # without the choice (and with the kernel switched off): the two launches, the same texels to rounding
    pm.plan.fold_s2 = False
    pm.plan._fold_ok = engine.RenderPlan._fold_ok.__get__(pm.plan)
    pm.plan._drop_tapes()
    HA.Scripted.log.append([])
    two = pm.call(cb, 'test')[3]['pred']
    names = {l: fn for l, fn, _ in HA.Scripted.log[-1]}
    assert names[LABEL] == 'conv_tile3r_forward' and PARTNER in names
    assert torch.allclose(folded, two, rtol=1e-5, atol=1e-6)
    assert engine.RenderPlan._fold_partner(LABEL) == PARTNER and engine.RenderPlan._fold_partner('L2.q.s1') is None
    assert engine.hint_word(engine.FOLD_HINT) == (32, False, True) and engine.FOLD_HINT & 255 == 32
