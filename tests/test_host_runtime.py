"""CPU: host-side runtime pieces that need no GPU -- the launch-tape bookkeeping of nlt_amd._capi (what is recorded, when
a tape stops being valid) and the PackRegistry that refreshes every packed weight buffer with one launch."""
import pytest
import torch

import nlt_amd
from nlt_amd import capi as C
from nlt_amd.networks.elements import Conv2D, PackRegistry
from oracle import nlt_oracle as O
import fake_capi
from test_host_orchestration import make, cpu_batch


def test_tape_records_only_successful_launches_and_is_invalidated_by_reallocation():
    C.tape_begin()
    with pytest.raises(C.NLTError):
        C.tape_begin()                                             # one tape at a time
    L = C.lib()
    assert L.nlt_packed_weight_floats(C.CONV_K2S1, 16, 0, 16) > 0  # size query: pure, never recorded
    assert L.nlt_conv_forward(C.CONV_K2S1, C.ALGO_DIRECT, 0, None, 16, 16, None, 0, 0, 1, 4, 4, None, None, None, 16, None, 16,
                              1, 0.3, None, 0, 0, None) == -1      # rejected before any launch: not recorded either
    ev_calls = []

    class Ev:
        def record(self, stream):
            ev_calls.append(('record', stream))

    class St:
        def wait_event(self, ev):
            ev_calls.append(('wait', ev))
    ev, st = Ev(), St()
    C.record_event(ev, 'main')
    C.wait_event(st, ev)
    tape = C.tape_end(tag=7)
    assert [a for _, a in tape[0]] == [('main',), (ev,)] and tape[2] == 7
    assert C.tape_valid(tape, 7) and not C.tape_valid(tape, 8) and not C.tape_valid(None, 7)
    C.replay(tape)                                                 # event helpers return None = success
    assert ev_calls == [('record', 'main'), ('wait', ev)] * 2
    C._workspace('test_host_runtime', torch.device('cpu'), 16)     # a cached buffer is (re)allocated ...
    assert not C.tape_valid(tape, 7)                               # ... every older tape may point into freed memory
    C.tape_begin()
    C._workspace('test_host_runtime', torch.device('cpu'), 64)     # growth WHILE recording: the tape is discarded
    assert C.tape_end() is None
    assert C.lib() is C._load()                                    # the recording proxy is gone once the tape is closed


def test_pack_registry_refreshes_once_per_weight_update_and_tracks_its_buffers(monkeypatch):
    fake_capi.install(monkeypatch)
    calls = []
    monkeypatch.setattr(C, 'repack_weights', lambda *a: calls.append(a))
    om, pm = make(256, 64, 32)
    pm.build('cpu'); pm.register_trainable()
    reg = pm.pack_registry
    batch, nn = O.synth_batch(1, 64, 64, 32, 32, 32, 32, k=2, seed=3)
    b = cpu_batch(batch, nn)
    with torch.no_grad():
        pm.call(b, 'test')
    n_entries, v0 = len(reg.entries), reg.version
    assert n_entries > 20 and v0 == n_entries and not calls         # first use packs layer by layer and registers
    with torch.no_grad():
        pm.call(b, 'test')
    assert not calls and reg.version == v0                          # nothing changed: no refresh, no new buffers
    with torch.no_grad():
        pm.flat_params.mul_(1.5)                                    # in-place write of the bucket (version counter)
        pm.call(b, 'test')
    assert len(calls) == 1                                          # ONE launch for all of them, at the top of the forward
    pm.mark_weights_updated()                                       # raw-pointer write (optimizer kernel): epoch counter
    with torch.no_grad():
        pm.call(b, 'test')
        pm.call(b, 'test')
    assert len(calls) == 2 and reg.version == v0
    conv = pm.net['query'].layers[1].convs()[0][0]
    conv.set_weights(conv.kernel.clone() * 2, conv.bias.clone())    # same shape: in place, buffers keep their slots
    assert reg.version == v0 + 1 and all(v[0] is not conv for v in reg.entries.values())   # its stale buffers are dropped


def test_replay_stamp_changes_on_the_three_events_that_let_baked_in_memory_go_and_on_nothing_else(monkeypatch):
    """RenderPlan.replay_stamp: what a captured hipGraph (Model._graphs, trainvali.GraphedTrainStep) compares before it replays.
    It moves when the plan's buffer set is replaced, when cached scratch is re-allocated and when the set of packed fragment
    buffers changes -- and stays put over repeated calls, in-place input changes and weight updates (the refresh is in place)."""
    fake_capi.install(monkeypatch)
    monkeypatch.setattr(C, 'repack_weights', lambda *a: None)
    om, pm = make(256, 64, 32)
    pm.build('cpu'); pm.register_trainable()
    reg, plan = pm.pack_registry, pm.plan
    a = cpu_batch(*O.synth_batch(2, 64, 64, 32, 32, 32, 32, k=2, seed=3))
    b = cpu_batch(*O.synth_batch(1, 64, 64, 32, 32, 32, 32, k=2, seed=4))
    with torch.no_grad():
        pm.call(a, 'test')
        s0 = plan.replay_stamp(reg)
        assert s0 == (plan.buffer_serial, C._alloc_epoch[0], reg.version) and all(type(x) is int for x in s0)
        pm.call(a, 'test'); pm.call(a, 'test')
        assert plan.replay_stamp(reg) == s0                          # a repeated call
        a[1].mul_(0.5); a[9].add_(0.1)
        pm.call(a, 'test')
        assert plan.replay_stamp(reg) == s0                          # inputs changed in place
        pm.flat_params.mul_(1.01); pm.mark_weights_updated()
        pm.call(a, 'test')
        assert plan.replay_stamp(reg) == s0                          # a weight update: fragments refreshed where they are
        pm.call(b, 'test')                                           # 1. another shape: the buffer set is replaced
        s1 = plan.replay_stamp(reg)
        assert s1[0] == s0[0] + 1 and s1[1:] == s0[1:]
        pm.call(a, 'test')                                           # ... and coming back replaces it again (one shape resident)
        s2 = plan.replay_stamp(reg)
        assert s2[0] == s1[0] + 1 and s2[1:] == s0[1:]
    C._workspace('test_replay_stamp', torch.device('cpu'), 16)       # 2. cached scratch (re)allocated, by whomever
    s3 = plan.replay_stamp(reg)
    assert s3[1] == s2[1] + 1 and (s3[0], s3[2]) == (s2[0], s2[2])
    C._workspace('test_replay_stamp', torch.device('cpu'), 8)        # (fits: the same tensor)
    assert plan.replay_stamp(reg) == s3
    C._workspace('test_replay_stamp', torch.device('cpu'), 64)
    assert plan.replay_stamp(reg)[1] == s3[1] + 1
    s4 = plan.replay_stamp(reg)
    conv = pm.net['query'].layers[1].convs()[0][0]
    conv.set_weights(conv.kernel.clone() * 2, conv.bias.clone())     # 3. the set of packed buffers changes
    s5 = plan.replay_stamp(reg)
    assert s5[2] == s4[2] + 1 and s5[:2] == s4[:2]
    reg.begin_census(passes=0); reg.tick()                           # (a census retiring fragment buffers nobody asked for)
    assert plan.replay_stamp(reg)[2] == s5[2] + 1
    assert plan.replay_stamp(None) == (s5[0], s5[1], -1)             # a model without a registry


def test_a_later_round_of_trials_cannot_take_a_launch_away_from_the_kind_that_won_it_first():
    """RenderPlan.set_choice: a second round of plan-time trials (another kind of pass over the same labels) may add what ranks
    BELOW a stored choice -- a wave tile / split-K for the passes the LDS kernel cannot take -- never a direct / lds / wino / c32
    choice that would re-route a launch whose tape or graph is already recorded."""
    _, pm = make(256, 64, 32)
    plan = pm.plan
    plan.clear_choices()
    plan.set_choice('L4.q.s1', 'splitk', (17, 16))                   # round 1: split-K won the label
    for kind, hint in (('lds', 32), ('wino', 32), ('c32', 1), ('direct', 0), ('tile', 34), ('splitk', (18, 4))):
        plan.set_choice('L4.q.s1', kind, hint)                       # round 2: whatever its clock says
    assert plan.export_tuning() == {'tile_hints': {'L4.q.s1': 17}, 'splitk_hints': {'L4.q.s1': 16}, 'algo_hints': {},
                                    'lds_hints': {}, 'wino_hints': {}, 'c32_hints': {}}
    plan.clear_choices()
    plan.set_choice('L3.o.s1', 'lds', 1024 + 512 + 32)               # the level hand-off takes the stride-1 label first ...
    plan.set_choice('L3.o.s1', 'tile', 18)                           # ... and the label's own winner ranks below it: stored
    plan.set_choice('L3.o.s1', 'wino', 32); plan.set_choice('L3.o.s1', 'lds', 64); plan.set_choice('L3.o.s1', 'c32', 2)
    assert plan.lds_hints == {'L3.o.s1': 1024 + 512 + 32} and plan.tile_hints == {'L3.o.s1': 18}
    assert not plan.wino_hints and not plan.c32_hints and not plan.algo_hints and not plan.splitk_hints


def test_registry_is_optional_for_stand_alone_layers(monkeypatch):
    fake_capi.install(monkeypatch)
    conv = Conv2D(16, 2, 1)
    conv.build(16, 'cpu', seed=1)
    a = conv.packed(16, 0)
    conv.kernel.mul_(2.0)
    assert conv.packed(16, 0) is not a or True                      # re-packed by itself (no registry): must not raise
    reg = PackRegistry()
    reg.refresh(); reg.refresh_if_stale()                           # empty registry: no-ops
