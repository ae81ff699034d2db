"""tests/stream_delay_util.py on the CPU: the delay-point hooks fire once per event record / launch of a pass, in issue order, see
the stream each belongs to, and put back what they patched; `poison` fills exactly the per-pass buffers of a plan (fake_capi's
emulated kernels) and nothing that is an input or state -- and a poisoned pass computes the bits of a clean one."""
import pytest
import torch

import fake_capi
import retire_util as R
import stream_delay_util as SD
from nlt_amd import capi as C
from oracle import nlt_oracle as O
from test_host_orchestration import make, cpu_batch


class _Stream:
    def __init__(self, handle):
        self.cuda_stream = handle


class _Event:
    def __init__(self, log):
        self.log = log

    def record(self, stream):
        self.log.append(('record', stream.cuda_stream))


class _Lib:
    """Stands where the loaded library stands: every entry point takes its arguments + the stream and reports success."""

    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        return lambda *args: self.log.append(('launch', name, args[-1])) or 0


def _scripted_pass(log, current):
    """A pass shaped like the fused forward: front launch, fork (record on main), two launches per stream, join (record on side)."""
    main, side = _Stream(11), _Stream(22)
    ev = [_Event(log) for _ in range(3)]
    current[0] = 11
    C._call('nlt_front', 1, 2)
    C.record_event(ev[0], main)
    C._call('nlt_obs_a', 3)
    C.record_event(ev[1], main)
    current[0] = 22
    C._call('nlt_query_a')
    C._call('nlt_query_b')
    C.record_event(ev[2], side)
    current[0] = 11
    C._call('nlt_back', 4)


def test_hooks_fire_once_per_record_and_launch_in_issue_order_and_are_taken_out_again(monkeypatch):
    log, current = [], [11]
    monkeypatch.setattr(C, 'lib', lambda: _Lib(log))
    monkeypatch.setattr(C, '_stream', lambda: current[0])
    real_record, real_call = C.record_event, C._call
    seen = []
    with SD.delay_points(monkeypatch, after_record=lambda k, s: (seen.append(('after_record', k, s.cuda_stream)), log.append(('hook_r', k))),
                         before_call=lambda n, name: (seen.append(('before_call', n, name, current[0])), log.append(('hook_c', n)))) as dp:
        assert C.record_event is not real_record and C._call is not real_call
        _scripted_pass(log, current)
        dp.mark('end')
    assert C.record_event is real_record and C._call is real_call            # restored, also for the code that looks them up late
    assert [s.cuda_stream for s in dp.records] == [11, 11, 22]
    assert dp.calls == [('nlt_front', 11), ('nlt_obs_a', 11), ('nlt_query_a', 22), ('nlt_query_b', 22), ('nlt_back', 11)]
    assert dp.marks == [('end', 3, 5)]
    assert seen == [('before_call', 0, 'nlt_front', 11), ('after_record', 0, 11), ('before_call', 1, 'nlt_obs_a', 11),
                    ('after_record', 1, 11), ('before_call', 2, 'nlt_query_a', 22), ('before_call', 3, 'nlt_query_b', 22),
                    ('after_record', 2, 22), ('before_call', 4, 'nlt_back', 11)]
    # a launch hook runs BEFORE its launch, a record hook AFTER its record; every launch and record happened exactly once
    assert log == [('hook_c', 0), ('launch', 'nlt_front', 11), ('record', 11), ('hook_r', 0),
                   ('hook_c', 1), ('launch', 'nlt_obs_a', 11), ('record', 11), ('hook_r', 1),
                   ('hook_c', 2), ('launch', 'nlt_query_a', 22), ('hook_c', 3), ('launch', 'nlt_query_b', 22), ('record', 22), ('hook_r', 2),
                   ('hook_c', 4), ('launch', 'nlt_back', 11)]
    # outside the block nothing is counted any more
    del log[:]
    _scripted_pass(log, current)
    assert len(dp.calls) == 5 and len(dp.records) == 3 and len([x for x in log if x[0] == 'launch']) == 5


def test_hooks_are_taken_out_when_the_pass_raises_and_a_failing_launch_still_raises(monkeypatch):
    class Failing:
        def __getattr__(self, name):
            if name == 'nlt_status_string':
                return lambda status: b'refused'
            return lambda *args: 1 if name == 'nlt_bad' else 0
    monkeypatch.setattr(C, 'lib', lambda: Failing())
    monkeypatch.setattr(C, '_stream', lambda: 0)
    real_record, real_call = C.record_event, C._call
    with pytest.raises(C.NLTError):
        with SD.delay_points(monkeypatch) as dp:
            C._call('nlt_good')
            C._call('nlt_bad')
    assert dp.calls == [('nlt_good', 0), ('nlt_bad', 0)]
    assert C.record_event is real_record and C._call is real_call


def test_the_nth_hooks_pick_one_point(monkeypatch):
    hits = []
    monkeypatch.setattr(SD, 'stall', lambda stream, ms: hits.append((stream, ms)))
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a: 'cur')
    r, c = SD.stall_after_record(2, 7.0), SD.stall_before_call(1, 9.0)
    for i in range(4):
        r(i, 's%d' % i)
        c(i, 'nlt_x')
    assert hits == [('cur', 9.0), ('s2', 7.0)]


# ------------------------------------------------------------------------------------------------------------ poison
def _tensors(x, path=''):
    if torch.is_tensor(x):
        return [(path, x)] if x.numel() else []
    if isinstance(x, dict):
        return [t for k, v in x.items() for t in _tensors(v, '%s[%r]' % (path, k))]
    if isinstance(x, (list, tuple)):
        return [t for i, v in enumerate(x) for t in _tensors(v, '%s[%d]' % (path, i))]
    return []


def _trained_model(monkeypatch):
    fake_capi.install(monkeypatch)
    monkeypatch.setattr(C, '_ws_cache', {})
    _, pm = make(256, 64, 32)
    pm.build('cpu'); pm.register_trainable()
    a = cpu_batch(*O.synth_batch(2, 64, 64, 32, 32, 32, 32, k=2, seed=3))
    pm.train_forward_backward(a, 2)                                   # activations AND gradient buffers exist
    return pm, a


def test_poison_fills_the_per_pass_buffers_of_a_plan_and_nothing_else(monkeypatch):
    pm, a = _trained_model(monkeypatch)
    (bufs,) = pm.plan._bufs.values()
    bufs['tapes'] = {'k': (torch.zeros(3),)}
    bufs['idx'] = torch.arange(4, dtype=torch.int32)
    ws = C._workspace('poison_fam', 'cpu', 16, zero=True)
    if not _tensors(pm.plan._front_blob):
        pm.plan._front_blob = [('stamp',), torch.ones(7), torch.ones(11), ('stamp',)]
    reg = pm.pack_registry
    keep = [(p, t, t.clone()) for p, t in _tensors(pm.plan._front_blob, 'blob') + [('ws', ws)] + _tensors(bufs['tapes'], 'tapes')
            + [('idx', bufs['idx']), ('zero_bias', bufs['grads']['zero_bias'])]
            + [('pack%d' % i, e[2]) for i, e in enumerate(reg.entries.values()) if torch.is_tensor(e[2])]
            + [('params', pm.flat_params.detach()), ('grads', pm.flat_grads)]]
    paths = SD.poison(pm)
    want = [(p, t) for p, t in _tensors({k: v for k, v in bufs.items() if k != 'tapes'}, 'plan._bufs[%r]' % (next(iter(pm.plan._bufs)),))
            if t.dtype.is_floating_point and not p.endswith("['grads']['zero_bias']")]
    assert sorted(paths) == sorted(p for p, _ in want) and len(paths) > 40
    for name in ('fm', 'obs', 'qtmp', 'otmp', 'dtmp', 'dec'):
        assert any("[%r]" % name in p and "['grads']" not in p for p in paths) and any("['grads'][%r]" % name in p for p in paths)
    assert any(p.endswith("['pred']") for p in paths)
    for p, t in want:
        assert bool((t == R.SENTINEL).all()), p
    for p, t, before in keep:
        assert torch.equal(t, before), p
    assert not bool(bufs['grads']['zero_bias'].any())
    # an exclusion by name
    for _, t in want:
        t.zero_()
    paths2 = SD.poison(pm, exclude=("['fm'][3]",))
    assert set(paths) - set(paths2) == {p for p in paths if p.endswith("['fm'][3]")} and len(paths) - len(paths2) == 2
    assert not bool(bufs['fm'][3].any()) and not bool(bufs['grads']['fm'][3].any())
    # several models: every plan under its own name
    import copy
    from nlt_amd.engine import RenderPlan
    lane = copy.copy(pm)
    lane.plan = RenderPlan(pm.net['query'], pm.net['obs'], pm.use_obs)
    with torch.no_grad():
        lane.call(a, 'test')
    both = SD.poison([pm, lane])
    assert any(p.startswith('models[0].plan._bufs[') for p in both) and any(p.startswith('models[1].plan._bufs[') for p in both)
    (lb,) = lane.plan._bufs.values()
    assert bool((lb['pred'] == R.SENTINEL).all())


def test_a_poisoned_pass_computes_what_a_clean_pass_computes(monkeypatch):
    """The self-check of every GPU scenario, on the emulated kernels: no pass reads one of its buffers before writing it."""
    pm, a = _trained_model(monkeypatch)
    with torch.no_grad():
        ref = [t.clone() for t in pm.call(a, 'test')[3].values() if torch.is_tensor(t)]
        SD.poison(pm)
        got = [t.clone() for t in pm.call(a, 'test')[3].values() if torch.is_tensor(t)]
    assert len(ref) >= 3 and all(torch.equal(x, y) for x, y in zip(ref, got))
    loss, _ = pm.train_forward_backward(a, 2)
    grads = pm.flat_grads.clone()
    SD.poison(pm)
    loss2, _ = pm.train_forward_backward(a, 2)
    assert torch.equal(loss, loss2) and torch.equal(grads, pm.flat_grads) and float(grads.abs().sum()) > 0


def test_blame_names_the_buffer_a_pass_reads_before_writing_it():
    class Plan:
        _bufs = {'k': {'a': torch.zeros(4), 'state': torch.ones(4), 'out': torch.zeros(4)}}

    class Model:
        plan = Plan()
    b = Plan._bufs['k']

    def run():
        b['a'].copy_(torch.arange(4.0))                             # rewritten by every pass
        b['out'].copy_(b['a'] + b['state'])                         # 'state' is read and never written
        return b['out'].clone()
    ref = run()
    bad = SD.blame(Model(), run, lambda out: torch.equal(out, ref))
    assert bad[0] == "plan._bufs['k']['state']"                     # (and whatever follows it: nothing restores a state buffer)
    b['state'].fill_(1.0)
    assert SD.blame(Model(), run, lambda out: torch.equal(out, ref), exclude=("['state']",)) == []


def test_independent_streams_keeps_only_streams_that_no_chosen_one_holds_back(monkeypatch):
    """Four queues, candidates bound to them in turn (the caller's stream on queue 0): the choice is one stream per queue, the
    caller's first, found once; asking for more than there are queues raises instead of handing out streams that share one."""
    made = []

    class Stream:
        def __init__(self, priority=0, handle=None):
            self.cuda_stream = len(made) + 100 if handle is None else handle
            self.queue = 0 if handle == 0 else (len(made) * 2) % 4       # queues 0, 2, 0, 2, ... then the odd ones by priority
            if priority:
                self.queue = 1 + (len(made) % 2) * 2
            made.append(self)
    cur = Stream(handle=0)
    probes = []
    monkeypatch.setattr(SD, '_independent', [])
    monkeypatch.setattr(torch.cuda, 'Stream', Stream)
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a: cur)
    monkeypatch.setattr(SD, 'holds_back', lambda a, b, ms=None: probes.append((a, b)) or a.queue == b.queue)
    two = SD.independent_streams(2)
    assert two[0] is cur and two[1].queue == 2 and len(made) == 2
    n_probes = len(probes)
    assert SD.independent_streams(2) == two and len(probes) == n_probes          # found once per process
    four = SD.independent_streams(4)
    assert four[:2] == two and sorted(s.queue for s in four) == [0, 1, 2, 3]
    assert all(s.cuda_stream >= 100 + 32 for s in four[2:])                     # (the odd queues only came with the other priority)
    with pytest.raises(AssertionError, match="only 4 of 5 streams"):
        SD.independent_streams(5)
