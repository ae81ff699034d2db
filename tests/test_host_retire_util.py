"""tests/retire_util.py on CPU (the plan on fake_capi's emulated kernels): the walk reaches every container the project keeps
device tensors in, a shape change retires exactly the previous buffer set, scratch growth exactly the previous scratch, and
`check()` sees a single element written into a retired tensor -- and nothing else."""
import pytest
import torch

import fake_capi
import retire_util as R
from nlt_amd import capi as C
from oracle import nlt_oracle as O
from test_host_orchestration import make, cpu_batch


def _model(monkeypatch):
    fake_capi.install(monkeypatch)
    monkeypatch.setattr(C, '_ws_cache', {})                         # (this test's scratch families only; undone on the way out)
    _, pm = make(256, 64, 32)
    pm.build('cpu'); pm.register_trainable()
    a = cpu_batch(*O.synth_batch(2, 64, 64, 32, 32, 32, 32, k=2, seed=3))
    b = cpu_batch(*O.synth_batch(1, 64, 64, 32, 32, 32, 32, k=2, seed=4))
    with torch.no_grad():
        pm.call(a, 'test')
    return pm, a, b


def _tensors(x, skip=('tapes',)):
    if torch.is_tensor(x):
        return [x] if x.numel() else []
    if isinstance(x, dict):
        return [t for k, v in x.items() if k not in skip for t in _tensors(v)]
    if isinstance(x, (list, tuple)):
        return [t for v in x for t in _tensors(v)]
    return []


def _keys(ts):
    return {(t.data_ptr(), t.numel() * t.element_size()) for t in ts}


def test_the_walk_reaches_every_container(monkeypatch):
    pm, a, _ = _model(monkeypatch)
    (bufs,) = pm.plan._bufs.values()
    bufs['tapes'] = {'k': (torch.zeros(3),)}                        # whatever hangs under 'tapes' is nobody's buffer
    bufs['nested'] = {'deep': [(torch.zeros(5), [torch.zeros(6, dtype=torch.int32)])]}
    ws = C._workspace('retire_fam', 'cpu', 16)
    ws2 = C._workspace((7, 11), 'cpu', 8)                            # the split-K kind of key: (device, stream, plan token)
    reg = pm.pack_registry
    assert len(reg.entries) > 20
    reg.table = (torch.zeros(9), len(reg.entries), 0)               # (the emulated table holds no tensor)
    if not _tensors(pm.plan._front_blob):                            # (the emulated front kernel folds no weights)
        pm.plan._front_blob = [('stamp',), torch.zeros(7), torch.zeros(11), ('stamp',)]
    own = R.owned(pm)
    census = R._census(pm)
    path = lambda t: census[(t.data_ptr(), t.numel() * t.element_size())][0]
    for name in ('fm', 'obs', 'qtmp', 'otmp', 'dtmp', 'dec'):
        for i, t in enumerate(bufs[name]):
            if t is not None:
                assert own[(t.data_ptr(), t.numel() * t.element_size())] is t and path(t).endswith("[%r][%d]" % (name, i)), (name, i)
    assert path(bufs['pred']).startswith('plan._bufs[') and path(bufs['pred']).endswith("['pred']")
    assert path(bufs['nested']['deep'][0][0]).endswith("['nested']['deep'][0][0]")
    assert path(bufs['nested']['deep'][0][1][0]).endswith("['nested']['deep'][0][1][0]")
    assert _keys(_tensors(bufs['tapes'])).isdisjoint(own)
    assert path(ws) == "_ws_cache[('cpu', 'retire_fam')]" and path(ws2) == "_ws_cache[('cpu', 7, 11)]"
    blobs = _tensors(pm.plan._front_blob)
    assert blobs and all(path(t).startswith('plan._front_blob[') for t in blobs)
    assert all(path(ent[2]).startswith('pack_registry.entries[') for ent in reg.entries.values())
    assert path(reg.table[0]) == 'pack_registry.table[0]'
    want = _keys(_tensors(bufs) + _tensors(pm.plan._front_blob) + [ws, ws2, reg.table[0]] + [e[2] for e in reg.entries.values()])
    assert set(own) == want                                          # ... and nothing else
    # several models (pipeline lanes): each plan under its own name, the shared registry and scratch once
    import copy
    from nlt_amd.engine import RenderPlan
    lane = copy.copy(pm)
    lane.plan = RenderPlan(pm.net['query'], pm.net['obs'], pm.use_obs)
    with torch.no_grad():
        lane.call(a, 'test')
    both = R._census([pm, lane])
    (lb,) = lane.plan._bufs.values()
    assert both[(lb['pred'].data_ptr(), lb['pred'].numel() * 4)][0].startswith('models[1].plan._bufs[')
    assert both[(bufs['pred'].data_ptr(), bufs['pred'].numel() * 4)][0].startswith('models[0].plan._bufs[')
    assert set(both) == want | _keys(_tensors(lb) + _tensors(lane.plan._front_blob))


def test_a_shape_change_retires_exactly_the_old_buffer_set(monkeypatch):
    pm, a, b = _model(monkeypatch)
    (old,) = pm.plan._bufs.values()
    old['idx'] = torch.zeros(3, dtype=torch.int32)                   # an integer tensor: retired, never armed, listed
    serial = pm.plan.buffer_serial
    with R.Retired(pm) as r:
        with torch.no_grad():
            pm.call(a, 'test')                                       # the same shape: nothing is let go
    assert not r.retired and pm.plan.buffer_serial == serial
    with R.Retired(pm) as r:
        with torch.no_grad():
            pm.call(b, 'test')
    (new,) = pm.plan._bufs.values()
    assert new is not old and pm.plan.buffer_serial == serial + 1
    assert set(r.retired) == _keys(_tensors(old))
    assert all(p.startswith("plan._bufs[(2, 2, 64, 64, 'cpu', 'fp32')]") for p in r.paths())
    r.arm()
    assert r.skipped == ["plan._bufs[(2, 2, 64, 64, 'cpu', 'fp32')]['idx']"] and len(r.armed) == len(r.retired) - 1
    assert all(bool((t == R.SENTINEL).all()) for _, t in r.armed) and not bool(old['idx'].any())
    with torch.no_grad():
        pm.call(b, 'test'); pm.call(a, 'test'); pm.call(a, 'test')   # new sets every time the shape changes: none is the old one
    r.check()


def test_workspace_growth_retires_exactly_the_old_scratch(monkeypatch):
    pm, _, _ = _model(monkeypatch)
    small = C._workspace('retire_fam', 'cpu', 16)
    other = C._workspace('retire_other', 'cpu', 16)
    e0 = C._alloc_epoch[0]
    with R.Retired(pm) as r:
        assert C._workspace('retire_fam', 'cpu', 8) is small         # fits: the cached tensor, no epoch
    assert not r.retired and C._alloc_epoch[0] == e0
    with R.Retired(pm) as r:
        big = C._workspace('retire_fam', 'cpu', 64)
    assert big is not small and C._alloc_epoch[0] == e0 + 1
    assert set(r.retired) == _keys([small]) and r.paths() == ["_ws_cache[('cpu', 'retire_fam')]"]
    r.arm()
    big.zero_(); other.zero_()
    r.check()


@pytest.mark.parametrize('value', [0.0, float('nan'), -7.250001])
def test_check_fails_after_one_element_of_a_retired_tensor_is_written(monkeypatch, value):
    pm, _, b = _model(monkeypatch)
    (old,) = pm.plan._bufs.values()
    C._workspace('retire_fam', 'cpu', 16)
    with R.Retired(pm) as r:
        with torch.no_grad():
            pm.call(b, 'test')
        C._workspace('retire_fam', 'cpu', 64)
    r.arm().check()                                                  # armed and untouched: passes, as often as asked
    r.check()
    old['fm'][3].view(-1)[5] = value
    with pytest.raises(AssertionError, match=r"^plan\._bufs\[\(2, 2, 64, 64, 'cpu', 'fp32'\)\]\['fm'\]\[3\] was written after the "
                                             r"project let it go: 1 of \d+ elements, first at flat index 5 "):
        r.check()
    r.arm().check()                                                  # armed again: clean again
    r.retired[next(k for k, (p, _) in r.retired.items() if p.startswith('_ws_cache'))][1][15] = value
    with pytest.raises(AssertionError, match=r"^_ws_cache\[\('cpu', 'retire_fam'\)\] was written .* first at flat index 15 "):
        r.check()
