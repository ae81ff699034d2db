"""CPU: the plan-time trials of RenderPlan (`_autotune`) under a SCRIPTED timer -- which candidates they launch, what they record
in `plan.tuned` and which winner they store per label -- driven through the TEST-ONLY adapters of tests/fake_capi.py.

The "time" of a launch is a fixed function of what was launched (label, entry point, its integer and boolean arguments), never of
the plan's state: a restructuring of the host code cannot be noticed by the timing script, while any change in what a trial
launches moves the winners.  test_host_autotune.json was recorded from the code before `_trial` / `set_choice` existed and is never
regenerated from newer code (NLT_AUTOTUNE_DUMP names a file that receives what this run got, for a comparison by hand)."""
import json
import os
import zlib

import pytest
import torch

from nlt_amd import _capi as C
from nlt_amd import engine
from oracle import nlt_oracle as O
import fake_capi
import test_host_launch_trace as LT
from test_host_orchestration import make, cpu_batch

DUMP = os.environ.get('NLT_AUTOTUNE_DUMP')
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_host_autotune.json')
HINT_DICTS = ('tile_hints', 'algo_hints', 'lds_hints', 'splitk_hints', 'wino_hints', 'c32_hints')
# The script's price per entry point (16 = par), set on the recording code until every kernel family won a label somewhere.
BIAS = {'conv_c32_forward': 9, 'conv_tile_forward': 11, 'conv_tile3r_forward': 13, 'conv_tile_backward_data': 9,
        'conv_wino_backward_data': 9, 'obs_mean_forward': 6, 'conv_forward.direct': 9}


def _ints(x):
    """The integers and booleans among (nested) arguments, keyword names included; tensors, floats and None leave nothing."""
    if isinstance(x, bool):
        return [repr(x)]
    if isinstance(x, int):
        return [x]
    if isinstance(x, (list, tuple)):
        return [v for y in x for v in _ints(y)]
    if isinstance(x, dict):
        return [v for k in sorted(x) for v in [k] + _ints(x[k])]
    return []


class Scripted(engine.OpTimer):
    """An OpTimer whose clock is the script.  Every new timer (one per trial) opens a segment of the launch log."""
    log = None

    def __init__(self):
        super().__init__()
        Scripted.log.append([])

    def launch(self, label, nbytes, fn, *a, **kw):
        fn(*a, **kw)
        crc = zlib.crc32(repr((label, fn.__name__, _ints([a, kw]))).encode())
        r = self.records.setdefault(label, [0, 0.0, nbytes])
        r[0] += 1
        name = fn.__name__ + ('.direct' if kw.get('algo') == C.ALGO_DIRECT else '')
        r[1] += float(BIAS.get(name, 16) * (65536 + crc % 65536))             # (integers: sums and means stay exact)

    def collect(self):
        return self.records


# ---- stand-ins for the entry points fake_capi cannot compute or does not have.  The values they write do not matter to the
# selection; what they are asked to do is in the log.
def pack_conv_weights(mode, w_keras, c0, c1, cout):
    return w_keras                                  # (so that the split-K stand-in has the Keras array at hand)


def conv_forward_splitk(mode, ksplit, *a, **kw):
    srcs, packed, dst = a[:9], a[9], a[10:]
    fake_capi.conv_forward(mode, *srcs, packed, packed, *dst, **kw)


def conv_backward_data(*a, ksplit=1, **kw):
    fake_capi.conv_backward_data(*a, **kw)


def pack_conv_tile_weights_adjoint(adj_mode, w_keras, cpre, cout, tn, full, lo):
    return w_keras


def conv_tile_backward_data(adj_mode, dpre, cpre, ldp, n, h, w, packed, cout, tn, out, ldo, **kw):
    fake_capi.conv_backward_data(adj_mode, dpre, cpre, ldp, n, h, w, None, torch.zeros(cout), cout, out, ldo, **kw)


def conv_tile3r_forward(*a, max_workgroups=0, **kw):
    LT.conv_tile3_forward(*a, **kw)


def conv_backward_weights(*a, **kw):
    pass                                            # (nothing downstream of a weight gradient is timed: three quarters of the CPU time)


conv_backward_weights_tiled = conv_backward_weights_narrow = conv_backward_weights


def install(monkeypatch):
    fake_capi.install(monkeypatch)
    monkeypatch.setattr(C, 'pack_conv_tile3_weights', LT.pack_conv_tile3_weights)
    monkeypatch.setattr(C, 'conv_tile3_forward', LT.conv_tile3_forward)
    for name in ('pack_conv_weights', 'conv_forward_splitk', 'conv_backward_data', 'pack_conv_tile_weights_adjoint',
                 'conv_tile_backward_data', 'conv_tile3r_forward', 'conv_backward_weights', 'conv_backward_weights_tiled',
                 'conv_backward_weights_narrow'):
        monkeypatch.setattr(C, name, globals()[name])
    monkeypatch.setattr(engine, 'OpTimer', Scripted)
    monkeypatch.delenv('NLT_SPLITK', raising=False)
    monkeypatch.delenv('NLT_SPLITK_FORMS', raising=False)
    Scripted.log = [[]]


def _spy_launches(plan):
    """Every launch of the plan, timed or not, into the open segment of the log."""
    real = plan._launch

    def launch(label, nbytes, fn, *a, flops=0, moved=None, **kw):
        Scripted.log[-1].append((label, fn.__name__, _ints([a, kw])))
        real(label, nbytes, fn, *a, flops=flops, moved=moved, **kw)
    plan._launch = launch


def _forward_case(fused, precision='fp32'):
    """Inference at depth 256, 64 x 64, 3 observations, 2 frames."""
    _, pm = make(256, 64, 32)
    pm.plan.fuse_ends, pm.plan.precision = fused, precision
    batch, nn = O.synth_batch(2, 64, 64, 32, 32, 32, 32, k=3, seed=2)
    cb = cpu_batch(batch, nn)
    return pm.plan, (lambda: pm.call(cb, 'test')), {}


def _backward_case():
    """The backward of a train step (one observation per frame): an untuned step first, whose `backward` call is kept."""
    _, pm = make(256, 64, 32, loss='l2')
    pm.build('cpu'); pm.register_trainable()
    pm.plan.autotune = False
    batch, nn = O.synth_batch(2, 64, 64, 32, 32, 32, 32, k=1, seed=12)
    real, kept = pm.plan.backward, []
    pm.plan.backward = lambda *a, **kw: (kept.append((a, kw)), real(*a, **kw))[1]
    pm.train_forward_backward(cpu_batch(batch, nn), 2)
    del pm.plan.backward
    (a, kw), = kept
    kw.pop('generation', None)
    return pm.plan, (lambda: pm.plan.backward(*a, **kw)), {'backward': True}


CASES = {'fwd.fused': (lambda: _forward_case(True), 'all'),
         'fwd.plain': (lambda: _forward_case(False), 'all'),
         'fwd.f32x3_9.fused': (lambda: _forward_case(True, 'f32x3_9'), 'off'),
         'bwd.train.k1': (_backward_case, 'all')}


def _run_case(monkeypatch, name):
    install(monkeypatch)
    setup, splitk = CASES[name]
    monkeypatch.setenv('NLT_SPLITK', splitk)
    plan, run, kw = setup()
    Scripted.log = [[]]
    _spy_launches(plan)
    plan._autotune(run, **kw)
    segs = [[len(s), zlib.crc32(repr(s).encode())] for s in Scripted.log]
    got = {'tuning': plan.export_tuning(), 'tuned': plan.tuned, 'launches': segs}
    return json.loads(json.dumps(got))              # (tuples as lists, like the fixture)


_got = {}


@pytest.mark.parametrize('name', sorted(CASES))
def test_trials_launch_record_and_choose_what_was_recorded(monkeypatch, name):
    """`export_tuning()`, `plan.tuned` and the launches of every trial (per segment: how many, and a digest of their ordered
    (label, entry point, integer arguments)) equal the recorded ones."""
    got = _got[name] = _run_case(monkeypatch, name)
    if DUMP:
        os.makedirs(os.path.dirname(DUMP) or '.', exist_ok=True)
        with open(DUMP, 'w') as f:
            json.dump(_got, f, separators=(',', ':'), sort_keys=True)
            f.write('\n')
    with open(FIXTURE) as f:
        want = json.load(f)[name]
    assert got['tuning'] == want['tuning']
    assert got['launches'] == want['launches'], [i for i, (g, w) in enumerate(zip(got['launches'], want['launches'])) if g != w]
    assert sorted(got['tuned']) == sorted(want['tuned'])
    for label in want['tuned']:
        assert got['tuned'][label] == want['tuned'][label], label


def test_the_recorded_script_lets_every_kernel_family_win():
    """The fixture covers the whole selection: tile, direct, lds folded / unfolded / resident, wino, c32, split-K of both signs."""
    with open(FIXTURE) as f:
        want = json.load(f)
    assert sorted(want) == sorted(CASES)
    won = {a: [v for case in want.values() for v in case['tuning'][a].values()] for a in HINT_DICTS}
    assert won['tile_hints'] and won['algo_hints'] and won['wino_hints'] and won['c32_hints']
    assert any(v < 256 for v in won['lds_hints']) and any(256 <= v < 512 for v in won['lds_hints'])
    assert any(v >= 512 for v in want['fwd.f32x3_9.fused']['tuning']['lds_hints'].values())
    assert any(v > 1 for v in won['splitk_hints']) and any(v < -1 for v in won['splitk_hints'])
    assert any('dgrad' in label for a in HINT_DICTS for label in want['bwd.train.k1']['tuning'][a])


def test_a_trial_that_raises_leaves_the_plan_as_it_was(monkeypatch):
    """An exception inside a trial: the six dicts are what they were, no trial is running, the timer is the caller's."""
    install(monkeypatch)
    plan, run, _ = _forward_case(True)
    plan.lds_hints, plan.tile_hints, plan.splitk_hints = {'L3.q.s1': 32}, {'*': 18, 'L5.q.s2': 20}, {'L5.q.s2': 4}
    before = plan.export_tuning()
    runs = []

    def failing():
        runs.append(1)
        if len(runs) == 5:                          # (inside the second trial)
            raise RuntimeError("trial failed")
        run()
    with pytest.raises(RuntimeError, match="trial failed"):
        plan._autotune(failing)
    assert plan.export_tuning() == before
    assert plan._trial is None and plan._tuning is False and plan.timer is None


def test_a_stored_star_tile_is_honoured_on_every_register_tiled_launch(monkeypatch):
    """tools/tune_tiles.py's way of forcing one wave tile: `tile_hints = {'*': hint}` outside any trial."""
    install(monkeypatch)
    plan, run, _ = _forward_case(False)
    plan.autotune = False
    plan.tile_hints = {'*': 34, 'L3.q.s1': 17}
    _spy_launches(plan)
    run()
    hints = {label: ints[ints.index('tile_hint') + 1] for label, fn, ints in Scripted.log[-1] if fn == 'conv_forward'}
    assert len(hints) > 20 and hints.pop('L3.q.s1') == 17
    assert set(hints.values()) == {0, 34}           # 0: the launches the tile does not fit (channel counts, CT)
    assert sum(v == 34 for v in hints.values()) > 15
