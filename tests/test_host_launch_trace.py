"""CPU: the ordered launch trace of RenderPlan -- per launch its label, the C entry point, the algorithmic bytes, the FLOPs and the
moved bytes handed to the timer, and a digest of every argument -- over the plan's routes (fused / layer-by-layer ends, the
override plan, every hint route, a train step), driven through the TEST-ONLY adapters of tests/fake_capi.py.

Two uses.  (1) A restructuring of the host code must not change a launch: set NLT_LAUNCH_TRACE_DUMP to a file, run this module
on the old and on the new code, and the two files must be identical.  (2) The label / entry point / bytes / FLOPs / moved columns
of a few cases are recorded in test_host_launch_trace.json and compared on every run: the benchmark's roofline lines are
computed from exactly these figures."""
import json
import os

import torch

from nlt_amd import _capi as C
from nlt_amd.engine import OpTimer
from oracle import nlt_oracle as O
import fake_capi
from test_host_orchestration import make, cpu_batch

DUMP = os.environ.get('NLT_LAUNCH_TRACE_DUMP')
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_host_launch_trace.json')
LABELS = ['L%d.%s.%s' % (l, p, s) for l in range(1, 13) for p in 'qo' for s in ('s1', 's2')]


def _digest(x):
    """Tensors by (shape, stride, storage offset, dtype); ints, floats, bools, strings and None as they are."""
    if torch.is_tensor(x):
        return ['T', list(x.shape), list(x.stride()), x.storage_offset(), str(x.dtype)]
    if isinstance(x, (list, tuple)):
        return [_digest(v) for v in x]
    if isinstance(x, dict):
        return {str(k): _digest(v) for k, v in sorted(x.items())}
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    return type(x).__name__


class Rec(OpTimer):
    def __init__(self):
        super().__init__()
        self.trace = []

    def launch(self, label, nbytes, fn, *a, **kw):
        self.trace.append([label, fn.__name__, nbytes, self.flops[label], self.moved.get(label), _digest([a, kw])])
        fn(*a, **kw)


def pack_conv_tile3_weights(mode, w_keras, cin, cout, tn):
    return fake_capi.pack_conv_tile_weights(mode, w_keras, cin, cout, tn)


def conv_tile3_forward(mode, src, ld, cin, frames, kobs, h, w, packed, bias, cout, tn, out, ldo, mean_out, ldm,
                       act=True, alpha=0.3, nprod=6):
    assert nprod in (6, 9)
    fake_capi.conv_tile_forward(mode, src, ld, cin, frames, kobs, h, w, packed, bias, cout, tn, out, ldo, mean_out, ldm, act, alpha)


def _set(**attrs):
    def setup(plan):
        for name, v in attrs.items():
            setattr(plan, name, v)
    return setup


def _maps(pm, h, w):
    g = torch.Generator().manual_seed(5)
    return [torch.rand(1, h >> l, w >> l, c, generator=g) for l, c in enumerate(pm.plan._level_channels())]


def _infer(depth, uvh, uvw, k, setup=None, n=1, mode='test', override=False, **mk):
    def run():
        _, pm = make(depth, 0, 32, uvh=uvh, uvw=uvw, **mk)
        batch, nn = O.synth_batch(n, uvh, uvw, 32, 32, 32, 32, k=k, seed=2)
        if setup is not None:
            setup(pm.plan)
        rec = pm.plan.timer = Rec()
        kw = {'obs_override': _maps(pm, uvh, uvw)} if override else {}
        pm.call(cpu_batch(batch, nn), mode, **kw)
        return rec.trace
    return run


def _obs_weights():
    _, pm = make(256, 64, 32)
    batch, nn = O.synth_batch(2, 64, 64, 32, 32, 32, 32, k=2, seed=3)
    cb = cpu_batch(batch, nn)
    rec = pm.plan.timer = Rec()
    pm.plan.forward(cb[1], cb[2], cb[3], cb[9], cb[8], obs_weights=torch.rand(2, 2), skip_connect_base=False)
    return rec.trace


def _resident(override):
    def run():
        from nlt_amd.datasets.nlt import ResidentTexels
        _, pm = make(256, 64, 32)
        g = torch.Generator().manual_seed(3)
        U = lambda *s: torch.randint(0, 256, s, generator=g, dtype=torch.uint8)
        store = {'diffuse': U(5, 64, 64, 3), 'rgb': U(5, 64, 64, 3), 'cvis': U(5, 64, 64), 'lvis': U(5, 64, 64),
                 'uv2cam': torch.rand(5, 32, 32, 2, generator=g).half()}
        res = ResidentTexels(store, torch.tensor([3, 1], dtype=torch.int32), torch.tensor([[0], [2]], dtype=torch.int32),
                             test_mode=True)
        pm.plan.autotune = False            # (the store-resident forward does not ask whether it is on a GPU before its trials)
        rec = pm.plan.timer = Rec()
        pm.plan.forward(None, None, None, None, None, obs_override=_maps(pm, 64, 64) if override else None, inference=True,
                        resident=res)
        return rec.trace
    return run


def _train(k, setup=None):
    def run():
        _, pm = make(256, 64, 32, loss='l2')
        pm.build('cpu'); pm.register_trainable()
        if setup is not None:
            setup(pm.plan)
        rec = pm.plan.timer = Rec()
        batch, nn = O.synth_batch(2, 64, 64, 32, 32, 32, 32, k=k, seed=12)
        pm.train_forward_backward(cpu_batch(batch, nn), 2)
        return rec.trace
    return run


def _cases():
    c = {}
    for fused in (True, False):
        f = 'fused' if fused else 'plain'
        for k in (1, 3, 5):
            c['infer.d256.64x64.k%d.%s' % (k, f)] = _infer(256, 64, 64, k, _set(fuse_ends=fused))
        c['infer.d1024.256x256.k1.' + f] = _infer(1024, 256, 256, 1, _set(fuse_ends=fused))
        c['infer.d256.64x192.k2.' + f] = _infer(256, 64, 192, 2, _set(fuse_ends=fused), n=2)
        for name, hints in (('lds32', {'lds_hints': 32}), ('lds64', {'lds_hints': 64}), ('lds288', {'lds_hints': 256 + 32}),
                            ('wino32', {'wino_hints': 32}), ('wino64', {'wino_hints': 64}), ('wino288', {'wino_hints': 256 + 32}),
                            ('wino320', {'wino_hints': 256 + 64}), ('c32_1', {'c32_hints': 1}), ('c32_2', {'c32_hints': 2})):
            attrs = {a: {lab: v for lab in LABELS} for a, v in hints.items()}
            c['hint.%s.k3.%s' % (name, f)] = _infer(256, 64, 64, 3, _set(fuse_ends=fused, **attrs), n=2)
        for name, trial in (('wino32', ('wino', 32)), ('wino288', ('wino', 256 + 32)), ('lds32', ('lds', 32)),
                            ('lds320', ('lds', 256 + 64)), ('c32_1', ('c32', 1)), ('c32_2', ('c32', 2))):
            for k in (1, 3):
                c['trial.%s.k%d.%s' % (name, k, f)] = _infer(256, 64, 64, k, _set(fuse_ends=fused, autotune=False, _trial=trial), n=2)
        for prec in ('f32x3', 'f32x3_9'):
            c['%s.lds32.k3.%s' % (prec, f)] = _infer(256, 64, 64, 3, _set(fuse_ends=fused, precision=prec,
                                                                         lds_hints={lab: 32 for lab in LABELS}), n=2)
        for k in (1, 2):
            c['train.k%d.%s' % (k, f)] = _train(k, _set(fuse_ends=fused))
        c['train.trial_wino32.k1.' + f] = _train(1, _set(fuse_ends=fused, autotune=False, _trial=('wino', 32)))
    c['infer.d256.64x64.k5.front_v4_off'] = _infer(256, 64, 64, 5, _set(front_v4=False))
    c['infer.d256.64x64.k1.alias_obs_off'] = _infer(256, 64, 64, 1, _set(alias_obs=False))
    c['infer.d256.64x64.k3.fuse_dec_off'] = _infer(256, 64, 64, 3, _set(fuse_dec=False))
    c['train.k1.fold_split_off'] = _train(1, _set(fold_split=False))
    c['train.k2.front4_train_off'] = _train(2, _set(front4_train=False))
    c['obs_weights.k2'] = _obs_weights
    c['use_obs_off.k1'] = _infer(256, 64, 64, 1, mode='vali', use_obs=False, skip_connect_base=False)
    for depth, uv in ((256, 64), (1024, 256)):
        c['override.d%d.fused' % depth] = _infer(depth, uv, uv, 1, n=2, override=True)
        c['override.d%d.general' % depth] = _infer(depth, uv, uv, 1, _set(fuse_override=False), n=2, override=True)
    c['override.d256.fuse_dec_off'] = _infer(256, 64, 64, 1, _set(fuse_dec=False), n=2, override=True)
    c['resident'] = _resident(False)
    c['resident.override'] = _resident(True)
    return c


RECORDED = ('infer.d256.64x64.k1.fused', 'infer.d256.64x64.k3.fused', 'train.k1.fused')


def collect(monkeypatch, names=None):
    fake_capi.install(monkeypatch)
    monkeypatch.setattr(C, 'pack_conv_tile3_weights', pack_conv_tile3_weights)
    monkeypatch.setattr(C, 'conv_tile3_forward', conv_tile3_forward)
    cases = _cases()
    return {name: cases[name]() for name in (names or cases)}


def test_recorded_roofline_accounting_of_the_flagship_cases(monkeypatch):
    """Labels, entry points, algorithmic bytes, FLOPs and moved bytes of the k = 1 / k = 3 fused inference passes and of one train
    step equal the recorded ones, launch for launch."""
    got = {name: [e[:5] for e in tr] for name, tr in collect(monkeypatch, RECORDED).items()}
    with open(FIXTURE) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for name in RECORDED:
        assert len(got[name]) == len(want[name]), name
        for g, w in zip(got[name], want[name]):
            assert g == w, (name, g, w)


def test_every_route_of_the_plan_leaves_a_trace(monkeypatch):
    """Every case runs through the emulated adapters; routes that are meant to differ do (the full trace goes to
    NLT_LAUNCH_TRACE_DUMP for a comparison between two versions of the host code)."""
    tr = collect(monkeypatch)
    if DUMP:
        os.makedirs(os.path.dirname(DUMP) or '.', exist_ok=True)
        with open(DUMP, 'w') as f:
            json.dump(tr, f, indent=0, sort_keys=True)
            f.write('\n')
    assert all(len(t) > 10 for t in tr.values())
    fns = lambda name: {e[1] for e in tr[name]}
    labels = lambda name: [e[0] for e in tr[name]]
    assert 'conv_tile_forward' in fns('hint.lds32.k3.fused') and 'conv_tile3_forward' in fns('f32x3_9.lds32.k3.plain')
    assert 'conv_wino_forward' in fns('trial.wino32.k1.plain') and 'conv_c32_forward' in fns('trial.c32_2.k3.fused')
    assert 'conv_wino_backward_data' in fns('train.trial_wino32.k1.fused')
    assert 'front_ovr_forward_u8' in fns('resident.override') and 'front4_forward_u8' in fns('resident')
    assert 'L2.o.mean' in labels('hint.c32_2.k3.fused') and 'L2.o.mean' not in labels('hint.c32_1.k3.fused')
    assert 'bwd.L3.split' in labels('train.k2.fused') and 'bwd.L3.split' not in labels('train.k1.fused')
    assert 'bwd.L3.split' in labels('train.k1.fold_split_off')
    assert 'V3.q.s2' in labels('override.d256.fused') and 'V3.q.s2' not in labels('override.d256.general')
    assert tr['infer.d256.64x64.k3.fused'] != tr['infer.d256.64x64.k3.plain']
