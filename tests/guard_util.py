"""Guard bands for the buffers, pads and workspaces a kernel is handed (TEST-ONLY; a helper module, not a conftest or plugin).

A HIP entry point takes raw pointers, per-texel strides and sometimes scratch.  Torch's caching allocator owns the memory around
them, so a store a few floats past an output, a halo read past the last frame or a scratch slot read before it is written faults
nothing and usually changes nothing a value test sees.  `Guarded` puts each operand in the middle of a larger allocation whose
bands (and the pad columns of a channel slice) hold one of three fills -- quiet NaN, +3.0e38, -3.0e38; bytes 0xA5 / 0xFF / 0x00
for integer stores -- and checks them bit for bit afterwards.  Three fills: a NaN does not pass a `y > 0 ? 1 : alpha` mask, an
fmaxf or a max-pool, a sign flip does; a value that reaches a result differs across fills or is not finite.

Bands are GUARD_BYTES (256 KiB: a condition, not a measurement -- four 16-texel tile rows at 1024 channels) before and after, a
multiple of 256 bytes, so the payload keeps the 16-byte alignment several entry points insist on.  What this does not see: a read
past the end whose value is discarded, and any access beyond the bands.

Works on 'cuda' and on 'cpu' (tests/test_host_guard_util.py proves every detection path on CPU).

Lifetime rules:
  * guarded buffers are ordinary torch tensors, held by the test (`run_guarded` / the recorder objects keep them) until after
    torch.cuda.synchronize();
  * nothing here runs while a launch tape or a graph capture is open;
  * nothing here frees a buffer a recorded tape could still point at (`guarded_workspace` keeps every buffer it handed out until
    the test ends, and the real cache is untouched);
  * nothing under engine.py's plans is touched: only `capi._workspace` (and, for adapters that allocate their own outputs,
    `capi.torch.empty` / `empty_like`) is replaced, through monkeypatch, for one test.
"""
import math

import torch

FILLS = ('nan', 'pos', 'neg')
GUARD_BYTES = 256 * 1024
_FLOAT_FILL = {'nan': float('nan'), 'pos': 3.0e38, 'neg': -3.0e38}
_BYTE_FILL = {'nan': 0xA5, 'pos': 0xFF, 'neg': 0x00}
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _sync(device):
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize()


class Guarded:
    """`.t`: a tensor of `shape` / `dtype` viewing the middle of a larger flat allocation.  ld > shape[-1]: `.t` is the channel
    slice [..., :c] of texels `ld` elements apart (ld - c pad columns per texel, the last texel's included).  data: the payload
    (else it holds the fill too, so an element an output kernel skips shows).  Bands and pads hold `fill`."""

    def __init__(self, name, shape, dtype=torch.float32, fill='nan', device='cpu', ld=None, data=None, guard_bytes=GUARD_BYTES):
        assert fill in FILLS, fill
        assert guard_bytes >= GUARD_BYTES and guard_bytes % 256 == 0
        self.name, self.fill, self.shape, self.dtype = name, fill, tuple(shape), dtype
        item = torch.empty((), dtype=dtype).element_size()
        self.c = self.shape[-1] if self.shape else 1
        self.ld = self.c if ld is None else int(ld)
        assert self.ld >= self.c, (name, ld, self.c)
        self.texels = math.prod(self.shape[:-1]) if self.shape else 1
        self.count = self.texels * self.ld
        self.g = guard_bytes // item
        self._idt = _INT_VIEW[item]
        raw = torch.empty(2 * guard_bytes + self.count * item, dtype=torch.uint8, device=device)
        self.flat = raw.view(dtype)
        if dtype.is_floating_point:
            v = _FLOAT_FILL[fill]
            if math.isfinite(v):
                v = math.copysign(min(abs(v), torch.finfo(dtype).max), v)
            self.flat.fill_(v)
        else:
            raw.fill_(_BYTE_FILL[fill])
        self._bits = self.flat.view(self._idt)
        self._pattern = self._bits[:1].clone()
        store = self.flat[self.g:self.g + self.count]
        if self.shape:
            self.t = store.view(self.shape[:-1] + (self.ld,))[..., :self.c]
        else:
            self.t = store.view(())
        if data is not None:
            self.t.copy_(torch.as_tensor(data).to(device=device, dtype=dtype).reshape(self.shape))
        self.snapshot()

    def snapshot(self):
        """Remembers the payload for `check_unchanged`."""
        self._saved = self.t.view(self._idt).clone()

    def payload(self):
        """A dense CPU copy of the payload."""
        return self.t.detach().clone().cpu().contiguous()

    def _fail(self, side, where, bad, shift=0):
        idx = bad.nonzero()
        n = int(idx.shape[0])
        if n:
            first = [int(i) + shift for i in idx[0]]
            raise AssertionError("%s: %s was overwritten: first at %s %s, %d element(s)"
                                 % (self.name, side, where, first[0] if len(first) == 1 else tuple(first), n))

    def check_intact(self):
        """Bands and pad columns still hold the fill, bit for bit; else AssertionError naming the tensor, the side (before / after
        / pad), the first offending element and the count.  Offsets: before, relative to the first payload element (-1 = the one
        just before it); after, past the last element of the payload's storage (0 = the first one past it); pad, (texel, column)."""
        p = self._pattern
        self._fail('guard band before the payload', 'element offset', self._bits[:self.g] != p, -self.g)
        self._fail('guard band after the payload', 'element offset', self._bits[self.g + self.count:] != p)
        if self.ld > self.c:
            self._fail('pad columns', '(texel, pad column)',
                       self._bits[self.g:self.g + self.count].view(self.texels, self.ld)[:, self.c:] != p)

    def check_unchanged(self):
        """The payload of a read-only operand is bitwise what `snapshot` (or the constructor) saw."""
        bad = self.t.view(self._idt) != self._saved
        if bool(bad.any()):
            idx = bad.reshape(self.texels, self.c).nonzero() if self.shape else bad.reshape(1, 1).nonzero()
            raise AssertionError("%s: read-only payload was modified: first at (texel, column) %s, %d element(s)"
                                 % (self.name, tuple(int(i) for i in idx[0]), int(idx.shape[0])))


class WorkspaceRecorder:
    """What `guarded_workspace` returns: `.requests` = [(key, need, zero, Guarded)]; `.check()` after the launch (and a sync)."""

    def __init__(self, fill, short=0, zero_words=None):
        self.fill, self.short, self.zero_words, self.requests = fill, short, zero_words, []

    def __call__(self, key, device, need, zero=False):
        need = int(need) - self.short
        g = Guarded('workspace %r' % (key,), (need,), torch.float32, self.fill, device)
        if zero:
            g.t[:self.zero_words].zero_()
        self.requests.append((key, int(need), bool(zero), g))
        return g.t

    def check(self):
        for key, need, zero, g in self.requests:
            _sync(g.t.device)
            g.check_intact()
            if zero:
                nz = (g.t[:self.zero_words].view(torch.int32) != 0).nonzero()
                if nz.shape[0]:
                    raise AssertionError("%s: zero-on-entry scratch is not zero on exit: first at float %d, %d float(s)"
                                         % (g.name, int(nz[0]), int(nz.shape[0])))


def guarded_workspace(monkeypatch, fill, capi=None, short=0, zero_words=None):
    """Replaces `capi._workspace` for this test: every request gets a fresh guarded view of EXACTLY `need` floats (never a cached,
    grown buffer), pre-filled with `fill` (zeros for zero=True).  Returns the recorder; call `.check()` after the launch.
    short = 1: `need - 1` floats instead -- the adapters pass the buffer's length on as the capacity, so the entry point has to
    refuse (the refusal cases).  zero_words: where the entry point's documented zero-on-entry / zero-on-exit contract covers only the
    first `zero_words` floats of a zero=True request (the split-K ticket counters), only those are zeroed and checked; the rest holds
    `fill`, which is the stricter start for plain scratch."""
    if capi is None:
        from nlt_amd import capi
    rec = WorkspaceRecorder(fill, short, zero_words)
    monkeypatch.setattr(capi, '_workspace', rec)
    return rec


class _TorchShim:
    """`torch` as an adapter sees it, with empty / empty_like handing out guarded views (`guarded_allocs`)."""

    def __init__(self, fill):
        self._fill, self.made = fill, []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, device='cpu', dtype=torch.float32):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        elif len(size) == 1:
            size = (int(size[0]),)
        g = Guarded('adapter allocation #%d %s' % (len(self.made), tuple(size)), tuple(size), dtype, self._fill, device)
        self.made.append(g)
        return g.t

    def empty_like(self, x):
        return self.empty(tuple(x.shape), device=x.device, dtype=x.dtype)

    def check(self):
        for g in self.made:
            _sync(g.t.device)
            g.check_intact()


def guarded_allocs(monkeypatch, fill, capi=None):
    """For adapters that allocate their own outputs or scratch (mul_forward, barron_loss, ...): the `torch` name inside `capi` is
    replaced for this test, so those allocations are guarded and fill-initialised too.  `.made` lists them, `.check()` checks them."""
    if capi is None:
        from nlt_amd import capi
    shim = _TorchShim(fill)
    monkeypatch.setattr(capi, 'torch', shim)
    return shim


def run_guarded(call, operands, outputs=(), fills=FILLS, device='cpu', checks=()):
    """Runs `call(ops, fill)` once per fill on freshly built operands, synchronises, checks every guard and every read-only
    operand, and returns [{output name: dense CPU payload}] (one dict per fill; a value `call` returns that is a tensor or a tuple
    of tensors is added under 'ret' / 'ret0', 'ret1', ...).

    operands: {name: spec}; spec = a tensor / array (the payload, dense), or a dict(data=..., shape=..., dtype=..., ld=...), or
    None (the argument is absent).  outputs: the names `call` writes; every other operand must come back bitwise unchanged.
    checks: callables(fill) run after the sync (a workspace recorder's check, built per fill by `call`)."""
    results = []
    for fill in fills:
        ops = {}
        for name, spec in operands.items():
            if spec is None:
                ops[name] = None
                continue
            if not isinstance(spec, dict):
                spec = dict(data=spec)
            data = spec.get('data')
            if data is not None and not torch.is_tensor(data):
                data = torch.as_tensor(data)
            shape = spec.get('shape', None if data is None else tuple(data.shape))
            dtype = spec.get('dtype', torch.float32 if data is None else data.dtype)
            ops[name] = Guarded(name, shape, dtype, fill, device, ld=spec.get('ld'), data=data)
        ret = call(ops, fill)
        _sync(device)
        for name, g in ops.items():
            if g is None:
                continue
            g.check_intact()
            if name not in outputs:
                g.check_unchanged()
        for chk in checks:
            chk(fill)
        res = {name: ops[name].payload() for name in outputs if ops[name] is not None}
        if torch.is_tensor(ret):
            res['ret'] = ret.detach().clone().cpu()
        elif isinstance(ret, (tuple, list)):
            for i, r in enumerate(ret):
                if torch.is_tensor(r):
                    res['ret%d' % i] = r.detach().clone().cpu()
        results.append(res)
    return results


def run_case(monkeypatch, call, operands, outputs=(), det=True, fills=FILLS, device='cuda', capi=None, what='', short=0,
             zero_words=None):
    """`run_guarded` of `call(ops)` with the adapters' scratch (`guarded_workspace`) and own allocations (`guarded_allocs`) guarded
    as well, all under each fill; then bit-identical outputs across the fills (det) or finite ones (the float-atomic forms).
    Returns (results per fill, {fill: (workspace recorder, allocation recorder)})."""
    state = {}

    def check(fill):
        for rec in state[fill]:
            rec.check()
    with monkeypatch.context() as patch:            # (undone on the way out: what the test does next sees the real adapters)
        def wrapped(ops, fill):
            state[fill] = (guarded_workspace(patch, fill, capi, short, zero_words), guarded_allocs(patch, fill, capi))
            return call(ops)
        res = run_guarded(wrapped, operands, outputs, fills, device, checks=[check])
    (assert_same_across_fills if det else assert_finite)(res, what)
    return res, state


def assert_same_across_fills(results, what=''):
    """Deterministic entry points: bit-identical outputs whatever the bands, pads and scratch held (and finite)."""
    assert_finite(results, what)
    for res in results[1:]:
        for name, v in res.items():
            a, b = results[0][name], v
            idt = _INT_VIEW[a.element_size()]
            same = torch.equal(a.view(idt), b.view(idt)) if a.dim() else bool(a == b)
            assert same, "%s%s differs between fills: a guard, pad or unwritten scratch value reached the result" % (what, name)


def assert_finite(results, what=''):
    for fill, res in zip(FILLS, results):
        for name, v in res.items():
            if v.dtype.is_floating_point:
                bad = ~torch.isfinite(v.float()) | (v.float().abs() > 1e30)
                assert not bool(bad.any()), ("%s%s is not finite under the %s fill (%d element(s)): a guard, pad or unwritten scratch "
                                             "value reached the result" % (what, name, fill, int(bad.sum())))


def plain_operand(spec, device='cuda'):
    """An operand spec of `run_guarded` as a plain tensor: dense, or (ld) a channel slice of a wider tensor."""
    if spec is None:
        return None
    if not isinstance(spec, dict):
        return torch.as_tensor(spec).to(device).clone()
    data = spec.get('data')
    shape = tuple(spec['shape']) if 'shape' in spec else tuple(data.shape)
    dtype = spec.get('dtype', torch.float32 if data is None else data.dtype)
    ld = spec.get('ld') or (shape[-1] if shape else 1)
    if not shape:
        t = torch.zeros((), dtype=dtype, device=device)
    else:
        t = torch.full(shape[:-1] + (ld,), 7, dtype=dtype, device=device)[..., :shape[-1]]
    if data is not None:
        t.copy_(torch.as_tensor(data))
    return t


def _bits(t):
    return t.contiguous().view(_INT_VIEW[t.element_size()])


def _rets(ret):
    if torch.is_tensor(ret):
        return {'ret': ret}
    if isinstance(ret, (tuple, list)):
        return {'ret%d' % i: r for i, r in enumerate(ret) if torch.is_tensor(r)}
    return {}


def bitwise_case(monkeypatch, call, ins, outs=None, det=True, device='cuda', **kw):
    """`call(t)` (t: operand name -> tensor or None) once on plain tensors -- the adapter as its own oracle test runs it -- then
    through `run_case` on guarded ones under every fill.  det: outputs and returned tensors are the plain run's, bit for bit;
    else (float atomics) they are finite, and the caller holds them to the reference.  Returns (results per fill, recorders,
    the plain run's outputs on the CPU)."""
    outs = outs or {}
    ops = dict(ins)
    ops.update(outs)
    plain = {k: plain_operand(v, device) for k, v in ops.items()}
    ret = call(plain)
    _sync(device)
    want = {k: plain[k].detach().cpu() for k in outs}
    want.update({k: v.detach().cpu() for k, v in _rets(ret).items()})
    res, state = run_case(monkeypatch, lambda o: call({k: (None if g is None else g.t) for k, g in o.items()}), ops, outputs=tuple(outs),
                          det=det, device=device, **kw)
    assert set(res[0]) == set(want), (sorted(res[0]), sorted(want))
    if det:
        for k, w in want.items():
            assert torch.equal(_bits(res[0][k]), _bits(w)), "%s differs from the run on plain tensors" % k
    return res, state, want
