"""Which device tensors did the project let go during an action, and did anything write into them afterwards?

Launch tapes and captured hipGraphs bake device addresses into something that outlives the call.  The project frees such memory
in two places: `RenderPlan._buffers` keeps ONE shape resident, and `_capi._workspace` replaces a cached scratch tensor when a
larger one is asked for.  A replay that still points at the old tensors computes the right result (it reads what it wrote) and
silently overwrites whoever got that memory next.  `Retired` makes that visible without any such victim: it keeps a reference to
everything the models own on entry, so the memory stays allocated (a stale write can only land in a tensor this test holds),
fills what the models no longer own on exit with a sentinel (`arm`), and looks at it again after the replay (`check`)."""
import torch

from nlt_amd import capi as C

SENTINEL = -7.25                # (exact in fp32 and bf16; no kernel of the project produces a map of it)


def _walk(x, path, out):
    if torch.is_tensor(x):
        if x.numel():
            out.setdefault((x.data_ptr(), x.numel() * x.element_size()), (path, x))
    elif isinstance(x, dict):
        for k, v in x.items():
            if k != 'tapes':                                    # recorded launches: host objects, walked by nobody
                _walk(v, '%s[%r]' % (path, k), out)
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            _walk(v, '%s[%d]' % (path, i), out)


def _census(models):
    """{(data_ptr, nbytes): (container path, tensor)} of everything reachable from the models' plans, the scratch cache and the
    pack registries.  The first path found names a tensor (lanes share one registry and one scratch cache)."""
    out = {}
    models = list(models) if isinstance(models, (list, tuple)) else [models]
    for i, m in enumerate(models):
        who = 'plan' if len(models) == 1 else 'models[%d].plan' % i
        _walk(m.plan._bufs, who + '._bufs', out)
        _walk(m.plan._front_blob, who + '._front_blob', out)
    _walk(C._ws_cache, '_ws_cache', out)
    for i, m in enumerate(models):
        reg = getattr(m, 'pack_registry', None)
        if reg is None:
            continue
        who = 'pack_registry' if len(models) == 1 else 'models[%d].pack_registry' % i
        for (_, key), ent in reg.entries.items():
            _walk(ent[2], '%s.entries[%r]' % (who, key), out)
        _walk(reg.table, who + '.table', out)
    return out


def owned(models):
    """{(data_ptr, nbytes): tensor} of every tensor reachable from each model's `plan._bufs` (through dicts, lists and tuples,
    the 'tapes' entries skipped) and `plan._front_blob`, every value of `_capi._ws_cache`, and the pack registry's entry buffers
    and descriptor table.  `models`: one model or a list (pipeline lanes are models)."""
    return {k: t for k, (_, t) in _census(models).items()}


class Retired:
    """with Retired(models) as r: <the disturbing action>  ->  r.retired = what the models owned on entry and no longer own.

    r.arm() fills every retired floating-point tensor with SENTINEL (integer tensors are left alone and listed in r.skipped);
    r.check() asserts that every armed tensor still holds nothing else, and names the first that does by its container path
    on entry -- e.g. plan._bufs[(2, 2, 64, 64, 'cuda:0', 'fp32')]['fm'][3] or _ws_cache[('cuda:0', 'front_bwd')]."""

    def __init__(self, models):
        self.models = models
        self.before = self.retired = None
        self.armed, self.skipped = [], []

    def __enter__(self):
        self.before = _census(self.models)                      # (holds the tensors: their memory stays allocated)
        return self

    def __exit__(self, *exc):
        after = _census(self.models)
        self.retired = {k: v for k, v in self.before.items() if k not in after}
        return False

    def paths(self):
        return sorted(p for p, _ in self.retired.values())

    def arm(self):
        self._sync()
        self.armed, self.skipped = [], []
        for path, t in self.retired.values():
            if t.dtype.is_floating_point:
                t.fill_(SENTINEL)
                self.armed.append((path, t))
            else:
                self.skipped.append(path)
        self._sync()
        return self

    def check(self):
        self._sync()
        for path, t in self.armed:
            dirty = t != SENTINEL                               # (NaN != x is True: a NaN written there is dirty too)
            if bool(dirty.any()):
                first = int(dirty.reshape(-1).nonzero()[0])
                raise AssertionError("%s was written after the project let it go: %d of %d elements, first at flat index %d "
                                     "(a replay still points into memory that went back to the allocator)"
                                     % (path, int(dirty.sum()), t.numel(), first))

    def _sync(self):
        if any(t.is_cuda for _, t in self.retired.values()):
            torch.cuda.synchronize()
