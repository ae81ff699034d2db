"""tests/guard_util.py on CPU: every detection path, proven with deliberately wrong pure-Python "kernels" (each must make the
helper raise with the right tensor name and side), and a correct kernel (fake_capi.conv_forward on strided views) passing all of
it under all three fills."""
import numpy as np
import pytest
import torch

import fake_capi as F
import guard_util as G
from nlt_amd import capi as C
from oracle import tf_ops as T


def _ops(texels=6, c=4, ld=None):
    rng = np.random.default_rng(0)
    return {'x': dict(data=torch.tensor(rng.standard_normal((texels, c)).astype(np.float32)), ld=ld),
            'out': dict(shape=(texels, c), ld=ld)}


def _good(ops, fill):
    ops['out'].t.copy_(2 * ops['x'].t)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64, torch.bfloat16, torch.float16, torch.uint8, torch.uint16, torch.int16,
                                   torch.int32, torch.int64])
@pytest.mark.parametrize('fill', G.FILLS)
def test_layout(dtype, fill):
    g = G.Guarded('t', (3, 5, 6), dtype, fill, ld=10)
    item = g.t.element_size()
    assert g.t.shape == (3, 5, 6) and g.t.stride() == (50, 10, 1) and g.t.dtype == dtype
    assert g.g * item >= 256 * 1024 and (g.g * item) % 256 == 0 and g.t.data_ptr() % 16 == 0
    assert g.flat.numel() == 2 * g.g + 3 * 5 * 10 and g.t.data_ptr() - g.flat.data_ptr() == g.g * item
    pat = {'nan': 0xA5, 'pos': 0xFF, 'neg': 0x00}[fill]
    if dtype.is_floating_point:
        v = g.flat[0].double()
        assert torch.isnan(v) if fill == 'nan' else (torch.isfinite(v) and abs(float(v)) >= 6e4 and (float(v) > 0) == (fill == 'pos'))
    else:
        assert bool((g.flat.view(torch.uint8) == pat).all())
    g.check_intact(); g.check_unchanged()
    d = G.Guarded('d', (4, 3), dtype, fill)                     # dense: no pads, contiguous
    assert d.t.is_contiguous() and d.count == 12
    d.check_intact()


def test_payload_alignment_for_odd_lengths():
    for n in (1, 3, 7, 1023):
        assert G.Guarded('w', (n,), torch.float32).t.data_ptr() % 16 == 0


def test_correct_kernel_passes_under_every_fill():
    res = G.run_guarded(_good, _ops(ld=7), outputs=('out',))
    G.assert_same_across_fills(res)
    assert len(res) == 3 and res[0]['out'].shape == (6, 4)


def test_fake_capi_conv_on_strided_views_passes():
    rng = np.random.default_rng(1)
    n, h, w, c0, c1, cout = 2, 5, 7, 8, 4, 12
    wk = torch.tensor((rng.standard_normal((2, 2, c0 + c1, cout)) * 0.2).astype(np.float32))
    x0 = torch.tensor(rng.standard_normal((n, h, w, c0)).astype(np.float32))
    x1 = torch.tensor(rng.standard_normal((n, h, w, c1)).astype(np.float32))
    b = torch.tensor(rng.standard_normal(cout).astype(np.float32))
    ops = {'src0': dict(data=x0, ld=c0 + 4), 'src1': dict(data=x1, ld=c1 + 4), 'w': wk, 'bias': b,
           'out': dict(shape=(n, h, w, cout), ld=cout + 4)}

    def call(o, fill):
        # (fake_capi's _view wants the storage behind a slice: as_strided from the payload's first element)
        F.conv_forward(C.CONV_K2S1, o['src0'].t, c0, c0 + 4, o['src1'].t, c1, c1 + 4, n, h, w, o['w'].t, None, o['bias'].t, cout,
                       o['out'].t, cout + 4, act=True, alpha=0.3)
    res = G.run_guarded(call, ops, outputs=('out',))
    G.assert_same_across_fills(res)
    ref = T.leaky_relu(T.conv2d_same(torch.cat((x0, x1), -1), wk, b, 1), 0.3)
    assert torch.allclose(res[0]['out'], ref, atol=1e-5)


def _past_end(ops, fill):
    _good(ops, fill)
    o = ops['out']
    o.flat[o.g + o.count] = 1.0


def _before(ops, fill):
    _good(ops, fill)
    o = ops['out']
    o.flat[o.g - 1] = 1.0


def _pad(ops, fill):
    o = ops['out']
    _good(ops, fill)
    o.flat[o.g + 2 * o.ld + o.c] = 1.0                            # texel 2, first pad column


def _modifies_input(ops, fill):
    _good(ops, fill)
    ops['x'].t[3, 1] += 1.0


@pytest.mark.parametrize('kernel,ld,pattern', [
    (_past_end, None, r"^out: guard band after the payload was overwritten: first at element offset 0, 1 element"),
    (_before, None, r"^out: guard band before the payload was overwritten: first at element offset -1, 1 element"),
    (_pad, 7, r"^out: pad columns was overwritten: first at \(texel, pad column\) \(2, 0\), 1 element"),
    (_modifies_input, 7, r"^x: read-only payload was modified: first at \(texel, column\) \(3, 1\), 1 element"),
])
@pytest.mark.parametrize('fill', G.FILLS)
def test_wrong_kernels_that_write_are_named(kernel, ld, pattern, fill):
    with pytest.raises(AssertionError, match=pattern):
        G.run_guarded(kernel, _ops(ld=ld), outputs=('out',), fills=(fill,))


def test_kernel_that_adds_an_input_pad_column_into_its_output_is_caught():
    def leaky(ops, fill):
        x = ops['x']
        rows = x.flat[x.g:x.g + x.count].view(x.texels, x.ld)
        ops['out'].t.copy_(2 * x.t)
        ops['out'].t[:, 0] += 0.0 * rows[:, x.c]                # "times a zero weight": NaN survives, +-3e38 does not
        ops['out'].t[:, 1] += torch.where(rows[:, x.c] > 0, 1.0, 0.3)        # a mask: NaN does not survive, the sign does
    res = G.run_guarded(leaky, _ops(ld=7), outputs=('out',))
    with pytest.raises(AssertionError, match=r"out is not finite under the nan fill \(6 element"):
        G.assert_finite(res)
    with pytest.raises(AssertionError, match=r"out differs between fills"):
        G.assert_same_across_fills(res[1:])


class _Capi:
    """The slice of `capi` a workspace kernel needs (`guarded_workspace` patches `_workspace` on whatever it is given)."""
    _workspace = staticmethod(C._workspace)


def _ws_case(monkeypatch, kernel, zero, fills=G.FILLS):
    recs = {}

    def call(ops, fill):
        recs[fill] = rec = G.guarded_workspace(monkeypatch, fill, capi=_Capi)
        ws = _Capi._workspace('fam', 'cpu', 8, zero=zero)
        kernel(ops, ws)
    return G.run_guarded(call, _ops(), outputs=('out',), fills=fills, checks=[lambda fill: recs[fill].check()]), recs


def test_workspace_correct_use_passes_and_is_exact(monkeypatch):
    def two_pass(ops, ws):
        ws[:4] = ops['x'].t.sum(0); ws[4:] = 0
        ops['out'].t.copy_(ops['x'].t + ws[:4] + ws[4:])
    res, recs = _ws_case(monkeypatch, two_pass, zero=False)
    G.assert_same_across_fills(res)
    (key, need, zero, g), = recs['nan'].requests
    assert (key, need, zero) == ('fam', 8, False) and g.t.numel() == 8 and bool(torch.isnan(g.flat[g.g - 1]))


def test_workspace_slot_read_before_written_is_caught(monkeypatch):
    def reads_first(ops, ws):
        ws[:4] = ops['x'].t.sum(0)                                # never writes ws[4:]
        ops['out'].t.copy_(ops['x'].t + ws[:4] + torch.clamp(ws[4:], -1, 1))
    res, _ = _ws_case(monkeypatch, reads_first, zero=False)
    with pytest.raises(AssertionError, match=r"out (is not finite under the nan fill|differs between fills)"):
        G.assert_same_across_fills(res)
    with pytest.raises(AssertionError, match=r"out differs between fills"):
        G.assert_same_across_fills(res[1:])


def test_workspace_overrun_is_caught(monkeypatch):
    def overrun(ops, ws):
        torch.as_strided(ws, (9,), (1,))[8] = 0.0                 # one float past `need`
        ops['out'].t.copy_(ops['x'].t)
    with pytest.raises(AssertionError, match=r"^workspace 'fam': guard band after the payload was overwritten: first at element offset 0"):
        _ws_case(monkeypatch, overrun, zero=False, fills=('pos',))


def test_zero_workspace_left_dirty_is_caught(monkeypatch):
    def dirty(ops, ws):
        assert not bool(ws.any())                                 # zero on entry, whatever the fill
        ws[5] = 1.0
        ops['out'].t.copy_(ops['x'].t)
    with pytest.raises(AssertionError, match=r"^workspace 'fam': zero-on-entry scratch is not zero on exit: first at float 5, 1 float"):
        _ws_case(monkeypatch, dirty, zero=True, fills=('nan',))

    def clean(ops, ws):
        ws[5] = 1.0; ops['out'].t.copy_(ops['x'].t * ws[5]); ws[5] = 0.0
    res, _ = _ws_case(monkeypatch, clean, zero=True)
    G.assert_same_across_fills(res)


def test_guarded_allocs_guards_what_an_adapter_allocates(monkeypatch):
    class Mod:
        torch = torch

        @staticmethod
        def scale(x):
            out = Mod.torch.empty_like(x)
            ws = Mod.torch.empty(4, device=x.device, dtype=torch.float32)
            ws[:] = 2.0
            out.copy_(x * ws[0])
            return out, ws
    shim = G.guarded_allocs(monkeypatch, 'neg', capi=Mod)
    out, ws = Mod.scale(torch.ones(3, 2))
    shim.check()
    assert len(shim.made) == 2 and bool((out == 2).all()) and Mod.torch.float32 is torch.float32
    torch.as_strided(ws, (5,), (1,))[4] = 1.0
    with pytest.raises(AssertionError, match=r"adapter allocation #1 \(4,\): guard band after"):
        shim.check()


def test_bitwise_case_holds_the_guarded_runs_to_the_plain_run(monkeypatch):
    class Mod:
        torch = torch
        _workspace = staticmethod(lambda key, device, need, zero=False: torch.zeros(need))

    def good(t):
        ws = Mod._workspace('fam', 'cpu', 4)
        ws[:] = 1.0
        out = Mod.torch.empty_like(t['x'])
        out.copy_(t['x'] * 2 + ws[0])
        t['y'].copy_(out)
        return out
    x = torch.arange(24, dtype=torch.float32).reshape(6, 4)
    res, state, want = G.bitwise_case(monkeypatch, good, dict(x=dict(data=x, ld=7)), dict(y=dict(shape=(6, 4), ld=9)), device='cpu', capi=Mod)
    assert torch.equal(want['y'], 2 * x + 1) and torch.equal(res[2]['ret'], 2 * x + 1) and set(state) == set(G.FILLS)
    assert Mod.torch is torch                                     # the patches are undone on the way out

    def reads_scratch(t):                                         # right on a zeroed plain buffer, wrong on scratch that holds the fill
        ws = Mod._workspace('fam', 'cpu', 4)
        t['y'].copy_(t['x'] + torch.clamp(ws[0], -1, 1))
    with pytest.raises(AssertionError, match=r"y (is not finite|differs)"):
        G.bitwise_case(monkeypatch, reads_scratch, dict(x=x), dict(y=dict(shape=(6, 4))), device='cpu', capi=Mod)


def test_zero_words_limits_the_zero_contract_to_the_head_of_the_scratch(monkeypatch):
    rec = G.guarded_workspace(monkeypatch, 'nan', capi=_Capi, zero_words=2)
    ws = _Capi._workspace('fam', 'cpu', 6, zero=True)
    assert not bool(ws[:2].any()) and bool(torch.isnan(ws[2:]).all())
    ws[4] = 3.0                                                   # plain scratch behind the counters: no contract on exit
    rec.check()
    ws[1] = 1.0
    with pytest.raises(AssertionError, match=r"zero-on-entry scratch is not zero on exit: first at float 1, 1 float"):
        rec.check()
