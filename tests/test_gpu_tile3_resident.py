"""-m gpu: the resident form of the three-term split conv (csrc/conv_tile3.hip, conv_tile3r_kernel / conv_tile3w_kernel: persistent
workgroups, a group's split weights in LDS for the workgroup's run of items) against the streaming form -- the two add the same terms in the
same order per output element, so `out` and `mean_out` have to be the same BITS -- against float64 at the streaming form's bar,
its refusal of what does not fit the CU's LDS, and a plan with the resident bit (512) of `lds_hints` set on every launch."""
import numpy as np
import pytest
import torch

from nlt_amd import capi as C
from oracle import nlt_oracle as O
from oracle import tf_ops as T
from gpu_util import rel_l2, make_pair, to_device_batch

pytestmark = pytest.mark.gpu

FRAMES = 2
# (mode, cin, cout, tn, h, w): 20 x 24 outputs = 3 x 2 tiles of 8 x 16 (5 x 2 of 4 x 16, 10 x 2 of 2 x 16) with a partial tile on
# both edges.  Wave-private form (stride 1, tn = 32): 4-row tiles at 32 / 32 / 32 and 64 / 64 / 32, 2-row tiles at 128 / 64 / 32.
# Shared-stage form: one 8-wave workgroup at 64 / 64 / 64 and both listed stride-2 shapes, two 4-wave workgroups at 32 / 64 / 64
# (stride 1) and 32 / 32 / 32 (stride 2).  Two groups (a group change inside a run of items when few workgroups share them):
# 64 / 64 / 32, 128 / 64 / 32, 64 / 128 / 32.
SHAPES = [(C.CONV_K2S1, 32, 32, 32, 20, 24), (C.CONV_K2S1, 64, 64, 32, 20, 24), (C.CONV_K2S1, 64, 64, 64, 20, 24),
          (C.CONV_K2S1, 128, 64, 32, 20, 24), (C.CONV_K2S2, 32, 64, 64, 40, 48), (C.CONV_K2S2, 64, 128, 32, 40, 48),
          (C.CONV_K2S2, 32, 32, 32, 40, 48), (C.CONV_K2S1, 32, 64, 64, 20, 24)]
SENTINEL = -7.25


def _operands(mode, cin, cout, h, w, kobs, seed):
    rng = np.random.default_rng(seed)
    ld = cin + 8
    src = torch.from_numpy(rng.standard_normal((FRAMES * kobs, h, w, ld)).astype(np.float32))
    wk = torch.from_numpy((rng.standard_normal((2, 2, cin, cout)) * (1.0 / np.sqrt(4 * cin))).astype(np.float32))
    bias = torch.from_numpy(rng.standard_normal(cout).astype(np.float32) * 0.1)
    return src, ld, wk, bias


@pytest.mark.parametrize('kobs', [1, 4])
@pytest.mark.parametrize('nprod', [6, 9])
@pytest.mark.parametrize('mode,cin,cout,tn,h,w', SHAPES)
def test_resident_form_gives_the_streaming_forms_bits(mode, cin, cout, tn, h, w, nprod, kobs):
    """kobs = 1: per-frame output only; kobs = 4: output in a wider row (ldo = cout + 4) and the observation mean into the upper
    half of an interleaved map (ldm = 2 cout).  Whole buffers are compared, so a store outside the slice shows as well.  Each case
    with the grid sized from the device, with 3 workgroups and with 1 (runs of several items per workgroup and per wave, hand-over
    between items and groups)."""
    src, ld, wk, bias = _operands(mode, cin, cout, h, w, kobs, cin + cout + tn + h + kobs)
    oh, ow = (h // 2, w // 2) if mode == C.CONV_K2S2 else (h, w)
    src, bias = src.cuda(), bias.cuda()
    packed = C.pack_conv_tile3_weights(mode, wk.cuda(), cin, cout, tn)
    assert C.conv_tile3r_plan(mode, cin, tn) is not None

    def run(fn, **kw):
        out = torch.full((FRAMES * kobs, oh, ow, cout + 4), SENTINEL, device='cuda')
        mean = torch.full((FRAMES, oh, ow, 2 * cout), SENTINEL, device='cuda') if kobs > 1 else None
        fn(mode, src, ld, cin, FRAMES, kobs, h, w, packed, bias, cout, tn, out, cout + 4,
           mean.view(-1)[cout:] if kobs > 1 else None, 2 * cout if kobs > 1 else 0, act=True, alpha=0.3, nprod=nprod, **kw)
        torch.cuda.synchronize()
        return out, mean
    want_out, want_mean = run(C.conv_tile3_forward)
    assert not (want_out[..., :cout] == SENTINEL).any() and (want_out[..., cout:] == SENTINEL).all()
    for max_wg in (0, 3, 1):
        out, mean = run(C.conv_tile3r_forward, max_workgroups=max_wg)
        assert torch.equal(out, want_out), (max_wg, int((out != want_out).sum()))
        if kobs > 1:
            assert not (want_mean[..., cout:] == SENTINEL).any()
            assert torch.equal(mean, want_mean), (max_wg, int((mean != want_mean).sum()))


@pytest.mark.parametrize('nprod', [6, 9])
@pytest.mark.parametrize('mode,cin,cout,tn,h,w,kobs', [(C.CONV_K2S1, 64, 64, 32, 33, 47, 3), (C.CONV_K2S2, 64, 64, 64, 66, 94, 2)])
def test_resident_form_vs_float64(mode, cin, cout, tn, h, w, kobs, nprod):
    """The bar of test_gpu_tile.py::test_conv_tile3_three_term_bf16_split_vs_float64, restated: as close to the conv evaluated in
    float64 as the native fp32 MFMA kernel (x 1.5, + 1e-9 with nine products / 3e-8 with six; the mean + 1e-7), with activation and
    mean, and mean only without activation."""
    src, ld, wk, bias = _operands(mode, cin, cout, h, w, kobs, cin + cout + h + kobs)
    stride = 2 if mode == C.CONV_K2S2 else 1
    with torch.no_grad():
        pre64 = T.conv2d_same(src[:, :, :, :cin].double().contiguous(), wk.double(), bias.double(), stride)
        ref = T.leaky_relu(pre64, 0.3)
    oh, ow = ref.shape[1:3]
    E = lambda: torch.full((FRAMES * kobs, oh, ow, cout + 4), float('nan'), device='cuda')
    out3, out1 = E(), E()
    mean = torch.full((FRAMES, oh, ow, 2 * cout), float('nan'), device='cuda')
    packed = C.pack_conv_tile3_weights(mode, wk.cuda(), cin, cout, tn)
    C.conv_tile3r_forward(mode, src.cuda(), ld, cin, FRAMES, kobs, h, w, packed, bias.cuda(), cout, tn, out3, cout + 4,
                          mean.view(-1)[cout:], 2 * cout, act=True, alpha=0.3, nprod=nprod)
    C.conv_tile_forward(mode, src.cuda(), ld, cin, FRAMES, kobs, h, w, C.pack_conv_tile_weights(mode, wk.cuda(), cin, cout, tn),
                        bias.cuda(), cout, tn, out1, cout + 4, None, 0, act=True, alpha=0.3)
    torch.cuda.synchronize()
    got = out3[..., :cout].cpu()
    assert not torch.isnan(got).any() and torch.isnan(out3[..., cout:]).all()
    e3, e1 = rel_l2(got, ref), rel_l2(out1[..., :cout].cpu(), ref)
    print("resident f32x3 nprod=%d: rel-L2 vs float64 %.2e (native fp32 MFMA kernel %.2e)" % (nprod, e3, e1))
    assert e3 <= 1.5 * e1 + (1e-9 if nprod == 9 else 3e-8), (e3, e1)
    m = mean[..., cout:].cpu()
    assert torch.isnan(mean[..., :cout]).all() and rel_l2(m, ref.reshape(FRAMES, kobs, oh, ow, cout).mean(1)) <= 1.5 * e1 + 1e-7
    mean2 = torch.empty((FRAMES, oh, ow, cout), device='cuda')
    C.conv_tile3r_forward(mode, src.cuda(), ld, cin, FRAMES, kobs, h, w, packed, bias.cuda(), cout, tn, None, 0, mean2, cout,
                          act=False, nprod=nprod)
    assert rel_l2(mean2.cpu(), pre64.reshape(FRAMES, kobs, oh, ow, cout).mean(1)) <= 1.5 * e1 + 1e-7


def test_resident_form_refuses_what_does_not_fit_and_launches_nothing():
    """cin = 256 at tn = 64: 384 KB of split weights per group.  NLT_ERR_UNSUPPORTED, the output untouched; so are the untiled
    nprod = 3 / 1 rungs of the precision ladder."""
    cin, cout, tn, h, w = 256, 64, 64, 8, 16
    assert C.conv_tile3r_plan(C.CONV_K2S1, cin, tn) is None
    src = torch.zeros(1, h, w, cin, device='cuda')
    packed = C.pack_conv_tile3_weights(C.CONV_K2S1, torch.ones(2, 2, cin, cout, device='cuda'), cin, cout, tn)
    bias = torch.ones(cout, device='cuda')
    out = torch.full((1, h, w, cout), SENTINEL, device='cuda')
    with pytest.raises(C.NLTError, match='unsupported'):
        C.conv_tile3r_forward(C.CONV_K2S1, src, cin, cin, 1, 1, h, w, packed, bias, cout, tn, out, cout, None, 0, nprod=9)
    packed = C.pack_conv_tile3_weights(C.CONV_K2S1, torch.ones(2, 2, 32, cout, device='cuda'), 32, cout, tn)
    with pytest.raises(C.NLTError, match='unsupported'):
        C.conv_tile3r_forward(C.CONV_K2S1, src, cin, 32, 1, 1, h, w, packed, bias, cout, tn, out, cout, None, 0, nprod=3)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


def test_plan_with_the_resident_bit_renders_the_same_bits(monkeypatch):
    """A small f32x3_9 plan (depth 64, 64 x 64 UV, k = 2, 2 frames) with `lds_hints` = 32 on every encoder label, and the same
    plan with the resident bit (512) added: `pred` bit-identical; the second goes through nlt_conv_tile3r_forward wherever the
    resident form takes the launch and through the streaming kernel where it refuses."""
    import nlt_amd
    from nlt_amd.models import get_model_class
    uv = 64
    om, _ = make_pair(depth=64, uv=uv, im=uv // 2, seed=9)
    batch, nn = O.synth_batch(2, uv, uv, uv // 2, uv // 2, uv // 2, uv // 2, k=2, seed=31)
    resident_calls = []
    real = C.conv_tile3r_forward
    monkeypatch.setattr(C, 'conv_tile3r_forward', lambda *a, **kw: (resident_calls.append(a[3]), real(*a, **kw))[1])
    preds, ran = [], []
    for bit in (0, 512):
        pm = get_model_class('nlt')(nlt_amd.make_config(depth=64, uvh=uv, uvw=uv, imh=uv // 2, imw=uv // 2, precision='f32x3_9'))
        pm.load_weights(om.numpy_weights())
        pm.register_trainable()
        nlev = sum(pm.net['query'].is_contracting) - 1
        pm.plan.autotune = False
        pm.plan.lds_hints = {'L%d.%s.%s' % (l, p, s): bit + 32 for l in range(1, nlev + 1) for p in 'qo' for s in ('s1', 's2')}
        before = len(resident_calls)
        preds.append(pm.call(to_device_batch(batch, nn), 'test')[3]['pred'].clone())
        torch.cuda.synchronize()
        ran.append((len(resident_calls) - before, pm.plan.ran('lds')))
    assert ran[0][0] == 0 and ran[1][0] >= 4, [r[0] for r in ran]
    assert ran[0][1] == ran[1][1] and len(ran[0][1]) >= 4             # the same launches on the LDS-tiled family both times
    assert torch.equal(preds[0], preds[1])
