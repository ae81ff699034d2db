"""-m gpu: memory discipline of the three entry points of csrc/relight.hip with tests/guard_util.py.  Every tensor argument is a
guarded view under the three fills; the weights' row partials are a workspace of exactly the queried size that starts as the fill
(`guard_util.guarded_workspace`), the adapters' own outputs are guarded through `guarded_allocs`.  Per case: bands and read-only
operands intact, outputs fully written, the same bits under every fill -- so no workspace slot is read before it is written --
and bit for bit the result on plain tensors, which tests/test_gpu_relight.py holds to the float64 restatement.  One float less
workspace is refused and nothing is touched.  Shapes: texels = 63 and 257 (the element-wise form and its tail) and 64 (the
16-byte form), 5 lights, 1 and 9 rotations (one r-tile and a second, short one), a 4 x 8 probe."""
import numpy as np
import pytest
import torch

from nlt_amd import capi as C
import guard_util as G
import relight_ref as R

pytestmark = pytest.mark.gpu

N_LIGHTS = 5
t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


@pytest.mark.parametrize('n_rot', [1, 9])
def test_envmap_light_weights(monkeypatch, n_rot):
    he, we = 4, 8
    ins = dict(envmap=t32(np.random.default_rng(1).random((he, we, 3)) + 0.05), dirs=t32(R.random_directions(N_LIGHTS, 5000)),
               rot=t32(R.random_rotations(n_rot, 77)))
    res, state, _ = G.bitwise_case(monkeypatch, lambda t: C.envmap_light_weights(t['envmap'], t['dirs'], t['rot']), ins)
    assert res[0]['ret'].shape == (n_rot, N_LIGHTS, 3)
    need = C.lib().nlt_envmap_light_weights_workspace_floats(he, we, N_LIGHTS, n_rot)
    assert [r[1] for r in state['nan'][0].requests] == [need]                     # exactly the queried size, undefined on entry

    def refused(o):
        with pytest.raises(C.NLTError, match='bad argument'):
            C.envmap_light_weights(o['envmap'].t, o['dirs'].t, o['rot'].t)
    G.run_case(monkeypatch, refused, ins, short=1)


@pytest.mark.parametrize('is_linear', [True, False])
@pytest.mark.parametrize('n_rot', [1, 9])
@pytest.mark.parametrize('texels', [63, 64, 257])
def test_relight_accumulate(monkeypatch, texels, n_rot, is_linear):
    rng = np.random.default_rng(texels + n_rot)
    ins = dict(pred=t32(rng.random((3, texels, 3)) * 1.5 - 0.25), weights=t32(rng.random((n_rot, N_LIGHTS, 3)) * 0.4))
    outs = dict(acc=t32(rng.random((n_rot, texels, 3)) * 0.1))                    # read and written: it carries data, not the fill
    G.bitwise_case(monkeypatch, lambda t: C.relight_accumulate(t['pred'], t['weights'], 2, t['acc'], is_linear), ins, outs)


@pytest.mark.parametrize('to_srgb', [True, False])
@pytest.mark.parametrize('n_rot', [1, 9])
@pytest.mark.parametrize('texels', [63, 64, 257])
def test_relight_finish(monkeypatch, texels, n_rot, to_srgb):
    ins = dict(acc=t32(np.random.default_rng(texels * n_rot).random((n_rot, texels, 3)) * 1.4 - 0.1))
    res, _, _ = G.bitwise_case(monkeypatch, lambda t: C.relight_finish(t['acc'], 1.3, to_srgb), ins)
    assert res[0]['ret'].shape == (n_rot, texels, 3)
