"""-m gpu: memory discipline of csrc/unwrap.hip with tests/guard_util.py, as tests/test_gpu_guard_shade.py does it for the renders.
Every adapter of the unwrap runs on guarded views of its inputs under the three fills; its outputs and scratch are guarded
through `guarded_allocs` / `guarded_workspace` (exactly the queried sizes) and start as the fill: bands and read-only operands
intact, every output element written (a fill left behind is not finite, or differs between fills) and the same bits under every
fill as on plain tensors (tests/test_gpu_unwrap.py holds those to the restatement).
The mesh: a flat 12 x 12 grid, 288 triangles (two blocks: a second tree level, a partial last workgroup) in one group and one
island (several hooking rounds), a quad, and two degenerate faces."""
import numpy as np
import pytest
import torch

import guard_util as G
import unwrap_ref as R
from nlt_amd import capi as C
from nlt_amd.data_gen import unwrap as U

pytestmark = pytest.mark.gpu


def _mesh():
    verts, faces = R.grid_mesh(12)
    k = len(verts)
    verts = np.concatenate((verts, [[0.0, 0.0, 1.0], [0.25, 0.0, 1.0], [0.25, 0.0, 1.25], [0.0, 0.0, 1.25]]))
    return R.mesh_arrays(verts, faces + [[0, 0, 1], [k, k + 1, k + 2, k + 3], [3, 4]]) + (verts, faces)


VERTS, LV, FO, _, _ = _mesh()
F, L = len(FO) - 1, len(LV)
COS_HALF, COS_FULL = U.angle_cosines(66.)
T = torch.from_numpy


@pytest.fixture(scope='module')
def stages():
    """The plain run's intermediate tensors, on the CPU: each guarded case starts from them."""
    dv, dl, do = T(VERTS).cuda(), T(LV).cuda(), T(FO).cuda()
    n, unit, area, ok = C.unwrap_frames(dv, dl, do)
    vectors, seeds = C.unwrap_vectors(unit, area, ok, COS_HALF, COS_FULL, 0.5, 0.5)
    vectors = vectors.contiguous()
    group = C.unwrap_assign(unit, ok, vectors)
    label, loop_face, _ = C.unwrap_islands(dl, do, len(VERTS), group)
    labels, island = U.island_numbers(label.cpu().numpy())
    frames = np.stack([np.stack(U.projection_basis(v)) for v in vectors.cpu().numpy()])
    puv, boxes = C.unwrap_boxes(dv, dl, loop_face, group, T(island).cuda(), T(frames).cuda(), len(labels))
    b = boxes.cpu().numpy()
    scale, rot, offsets = U.pack_islands(b[:, 2:] - b[:, :2], labels, 0.002)
    torch.cuda.synchronize()
    cpu = lambda t: t.cpu()
    return dict(unit=cpu(unit), area=cpu(area), ok=cpu(ok), vectors=cpu(vectors), group=cpu(group), loop_face=cpu(loop_face),
                island=T(island), frames=T(frames), n_islands=len(labels), puv=cpu(puv), boxes=cpu(boxes), scale=scale,
                rot=T(rot.astype(np.uint8)), offsets=T(offsets), n_vectors=len(seeds))


MESH = dict(verts=T(VERTS), loop_verts=T(LV), face_off=T(FO))


def test_frames(monkeypatch):
    _, state, want = G.bitwise_case(monkeypatch, lambda t: C.unwrap_frames(t['verts'], t['loop_verts'], t['face_off']), MESH)
    assert [g.shape for g in state['nan'][1].made] == [(3, F), (3, F), (F,), (F,)]
    assert list(want['ret3'][-3:]) == [0, 1, 0] and int(want['ret3'].sum()) == F - 2


def test_vectors(monkeypatch, stages):
    ins = {k: stages[k] for k in ('unit', 'area', 'ok')}
    _, state, want = G.bitwise_case(monkeypatch, lambda t: C.unwrap_vectors(t['unit'], t['area'], t['ok'], COS_HALF, COS_FULL, 0.5, 0.5, 4), ins)
    ws, made = state['nan']
    # remaining, best, the [max_groups, 3] vectors, the pair; one scratch request of exactly the queried bytes
    assert [g.shape for g in made.made] == [(F,), (F,), (4, 3), (2,)]
    assert [r[1] for r in ws.requests] == [C.lib().nlt_unwrap_workspace_bytes(F) // 4]
    assert tuple(want['ret0'].shape) == (stages['n_vectors'], 3) == (2, 3)


def test_assign(monkeypatch, stages):
    ins = {k: stages[k] for k in ('unit', 'ok', 'vectors')}
    _, state, want = G.bitwise_case(monkeypatch, lambda t: C.unwrap_assign(t['unit'], t['ok'], t['vectors']), ins)
    assert [g.shape for g in state['nan'][1].made] == [(F,)] and sorted(set(want['ret'].tolist())) == [-1, 0, 1]


def test_islands(monkeypatch, stages):
    ins = dict(loop_verts=MESH['loop_verts'], face_off=MESH['face_off'], group=stages['group'])
    _, state, want = G.bitwise_case(monkeypatch, lambda t: C.unwrap_islands(t['loop_verts'], t['face_off'], len(VERTS), t['group']), ins)
    assert [g.shape for g in state['nan'][1].made] == [(L,), (L,), (F,), (1,)]                  # keys, loop_face, label, changed
    assert sorted(set(want['ret0'].tolist())) == [-1, 0, F - 2]


def test_boxes(monkeypatch, stages):
    ins = dict(verts=MESH['verts'], loop_verts=MESH['loop_verts'], **{k: stages[k] for k in ('loop_face', 'group', 'island', 'frames')})
    call = lambda t: C.unwrap_boxes(t['verts'], t['loop_verts'], t['loop_face'], t['group'], t['island'], t['frames'], stages['n_islands'])
    _, state, want = G.bitwise_case(monkeypatch, call, ins)
    assert [g.shape for g in state['nan'][1].made] == [(L, 2), (2, 4)]
    assert bool((want['ret1'][:, 2:] > want['ret1'][:, :2]).all())


def test_uv(monkeypatch, stages):
    ins = dict(face_off=MESH['face_off'], **{k: stages[k] for k in ('puv', 'island', 'boxes', 'rot', 'offsets')})
    call = lambda t: C.unwrap_uv(t['puv'], t['face_off'], t['island'], t['boxes'], t['rot'], t['offsets'], stages['scale'], 4)
    _, state, want = G.bitwise_case(monkeypatch, call, ins)
    assert [g.shape for g in state['nan'][1].made] == [(F, 4, 2)]
    uv = want['ret']
    assert float(uv.min()) >= 0 and float(uv.max()) <= 1 and not bool(uv[:288, 3].any()) and not bool(uv[288].any()) and bool(uv[289].all())
