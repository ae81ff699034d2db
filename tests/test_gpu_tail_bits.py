"""-m gpu: the tile kernels of the decoder tail and the fused train ends (csrc/dec_block.hip, fused.hip, train_back.hip,
train_fused.hip) against the BITS an earlier commit's build wrote.

These kernels have no atomics, their grids are fixed by the shape alone (the two backward launchers cap their workgroup counts by
shape) and they add in a fixed order, so their results are a function of the inputs.  The parity tests (test_gpu_dec_block.py,
test_gpu_fused.py, test_gpu_train_fused.py) hold them to float64 or to the layer-by-layer kernels within a bar; every copy moving
together inside that bar would pass them.  Here each case runs one entry point on fixed inputs (numpy's default_rng on the CPU,
seeded per case), into output buffers pre-filled with a fixed sentinel -- gradient accumulators (`+=`) start from a fixed non-zero
pattern --, and the SHA-256 of the WHOLE of every output buffer, and of the whole workspace for the two backward entries (sized by
the library's own query, sentinel-filled), is compared with tests/golden/tail_bits.json.  That file names the commit whose build
recorded it:

    NLT_HIP_LIB=<libnlt_hip.so built from that commit> python tests/test_gpu_tail_bits.py > default.json
    NLT_HIP_LIB=<the same> NLT_DEC_GENERIC=1 python tests/test_gpu_tail_bits.py > generic.json

(one fresh process per run: the library path and NLT_DEC_GENERIC are read once per process; the second run's digests go under the
key 'generic' of the first's file.)  A change that is meant to alter the sequence of floating-point operations of these kernels
records the file anew from its own parent and says so.

What the cases reach (a tile = 8 x 16 input texels; n x h x w = frames and the tile kernels' INPUT size, raw size for the fronts):
  dec       balanced kernel (cx, cs) = (2c, 8c), c = 8 and 16: 1x1x1 (a tile that is almost all halo and padding), 1x9x17 (one texel
            into the second tile both ways), 1x3x35 (three tile columns, the last partial), 2x16x32 (eight workgroups: the XCD
            remap is active), 2x24x40 (twelve: inactive).  The generic kernel: the same ten under NLT_DEC_GENERIC=1 (a child
            interpreter), and by its own widths (8, 8, 32) at 1x20x12, (16, 20, 36) at 1x11x7 (K = 56: a partial last chunk, the
            x | skip boundary inside a chunk) and (8, 16, 160) at 1x9x17 (K = 176: eleven chunks, the second pass of the group loop).
  dec_map   c = 8 and 16, skip stride 4c (dense query map) and 8c (interleaved) at 1x1x1, 1x9x17, 2x16x32.
  back      back_forward, back_forward_train (u and v in the digest) and back_forward_map (ldq 16 and 32) at 1x1x1, 1x9x17, 1x3x35
            and 2x16x32.
  front     front_forward k = 1, 2, 5, front_forward_train and front2_forward k = 1, 2 at raw 1x4x4, 2x24x40 and (not front2)
            1x36x100; the two packed weight blobs.
  back_bwd  1x1x1, 1x9x17, 2x16x32 and one long walk, 3x152x304: 1083 tiles on 1024 workgroups, so some keep their sums across
            two tiles.
  front_bwd first generation: 1x1x2x8 (one group, three idle waves), 2x3x24x40, 1x5x8x64 (k > 4 at a width the staged kernel would
            take), the long walk 2x2x96x520 (6240 groups on 6144 waves); staged: k = 1 .. 4 at 1xkx2x32 and 2xkx24x64, the long
            walk 4x1x256x512 (8192 runs on 6144 waves)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nlt_amd import capi as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tail_bits.json')
SENTINEL = -7.25
ALPHA = 0.3
KINDS = ('dec', 'dec_map', 'back', 'back_train', 'back_map', 'front', 'front_train', 'front2', 'pack', 'pack_l2', 'back_bwd',
         'front_bwd')

TILE5 = ((1, 1, 1), (1, 9, 17), (1, 3, 35), (2, 16, 32), (2, 24, 40))
CASES = []                                                               # (kind, parameters)
for _c in (8, 16):
    CASES += [('dec', (_c, 2 * _c, 8 * _c) + s) for s in TILE5]
CASES += [('dec', (8, 8, 32, 1, 20, 12)), ('dec', (16, 20, 36, 1, 11, 7)), ('dec', (8, 16, 160, 1, 9, 17))]
for _c in (8, 16):
    CASES += [('dec_map', (_c, _l * _c) + s) for _l in (4, 8) for s in (TILE5[0], TILE5[1], TILE5[3])]
for _s in TILE5[:4]:
    CASES += [('back', _s), ('back_train', _s), ('back_map', (16,) + _s), ('back_map', (32,) + _s)]
for _n, _h, _w in ((1, 4, 4), (2, 24, 40), (1, 36, 100)):
    CASES += [('front', (_n, _k, _h, _w)) for _k in (1, 2, 5)] + [('front_train', (_n, _k, _h, _w)) for _k in (1, 2)]
    if (_h, _w) != (36, 100):
        CASES += [('front2', (_n, _k, _h, _w)) for _k in (1, 2)]
CASES += [('pack', ()), ('pack_l2', ())]
CASES += [('back_bwd', s) for s in ((1, 1, 1), (1, 9, 17), (2, 16, 32), (3, 152, 304))]
CASES += [('front_bwd', s) for s in ((1, 1, 2, 8), (2, 3, 24, 40), (1, 5, 8, 64), (2, 2, 96, 520))]
CASES += [('front_bwd', (_n, _k, _h, _w)) for _k in (1, 2, 3, 4) for _n, _h, _w in ((1, 2, 32), (2, 24, 64))]
CASES += [('front_bwd', (4, 1, 256, 512))]


def case_id(c):
    return '-'.join([c[0]] + [str(v) for v in c[1]])


def generic_cases():
    """What NLT_DEC_GENERIC=1 sends to another kernel: the dec cases at the U-Net's own widths."""
    return [c for c in CASES if c[0] == 'dec' and c[1][1] == 2 * c[1][0] and c[1][2] == 8 * c[1][0]]


def sha(*tensors):
    m = hashlib.sha256()
    for t in tensors:
        m.update(t.detach().cpu().contiguous().numpy().tobytes())
    return m.hexdigest()


def front_weights(rng):
    R = lambda s, a: torch.from_numpy(((rng.random(s, dtype=np.float32) - 0.5) * (2 * a)).astype(np.float32)).cuda()
    return dict(wq0=R((1, 1, 5, 16), 0.5), bq0=R((16,), 0.1), wo0=R((1, 1, 3, 16), 0.5), bo0=R((16,), 0.1),
                wqa=R((2, 2, 32, 16), 0.2), bqa=R((16,), 0.1), wqb=R((2, 2, 16, 16), 0.2), bqb=R((16,), 0.1),
                woa=R((2, 2, 16, 16), 0.2), boa=R((16,), 0.1), wob=R((2, 2, 16, 16), 0.2), bob=R((16,), 0.1),
                wh=R((1, 1, 36, 3), 0.5), bh=R((3,), 0.1),
                wq2=R((2, 2, 32, 32), 0.2), bq2=R((32,), 0.1), wo2=R((2, 2, 16, 32), 0.2), bo2=R((32,), 0.1))


_blobs = []


def blobs():
    """(weights, blob, blob_l2), once, on the device, never written."""
    if not _blobs:
        W = front_weights(np.random.default_rng(77))
        _blobs.append((W, C.front_pack_weights(*[W[k] for k in ('wq0', 'bq0', 'wo0', 'bo0', 'wqa', 'bqa', 'wqb', 'bqb', 'woa', 'boa',
                                                                  'wob', 'bob', 'wh', 'bh')]),
                       C.front_pack_l2_weights(W['wq2'], W['bq2'], W['wo2'], W['bo2'])))
    return _blobs[0]


def digest(c):
    kind, prm = c
    rng = np.random.default_rng([KINDS.index(kind)] + list(prm))
    U = lambda *s: torch.from_numpy(rng.random(s, dtype=np.float32) - np.float32(0.5)).cuda()
    S = lambda *s: torch.full(s, SENTINEL, device='cuda')
    G = lambda m: (((torch.arange(m, dtype=torch.float32) % 7) - 3.5) * 0.125).cuda()      # accumulators: never zero
    accs = ()
    if kind == 'dec':
        c_, cx, cs, n, h, w = prm
        x, skip = U(n, h, w, cx), U(n, h, w, cs)
        w2, b2, w1, b1 = U(2, 2, c_, cx + cs), U(c_), U(2, 2, c_, c_), U(c_)
        outs = (S(n, 2 * h, 2 * w, c_),)
        C.dec_block_forward(x, cx, skip, cs, n, h, w, w2, b2, w1, b1, c_, ALPHA, outs[0])
    elif kind == 'dec_map':
        c_, lds, n, h, w = prm
        x, skip = U(n, h, w, 2 * c_), U(n, h, w, lds)
        w2q, w1, b1, bmap = U(2, 2, c_, 6 * c_), U(2, 2, c_, c_), U(c_), U(1, 2 * h, 2 * w, c_)
        outs = (S(n, 2 * h, 2 * w, c_),)
        C.dec_block_forward_map(x, skip, lds, n, h, w, w2q, w1, b1, c_, ALPHA, bmap, outs[0])
    elif kind in ('back', 'back_train'):
        n, h2, w2_ = prm
        x, fm1, skip3 = U(n, h2, w2_, 8), U(n, h2, w2_, 32), U(n, 2 * h2, 2 * w2_, 3)
        ws2, bs2, ws1, bs1, wh = U(2, 2, 4, 40), U(4), U(2, 2, 4, 4), U(4), U(4, 3)
        outs = (S(n, 2 * h2, 2 * w2_, 3),)
        if kind == 'back':
            C.back_forward(x, fm1, skip3, n, h2, w2_, ws2, bs2, ws1, bs1, wh, ALPHA, outs[0])
        else:
            outs += (S(n, 2 * h2, 2 * w2_, 4), S(n, 2 * h2, 2 * w2_, 4))                    # u, v
            C.back_forward_train(x, fm1, skip3, n, h2, w2_, ws2, bs2, ws1, bs1, wh, ALPHA, *outs)
    elif kind == 'back_map':
        ldq, n, h2, w2_ = prm
        x, q1, skip3 = U(n, h2, w2_, 8), U(n, h2, w2_, ldq), U(n, 2 * h2, 2 * w2_, 3)
        ws2q, ws1, bs1, wh, bmap = U(2, 2, 4, 24), U(2, 2, 4, 4), U(4), U(4, 3), U(1, 2 * h2, 2 * w2_, 4)
        outs = (S(n, 2 * h2, 2 * w2_, 3),)
        C.back_forward_map(x, q1, ldq, skip3, n, h2, w2_, ws2q, ws1, bs1, wh, ALPHA, bmap, outs[0])
    elif kind in ('front', 'front_train', 'front2'):
        n, k, h, w = prm
        _, blob, blob_l2 = blobs()
        base, cvis, lvis, nn_rgb, nn_base = U(n, h, w, 3), U(n, h, w, 1), U(n, h, w, 1), U(n, k, h, w, 3), U(n, k, h, w, 3)
        fm1, skip3 = S(n, h // 2, w // 2, 32), S(n, h, w, 3)
        if kind == 'front2':
            outs = (fm1, skip3, S(n, h // 4, w // 4, 32), S(n, k, h // 4, w // 4, 32))      # ... qtmp2, otmp2
            C.front2_forward(base, cvis, lvis, nn_rgb, nn_base, n, k, h, w, blob, blob_l2, True, ALPHA, *outs)
        elif kind == 'front':
            outs = (fm1, S(n, k, h // 2, w // 2, 16), skip3)                                # fm1, obs1, skip3
            C.front_forward(base, cvis, lvis, nn_rgb, nn_base, n, k, h, w, blob, True, ALPHA, *outs)
        else:
            outs = (fm1, S(n, k, h // 2, w // 2, 16), skip3, S(n, h // 2, w // 2, 16), S(n, k, h // 2, w // 2, 16))   # ... qtmp1, otmp1
            C.front_forward_train(base, cvis, lvis, nn_rgb, nn_base, n, k, h, w, blob, True, ALPHA, *outs)
    elif kind in ('pack', 'pack_l2'):
        W = front_weights(rng)
        if kind == 'pack':
            outs = (S(C._size('nlt_front_packed_floats')),)
            C.front_pack_weights(*[W[k] for k in ('wq0', 'bq0', 'wo0', 'bo0', 'wqa', 'bqa', 'wqb', 'bqb', 'woa', 'boa', 'wob', 'bob',
                                                  'wh', 'bh')], out=outs[0])
        else:
            outs = (S(C._size('nlt_front_l2_packed_floats')),)
            C.front_pack_l2_weights(W['wq2'], W['bq2'], W['wo2'], W['bo2'], out=outs[0])
    elif kind == 'back_bwd':
        n, h2, w2_ = prm
        h, w = 2 * h2, 2 * w2_
        ins = (U(n, h2, w2_, 8), U(n, h2, w2_, 32), U(n, h, w, 4), U(n, h, w, 4), U(n, h, w, 3))   # x, fm1, u, v, dpred
        wts = (U(2, 2, 4, 40), U(2, 2, 4, 4), U(4, 3))
        outs = (S(n, h2, w2_, 8), S(n, h2, w2_, 32))                                        # dx, dfm1
        accs = tuple(G(m) for m in (640, 4, 64, 4, 12, 3))                                  # dw_s2 db_s2 dw_s1 db_s1 dw_head db_head
        ws = S(C._size('nlt_back_backward_workspace_floats', n, h2, w2_))
        C._call('nlt_back_backward', *[C._ptr(t) for t in ins], n, h2, w2_, *[C._ptr(t) for t in wts], ALPHA,
                *[C._ptr(t) for t in outs + accs], C._ptr(ws))
        outs += (ws,)
    else:
        n, k, h, w = prm
        W = blobs()[0]
        ins = (U(n, h, w, 3), U(n, h, w, 1), U(n, h, w, 1), U(n, k, h, w, 3), U(n, k, h, w, 3))
        dys = (U(n, h // 2, w // 2, 16), U(n, k, h // 2, w // 2, 16), U(n, h, w, 3))       # dy1q, dy1o, dpred
        accs = tuple(G(m) for m in (80, 16, 48, 16, 2048, 16, 1024, 16, 108))              # dwq0 dbq0 dwo0 dbo0 dwqa dbqa dwoa dboa dwh
        ws = S(C._size('nlt_front_backward_workspace_floats', n, h, w))
        C._call('nlt_front_backward', *[C._ptr(t) for t in ins], n, k, h, w, *[C._ptr(t) for t in dys],
                *[C._ptr(W[nm]) for nm in ('wq0', 'bq0', 'wo0', 'bo0', 'wqa', 'woa', 'wh')], *[C._ptr(t) for t in accs], C._ptr(ws))
        outs = (ws,)
    torch.cuda.synchronize()
    for o in outs:                                                       # (the launch ran: a digest of the pre-fill proves nothing)
        assert not bool((o == SENTINEL).all())
    for a in accs:
        assert not torch.equal(a.cpu(), G(a.numel()).cpu())
    return sha(*(outs + accs))


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_tail_bits_of_the_recorded_commit(c):
    assert digest(c) == golden()['digests'][case_id(c)]


def test_tail_bits_of_the_recorded_commit_generic_dec_block():
    """NLT_DEC_GENERIC=1 (read once per process): the recorder below in ONE fresh child process, against the file's second key."""
    env = dict(os.environ, NLT_DEC_GENERIC='1')
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got, want = json.loads(r.stdout.decode())['digests'], golden()['generic']
    assert set(got) == set(want)
    assert [k for k in sorted(want) if got[k] != want[k]] == []


def test_every_case_is_recorded_once():
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids) and set(ids) == set(golden()['digests'])
    assert {case_id(c) for c in generic_cases()} == set(golden()['generic'])


if __name__ == '__main__':
    generic = os.environ.get('NLT_DEC_GENERIC', '') == '1'
    d = {case_id(c): digest(c) for c in (generic_cases() if generic else CASES)}
    json.dump({'commit': os.environ.get('NLT_BITS_COMMIT', ''), 'library': 'libnlt_hip.so built from that commit, gfx950',
               'digest': 'SHA-256 of the whole of every output buffer, gradient accumulator and (backward entries) workspace '
                         '(float32 bytes; outputs and workspace pre-filled with %s, accumulators with a fixed non-zero pattern)'
                         % SENTINEL,
               'digests': d}, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write('\n')
