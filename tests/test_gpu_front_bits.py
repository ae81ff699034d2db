"""-m gpu: every entry point of csrc/front4.hip and csrc/front_ovr.hip against the BITS an earlier commit's build wrote.

The wave-per-strip front kernels have no atomics and a fixed order of operations, so their results are a function of the inputs
alone.  The parity tests (test_gpu_front4.py, test_gpu_infer.py) hold them to another kernel or to float64 within a bar; both
files moving together inside that bar would pass them.  Here each case runs one entry point on fixed inputs (numpy's default_rng on
the CPU, seeded per case; weight blobs from front_pack_weights / front_pack_l2_weights on such weights, the observation L0 zero for
front_ovr as in test_gpu_infer.py), into output buffers pre-filled with a fixed sentinel, and the SHA-256 of the WHOLE of every
output buffer -- so a store outside the image, or into the half of q1 that is the given map, shows too -- is compared with
tests/golden/front_bits.json.  That file names the commit whose build recorded the digests:

    NLT_HIP_LIB=<libnlt_hip.so built from that commit> python tests/test_gpu_front_bits.py > tests/golden/front_bits.json

(one fresh process per library: the library path is read once per process).  A change that is meant to alter the sequence of
floating-point operations of these kernels records the file anew from its own parent and says so.

What the cases reach ((n, k, h, w) = frames, observations, raw size; a strip = 4 x 16 level-1 texels = 8 x 32 raw texels):
  front4 float  1x1x8x8, 1x2x4x4: one border strip, seven XCD runs empty, the k = 1 prologue (query inputs as item 1); 2x3x24x40:
                two border strips a row, the clamped staging on both edges; 1x4x36x100: width no multiple of 8 (a strip 2 level-1
                texels wide, a row of strips 2 texels high); 2x1x24x80: 4 interior + 5 border strips per frame, item sequence
                across strips at k = 1; 1x6x64x64: k > 4, the load_obs(i + 2) branch; 2x2x24x40 without `+ base`.
  front4 uint8  the byte staging (8-byte pieces, 13 / 5 per row) at the same edges; 3x4x64x64 with a missing neighbour (-1) as one
                sample's FIRST observation (zeros staged by the previous strip's tail / the prologue) and as another's last.
  front4 train  the three kept maps (owned texels of the haloed stage-1 tile of both paths, the per-observation level-1 maps) on
                border-only, mixed and odd-width shapes.
  front_ovr     float and uint8: 1 frame 8x8 (border loop only, one wave); 2 x 24x40 (border only, both edges); 2 x 24x80
                (interior pipeline of one to two strips per wave + border loop) with q1 at ldq 32 (the untouched half is in the
                digest) and ldq 16; 36x132 / 36x136 (odd widths: partial last strip); 3 x 128x96 without `+ base`.
  long walk     512 x 768 frames: 1536 strips per frame, 23 of 24 strip columns interior.  front4 float k = 2, uint8 k = 2, train
                k = 1 with 3 frames = 4608 strips, 576 per XCD at a wave stride of 256: every wave walks two or three strips, the
                item sequence continues into the next strip and runs of an XCD cross frame boundaries.  front_ovr float and uint8
                with 5 frames = 7680 strips, 960 per XCD: three or four strips per wave -- the peeled iteration, the steady loop,
                the clamped prefetch past the last strip and the skipping of border strips inside the interior walk all run."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nlt_amd import capi as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'front_bits.json')
SENTINEL = -7.25
ALPHA = 0.3
KINDS = ('front4', 'front4_u8', 'front4_train', 'front_ovr', 'front_ovr_u8')


def case(kind, n, k, h, w, *flags):
    """flags: 'nobase' (add_base = 0), 'ldq16' (q1 dense instead of interleaved with the given half), 'miss' (two -1 neighbours)."""
    return (kind, n, k, h, w, tuple(sorted(flags)))


CASES = [case('front4', 1, 1, 8, 8), case('front4', 1, 2, 4, 4), case('front4', 2, 3, 24, 40), case('front4', 1, 4, 36, 100),
         case('front4', 2, 1, 24, 80), case('front4', 1, 6, 64, 64), case('front4', 2, 2, 24, 40, 'nobase'),
         case('front4_u8', 1, 1, 8, 8), case('front4_u8', 2, 3, 24, 40), case('front4_u8', 1, 2, 40, 72),
         case('front4_u8', 3, 4, 64, 64, 'miss'),
         case('front4_train', 1, 1, 8, 8), case('front4_train', 2, 3, 24, 40), case('front4_train', 1, 3, 36, 100),
         case('front4_train', 2, 1, 24, 80),
         # the long walks
         case('front4', 3, 2, 512, 768), case('front4_u8', 3, 2, 512, 768), case('front4_train', 3, 1, 512, 768),
         case('front_ovr', 5, 0, 512, 768), case('front_ovr_u8', 5, 0, 512, 768)]
for _kind in ('front_ovr', 'front_ovr_u8'):
    CASES += [case(_kind, 1, 0, 8, 8), case(_kind, 2, 0, 24, 40), case(_kind, 2, 0, 24, 80), case(_kind, 2, 0, 24, 80, 'ldq16'),
              case(_kind, 1, 0, 36, 132 if _kind == 'front_ovr' else 136), case(_kind, 3, 0, 128, 96, 'nobase')]


def case_id(c):
    kind, n, k, h, w, flags = c
    return '-'.join(['%s-%dx%dx%dx%d' % (kind, n, k, h, w)] + list(flags))


def sha(*tensors):
    m = hashlib.sha256()
    for t in tensors:
        m.update(t.detach().cpu().contiguous().numpy().tobytes())
    return m.hexdigest()


_blobs = {}


def blobs(ovr):
    """(blob, blob_l2), once per family, on the device, never written.  ovr: the observation L0 is zero (test_gpu_infer.py)."""
    if ovr not in _blobs:
        rng = np.random.default_rng([77, int(ovr)])
        R = lambda s, a: torch.from_numpy(((rng.random(s, dtype=np.float32) - 0.5) * (2 * a)).astype(np.float32)).cuda()
        Z = lambda s: torch.zeros(s, device='cuda')
        O = (lambda s, a: Z(s)) if ovr else R
        wq0, bq0, wo0, bo0 = R((1, 1, 5, 16), 0.5), R((16,), 0.1), O((1, 1, 3, 16), 0.5), O((16,), 0.1)
        wqa, bqa, wqb, bqb = R((2, 2, 32, 16), 0.2), R((16,), 0.1), R((2, 2, 16, 16), 0.2), R((16,), 0.1)
        woa, boa, wob, bob = O((2, 2, 16, 16), 0.2), O((16,), 0.1), O((2, 2, 16, 16), 0.2), O((16,), 0.1)
        wh, bh = R((1, 1, 36, 3), 0.5), R((3,), 0.1)
        wq2, bq2, wo2, bo2 = R((2, 2, 32, 32), 0.2), R((32,), 0.1), O((2, 2, 16, 32), 0.2), O((32,), 0.1)
        _blobs[ovr] = (C.front_pack_weights(wq0, bq0, wo0, bo0, wqa, bqa, wqb, bqb, woa, boa, wob, bob, wh, bh),
                       C.front_pack_l2_weights(wq2, bq2, wo2, bo2))
    return _blobs[ovr]


def digest(c):
    kind, n, k, h, w, flags = c
    rng = np.random.default_rng([KINDS.index(kind), n, k, h, w, len(flags)] + [ord(f[0]) for f in flags])
    U = lambda *s: torch.from_numpy(rng.random(s, dtype=np.float32)).cuda()
    B = lambda *s: torch.from_numpy(rng.integers(0, 256, s, dtype=np.uint8)).cuda()
    I = lambda hi, *s: torch.from_numpy(rng.integers(0, hi, s).astype(np.int32))
    S = lambda *s: torch.full(s, SENTINEL, device='cuda')
    add_base = 'nobase' not in flags
    ovr, u8 = kind.startswith('front_ovr'), kind.endswith('_u8')
    blob, blob_l2 = blobs(ovr)
    F = 5
    if u8:
        diffuse, rgb, cvis, lvis = B(F, h, w, 3), (None if ovr else B(F, h, w, 3)), B(F, h, w), B(F, h, w)
        ids = I(F, n).cuda()
    else:
        base, cvis, lvis = U(n, h, w, 3), U(n, h, w, 1), U(n, h, w, 1)
    if ovr:
        ldq = 16 if 'ldq16' in flags else 32
        p1, s0, p2 = U(1, h // 2, w // 2, 16) - 0.5, U(1, h, w, 4) - 0.5, U(1, h // 4, w // 4, 32) - 0.5
        outs = (S(n, h // 2, w // 2, ldq), S(n, h, w, 3), S(n, h // 4, w // 4, 32))                  # q1, skip3, qtmp2
        if u8:
            C.front_ovr_forward_u8(diffuse, cvis, lvis, ids, n, h, w, blob, blob_l2, p1, s0, p2, add_base, ALPHA, outs[0], ldq, *outs[1:])
        else:
            C.front_ovr_forward(base, cvis, lvis, n, h, w, blob, blob_l2, p1, s0, p2, add_base, ALPHA, outs[0], ldq, *outs[1:])
    else:
        outs = (S(n, h // 2, w // 2, 32), S(n, h, w, 3), S(n, h // 4, w // 4, 32), S(n, k, h // 4, w // 4, 32))   # fm1 skip3 qtmp2 otmp2
        if u8:
            nn_ids = I(F, n, k)
            if 'miss' in flags:
                nn_ids[0, 0] = -1                                        # a strip's FIRST observation
                nn_ids[1, k - 1] = -1                                    # ... and its last
            C.front4_forward_u8(diffuse, rgb, cvis, lvis, ids, nn_ids.cuda(), n, k, h, w, blob, blob_l2, add_base, ALPHA, *outs)
        else:
            nn_rgb, nn_base = U(n, k, h, w, 3), U(n, k, h, w, 3)
            if kind == 'front4_train':
                outs += (S(n, k, h // 2, w // 2, 16), S(n, h // 2, w // 2, 16), S(n, k, h // 2, w // 2, 16))   # obs1 qtmp1 otmp1
                C.front4_forward_train(base, cvis, lvis, nn_rgb, nn_base, n, k, h, w, blob, blob_l2, add_base, ALPHA, *outs)
            else:
                C.front4_forward(base, cvis, lvis, nn_rgb, nn_base, n, k, h, w, blob, blob_l2, add_base, ALPHA, *outs)
    torch.cuda.synchronize()
    for o in outs:                                                       # (the launch ran: a digest of the pre-fill proves nothing)
        assert not bool((o == SENTINEL).all())
    return sha(*outs)


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_front_bits_of_the_recorded_commit(c):
    assert digest(c) == golden()['digests'][case_id(c)]


def test_every_case_is_recorded_once():
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids) and set(ids) == set(golden()['digests'])


if __name__ == '__main__':
    d = {case_id(c): digest(c) for c in CASES}
    json.dump({'commit': os.environ.get('NLT_BITS_COMMIT', ''), 'library': 'libnlt_hip.so built from that commit, gfx950',
               'digest': 'SHA-256 of the whole of every output buffer (float32 bytes, pre-filled with %s)' % SENTINEL,
               'digests': d}, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write('\n')
