"""-m gpu: both entry points of csrc/wgrad_tile.hip and csrc/wgrad_narrow.hip against the BITS an earlier commit's build wrote.

The tiled and narrow weight-gradient kernels are atomic-free and add in a fixed order, so their results are a function of the inputs
alone (tests/test_gpu_train_ops.py asserts that they repeat).  The parity tests hold them to float64 within a bar; every form moving
together inside that bar would pass them.  Here each case runs on fixed inputs (numpy's default_rng on the CPU, seeded per shape),
accumulates into a dw / db pre-filled with a fixed non-zero pattern, and the SHA-256 of the whole dw, db AND of the workspace the
test hands in (sized by the library's own query, sentinel-filled: the digest covers every slice's partial block, a store outside a
slice and the slice layout) is compared with tests/golden/wgrad_bits.json.  That file names the commit whose build recorded it:

    NLT_HIP_LIB=<libnlt_hip.so built from that commit> python tests/test_gpu_wgrad_bits.py > default.json
    NLT_HIP_LIB=<the same> NLT_WGRAD_GENERIC=1 python tests/test_gpu_wgrad_bits.py > generic.json

(one fresh process per run: the library path and NLT_WGRAD_GENERIC are read once per process; the second run's digests go under the
key 'generic' of the first's file.  NLT_WGRAD_S1T is read per call and is flipped in-process.)  The generic run leaves out the
cases marked `big` (more tiles than persistent workgroups of the LDS-tiled form, which the generic run never launches); its own
many-slice case is the 320 x 320 one: 400 slices through the index-deriving quad kernel and the eight-in-flight reduce loop.
A change that is meant to alter the sequence of floating-point operations of these kernels records the file anew from its own parent
and says so.

What the cases reach (n, h, w = frames and INPUT size; the GEMM row grid is the output's, the input's for Conv2DTranspose k2s2):
  tiled   all five families on a 6 x 12 grid (row walk) and a 6 x 10 grid (index-deriving); 5 x 2 blocks of dW; 1, 10 (no XCD order)
          and 178 (XCD order, the eight-in-flight reduce loop) slices; with and without db.
  narrow  scalar form with 2 / 4 / 8 row tiles and 1 / 2 column tiles, unaligned leading dimensions; quad form walking (grid 4 and
          12 wide: a wrap on every step / every third step; a second slice whose waves 1-3 have empty runs) and index-deriving
          (grid 10 wide; the k2s1 families at K = 128, N = 32); the LDS-tiled form at 16 and 32 channels, a clipped tile, more tiles
          than persistent workgroups, and the same shapes with NLT_WGRAD_S1T=0; more than 256 slices; Conv2DTranspose k2s2 with and
          without db."""
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

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wgrad_bits.json')
SENTINEL = -7.25
C1, K2S2, K2S1, D2S2, D2S1 = C.CONV1X1, C.CONV_K2S2, C.CONV_K2S1, C.DECONV_K2S2, C.DECONV_K2S1
NAMES = {C1: 'c1x1', K2S2: 'k2s2', K2S1: 'k2s1', D2S2: 'd2s2', D2S1: 'd2s1'}
FOUR = (K2S2, K2S1, D2S2, D2S1)


def grid(mode, gh, gw):
    """Input size of a gh x gw GEMM row grid."""
    return (2 * gh, 2 * gw) if mode == K2S2 else (gh, gw)


def case(entry, mode, c0, c1, cout, n, h, w, *flags):
    """flags: 'nodb' (no bias gradient), 'odd' (leading dimensions (c + 8) | 1 / cout + 1 instead of c + 8 / cout + 4), 's1t0'
    (NLT_WGRAD_S1T=0 for the call), 'big' (left out of the NLT_WGRAD_GENERIC=1 run)."""
    return (entry, mode, c0, c1, cout, n, h, w, tuple(sorted(flags)))


CASES = []
# ---- tiled entry
for _m in (C1, K2S2, K2S1, D2S2, D2S1):
    for _gw in (12, 10):
        CASES.append(case('tiled', _m, 8, 4, 12, 2, *grid(_m, 6, _gw)))
CASES += [case('tiled', K2S2, 48, 32, 80, 2, 12, 24),                    # 5 k-blocks x 2 n-blocks
          case('tiled', K2S1, 16, 0, 64, 2, 160, 160),                  # 178 slices: XCD order, the eight-in-flight reduce loop
          case('tiled', K2S1, 16, 0, 64, 2, 36, 40),                    # 10 slices: many, not in XCD order
          case('tiled', K2S1, 16, 0, 64, 2, 36, 40, 'nodb'),
          case('tiled', D2S1, 16, 0, 64, 2, 20, 24),                    # 4 slices: the one-thread-per-entry-quad reduce
          case('tiled', D2S2, 8, 4, 12, 2, 6, 12, 'nodb')]
# ---- narrow entry, scalar A (channel counts / leading dimensions that are no multiples of 4)
for _m in FOUR:
    _h, _w = grid(_m, 15, 10)
    for _co in ((3, 6) if _m == D2S2 else (12, 20)):                    # one / two column tiles
        CASES += [case('narrow', _m, 3, 0, _co, 2, _h, _w, 'odd'),      # 2 row tiles
                  case('narrow', _m, 10, 0, _co, 2, _h, _w),            # 4 row tiles (transposed k2s2: K = 10, 2 row tiles)
                  case('narrow', _m, 6, 14, _co, 2, _h, _w)]            # 8 row tiles (transposed k2s2: K = 20, 2 row tiles)
    if _m == D2S2:
        CASES += [case('narrow', _m, 40, 0, _co, 2, _h, _w, 'odd') for _co in (3, 6)]      # K = cin = 40: 4 row tiles
        CASES += [case('narrow', _m, 72, 0, _co, 2, _h, _w, 'odd') for _co in (3, 6)]      # K = cin = 72: 8 row tiles
# ---- narrow entry, quad A: 1 / 2 quad tiles x 1 / 2 column tiles; grids 4 and 12 wide walk (two slices), 10 wide does not
for _m in FOUR:
    for _gh, _gw in ((50, 4), (17, 12), (15, 10)):
        _h, _w = grid(_m, _gh, _gw)
        for _c0, _c1 in (((24, 16), (64, 32)) if _m == D2S2 else ((8, 8), (16, 16))):
            for _co in ((4, 8) if _m == D2S2 else (12, 32)):
                CASES.append(case('narrow', _m, _c0, _c1, _co, 2, _h, _w))
# ---- narrow entry, the LDS-tiled stride-1 form, and the same shapes without it
for _m in (K2S1, D2S1):
    for _c, _tw in ((16, 64), (32, 32)):
        for _fl in ((), ('s1t0',)):
            CASES += [case('narrow', _m, _c, 0, _c, 2, 8, 2 * _tw, *_fl),
                      case('narrow', _m, _c, 0, _c, 1, 6, _tw + 3, *_fl)]                     # clipped tiles
    for _fl in ((), ('s1t0',)):
        CASES += [case('narrow', _m, 32, 0, 32, 1, 132, 512, 'big', *_fl),                    # 528 tiles on 512 workgroups
                  case('narrow', _m, 16, 0, 16, 1, 132, 1536, 'big', *_fl)]                   # 792 tiles on 768 workgroups
# ---- narrow entry: more than 256 slices (the eight-in-flight loop of its reduce pass); transposed k2s2 without db
CASES += [case('narrow', K2S1, 16, 0, 16, 1, 320, 320), case('narrow', K2S1, 16, 0, 16, 1, 320, 320, 's1t0'),
          case('narrow', D2S2, 24, 16, 8, 2, 17, 12, 'nodb'), case('narrow', D2S2, 3, 0, 6, 2, 15, 10, 'nodb', 'odd'),
          case('narrow', K2S2, 8, 8, 12, 2, 34, 24, 'nodb')]


def case_id(c):
    entry, mode, c0, c1, cout, n, h, w, flags = c
    return '-'.join(['%s-%s-%d+%d-%d-%dx%dx%d' % (entry, NAMES[mode], c0, c1, cout, n, h, w)] + list(flags))


def sha(*tensors):
    m = hashlib.sha256()
    for t in tensors:
        m.update(t.detach().cpu().contiguous().numpy().tobytes())
    return m.hexdigest()


_cache = {}


def operands(mode, c0, c1, cout, n, h, w, odd):
    """(src0, ld0, src1, ld1, dp, ldp), once per shape, on the device, never written."""
    key = (mode, c0, c1, cout, n, h, w, odd)
    if key not in _cache:
        rng = np.random.default_rng([mode, c0, c1, cout, n, h, w])
        ld = lambda c: (c + 8) | 1 if odd else c + 8
        ldp = cout + 1 if odd else cout + 4
        oh, ow = (h // 2, w // 2) if mode == K2S2 else ((2 * h, 2 * w) if mode == D2S2 else (h, w))
        R = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).cuda()
        _cache[key] = (R(n, h, w, ld(c0)), ld(c0), R(n, h, w, ld(c1)) if c1 else None, ld(c1) if c1 else 0, R(n, oh, ow, ldp), ldp)
    return _cache[key]


def digest(c):
    entry, mode, c0, c1, cout, n, h, w, flags = c
    src0, ld0, src1, ld1, dp, ldp = operands(mode, c0, c1, cout, n, h, w, 'odd' in flags)
    nw = (1 if mode == C1 else 4) * (c0 + c1) * cout
    dw0 = ((torch.arange(nw, dtype=torch.float32) % 7) - 3.5) * 0.125       # never zero
    db0 = ((torch.arange(cout, dtype=torch.float32) % 5) + 0.5) * -0.25
    dw, db = dw0.cuda(), (None if 'nodb' in flags else db0.cuda())
    size, fn = (('nlt_wgrad_workspace_floats', 'nlt_conv_backward_weights_tiled') if entry == 'tiled' else
                ('nlt_wgrad_narrow_workspace_floats', 'nlt_conv_backward_weights_narrow'))
    need = getattr(C.lib(), size)(mode, c0, c1, n, h, w, cout)
    assert need > 0, (size, need)
    ws = torch.full((need,), SENTINEL, device='cuda')
    C._call(fn, mode, C._ptr(src0), ld0, c0, C._ptr(src1), ld1, c1, n, h, w, C._ptr(dp), ldp, cout, C._ptr(dw), C._ptr(db),
            C._ptr(ws), need)
    torch.cuda.synchronize()
    assert not torch.equal(dw.cpu(), dw0)                                # (the launch ran: a digest of the pre-fill proves nothing)
    assert db is None or not torch.equal(db.cpu(), db0)
    return sha(dw, ws) if db is None else sha(dw, db, ws)


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def generic_cases():
    return [c for c in CASES if 'big' not in c[-1]]


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_wgrad_bits_of_the_recorded_commit(c, monkeypatch):
    if 's1t0' in c[-1]:
        monkeypatch.setenv('NLT_WGRAD_S1T', '0')
    else:
        monkeypatch.delenv('NLT_WGRAD_S1T', raising=False)
    assert digest(c) == golden()['digests'][case_id(c)]


def test_wgrad_bits_of_the_recorded_commit_generic_forms():
    """NLT_WGRAD_GENERIC=1 (read once per process): the recorder below in ONE fresh child process, against the file's second key."""
    env = dict(os.environ, NLT_WGRAD_GENERIC='1')
    env.pop('NLT_WGRAD_S1T', None)
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
    generic = os.environ.get('NLT_WGRAD_GENERIC', '') == '1'
    d = {}
    for c in (generic_cases() if generic else CASES):
        os.environ['NLT_WGRAD_S1T'] = '0' if 's1t0' in c[-1] else '1'     # (read per call)
        d[case_id(c)] = digest(c)
    json.dump({'commit': os.environ.get('NLT_BITS_COMMIT', ''), 'library': 'libnlt_hip.so built from that commit, gfx950',
               'digest': 'SHA-256 of the whole dw, db (where given) and workspace (float32 bytes, sentinel %s in what is not '
                         'written; dw / db pre-filled with a fixed non-zero pattern)' % SENTINEL,
               'digests': d}, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write('\n')
