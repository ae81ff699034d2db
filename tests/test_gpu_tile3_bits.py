"""-m gpu: every entry point of csrc/conv_tile3.hip against the BITS an earlier commit's build wrote.

The other tile3 tests show that the four forms (streaming, resident shared-stage, resident wave-private, level hand-off) agree with
each other and with float64 within a bar; all four changing together would pass them.  Here each entry point runs on fixed inputs
(numpy's default_rng on the CPU) and the SHA-256 of its whole output buffers -- sentinel-filled padding included, so a store outside
the slice shows too -- is compared with tests/golden/tile3_bits.json.  That file names the commit whose build recorded the digests:

    NLT_HIP_LIB=<libnlt_hip.so built from that commit> python tests/test_gpu_tile3_bits.py > tests/golden/tile3_bits.json

(one fresh process per library: the library path and NLT_TILE3_KO are read once per process; NLT_TILE3_KO stays unset, the KO = 2
and KO = 4 instantiations are reached through kobs = 4).  A change that is meant to alter the sequence of floating-point operations
of these kernels records the file anew from its own parent and says so."""
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

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tile3_bits.json')
FRAMES = 2
SENTINEL = -7.25
K2S1, K2S2 = C.CONV_K2S1, C.CONV_K2S2
# (mode, cin, cout, tn, h, w): 20 x 24 outputs, a partial 8 x 16 (4 x 16, 2 x 16) tile on both edges.  Wave-private 4-row and 2-row
# (two groups); shared stage with 8 and with 4 waves; stride 2 with 8 and with 4 waves.
SHAPES = [(K2S1, 32, 32, 32, 20, 24), (K2S1, 128, 64, 32, 20, 24), (K2S1, 64, 64, 64, 20, 24), (K2S1, 32, 64, 64, 20, 24),
          (K2S2, 32, 64, 64, 40, 48), (K2S2, 32, 32, 32, 40, 48)]
# form: -1 = streaming (nlt_conv_tile3_forward), else max_workgroups of nlt_conv_tile3r_forward
CONV_CASES = [(s, form, nprod, kobs) for s in SHAPES for form in (-1, 0, 1) for nprod in (6, 9) for kobs in (1, 4)]
CONV_CASES += [(s, -1, nprod, 1) for s in (SHAPES[0], SHAPES[4]) for nprod in (1, 3)]
# hand-off (nlt_conv_tile3w_s2_forward): (h, w, frames, kobs, max_workgroups)
S2_CASES = [(s, nprod) for s in ((6, 24, 2, 3, 1), (10, 18, 1, 4, 4)) for nprod in (6, 9)]


def conv_id(case):
    (mode, cin, cout, tn, h, w), form, nprod, kobs = case
    return '%s-%d-%d-%d-%s-nprod%d-kobs%d' % ('k2s1' if mode == K2S1 else 'k2s2', cin, cout, tn,
                                            'streaming' if form < 0 else 'resident_wg%d' % form, nprod, kobs)


def s2_id(case):
    return 'handoff-%dx%d-frames%d-kobs%d-wg%d-nprod%d' % (case[0] + (case[1],))


def sha(*tensors):
    m = hashlib.sha256()
    for t in tensors:
        m.update(t.detach().cpu().contiguous().numpy().tobytes())
    return m.hexdigest()


_cache = {}


def conv_operands(mode, cin, cout, tn, h, w, kobs):
    """As test_gpu_tile3_resident._operands; once per (shape, kobs), on the device, never written."""
    key = (mode, cin, cout, tn, h, w, kobs)
    if key not in _cache:
        rng = np.random.default_rng(cin + cout + tn + h + kobs)
        ld = cin + 8
        src = torch.from_numpy(rng.standard_normal((FRAMES * kobs, h, w, ld)).astype(np.float32))
        wk = torch.from_numpy((rng.standard_normal((2, 2, cin, cout)) * (1.0 / np.sqrt(4 * cin))).astype(np.float32))
        bias = torch.from_numpy(rng.standard_normal(cout).astype(np.float32) * 0.1)
        _cache[key] = (src.cuda(), ld, C.pack_conv_tile3_weights(mode, wk.cuda(), cin, cout, tn), bias.cuda())
    return _cache[key]


def conv_digest(case):
    (mode, cin, cout, tn, h, w), form, nprod, kobs = case
    src, ld, packed, bias = conv_operands(mode, cin, cout, tn, h, w, kobs)
    oh, ow = (h // 2, w // 2) if mode == K2S2 else (h, w)
    out = torch.full((FRAMES * kobs, oh, ow, cout + 4), SENTINEL, device='cuda')
    mean = torch.full((FRAMES, oh, ow, 2 * cout), SENTINEL, device='cuda')
    fn, kw = (C.conv_tile3_forward, {}) if form < 0 else (C.conv_tile3r_forward, dict(max_workgroups=form))
    fn(mode, src, ld, cin, FRAMES, kobs, h, w, packed, bias, cout, tn, out, cout + 4,
       mean.view(-1)[cout:] if kobs > 1 else None, 2 * cout if kobs > 1 else 0, act=True, alpha=0.3, nprod=nprod, **kw)
    torch.cuda.synchronize()
    assert not (out[..., :cout] == SENTINEL).any()                        # (the launch ran: a digest of sentinels proves nothing)
    return sha(out, mean)


def s2_digest(case):
    (h, w, frames, kobs, max_wg), nprod = case
    cin, c1, c2, ld = 32, 32, 64, 40
    key = ('s2', h, w, frames, kobs)
    if key not in _cache:
        rng = np.random.default_rng(h * 131 + w * 7 + frames + kobs)
        R = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
        src = R(frames * kobs, h, w, ld)
        w1, b1 = R(2, 2, cin, c1) * (1.0 / np.sqrt(4 * cin)), R(c1) * 0.1
        w2, b2 = R(2, 2, c1, c2) * (1.0 / np.sqrt(4 * c1)), R(c2) * 0.1
        _cache[key] = (src.cuda(), C.pack_conv_tile3_weights(K2S1, w1.cuda(), cin, c1, 32), b1.cuda(),
                       C.pack_conv_tile3w_s2_weights(w2.cuda(), c1, c2), b2.cuda())
    src, p1, b1, p2, b2 = _cache[key]
    mean = torch.full((frames, h, w, 2 * c1), SENTINEL, device='cuda')
    out2 = torch.full((frames * kobs, h // 2, w // 2, c2 + 4), SENTINEL, device='cuda')
    C.conv_tile3w_s2_forward(src, ld, cin, frames, kobs, h, w, p1, b1, c1, mean.view(-1)[c1:], 2 * c1, p2, b2, c2, out2, c2 + 4,
                             nprod=nprod, max_workgroups=max_wg, act=True, alpha=0.3, act2=True, alpha2=0.3)
    torch.cuda.synchronize()
    assert not (out2[..., :c2] == SENTINEL).any()
    return sha(mean, out2)


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize('case', CONV_CASES, ids=conv_id)
def test_conv_tile3_bits_of_the_recorded_commit(case):
    assert conv_digest(case) == golden()['digests'][conv_id(case)]


@pytest.mark.parametrize('case', S2_CASES, ids=s2_id)
def test_conv_tile3w_s2_bits_of_the_recorded_commit(case):
    assert s2_digest(case) == golden()['digests'][s2_id(case)]


def test_every_case_is_recorded_once():
    ids = [conv_id(c) for c in CONV_CASES] + [s2_id(c) for c in S2_CASES]
    assert len(set(ids)) == len(ids) and set(ids) == set(golden()['digests'])


if __name__ == '__main__':
    d = {conv_id(c): conv_digest(c) for c in CONV_CASES}
    d.update({s2_id(c): s2_digest(c) for c in S2_CASES})
    json.dump({'commit': os.environ.get('NLT_BITS_COMMIT', ''), 'library': 'libnlt_hip.so built from that commit, gfx950',
               'digest': 'SHA-256 of the whole output buffers (float32 bytes, sentinel %s in what is not written)' % SENTINEL,
               'digests': d}, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write('\n')
