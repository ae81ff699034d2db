"""CPU: the index arithmetic of deterministic mode's two gather-form adjoints (csrc/deterministic.hip), restated in NumPy.

Resampler adjoint: count -> exclusive scan (chunk sums, chunk offsets, rescan) -> fill in an ARBITRARY order through falling
integer counters -> per-texel sort by key = camera pixel * 4 + corner -> float32 sum in key order.  Whatever order the fill
ran in, the result has to be the straightforward accumulation in ascending key order, bit for bit.

Resize adjoint: the candidate range an input element walks (a generous estimate) filtered by the adjoint's own footprint
expressions has to be exactly the set of output pixels whose clamped {lo, hi} holds the element.
"""
import numpy as np
import pytest

F = np.float32
SCAN_CHUNK = 2048                      # csrc/deterministic.hip: 256 threads x 8 counters


def contributions(warp, uvh, uvw):
    """(key, texel, weight) of every contribution warp_bwd_kernel makes, float32 arithmetic as in warp_corner()."""
    n, hc, wc, _ = warp.shape
    w = warp.reshape(-1, 2).astype(F)
    x, y = w[:, 0] * F(uvw), w[:, 1] * F(uvh)
    inside = (x > F(-1)) & (y > F(-1)) & (x < F(uvw)) & (y < F(uvh))
    fx, fy = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    cx, cy = fx + 1, fy + 1
    dx, dy = cx.astype(F) - x, cy.astype(F) - y
    f = np.arange(w.shape[0]) // (hc * wc)
    keys, texs, wts = [], [], []
    for corner in range(4):
        right, r = corner & 1, corner >> 1
        wx = (F(1) - dx if right else dx).astype(F)
        wy = (F(1) - dy if r else dy).astype(F)
        wt = (wx * wy).astype(F)
        xi, yi = fx + right, (cy if r else fy)
        ok = inside & (xi >= 0) & (xi <= uvw - 1) & (yi >= 0) & (yi <= uvh - 1) & ~((xi == 0) & (yi == 0)) & (wt != 0)
        p = np.nonzero(ok)[0]
        keys.append(p * 4 + corner); texs.append((f[p] * uvh + yi[p]) * uvw + xi[p]); wts.append(wt[p])
    return np.concatenate(keys), np.concatenate(texs), np.concatenate(wts)


def exclusive_scan_three_launches(cnt):
    """scan_chunk_sums_kernel / scan_chunk_offsets_kernel / scan_downsweep_kernel: off[0..T], off[T] = total."""
    T = len(cnt)
    chunks = (T + SCAN_CHUNK - 1) // SCAN_CHUNK
    chunk_sum = np.array([cnt[c * SCAN_CHUNK:(c + 1) * SCAN_CHUNK].sum() for c in range(chunks)], np.int64)
    chunk_off = np.concatenate(([0], np.cumsum(chunk_sum)))            # [chunks + 1], last = total
    off = np.zeros(T + 1, np.int64)
    for c in range(chunks):
        seg = cnt[c * SCAN_CHUNK:(c + 1) * SCAN_CHUNK]
        off[c * SCAN_CHUNK:c * SCAN_CHUNK + len(seg)] = chunk_off[c] + np.cumsum(seg) - seg
    off[T] = chunk_off[chunks]
    return off


def csr_ordered_sum(keys, texs, wts, g, T, rng):
    cnt = np.bincount(texs, minlength=T).astype(np.int64)              # (a) integer atomics: order-free
    off = exclusive_scan_three_launches(cnt)                           # (b)
    assert np.array_equal(off[:-1], np.cumsum(cnt) - cnt) and off[-1] == len(keys)
    slots = np.full(len(keys), -1, np.int64)
    left = cnt.copy()
    for i in rng.permutation(len(keys)):                               # (c) arrival order is arbitrary
        t = texs[i]
        slot = off[t] + left[t] - 1                                    # off + atomicSub(cnt, 1) - 1
        left[t] -= 1
        assert slots[slot] == -1
        slots[slot] = keys[i]
    assert (left == 0).all() and (slots >= 0).all()
    wt_of = dict(zip(keys.tolist(), wts.tolist()))                     # (the kernel recomputes the weight from the key)
    out = np.zeros((T, 3), F)
    for t in np.nonzero(cnt)[0]:                                       # (d)
        s = np.zeros(3, F)
        for k in np.sort(slots[off[t]:off[t + 1]]):
            s = (s + F(wt_of[int(k)]) * g[k >> 2]).astype(F)
        out[t] = s
    return out


def straightforward_ordered_sum(keys, texs, wts, g, T):
    out = np.zeros((T, 3), F)
    for i in np.argsort(keys, kind='stable'):
        out[texs[i]] = (out[texs[i]] + F(wts[i]) * g[keys[i] >> 2]).astype(F)
    return out


def _maps():
    rng = np.random.default_rng(3)
    n, hc, wc, uvh, uvw = 2, 12, 20, 24, 16
    jj, ii = np.meshgrid(np.arange(wc, dtype=F), np.arange(hc, dtype=F))
    chart = np.stack(((jj + F(0.37)) / F(wc) * F(0.9) + F(0.03), (ii + F(0.61)) / F(hc) * F(0.8) + F(0.1)), -1)[None].repeat(n, 0)
    rand = rng.random((n, hc, wc, 2), dtype=F)
    many = np.full((1, 64, 64, 2), 0.0, F)
    many[..., 0] = F(5.25) / F(uvw); many[..., 1] = F(7.5) / F(uvh)            # 4096 pixels on one texel quad
    edge = rng.random((n, hc, wc, 2), dtype=F)
    e = edge.reshape(-1, 2)
    e[0::7, 0] = F(-0.5) / F(uvw)                  # the (-1, 0) band
    e[1::7, 1] = F(-0.25) / F(uvh)
    e[2::7, 0] = (F(uvw) - F(0.5)) / F(uvw)        # the (W - 1, W) band
    e[3::7, 1] = (F(uvh) - F(0.75)) / F(uvh)
    e[4::7, 0] = F(3) / F(uvw)                     # exact integers: one weight of each pair is 0
    e[5::7, 1] = F(6) / F(uvh)
    e[6::7] = 0                                    # texel (0, 0): skipped
    return {'chart': (chart.astype(F), uvh, uvw), 'random': (rand, uvh, uvw), 'many_to_one': (many, uvh, uvw),
            'borders_and_integers': (edge, uvh, uvw)}


@pytest.mark.parametrize('kind', ['chart', 'random', 'many_to_one', 'borders_and_integers'])
def test_csr_steps_of_the_warp_adjoint_equal_the_ordered_accumulation(kind):
    warp, uvh, uvw = _maps()[kind]
    n, hc, wc, _ = warp.shape
    rng = np.random.default_rng(11)
    g = rng.standard_normal((n * hc * wc, 3)).astype(F)
    keys, texs, wts = contributions(warp, uvh, uvw)
    T = n * uvh * uvw
    assert len(keys) > 0 and len(set(keys.tolist())) == len(keys)                   # keys are distinct: the sort is total
    want = straightforward_ordered_sum(keys, texs, wts, g, T)
    for seed in (0, 1):
        got = csr_ordered_sum(keys, texs, wts, g, T, np.random.default_rng(seed))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not want[::uvh * uvw].any()                                              # texel (0, 0) of every frame gets nothing
    if kind == 'many_to_one':
        assert np.bincount(texs).max() == 4096
    if kind == 'borders_and_integers':
        x = warp.reshape(-1, 2)[:, 0] * F(uvw)
        assert ((x > -1) & (x < 0)).any() and ((x > uvw - 1) & (x < uvw)).any() and (x == np.floor(x)).any()


# ------------------------------------------------------------------------------------------------------------- resize
def footprint(o, scale, size):
    """resize_axis(): the adjoint's own float32 expressions (ceilf for hi, both clamped)."""
    src = (F(o) + F(0.5)) * scale - F(0.5)
    fl = np.floor(src)
    return max(int(fl), 0), min(int(np.ceil(src)), size - 1)


def candidates(i, scale, osize):
    """resize_candidates()"""
    lo = (F(i) - F(0.5)) / scale - F(0.5)
    hi = (F(i) + F(1.5)) / scale - F(0.5)
    return max(int(np.floor(lo)) - 1, 0), min(int(np.ceil(hi)) + 1, osize - 1)


SIZES = [(8, 16), (16, 12), (16, 8), (5, 13), (13, 5), (7, 7), (3, 10), (10, 3), (1, 4), (4, 1), (9, 11), (11, 9), (17, 64),
         (64, 17), (6, 9), (256, 192), (100, 301)]


@pytest.mark.parametrize('h,oh', SIZES)
def test_gather_range_of_the_resize_adjoint_is_the_brute_force_set(h, oh):
    assert (8, 16) in SIZES and (16, 12) in SIZES                       # the 2x and the 3/4x case
    scale = F(h) / F(oh)
    feet = [footprint(o, scale, h) for o in range(oh)]
    covered = 0
    for i in range(h):
        brute = [o for o in range(oh) if i in feet[o]]
        a, b = candidates(i, scale, oh)
        walked = [o for o in range(a, b + 1) if i in feet[o]]
        assert walked == brute, (h, oh, i, (a, b), brute)
        assert not brute or brute == list(range(brute[0], brute[-1] + 1))          # a contiguous range per axis
        covered += len(brute)
    assert covered >= oh                                                # every output touches at least one input
    # at an integer source coordinate both taps address the same element (hi from ceil, not floor + 1)
    if (h, oh) == (7, 7):
        assert all(lo == hi == o for o, (lo, hi) in enumerate(feet))
