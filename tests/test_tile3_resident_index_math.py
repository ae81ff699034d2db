"""CPU: the launch arithmetic of the resident three-term conv (csrc/conv_tile3.hip: launch3r / conv_tile3r_kernel, launch3w /
conv_tile3w_kernel) restated in Python: the LDS a workgroup asks for, waves per workgroup and workgroups per CU, the grid, and the
(group, frame, tile) items each workgroup -- in the wave-private form each wave -- walks.  Every item has to be visited exactly
once, no configuration may ask for more than the CU's 160 KB or run fewer than 8 waves per CU, and `_capi.conv_tile3r_plan` (what
the plan asks before it routes a launch there) has to agree."""
import pytest

from nlt_amd import _capi as C

LDS_CU = 160 * 1024
TW = 16
PL, QS2 = 160, 272                                   # slots per (term, channel half) plane of the shared texel stage: k2s1 / k2s2


def budget(mode, cin, tn):
    """(LDS bytes, waves per workgroup, workgroups per CU, rows of a tile) or None = refused."""
    a = cin * (tn // 16) * 384                       # [cc = cin / 16][pair 2][ct = tn / 16][term 3][lane 64] x 16 bytes
    assert a == (cin // 16) * 2 * (tn // 16) * 3 * 64 * 16
    if mode == C.CONV_K2S1 and tn == 32:             # wave-private staging: 8 regions of 6 planes of (rows + 1) x 17 slots, padded to 16
        for rows in (4, 2):
            plane = ((rows + 1) * 17 + 15) // 16 * 16
            if a + 8 * 6 * plane * 16 <= LDS_CU:
                return (a + 8 * 6 * plane * 16, 8, 1, rows)
    lds = a + 2 * 6 * (PL if mode == C.CONV_K2S1 else QS2) * 16
    if lds > LDS_CU:
        return None
    return (lds, 8, 1, 8) if 2 * lds > LDS_CU else (lds, 4, 2, 8)


def xcd(b, n):
    return b if n & 7 else (b & 7) * (n >> 3) + (b >> 3)


def walk(mode, cin, cout, tn, frames, oh, ow, cus, max_wg):
    """Yields (workgroup, wave or None, group, frame, tile row, tile column) in the order the kernels visit them."""
    lds, waves, per_cu, rows = budget(mode, cin, tn)
    wave_private = mode == C.CONV_K2S1 and tn == 32
    tiles_y, tiles_x = (oh + rows - 1) // rows, (ow + TW - 1) // TW
    tiles = frames * tiles_y * tiles_x
    items = tiles * (cout // tn)
    nwg = cus * per_cu
    if max_wg > 0:
        nwg = min(nwg, max_wg)
    nwg = min(nwg, items)
    assert nwg >= 1

    def decode(item):
        g, t = divmod(item, tiles)
        t, tx = divmod(t, tiles_x)
        f, ty = divmod(t, tiles_y)
        return g, f, ty, tx
    for b in range(nwg):
        r = xcd(b, nwg)
        it0, it1 = r * items // nwg, (r + 1) * items // nwg
        assert it1 > it0                                                # no workgroup without work
        if not wave_private:
            for item in range(it0, it1):
                yield (b, None) + decode(item)
            continue
        seg = it0
        while seg < it1:                                                # a segment per group; wave v: items v, v + 8, ...
            g = seg // tiles
            seg_end = min(it1, (g + 1) * tiles)
            for wave in range(8):
                for item in range(seg + wave, seg_end, 8):
                    assert decode(item)[0] == g
                    yield (b, wave) + decode(item)
            seg = seg_end


TEST_SHAPES = [(C.CONV_K2S1, 32, 32, 32, 2, 20, 24), (C.CONV_K2S1, 64, 64, 32, 2, 20, 24), (C.CONV_K2S1, 64, 64, 64, 2, 20, 24),
               (C.CONV_K2S1, 128, 64, 32, 2, 20, 24), (C.CONV_K2S2, 32, 64, 64, 2, 20, 24), (C.CONV_K2S2, 64, 128, 32, 2, 20, 24),
               (C.CONV_K2S2, 32, 32, 32, 2, 20, 24)]
# the encoder levels of the 1024 x 1024 forward (4 frames; output size of the level), channels per group 32 and 64
BENCH_ROWS = [(C.CONV_K2S1, 32, 32, 32, 4, 512, 512), (C.CONV_K2S2, 32, 64, 32, 4, 256, 256), (C.CONV_K2S2, 32, 64, 64, 4, 256, 256),
              (C.CONV_K2S1, 64, 64, 32, 4, 256, 256), (C.CONV_K2S2, 64, 128, 32, 4, 128, 128), (C.CONV_K2S1, 128, 128, 32, 4, 128, 128),
              (C.CONV_K2S2, 128, 256, 32, 4, 64, 64)]


@pytest.mark.parametrize('shape', TEST_SHAPES + BENCH_ROWS)
@pytest.mark.parametrize('max_wg', [0, 3])
def test_every_item_once_within_the_lds_and_wave_budget(shape, max_wg):
    mode, cin, cout, tn, frames, oh, ow = shape
    lds, waves, per_cu, rows = budget(mode, cin, tn)
    assert lds <= LDS_CU and lds * per_cu <= LDS_CU and waves * per_cu >= 8
    assert C.conv_tile3r_plan(mode, cin, tn) == (lds, waves, per_cu, rows)
    tiles_y, tiles_x = (oh + rows - 1) // rows, (ow + TW - 1) // TW
    seen = {}
    for b, wave, g, f, ty, tx in walk(mode, cin, cout, tn, frames, oh, ow, 256, max_wg):
        assert 0 <= g < cout // tn and 0 <= f < frames and 0 <= ty < tiles_y and 0 <= tx < tiles_x
        assert (g, f, ty, tx) not in seen, ((g, f, ty, tx), b, wave, seen[(g, f, ty, tx)])
        seen[(g, f, ty, tx)] = (b, wave)
    assert len(seen) == (cout // tn) * frames * tiles_y * tiles_x
    assert max_wg == 0 or len({b for b, _ in seen.values()}) <= max_wg


def test_the_table_of_the_resident_form():
    """Which launches fit how: stride 1 at 32 channels per group on 8 wave-private regions (4-row tiles to cin = 112, 2-row to 144);
    else two 4-wave workgroups per CU up to 80 KB each, one 8-wave workgroup up to 160 KB; refused above."""
    K1, K2 = C.CONV_K2S1, C.CONV_K2S2
    assert budget(K1, 32, 32) == (24 * 1024 + 8 * 6 * 96 * 16, 8, 1, 4) and budget(K1, 64, 32) == (48 * 1024 + 73728, 8, 1, 4)
    assert budget(K1, 112, 32)[3] == 4 and budget(K1, 128, 32) == (96 * 1024 + 8 * 6 * 64 * 16, 8, 1, 2) and budget(K1, 144, 32)[3] == 2
    assert budget(K1, 160, 32) == (160 * 768 + 30720, 8, 1, 8)           # past the wave-private budget: the shared stage
    assert budget(K2, 32, 32) == (24 * 1024 + 52224, 4, 2, 8)
    assert budget(K1, 32, 64) == (48 * 1024 + 30720, 4, 2, 8)            # 78 KB twice: 156 KB
    assert budget(K2, 32, 64)[1:3] == (8, 1) and budget(K2, 64, 32)[1:3] == (8, 1)      # 48 + 51 KB: one workgroup
    assert budget(K1, 64, 64) == (96 * 1024 + 30720, 8, 1, 8) and budget(K2, 128, 32) == (96 * 1024 + 52224, 8, 1, 8)
    assert budget(K1, 256, 32) is None and budget(K1, 256, 64) is None and budget(K2, 256, 32) is None
    assert C.conv_tile3r_plan(K1, 256, 32) is None and C.conv_tile3r_plan(K1, 256, 64) is None
    assert C.conv_tile3r_plan(K1, 24, 32) is None and C.conv_tile3r_plan(C.CONV1X1, 32, 32) is None


def test_the_hint_bits_of_the_plan():
    """'lds' hint = channel count (low byte) + 256 (observations unfolded) + 512 (resident form): the low byte alone prices the
    launch, bit 8 alone unfolds."""
    for hint, want in ((32, (32, 0, 0)), (256 + 64, (64, 1, 0)), (512 + 32, (32, 0, 1)), (512 + 256 + 64, (64, 1, 1))):
        assert (hint & 255, (hint >> 8) & 1, (hint >> 9) & 1) == want
