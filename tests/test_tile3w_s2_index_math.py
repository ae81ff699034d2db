"""CPU: the index arithmetic of the level hand-off kernel (csrc/conv_tile3.hip, conv_tile3w_s2_kernel) restated in Python.

  * the stride-1 stage keeps its MFMA column tiles by tap class: every B read of (class, tap pair, lane) finds, in the parity-split
    haloed planes, the texel and channel half conv_tile3w_kernel's row-organised read would multiply into the same output element;
  * every 16 lanes a ds_read_b128 serves together touch 16 different 16-byte slots modulo 16 (both for the four contiguous
    16-lane groups and for the groups of MI355X's LDS: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32);
  * the lane's eight handed-off values (the D fragments of both column tiles, after the epilogue) are the K octet the permuted
    stride-2 pack (csrc/pack_common.h, nlt_tile3s2_fragment) puts against them, for all four taps: the emulated MFMAs give the
    stride-2 conv of the tile.
"""
import numpy as np

PITCH, ODD, PLW = 20, 9, 112                       # S2_PITCH, S2_ODD, S2_PLW
LANES = np.arange(64)
KK, J = LANES >> 4, LANES & 15
YQ, XQ = J >> 3, J & 7
HW_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
HW_GROUPS += [[l + 32 for l in g] for g in HW_GROUPS]


def slot(row, x):
    return row * PITCH + (x & 1) * ODD + (x >> 1)


def write_units():
    """(lane, pass) -> (channel half, row, x, slot in the plane) or None, as the kernel's copy units enumerate them."""
    out = {}
    for i in range(3):
        for lane in range(64):
            u = lane + 64 * i
            t, hf = (u >> 4) * 8 + (u & 7), (u >> 3) & 1
            if t >= 85:
                out[(lane, i)] = None
                continue
            row, q = divmod(t, 17)
            x = 2 * q if q < ODD else 2 * (q - ODD) + 1
            out[(lane, i)] = (hf, row, x, hf * PLW + row * PITCH + q)
    return out


def read_slot(rs, tx):
    """Slot (within a term's pair of planes) every lane reads for fragment (row set rs = ty + pair, tx)."""
    xx = tx + (KK >> 1)
    return (KK & 1) * PLW + 2 * YQ * PITCH + XQ + rs * PITCH + (xx & 1) * ODD + (xx >> 1)


def test_every_texel_of_the_haloed_tile_is_written_once_where_the_reads_look_for_it():
    where = {}
    for key, u in write_units().items():
        if u is None:
            continue
        hf, row, x, s = u
        assert 0 <= row < 5 and 0 <= x < 17 and s == hf * PLW + slot(row, x) and s < 2 * PLW
        assert (hf, row, x) not in where and s not in where.values()
        where[(hf, row, x)] = s
    assert len(where) == 2 * 5 * 17
    assert max(s % PLW for s in where.values()) == 96                   # 97 slots of a 112-slot plane
    for c in range(4):                                                  # tap class (ty, tx) of the stride-2 conv
        ty, tx = c >> 1, c & 1
        for pl in range(2):                                             # tap pair of the stride-1 conv: taps (pl, 0), (pl, 1)
            s = read_slot(ty + pl, tx)
            for lane in range(64):
                kk, yq, xq = KK[lane], YQ[lane], XQ[lane]
                # output texel (2y' + ty, 2x' + tx); tap (a, b) = (pl, kk >> 1) reads input (y + a, x + b), channel half kk & 1
                want = (kk & 1, 2 * yq + ty + pl, 2 * xq + tx + (kk >> 1))
                assert where[want] == s[lane], (c, pl, lane)


def test_the_b128_reads_are_bank_conflict_free():
    groups = [list(range(16 * g, 16 * g + 16)) for g in range(4)] + HW_GROUPS
    for rs in range(3):
        for tx in range(2):
            s = read_slot(rs, tx)
            for t in range(3):                                          # the term planes lie 2 * PLW = 0 (mod 16) slots apart
                for g in groups:
                    assert len({int(s[l] + t * 2 * PLW) % 16 for l in g}) == 16, (rs, tx, t, g)
    assert PLW % 16 == 0 and (2 * PITCH) % 16 == 8


def s2_channel(kk, e):
    return (0 if e < 4 else 12) + 4 * kk + e


def pack_s2(w):
    """nlt_tile3s2_fragment without the term split: [tap 4][ct 4][lane 64][e 8] of a (2, 2, 32, 64) array."""
    cin, cout = w.shape[2:]
    wt = w.reshape(4, cin, cout)
    out = np.zeros((4, cout // 16, 64, 8))
    for t in range(4):
        for ct in range(cout // 16):
            for lane in range(64):
                for e in range(8):
                    out[t, ct, lane, e] = wt[t, s2_channel(lane >> 4, e), ct * 16 + (lane & 15)]
    return out


def test_the_handed_off_registers_are_the_k_octets_the_permuted_pack_expects():
    rng = np.random.default_rng(0)
    y1 = rng.standard_normal((4, 16, 32))                               # the wave's 4 x 16 tile of stride-1 results
    w2 = rng.standard_normal((2, 2, 32, 64))
    a = pack_s2(w2)
    assert sorted(s2_channel(kk, e) for kk in range(4) for e in range(8)) == list(range(32))
    out = np.zeros((2, 8, 64))
    for c in range(4):                                                  # K block = tap class
        ty, tx = c >> 1, c & 1
        # D layout of v_mfma_f32_16x16x32_bf16: lane (kk, j') holds rows 4kk..4kk+3 of column j' -- of column tile ct: channels
        # ct * 16 + 4kk + r.  The lane's eight values in hand-off order: column tile 0's four, then column tile 1's four.
        b = np.zeros((64, 8))
        for lane in range(64):
            kk, yq, xq = KK[lane], YQ[lane], XQ[lane]
            tex = y1[2 * yq + ty, 2 * xq + tx]
            b[lane] = [tex[ct * 16 + 4 * kk + r] for ct in range(2) for r in range(4)]
            assert [s2_channel(kk, e) for e in range(8)] == [ct * 16 + 4 * kk + r for ct in range(2) for r in range(4)]
        for ct2 in range(4):
            for lane in range(64):                                      # D[i][j'] += sum over (kk, e) A[lane (kk, i)][e] * B[lane (kk, j')][e]
                kk, i = KK[lane], J[lane]
                for jq in range(16):
                    out[jq >> 3, jq & 7, ct2 * 16 + i] += a[c, ct2, lane] @ b[kk * 16 + jq]
    want = np.einsum('yaxbc,abco->yxo', y1.reshape(2, 2, 8, 2, 32), w2)
    assert np.allclose(out, want, rtol=1e-12, atol=1e-12)


def test_the_launch_arithmetic_covers_every_tile_once_within_the_cu():
    """Items (frame, tile row, tile column) over workgroups and waves as the kernel walks them; the LDS the launcher asks for."""
    from nlt_amd import _capi as C
    lds = (2 * 2 * 2 * 3 * 64 + 4 * 4 * 3 * 64 + 8 * 6 * PLW) * 16 + 96 * 4
    assert lds <= 160 * 1024 and C.conv_tile3w_s2_plan(32, 32, 64) == lds
    assert C.conv_tile3w_s2_plan(64, 32, 64) is None and C.conv_tile3w_s2_plan(32, 64, 64) is None and C.conv_tile3w_s2_plan(32, 32, 32) is None
    xcd = lambda b, n: b if n & 7 else (b & 7) * (n >> 3) + (b >> 3)
    for frames, h, w, cus, max_wg in [(1, 4, 16, 256, 0), (2, 6, 24, 256, 1), (2, 32, 48, 256, 2), (1, 10, 18, 256, 4), (4, 256, 256, 256, 0)]:
        tiles_y, tiles_x = (h + 3) // 4, (w + 15) // 16
        items = frames * tiles_y * tiles_x
        nwg = min(cus, max_wg or cus, items)
        seen = []
        for b in range(nwg):
            r = xcd(b, nwg)
            it0, it1 = r * items // nwg, (r + 1) * items // nwg
            assert it1 > it0
            for wave in range(8):
                seen += list(range(it0 + wave, it1, 8))
        assert sorted(seen) == list(range(items))
