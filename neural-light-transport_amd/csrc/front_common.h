// Shared by the fused front kernels: the LDS plane of the first generation's haloed tile (fused.hip: front_kernel, its training
// variant and front2; the tile geometry itself is tail_tile.h's) and the packed-blob offsets: written by fused.hip's pack kernels,
// read by its front kernels and, through front_strip.h, by the wave-per-strip kernels (front4.hip, front_ovr.hip), which have their
// own geometry there.
#pragma once
#include "nlt_common.h"

namespace {

constexpr int PLT = 160;                   // LDS plane of one channel quad of one path's haloed tile (153 -> 160 slots)
constexpr int PATH = 4 * PLT * 4;          // floats per path: [kk][PLT][4] -- planar by channel quad, so the 16 lanes
                                           // a ds_read_b128 services together hit 16 different 16-byte slots

// packed-blob offsets (floats); written by front_pack_kernel, read by front_kernel
constexpr int OFF_AQ2 = 0;                 // [8][64]     folded q stride-2 conv, MFMA m x lane
constexpr int OFF_AO2 = 512;               // [3][64]     folded obs stride-2 conv
constexpr int OFF_AQ1 = 704;               // [4][64][4]  q stride-1 conv: tap x lane x s4
constexpr int OFF_AO1 = 1728;              // [4][64][4]
constexpr int OFF_BQ2 = 2752, OFF_BO2 = 2768, OFF_BQ1 = 2784, OFF_BO1 = 2800;   // [16] each
constexpr int OFF_WSK = 2816;              // [8][3]  head share of the raw channels
constexpr int OFF_BSK = 2840;              // [3]
constexpr int OFF_WSK8 = 2848;             // [8][3]  the same rows times fl(1 / 255): the uint8-store front kernel feeds raw BYTE values (r05)
constexpr int BLOB = 2880;

// second blob: level 2's stride-2 convs (fused into the front kernel when k <= 4)
constexpr int OFF3_AQ = 0;                 // [2 rt][8 = slab*4 + c4][64][4]  query (2,2,32,32): slab 0 = q1, 1 = mean o1
constexpr int OFF3_AO = 4096;              // [2 rt][4 c4][64][4]             obs   (2,2,16,32)
constexpr int OFF3_BQ = 6144, OFF3_BO = 6176, BLOB3 = 6208;

}  // namespace
