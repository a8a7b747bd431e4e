// nmpc_mmp_block2.h -- layer2's geometry of the one float32 residual-block kernel, mmp_blkf_kernel of nmpc_mmp_block_f32.h
// (resnet34.layer2 of the reference's ConvMultiHypoNet(lite=True), net_module/net.py:45-61, submodules.py:21-40: four BasicBlocks
// at 32 channels, the first 16 -> 32 at stride 2 with a 1 x 1, stride-2 projection; "next" row f3, predictor `mmp`, opt-in). The
// block's formula, the MFMA fragments, the flat domain with its pixel groups, the parity split of the strided input, the bank
// argument, m written over the dead input chunk, the m-slot permutation, the projection in the epilogue, the four steps and the
// fixed summation order are stated there; here is what is layer2's own. The norms are folded on the host by mmp_stem.fold_block2.
// The sibling of nmpc_mmp_block.h (16 channels, stride 1), whose building blocks it keeps. The 32 output channels are TWO A
// operands per tap, both in every wave: half the LDS reads per fma of the 16-channel kernel.
//
// Decision 1 -- tile geometry. The flat domain is kB2R x kB2S = 12 x 48 positions, the tile of 8 x 44 outputs with a halo of
// two; position q = 48 r + c is the output pixel (8 ty - 2 + r, 44 tx - 2 + c). The 37 x 42 plane of layer2 is one tile wide and
// five high: 5 tiles of 352 cover 1 554 pixels, 88 % filled (the 15 x 28 tile on a stride of 32 would take 3 x 2 = 6 tiles of
// 420: 62 %). The row stride is a multiple of 16: a pixel group lies in one row. m is computed on rows 1 .. 10 (30 groups of 16
// positions), out on rows 2 .. 9 (24 groups), all 48 columns; columns 0, 1, 46, 47 of out and 0, 47 of m are computed from
// wrapped neighbours and never stored or used. Group j of m belongs to wave j & 3 in the order rows 2 .. 9, then row 1, then
// row 10: the wave's first 6 groups are exactly its groups of out (24 = 4 x 6, no copies there); of the 8 groups per wave of m,
// two waves have 7 and recompute a neighbour (discarded). Of the issued MFMAs of a 32 -> 32 block 79 % are useful work on a
// full tile (halo rows of m, four wrapped columns of 48, the two recomputed copies), 83 % of the strided 16 -> 32 block.
// Decision 2 -- stride-2 taps: the parity split, here with the flat offset -48 for ky = 0. Layout in LDS [sub-plane][channel]
// [592]; the plane stride is kB2P = 592 = 16 mod 32.
// Decision 3 -- LDS and occupancy. 32 channels of m on 592 words are 75 776 B; the input chunk (8 channels at stride 1 = 8
// planes, 4 channels at stride 2 = 16 planes: a strided chunk of 8 would stage 72 registers per thread next to 112
// accumulators) goes under m: 75 792 B static, two workgroups per CU (160 KB), which is what feeds the MFMA pipe in the
// 16-channel kernel. min_wg = 2 states it: 256 registers per lane, VGPRs + AGPRs. A chunk divides into the workgroup exactly (18
// / 36 values per thread) and is no larger than Cin's granularity of 8: the staging tests neither.
// Decision 4 -- the accumulators of id are NOT resident. 8 x 2 x 4 = 64 registers of m next to 6 x 2 x 4 = 48 of id, the staged
// chunk (18 / 36) and 18 weights compiled to 25 (stride 1) and 126 (stride 2) spilled VGPRs under the bound of 256. The
// projection is therefore computed in the epilogue (at stride 2 on the (even, even) sub-plane). Likewise at stride 2 the 36
// addresses and masks of the staged chunk are recomputed per chunk instead of kept across the MFMAs as loop invariants (73
// spilled VGPRs otherwise): again(2).
//
// 256 threads = 4 waves per workgroup. Stores of out: runs of 16 (14, 12 at a tile's edges) consecutive floats.
// Words of LDS read without being written (positions -1 and 576 of a plane, 47 and 528 of an m plane) are neighbours of
// wrapped columns only; what they hold is discarded.
//
// Modelled before the device run, from the instruction count (four waves on the four SIMDs of a CU: a tile takes as long as
// one wave's MFMAs). Per wave and tile: the strided first block (Cin = 16) 4 channel groups x (9 x 8 x 2 + 6 x 2 of the
// projection) + 8 x 9 x 6 x 2 = 624 + 864 = 1 488 MFMA; each of the other three 8 x 144 + 864 = 2 016: 7 536 for a tile of all
// four, of 32 cycles each, for 352 x 69 632 useful fma = 5 984 MFMA-equivalents per wave: 79 % useful. At B = 256, 4 pedestrians,
// N_hor = 20 (20 480 rows x 5 tiles over 256 CUs at 2.4 GHz) that is 102 400 x 7 536 x 32 / (256 x 2.4e9) = 40 ms per lock-step if
// the MFMA pipe never waits; 28 ms at the 78.6 T fma/s fp32 peak for the 2.22e12 useful fma alone; 5.8 ms for the 36.6 GB
// (x of the first block once, three reads and four writes of [32][37][42]) at the 6.29 TB/s copy rate.
// Measured (profiles/mmp_layer2_evaluate.json): 71.5 ms, 31.0 T useful fma/s = 39 % of the fp32 peak,
// 0.51 TB/s; torch's own layer2, eager, on the same rows: 128.8 ms. The model is short by 1.78 x (the 16-channel kernel: 1.8 x).
// What is believed to cost the rest, from the code, not from counters: as there, two waves per SIMD that stop at two barriers
// per chunk (288 MFMA between them at stride 1, 144 at stride 2) and at the third in front of the m store; epilogues without
// conv MFMAs; the strided block (22.7 T fma/s against 32-33 T of the others) also recomputes its staging addresses, reads x
// two floats apart and runs its projection in the epilogue. Not built: a third workgroup per CU, a double-buffered chunk,
// resident id accumulators in AGPRs.
//
// Compiler (hipcc -O3 --offload-arch=gfx950; tools/kernel_resources.py on the shipped code object): mmp_blkf_kernel<MmpBlock2Geom, 2, true>
// 212 VGPRs, 74 SGPRs, no SGPR spills; <1, true> 244 VGPRs, 106 SGPRs and 33 SGPR spills; <1, false> 244 VGPRs, 106 SGPRs and 28
// SGPR spills (to VGPR lanes: no memory); all 0 AGPRs, no VGPR spills, scratch 0, 75 792 B LDS, occupancy 2 waves per SIMD
// (registers and LDS agree). tests/test_mmp_block2_cpu.py holds every kernel of this family to that.
#pragma once

#include <hip/hip_runtime.h>

#include "nmpc_mmp_block_f32.h"

namespace nmpc {

struct MmpBlock2Params {
    int M, Cin, H, W, H2, W2, tx, ty;                // H, W: the input plane; H2, W2: the output plane; tiles along x, y
    const float *x;                                  // [M][Cin][H][W]
    const float *w1, *s1, *b1;                       // [32][Cin][3][3], [32], [32]
    const float *w2, *s2, *b2;                       // [32][32][3][3], [32], [32]
    const float *wd, *sd, *bd;                       // [32][Cin], [32], [32] (kernel <., true>) or unused
    float slope_mid, slope_out;
    float* out;                                      // [M][32][H2][W2]
};

constexpr int kB2Threads = 256;
constexpr int kB2C = 32;                             // output channels
constexpr int kB2NH = kB2C / 16;                     // A operands per tap
constexpr int kB2TH = 8, kB2TW = 44;                 // outputs per tile
constexpr int kB2S = kB2TW + 4;                      // row stride of the flat domain: 48
constexpr int kB2R = kB2TH + 4;                      // rows of the flat domain: 12
constexpr int kB2Q = kB2R * kB2S;                    // positions of the flat domain: 576
constexpr int kB2P = 592;                            // plane stride in LDS
constexpr int kB2GR = kB2S / 16;                     // pixel groups per row: 3
constexpr int kB2GO = kB2TH * kB2GR;                 // pixel groups of out: 24
constexpr int kB2GM = (kB2TH + 2) * kB2GR;           // pixel groups of m: 30
constexpr int kB2NO = kB2GO / 4;                     // pixel groups of out per wave: 6
constexpr int kB2NI = (kB2GM + 3) / 4;               // pixel groups of m per wave: 8
constexpr int kB2Lds = kB2C * kB2P + 4;              // words of static LDS
static_assert(kB2S % 16 == 0 && kB2GO % 4 == 0, "the flat domain does not fit the waves");
static_assert(kB2P % 32 == 16 && kB2P >= kB2Q + 2, "plane stride: bank spread, and the taps of the last group stay inside");
static_assert(kB2Lds * 4 <= 80 * 1024, "static LDS over half a CU's");

// first position of m's pixel group j: rows 2 .. 9 (the groups of out) first, then row 1, then row 10
__device__ __forceinline__ constexpr int mmp_b2_group(int j)
{
    return j < kB2GO ? 2 * kB2S + 16 * j : j < kB2GO + kB2GR ? kB2S + 16 * (j - kB2GO) : (kB2R - 2) * kB2S + 16 * (j - kB2GO - kB2GR);
}

// layer2's waves, for this geometry and the one on binary16 operands (nmpc_mmp_block2_f16.h): every wave holds both A operands
// and takes the pixel groups j & 3 == wave in the order of mmp_b2_group
struct MmpBlock2Waves {
    // two waves have 7 groups of m: their eighth slot computes the last group again and stores nothing
    static __device__ __forceinline__ int pixel_wave(int wave) { return wave; }
    static __device__ __forceinline__ int group(int wave, int i) { return mmp_b2_group(wave + 4 * i < kB2GM ? wave + 4 * i : kB2GM - 1); }
    static __device__ __forceinline__ int first_a(int) { return 0; }
    static __device__ __forceinline__ bool live(int wave, int i) { return wave + 4 * i < kB2GM; }
};

// layer2's geometry of mmp_blkf_kernel (nmpc_mmp_block_f32.h): position q of an x plane sits at word q + 1 (the first tap of
// position 48 is q = -1)
struct MmpBlock2Geom : MmpBlock2Waves {
    using Params = MmpBlock2Params;
    static constexpr int C = kB2C, Threads = kB2Threads, min_wg = 2, S = kB2S, Q = kB2Q, TH = kB2TH, TW = kB2TW;
    static constexpr int P = kB2P, SH = 1, Lds = kB2Lds;
    static constexpr int NI = kB2NI, NO = kB2NO, NH = kB2NH;
    static constexpr bool Fitted = false, MaskedXc = false;
    static constexpr int cc(int stride) { return stride == 2 ? 4 : 8; }
    static constexpr bool again(int stride) { return stride == 2; }
};

} // namespace nmpc
