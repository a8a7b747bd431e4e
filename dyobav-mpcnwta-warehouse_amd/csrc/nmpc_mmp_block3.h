// nmpc_mmp_block3.h -- layer3's geometry of the one float32 residual-block kernel, mmp_blkf_kernel of nmpc_mmp_block_f32.h
// (resnet34.layer3 of the reference's ConvMultiHypoNet(lite=True), net_module/net.py:45-61, submodules.py:21-40: six BasicBlocks
// at 64 channels, the first 32 -> 64 at stride 2 with a 1 x 1, stride-2 projection; "next" row f3, predictor `mmp`, opt-in). The
// block's formula, the MFMA fragments, the flat domain with its pixel groups, the parity split of the strided input, the bank
// argument, m written over the dead input chunk, the m-slot permutation, the projection in the epilogue, the four steps and the
// fixed summation order are stated there; here is what is layer3's own. The norms are folded on the host by mmp_stem.fold_block3.
// The sibling of nmpc_mmp_block2.h (32 channels). The 64 output channels are FOUR A operands per tap, two per wave, and a group
// of 16 positions is 16 accumulator VGPRs per lane.
//
// Decision 1 -- tile geometry. The flat domain is kB3R x kB3S = 11 x 25 = 275 positions, the tile of 7 x 21 outputs with a halo
// of two; position q = 25 r + c is the output pixel (7 ty - 2 + r, 21 tx - 2 + c). The 19 x 21 plane of layer3 is one tile wide
// and three high. The row stride 25 is no multiple of 16: a pixel group runs across row ends.
//   m is needed on rows 1 .. 9, columns 1 .. 23: positions 26 .. 248, kB3GM = 14 groups from position 26 (26 + 16 a, a = 0 .. 13);
//   out on rows 2 .. 8, columns 2 .. 22: positions 52 .. 222, covered by the kB3GO = 12 groups a = 1 .. 12 (42 .. 233) of the same grid,
// so a group of out is a group of m. Positions in the two halo columns on either side (0, 1, 23, 24 for out; 0, 24 for m) are
// computed from wrapped neighbours and never stored or used.
// The alternatives, for the 19 x 21 plane and a 64 -> 64 block (useful = 2 x 399 / 16 = 49.9 group-convolutions per row):
//   - the whole plane in one workgroup of 512 threads: 23 x 25 = 575 positions, m 33 groups + out 30; 8 waves take 5 + 4 each:
//     72 issued, 69 % useful -- but m is 147 456 B, ONE workgroup per CU, and every barrier (two per chunk, one in front of
//     the m store) and every epilogue then stops the whole CU's MFMA pipes. The siblings' 1.8 x over their models is
//     believed to be exactly such stops with TWO workgroups per CU; with one there is nothing to fill them.
//   - three tiles of 7 rows, 256 threads, two workgroups per CU (m 77 824 B): 14 + 12 = 26 groups per tile, 78 issued, 64 %
//     useful. BUILT: 8 % more MFMAs issued than the whole plane, and a second workgroup to run while one waits.
// Decision 2 -- the waves. 14 and 12 groups do not divide by four waves, and four A operands per B read in every wave would
// round them to 16 + 12 (59 %). So the workgroup's four waves are 2 x 2: wave = 2 pw + hw computes the channel halves
// 2 hw, 2 hw + 1 (32 channels: TWO A operands per ds_read_b32, as in the 32-channel kernel -- one LDS instruction per 2 048
// fma, which is what that kernel runs at) for the groups of parity pw: 7 groups of m and 6 of out each, exactly. Group j of m
// (wave parity j & 1, index j >> 1) is a = j + 1 for j < 12 (the groups of out first), a = 0 for j = 12, a = 13 for j = 13.
// 7 x 2 x 4 = 56 accumulator VGPRs per lane.
// Decision 3 -- stride-2 taps: the parity split, here with the flat offset -25 for ky = 0. Layout in LDS [sub-plane][channel]
// [304]; the plane stride is kB3P = 304 = 16 mod 32; the second convolution's groups are g = 0 .. 15.
// Decision 4 -- LDS and occupancy. 64 channels of m on 304 words are 77 824 B; the input chunk (16 channels at stride 1 = 16
// planes, 8 channels at stride 2 = 32 planes; a thread stages 18 / 35 values) goes under m: 77 840 B static, two workgroups per
// CU. min_wg = 2 states it: two waves per SIMD, 256 registers per lane. A chunk of 16 channels (stride 1) puts 4 x 9 x 7 x 2 =
// 504 MFMA per wave between two barrier pairs (the sibling: 288); a Cin that is no multiple of 16 stages zeros for the missing
// channels and skips their MFMAs.
// Decision 5 -- the projection runs in the epilogue on x read again (L2), per pixel group of out, as in the sibling (there
// resident accumulators spilled; here they would fit, and are not built: the projection is 0.5 % of layer3's fma).
//
// 256 threads = 4 waves per workgroup; 7 pixel groups of m and 6 of out per wave.
// Words of LDS read without being written (positions 16 .. 25 and 250 .. 259 of an m plane, 275 of an x plane) feed wrapped
// columns and the unused ends of the first and last group only; what they hold is discarded.
//
// Modelled before the device run, from the instruction count (four waves on the four SIMDs of a CU: a tile takes as long as
// one wave's MFMAs). Per wave and tile: the strided first block (Cin = 32) 8 channel groups x 9 x 7 x 2 + 6 x 8 x 2 of the
// projection + 16 x 9 x 6 x 2 = 1 008 + 96 + 1 728 = 2 832 MFMA; each of the other five 16 x 126 + 1 728 = 3 744: 21 552 for a tile
// of all six, of 32 cycles each, for 133 (a third of the 399 pixels) x 426 112 useful fma = 13 837 MFMA-equivalents per wave: 64 % useful.
// At B = 256, 4 pedestrians, N_hor = 20 (20 480 rows x 3 tiles over 256 CUs at 2.4 GHz) that is 61 440 x 21 552 x 32 / (256 x
// 2.4e9) = 69 ms per lock-step if the MFMA pipe never waits; 44 ms at the 78.6 T fma/s fp32 peak for the 3.48e12 useful fma
// alone; 4.3 ms for the 27.1 GB (x of the first block once, five reads and six writes of [64][19][21]) at the 6.29 TB/s copy rate.
// Measured (profiles/mmp_layer3_evaluate.json): 121.8 ms, 28.6 T useful fma/s = 36 % of the fp32 peak,
// 0.22 TB/s; torch's own layer3, eager, on the same rows in the same process: 170.4 ms (169-174 over three runs; the kernels
// 121-122). The model is short by 1.77 x (the 32-channel kernel: 1.78 x, the 16-channel one: 1.8 x). The strided block runs at 22.3 T
// fma/s (28 %), the five others at 28.2-29.3 T (36-37 %): with 64 % of the issued MFMAs useful the pipe is busy 56-58 % of the
// time (the 32-channel kernel: 40-43 % at 79 % useful, busy 51-54 %). What is believed to cost the rest, from the code, not from counters: as in the siblings two waves
// per SIMD that stop at two barriers per chunk and at a third in front of the m store, and epilogues without conv MFMAs (here
// 48 dword stores per lane). One experiment: the next channel group's 18 weights loaded under the MFMAs of the group at work,
// in both convolutions (200 / 220 VGPRs): 2.594 ms against 2.618 ms for the six launches on 440 rows, 1 %, the spread between
// runs -- the weight loads are not what waits; not kept. Not built: resident id accumulators (registers are there: 0.5 % of
// the fma), a double-buffered chunk (LDS is not there beside m at two workgroups per CU), the whole-plane workgroup.
//
// Compiler (hipcc -O3 --offload-arch=gfx950; tools/kernel_resources.py on the shipped code object): mmp_blkf_kernel<MmpBlock3Geom, 2, true>
// 196 VGPRs, 105 SGPRs; <1, true> 177 VGPRs, 99 SGPRs; <1, false> 177 VGPRs, 86 SGPRs; all 0 AGPRs, no VGPR or SGPR spills,
// scratch 0, 77 840 B LDS, occupancy 2 waves per SIMD (registers -- at most 256 -- and LDS agree).
// tests/test_mmp_block3_cpu.py holds every kernel of this family to that.
#pragma once

#include <hip/hip_runtime.h>

#include "nmpc_mmp_block_f32.h"

namespace nmpc {

struct MmpBlock3Params {
    int M, Cin, H, W, H2, W2, tx, ty;                // H, W: the input plane; H2, W2: the output plane; tiles along x, y
    const float *x;                                  // [M][Cin][H][W]
    const float *w1, *s1, *b1;                       // [64][Cin][3][3], [64], [64]
    const float *w2, *s2, *b2;                       // [64][64][3][3], [64], [64]
    const float *wd, *sd, *bd;                       // [64][Cin], [64], [64] (kernel <., true>) or unused
    float slope_mid, slope_out;
    float* out;                                      // [M][64][H2][W2]
};

constexpr int kB3Threads = 256;
constexpr int kB3C = 64;                             // output channels
constexpr int kB3NH = 2;                             // A operands per tap and wave: the wave's two channel halves of four
constexpr int kB3TH = 7, kB3TW = 21;                 // outputs per tile
constexpr int kB3S = kB3TW + 4;                      // row stride of the flat domain: 25
constexpr int kB3R = kB3TH + 4;                      // rows of the flat domain: 11
constexpr int kB3Q = kB3R * kB3S;                    // positions of the flat domain: 275
constexpr int kB3P = 304;                            // plane stride in LDS
constexpr int kB3M0 = kB3S + 1;                      // first position of m: 26
constexpr int kB3GM = ((kB3TH + 2) * kB3S - 2 + 15) / 16; // pixel groups of m: positions 26 .. 248 -> 14
constexpr int kB3GO = kB3GM - 2;                     // pixel groups of out: 12 (all of m's but the first and the last)
constexpr int kB3NO = kB3GO / 2;                     // pixel groups of out per wave: 6
constexpr int kB3NI = kB3GM / 2;                     // pixel groups of m per wave: 7
constexpr int kB3Lds = kB3C * kB3P + 4;              // words of static LDS
static_assert(kB3GM % 2 == 0, "the groups do not fit the two wave parities");
static_assert(kB3M0 + 16 <= 2 * kB3S + 2 && kB3M0 + 16 * (kB3GO + 1) >= (kB3TH + 1) * kB3S + kB3TW + 2, "the groups of out do not cover the tile");
static_assert(kB3M0 + 16 * kB3GM + kB3S + 1 <= kB3Q + 1 && kB3M0 + 16 * kB3GM <= kB3Q, "a tap of the last group of m leaves the plane");
static_assert(kB3P % 32 == 16 && kB3P >= kB3Q + 2, "plane stride: bank spread, and the taps of the last group stay inside");
static_assert(kB3Lds * 4 <= 80 * 1024, "static LDS over half a CU's");

// first position of m's pixel group j: the groups of out first (a = 1 .. 12), then the first (a = 0), then the last (a = 13)
__device__ __forceinline__ constexpr int mmp_b3_group(int j) { return kB3M0 + 16 * (j < kB3GO ? j + 1 : j == kB3GO ? 0 : kB3GM - 1); }

// layer3's waves, for this geometry and the one on binary16 operands (nmpc_mmp_block3_f16.h): wave = 2 pw + hw takes the pixel
// groups of parity pw (7 of m, its first 6 of out) and the A operands 2 hw, 2 hw + 1 (decision 2)
struct MmpBlock3Waves {
    static __device__ __forceinline__ int pixel_wave(int wave) { return wave >> 1; }
    static __device__ __forceinline__ int group(int pw, int i) { return mmp_b3_group(pw + 2 * i); }
    static __device__ __forceinline__ int first_a(int wave) { return 2 * (wave & 1); }
    static __device__ __forceinline__ bool live(int, int) { return true; }
};

// layer3's geometry of mmp_blkf_kernel (nmpc_mmp_block_f32.h)
struct MmpBlock3Geom : MmpBlock3Waves {
    using Params = MmpBlock3Params;
    static constexpr int C = kB3C, Threads = kB3Threads, min_wg = 2, S = kB3S, Q = kB3Q, TH = kB3TH, TW = kB3TW;
    static constexpr int P = kB3P, SH = 1, Lds = kB3Lds;
    static constexpr int NI = kB3NI, NO = kB3NO, NH = kB3NH;
    static constexpr bool Fitted = false, MaskedXc = true;
    static constexpr int cc(int stride) { return stride == 2 ? 8 : 16; }
    static constexpr bool again(int) { return true; }
};

} // namespace nmpc
