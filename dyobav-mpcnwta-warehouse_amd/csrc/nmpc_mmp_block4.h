// nmpc_mmp_block4.h -- layer4's geometry of the one float32 residual-block kernel, mmp_blkf_kernel of nmpc_mmp_block_f32.h
// (resnet34.layer4 of the reference's ConvMultiHypoNet(lite=True), net_module/net.py:63-82, submodules.py:21-40: three BasicBlocks
// at 128 channels, the first 64 -> 128 at stride 2 with a 1 x 1, stride-2 projection; "next" row f4, predictor `mmp`, opt-in). The
// block's formula, the MFMA fragments, the flat domain with its pixel groups, the parity split of the strided input, the bank
// argument, m written over the dead input chunk, the m-slot permutation, the projection in the epilogue, the four steps and the
// fixed summation order are stated there; here is what is layer4's own. The norms are folded on the host by mmp_stem.fold_block4.
// The sibling of nmpc_mmp_block3.h (64 channels); what it does not keep is the tile. The 128 output channels are EIGHT A
// operands per tap, two per wave.
//
// Decision 1 -- tile geometry. ONE flat domain of the OUTPUT plane: kB4R x kB4S = 12 x 13 = 156 positions; m is computed on
// its inner kB4MH x kB4MW = 10 x 11 (rows 1 .. 10, columns 1 .. 11: positions 14 .. 141, kB4G = 8 groups of 16 from position 14,
// the last one ending exactly on (10, 11)), and OUT ON THE SAME EIGHT GROUPS. layer4's plane is 10 x 11: it is one tile, and
// the ring of m that the second convolution reads round it is the zero padding, so no halo of m is computed at all. Per axis:
//   - a side of the output plane that fits (H2 <= 10, W2 <= 11) is ONE tile whose position 0 is pixel -1; out is valid on the
//     whole inner side, the words of the ring are zeros written beside m;
//   - a longer side is cut into tiles of kB4MH - 2 = 8 rows (kB4MW - 2 = 9 columns): position 0 is pixel 8 t - 2, m on the inner
//     side is the tile with a halo of one, out is valid on rows 2 .. 9 (columns 2 .. 10). Same code: only the origin and the
//     first valid row differ (o = 1 or 2, uniform per launch and axis).
// The alternatives, for the 10 x 11 plane and a 128 -> 128 block (useful = 2 x 110 / 16 = 13.75 group-convolutions per row):
//   - a ring-of-two domain as in the sibling, 14 x 15: m 12 groups + out 10 = 22 issued, 62 % useful;
//   - the plane in two tiles of 5 rows, two workgroups per CU (m 128 x 144 words = 73 728 B): m on 7 rows = 6 groups + out 5
//     = 11 per tile, 22 issued, 62 % useful, and x and the weights read twice;
//   - the whole plane, no halo: 8 + 8 = 16 issued, 110 / 128 = 86 % useful. BUILT: 27 % fewer MFMAs than either.
// The sibling rejected its whole-plane workgroup: there it saved 8 % of the MFMAs and cost 147 KB (one workgroup per CU).
// Here it saves 27 % and the price is the same -- m is 128 x 176 words = 90 112 B, over half a CU's 160 KB, ONE workgroup per
// CU, so every barrier stops the CU's MFMA pipes with nothing to fill them. A saving of 27 % is believed to outweigh stops
// that cost the siblings' 1.8 x over their models WITH a second workgroup; the measurement below says what it did.
// Decision 2 -- the waves. One workgroup per CU must bring two waves per SIMD itself: 512 threads = 8 waves. 8 channel
// sixteenths x 8 groups = 64 (A, group) pairs, 8 per wave: wave = 4 pw + cw computes the channel sixteenths 2 cw, 2 cw + 1 (32
// channels: TWO A operands per ds_read_b32, one LDS instruction per 2 048 fma, what the siblings run at) for the four groups
// of parity pw (a = pw + 2 i). 4 x 2 x 4 = 32 accumulator VGPRs per lane. Four A operands on two groups would halve the LDS
// reads and double the weight loads per MFMA (36 registers of weights per channel group for 72 MFMAs); not built.
// Decision 3 -- stride-2 taps: the parity split, here with the flat offset -13 for ky = 0. Layout in LDS [sub-plane][channel]
// [176]; the plane stride is kB4P = 176 = 16 mod 32; the second convolution's groups are g = 0 .. 31.
// Decision 4 -- LDS and occupancy. 128 slots of m on 176 words are 90 112 B static; the input chunk (32 channels at stride 1 =
// 32 planes, 16 channels at stride 2 = 64 planes: cc(STRIDE); a thread stages 10 / 20 values) goes under m. Threads = 512,
// min_wg = 1: one workgroup per CU, two waves per SIMD, 256 registers per lane.
// A chunk of 32 channels (stride 1) puts 8 x 9 x 4 x 2 = 576 MFMA per wave between two barrier pairs (the sibling: 504); a Cin
// that is no multiple of the chunk stages zeros for the missing channels and skips their MFMAs.
// Decision 5 -- the projection runs in the epilogue on x read again (L2), per pixel group of out, as in the siblings (1 % of
// layer4's fma).
//
// 512 threads = 8 waves per workgroup; 4 pixel groups per wave, of m and of out alike. Step 2 also writes zeros to the positions
// 0 .. 13 and 142 .. 155 of every slot (the ring that no group covers: outside the plane wherever a valid out reads it).
// Every word of LDS that is read has been written: an x plane on 0 .. 155 by the staging, an m plane on 14 .. 141 by the
// groups and on the rest of 0 .. 155 by the zeros.
//
// Modelled before the device run, from the instruction count (two waves on each of the four SIMDs of a CU: a tile takes as
// long as two waves' MFMAs). Per wave and tile: the strided first block (Cin = 64) 16 channel groups x 9 x 4 x 2 + 4 x 16 x 2
// of the projection + 32 x 9 x 4 x 2 = 1 152 + 128 + 2 304 = 3 584 MFMA; each of the other two 2 304 + 2 304 = 4 608: 12 800 for a
// row of all three, of 32 cycles each, for 90.1 M useful fma = 11 000 MFMA-equivalents per wave: 86 % useful. At B = 256, 4
// pedestrians, N_hor = 20 (20 480 rows over 256 CUs at 2.4 GHz) that is 80 x 2 x 12 800 x 32 / 2.4e9 = 27.3 ms per lock-step if
// the MFMA pipe never waits; 23.5 ms at the 78.6 T fma/s fp32 peak for the 1.85e12 useful fma alone; 1.3 ms for the 8.2 GB
// ([64][19][21] once, two reads and three writes of [128][10][11]) at the 6.29 TB/s copy rate.
// Measured (profiles/mmp_layer4_evaluate.json): 58.3 ms, 31.7 T useful fma/s = 40 % of the fp32 peak; torch's
// own layer4, eager, on the same rows in the same process: 95.4 ms. The model is short by 2.14 x (the siblings: 1.77-1.8), and
// the arithmetic says where the difference to them is (no counter run was made): the launches come per chunk of 22 pedestrians
// = 440 rows = 440 workgroups, one per CU, so a chunk takes TWO rounds on 256 CUs where the model counted 1.72 (16 %), and per
// round a stride-1 workgroup takes 215 us against the 123 us of its 2 x 4 608 MFMAs: 1.75 x, the siblings' factor. What is
// believed to cost that, from the code: two waves per SIMD that stop at two barriers per chunk and at a third in front of
// the m store, and epilogues without conv MFMAs -- with nothing else on the CU to fill the stops, as Decision 1 feared; the
// 27 % fewer MFMAs paid for it (0.611 x torch's layer4; layer3 reached 0.715 x). Not built: the two-tile variant, a chunk size that
// fills the second round (the chunk is set by memory), resident id accumulators.
//
// Compiler (hipcc -O3 --offload-arch=gfx950; tools/kernel_resources.py on the shipped code object): mmp_blkf_kernel<MmpBlock4Geom, 2, true>
// 124 VGPRs, 94 SGPRs; <1, true> 102 VGPRs, 84 SGPRs; <1, false> 102 VGPRs, 71 SGPRs; all 0 AGPRs, no VGPR or SGPR spills,
// scratch 0, 90 112 B LDS, code 16-28 KB, occupancy one workgroup = 2 waves per SIMD (LDS decides; registers would allow more).
// tests/test_mmp_block4_cpu.py holds every kernel of this family to that.
#pragma once

#include <hip/hip_runtime.h>

#include "nmpc_mmp_block_f32.h"

namespace nmpc {

struct MmpBlock4Params {
    int M, Cin, H, W, H2, W2, tx, ty;                // H, W: the input plane; H2, W2: the output plane; tiles along x, y
    int oy, ox;                                      // the first valid row / column of out in the domain: 1 (one tile) or 2
    const float *x;                                  // [M][Cin][H][W]
    const float *w1, *s1, *b1;                       // [128][Cin][3][3], [128], [128]
    const float *w2, *s2, *b2;                       // [128][128][3][3], [128], [128]
    const float *wd, *sd, *bd;                       // [128][Cin], [128], [128] (kernel <., true>) or unused
    float slope_mid, slope_out;
    float* out;                                      // [M][128][H2][W2]
};

constexpr int kB4Threads = 512;
constexpr int kB4C = 128;                            // output channels
constexpr int kB4NH = 2;                             // A operands per tap and wave: the wave's two channel sixteenths of eight
constexpr int kB4MH = 10, kB4MW = 11;                // the plane of m in a tile; the outputs of a tile where the side fits
constexpr int kB4TH = kB4MH - 2, kB4TW = kB4MW - 2;  // outputs per tile along a side that does not fit: 8 x 9
constexpr int kB4S = kB4MW + 2;                      // row stride of the flat domain: 13
constexpr int kB4R = kB4MH + 2;                      // rows of the flat domain: 12
constexpr int kB4Q = kB4R * kB4S;                    // positions of the flat domain: 156
constexpr int kB4P = 176;                            // plane stride in LDS
constexpr int kB4M0 = kB4S + 1;                      // first position of m: 14
constexpr int kB4G = (kB4MH * kB4S - 2 + 15) / 16;   // pixel groups of m and of out: positions 14 .. 141 -> 8
constexpr int kB4NI = kB4G / 2;                      // pixel groups per wave: 4
constexpr int kB4M1 = kB4M0 + 16 * kB4G;             // one past the last position of the groups: 142
constexpr int kB4Ring = kB4M0 + kB4Q - kB4M1;        // positions of a slot that no group covers: 28
constexpr int kB4Lds = kB4C * kB4P;                  // words of static LDS
static_assert(kB4G % 2 == 0, "the groups do not fit the two wave parities");
static_assert(kB4M1 >= kB4MH * kB4S + kB4MW + 1, "the groups do not cover the plane of m");
static_assert(kB4M0 - kB4S - 1 >= 0 && kB4M1 - 1 + kB4S + 1 < kB4Q, "a tap leaves the domain");
static_assert(kB4P % 32 == 16 && kB4P >= kB4Q, "plane stride: bank spread, and the domain fits");
static_assert(kB4Lds * 4 <= 160 * 1024, "static LDS over a CU's");

// tiles along a side of n outputs that holds m of them in one tile and t = m - 2 per tile otherwise (host and tests)
__host__ __device__ constexpr long long mmp_b4_tiles(long long n, int m) { return n <= m ? 1 : (n + m - 3) / (m - 2); }

// layer4's geometry of mmp_blkf_kernel (nmpc_mmp_block_f32.h): wave = 4 pw + cw takes the four pixel groups of parity pw, of m
// and of out alike, and the A operands 2 cw, 2 cw + 1 (decision 2); the domain is fitted to the plane of m (decision 1)
struct MmpBlock4Geom {
    using Params = MmpBlock4Params;
    static constexpr int C = kB4C, Threads = kB4Threads, min_wg = 1, S = kB4S, Q = kB4Q, TH = kB4TH, TW = kB4TW;
    static constexpr int P = kB4P, SH = 0, Lds = kB4Lds;
    static constexpr int NI = kB4NI, NO = kB4NI, NH = kB4NH;
    static constexpr bool Fitted = true, MaskedXc = true;
    static constexpr int Ring = kB4Ring;
    static constexpr int cc(int stride) { return stride == 2 ? 16 : 32; }
    static constexpr bool again(int) { return true; }
    static __device__ __forceinline__ int pixel_wave(int wave) { return wave >> 2; }
    static __device__ __forceinline__ int group(int pw, int i) { return kB4M0 + 16 * (pw + 2 * i); }
    static __device__ __forceinline__ int first_a(int wave) { return 2 * (wave & 3); }
    static __device__ __forceinline__ bool live(int, int) { return true; }
    static __device__ __forceinline__ int ring(int j) { return j < kB4M0 ? j : kB4M1 - kB4M0 + j; }
};

} // namespace nmpc
