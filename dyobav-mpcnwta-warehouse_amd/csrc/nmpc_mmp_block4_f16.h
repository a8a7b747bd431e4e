// nmpc_mmp_block4_f16.h -- layer4's geometry of the one residual-block kernel on binary16 MFMA operands, mmp_blkh_kernel of
// nmpc_mmp_block_f16.h: the block of nmpc_mmp_block4.h (resnet34.layer4 of the multi-hypothesis predictor's network: 128 output
// channels, stride 1 or 2, projection or identity; predictor `mmp`, opt-in on top of the opt-in fused layer4:
// MmpFrontEnd(half=("layer4",))). The rounding rule, the MFMA fragments, the octet-plane LDS layout with its bank argument, the
// packed-weight order, the four steps and the fixed summation order are stated there; here is what is layer4's own. 128 output
// channels are eight A groups g; 128 input channels are four K blocks per tap, the strided block's 64 two.
//
// Ported unchanged from nmpc_mmp_block4.h (proven there, with wrong-variant controls): the flat domain of 12 x 13 = 156
// positions of the OUTPUT plane, m and out on the SAME eight pixel groups from position 14 when the plane fits 10 x 11 and tiles
// of 8 x 9 with a halo of one along a longer side (oy, ox = 1 or 2), the flat-offset taps, the parity split of the strided input
// into four sub-planes on the same domain (tap ky reads row parity ky != 1 at offset -13 for ky = 0), m zero outside the plane
// and zeros on the 28 positions of the ring that no group covers, m written over the dead input, the projection in the epilogue.
//
// LDS: the shared octet planes, of kB4HPL = 160 positions = 2 560 B = 10 x 256 B (the domain's 156 padded by 4), position q at
// slot q. The m store is one ds_write_b64 per pixel group and A group. m is 16 planes = 40 960 B.
//
// Decision 1 -- workgroup size and occupancy: 256 threads = 4 waves, 40 960 B, __launch_bounds__(256, 3): THREE workgroups per
// CU, 3 waves per SIMD, at most 168 registers. Four workgroups fit the LDS exactly (4 x 40 960 B = the CU's 163 840 B) and were
// tried first: at 128 registers the 64 accumulator registers, the four A fragments of the next tap and the epilogue's affines
// do not fit, and the compiler spilled 11-24 dwords per lane in every kernel; no scratch is a requirement, so the bound is 3
// (142-162 registers, no spills). A chunk of 440 rows is then one round on 256 CUs x 3 (the f32 kernel: two). The alternatives:
//   - 512 threads as the f32 kernel, 2 A groups x 4 pixel groups per wave: 32 accumulator registers, the same LDS per
//     workgroup, so 2 workgroups = 4 waves per SIMD, but every barrier stops 8 waves and not 4, only two workgroups are out
//     of phase to fill a third's staging and stores, and a B fragment feeds two MFMAs, not four;
//   - 128 threads, 8 A groups x 4 or 4 x 8 per wave: 128 accumulator registers, over what even 3 waves per SIMD leave.
// Decision 2 -- (A group, pixel group) pairs: 8 x 8 = 64 pairs, 16 per wave: wave = 2 pw + cw takes the A groups 4 cw .. 4 cw + 3
// on the four pixel groups of parity pw: 64 accumulator registers, FOUR MFMAs per ds_read_b128 (the sibling: two) and four
// 16-byte weight loads per tap and K block = per 16 MFMAs = 256 cycles. LDS reads per workgroup and 128 -> 128 convolution: 4
// waves x 9 x 4 x 4 KB = 576 KB = 2 304 clocks of the array against 9 216 cycles of MFMA per SIMD. The alternative 2 A groups x 8
// pixel groups loads every A fragment once per workgroup and not twice (below) and doubles the LDS reads to half the array's time
// beside the MFMAs they feed; the second load of a fragment comes from the other parity's wave of the same workgroup in step
// with the first, so it is expected in L1. Not measured against each other.
// Decision 3 -- staging: the stride-1 x (128 channels = 16 planes) is staged AT ONCE, and m goes over it: a 128 -> 128 block
// (two of the three) is ONE chunk, three barriers and the ring's zeros in all. Chunks of 32 or 64 channels would not lower the
// LDS (m needs the 16 planes) and add a barrier each. A longer Cin (256, tests only) stages chunk after chunk. The strided
// kernel stages 32 channels x 4 sub-planes = 16 planes per chunk: the network's 64 channels are two chunks; all 64 at once
// would be 81 920 B = two workgroups per CU for one launch of three.
// Decision 4 -- ONE row of the batch per workgroup. Two rows would halve the weight traffic (below) and need 128 accumulator
// registers or a second pass over LDS of twice the size; a row's bits would stay its own either way. Counted, not built: the
// weights of a launch (590 KB) stay in every XCD's 4 MB L2, so the traffic is L2 -> L1, not memory.
//
// Step counts per wave: 1. per K block 9 taps x 4 pixel groups x 4 A groups of MFMA; 2. m -> LDS and zeros to the ring; 3. 4 K
// blocks x 9 taps x 4 x 4 on m. Every word of LDS that is read has been written: a plane of x on 0 .. 155 by the staging, a plane
// of m on 14 .. 141 by the groups and on the rest of 0 .. 155 by the zeros; the positions 156 .. 159 are never read (a tap
// reaches 141 + 14).
//
// Modelled before the device run, from instruction and byte counts. Per wave and row: a 128 -> 128 block 2 x 4 x 9 x 16 = 1 152
// MFMA, the strided block (Cin = 64) 2 x 9 x 16 + 2 x 4 x 4 + 576 = 896: 3 200 for a row of all three, of 16 cycles each = 51 200
// cycles (the f32 kernel: 2 x 12 800 x 32 = 819 200 per SIMD). At B = 256, 4 pedestrians, N_hor = 20 (20 480 rows over 256 CUs at
// 2.4 GHz, one wave of a row per SIMD): 80 x 51 200 / 2.4e9 = 1.71 ms per lock-step if the MFMA pipe never waits (f32: 27.3 ms).
// Bytes: activations 8.2 GB as the f32 kernel = 1.3 ms at the copy rate. Weights, per row: the strided block 147 456 + 16 384 +
// 294 912 B, each of the others 2 x 294 912 B (against 2 x 56 320 B of activations): 1.64 MB, and every fragment is asked for by
// two waves: 33.6 GB per lock-step out of L2 if L1 serves the second, 67 GB if not; a chunk of 440 rows pulls 0.26 GB through
// L2 per 128 -> 128 launch. At the 17-19 TB/s that L2 gave shared rows: 1.8-3.9 ms. The f32 kernel hid that behind 27 ms of
// MFMAs; this one cannot: EXPECTED to be bound by the weight traffic and by the staging loads and final stores that no MFMA of
// the same workgroup covers (the sibling: 5.8 x its MFMA floor), several times 1.71 ms and well under the f32 kernel's 58.3 ms;
// the target is 0.47 x the f32 launches (that kernel's own MFMA floor over its measured time).
// Measured (profiles/mmp_layer4_f16_evaluate.json; both kernels in one process, three runs each): the three
// launches on 440 rows 0.199 ms (0.197-0.202) against the f32 kernel's 1.253 (1.250-1.253): 0.159 x (the target 0.47 x is met);
// 9.26 ms per lock-step against 58.3, 199 T useful fma/s, 0.85 TB/s of activations = 13.5 % of the copy rate; the strided block
// 0.070 ms, the others 0.067-0.068; the stage 245.9 ms per lock-step against 293.5. 5.4 x the MFMA floor, at the low end of what
// the model expected ("several times 1.71 ms"). The weights: a 128 -> 128 launch pulls 440 x 589 824 B = 0.26 GB through L2 in
// 0.067 ms = 3.9 TB/s counted once per workgroup, 7.7 TB/s if L1 serves no second request -- a fifth to two fifths of the rate
// L2 gave shared rows, so the weight traffic is a large part of the time but not alone the bound. What waits besides, from the
// code and not from counters: per row a thread issues 80 loads of x in front of the first barrier and 64 dword stores behind
// the last MFMA, neither under MFMAs of its own workgroup, with two other workgroups on the CU to fill them.
//
// Compiler (hipcc -O3 --offload-arch=gfx950; tools/kernel_resources.py on the shipped code object): mmp_blkh_kernel<MmpBlock4HGeom, 2, true>
// 162 VGPRs, 82 SGPRs; <1, true> 142 VGPRs, 82 SGPRs; <1, false> 146 VGPRs, 70 SGPRs; all 40 960 B LDS, no spills, scratch 0,
// code 19-25 KB. tests/test_mmp_block4_f16_cpu.py holds the three kernels to: scratch 0, no spills, 40 960 B and at most 168
// registers (3 waves per SIMD, three workgroups per CU).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmpc_mmp_block4.h"
#include "nmpc_mmp_block_f16.h"

namespace nmpc {

struct MmpBlock4HParams {
    int M, Cin, H, W, H2, W2, tx, ty;                // as MmpBlock4Params
    int oy, ox;                                      // the first valid row / column of out in the domain: 1 (one tile) or 2
    const float *x;                                  // [M][Cin][H][W]
    const uint16_t *w1;                              // packed [9][ceil(Cin / 32)][8][64][8] binary16
    const float *s1, *b1;                            // [128], [128]
    const uint16_t *w2;                              // packed [9][4][8][64][8]
    const float *s2, *b2;                            // [128], [128]
    const uint16_t *wd;                              // packed [ceil(Cin / 32)][8][64][8] (kernel <., true>) or unused
    const float *sd, *bd;                            // [128], [128] or unused
    float slope_mid, slope_out;
    float* out;                                      // [M][128][H2][W2]
};

constexpr int kB4HThreads = 256;
constexpr int kB4HNH = 4;                            // A groups per wave: the wave's half of the eight
constexpr int kB4HPL = 160;                          // positions (of 16 bytes) per plane in LDS
constexpr int kB4HMP = kB4C / 8;                     // planes of m: 16 octets of channels
static_assert(kB4HPL * 16 % 256 == 0, "the plane stride must keep a lane group's two runs on distinct 16-byte slots");
static_assert(kB4HPL >= kB4Q && kB4M1 - 1 + kB4S + 1 < kB4Q && kB4M0 - kB4S - 1 >= 0, "a tap leaves the plane");
static_assert(kB4HMP * kB4HPL * 16 * 3 <= 160 * 1024, "three workgroups do not fit a CU's LDS");

// layer4's geometry of mmp_blkh_kernel (nmpc_mmp_block_f16.h): wave = 2 pw + cw takes the four pixel groups of parity pw, of m
// and of out alike, and the A groups 4 cw .. 4 cw + 3 (decision 2)
struct MmpBlock4HGeom {
    using Params = MmpBlock4HParams;
    static constexpr int C = kB4C, Threads = kB4HThreads, S = kB4S, Q = kB4Q, TH = kB4TH, TW = kB4TW;
    static constexpr int PL = kB4HPL, SH = 0;
    static constexpr int NI = kB4NI, NO = kB4NI, NH = kB4HNH;
    static constexpr int Unroll = 1;
    // Fitted: the sibling's domain (oy, ox in Params; the 28 positions of the ring before the first and behind the last group).
    // RegTight (decision 1): beside the 64 accumulators the registers hold one A group's affine, or one pixel group's loads of
    // the epilogue, at a time; all at once spilled
    static constexpr bool Fitted = true, RegTight = true;
    static constexpr int Ring = kB4Ring;
    static constexpr int ck(int stride) { return stride == 2 ? 32 : 128; }
    static constexpr int min_wg(int) { return 3; }
    static __device__ __forceinline__ int pixel_wave(int wave) { return wave >> 1; }
    static __device__ __forceinline__ int group(int pw, int i) { return kB4M0 + 16 * (pw + 2 * i); }
    static __device__ __forceinline__ int first_a(int wave) { return kB4HNH * (wave & 1); }
    static __device__ __forceinline__ bool live(int, int) { return true; }
    static __device__ __forceinline__ int ring(int j) { return j < kB4M0 ? j : kB4M1 - kB4M0 + j; }
};

} // namespace nmpc
