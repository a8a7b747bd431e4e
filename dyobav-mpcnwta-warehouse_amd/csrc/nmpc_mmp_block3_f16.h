// nmpc_mmp_block3_f16.h -- layer3's geometry of the one residual-block kernel on binary16 MFMA operands, mmp_blkh_kernel of
// nmpc_mmp_block_f16.h: the block of nmpc_mmp_block3.h (resnet34.layer3 of the multi-hypothesis predictor's network: 64 output
// channels, stride 1 or 2, projection or identity; predictor `mmp`, opt-in on top of the opt-in fused layer3:
// MmpFrontEnd(half=("layer3",))). The rounding rule, the MFMA fragments, the octet-plane LDS layout with its bank argument, the
// packed-weight order, the four steps and the fixed summation order are stated there; here is what is layer3's own. 64 channels
// are two K blocks per tap and four A groups, the strided block's 32 input channels one K block.
//
// Ported unchanged from the sibling (proven there, with wrong-variant controls): the flat domain of 11 x 25 = 275 positions of
// the OUTPUT plane around a tile of 7 x 21 outputs, its 14 pixel groups of m from position 26 and 12 of out, the flat-offset
// taps, the parity split of the strided input into four sub-planes on the same domain (tap ky reads row parity ky != 1 at
// offset -25 for ky = 0), m zero outside the plane, m written over the dead input, the projection in the epilogue, 256
// threads = 2 x 2 waves (wave = 2 pw + hw: pixel groups of parity pw, channel halves 2 hw, 2 hw + 1: 7 + 6 groups and TWO A
// operands per B read each), one workgroup per [row][tile row][tile column].
//
// Decision 1 -- LDS layout: the shared octet planes, of kB3HPL = 288 positions = 4 608 B = 18 x 256 B, position q at slot q. The
// alternative [position][64 channels] is counted in nmpc_mmp_block_f16.h. The m store is one ds_write_b64 per pixel group and
// channel half.
// Decision 2 -- LDS size and occupancy: OCCUPANCY, not fewer barriers. m is 8 planes = 36 864 B. At stride 1 the chunk of x is 64
// channels = 8 planes, and m goes over it: 36 864 B static, FOUR workgroups per CU (147 456 of 163 840 B), 4 waves per SIMD,
// at most 128 registers per lane. A 64 -> 64 block (five of the six) is then ONE chunk: no chunk loop, three barriers in all
// (staged, conv1 read, m written) against the sibling's 2 x 4 + 2. Keeping x beside m (73 728 B, two workgroups) would save one
// barrier of the three and halve what can run while a workgroup waits at the other two or stores its 48 dwords per lane; with
// the MFMA time a sixteenth, those waits are what is left (below). The strided kernel stages its whole 32-channel K block in
// four sub-planes: 16 planes = 73 728 B, two workgroups per CU as the sibling -- one launch of six. Chunks of 16 channels with
// half the K block zero would fit four, and issue conv1's MFMAs twice.
// Decision 3 -- no register prefetch of the next chunk: the network's blocks are one chunk; a longer Cin (up to 256, tests
// only) stages chunk after chunk behind a barrier.
// Decision 4 -- MFMA-to-load ratio: per wave one ds_read_b128 (1 KB) feeds two MFMAs = 32 cycles, half the budget of two b128
// per 32-cycle gap; the CU's four waves read 936 KB per 64 -> 64 tile = 3 744 clocks of the LDS array at 256 B / clock against
// 7 488 of MFMA. The weights: two 16-byte loads per lane (2 KB per wave, L1 / L2 hits: 73 728 B of w1 / w2 in all) per tap and
// K block = per 14 or 12 MFMAs.
//
// Step counts per wave: 1. per K block 9 taps x 7 pixel groups x 2 halves of MFMA; 3. 2 K blocks x 9 taps x 6 groups x 2 halves
// on m. Words of LDS read without being written (position 275 .. 287 of a plane, 16 .. 25 and 250 .. 259 of m) feed wrapped
// columns and the unused ends of the first and last group only, as in the sibling.
//
// Modelled before the device run, instruction counts only. Per wave and tile: a 64 -> 64 block 2 x 9 x 7 x 2 + 2 x 9 x 6 x 2 =
// 252 + 216 = 468 MFMA, the strided block 126 + 12 + 216 = 354: 2 694 for a tile of all six, of 16 cycles each = 43 104 cycles
// (the f32 kernel: 21 552 x 32 = 689 664). At B = 256, 4 pedestrians, N_hor = 20 (61 440 tiles over 256 CUs at 2.4 GHz): 4.3 ms per
// lock-step if the MFMA pipe never waits (f32: 69 ms); 4.3 ms for the 27.1 GB at the copy rate, unchanged. Neither floor is
// expected: per tile a thread issues 72 loads of x, waits, converts, and at the end stores 48 dwords, none of it under MFMAs of
// its own workgroup; only the other three workgroups of the CU fill that. Expected from this: the kernel is bound by its loads
// and stores, well under the f32 kernel's 121.8 ms and several times over 4.3 ms.
// Measured (profiles/mmp_layer3_f16_evaluate.json; both kernels in one process, three runs each): the six
// launches on 440 rows 0.535 ms (0.534-0.542) against the f32 kernel's 2.628 (2.627-2.633): 0.204 x; 24.9 ms per lock-step, 150 T
// useful fma/s, 1.04 TB/s = 17 % of the copy rate; the strided block 0.127 ms, the others 0.085-0.088. 5.8 x the MFMA floor: what
// waits is, from the code and not from counters, the staging loads in front of the first barrier and the stores behind the last
// MFMA. The device keeps binary16 subnormals in the MFMA (tests/test_gpu_mmp_block3_f16.py): the model has no flush term.
//
// Compiler (hipcc -O3 --offload-arch=gfx950; tools/kernel_resources.py on the shipped code object): mmp_blkh_kernel<MmpBlock3HGeom, 2, true>
// 165 VGPRs, 86 SGPRs, 73 728 B LDS; <1, true> 124 VGPRs, 86 SGPRs, 36 864 B; <1, false> 124 VGPRs, 74 SGPRs, 36 864 B; no
// spills, scratch 0. tests/test_mmp_block3_f16_cpu.py holds them to: scratch 0, no spills, 36 864 B and at most 128 registers
// (4 waves per SIMD) at stride 1, 73 728 B and at most 256 (2 waves per SIMD) at stride 2.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmpc_mmp_block3.h"
#include "nmpc_mmp_block_f16.h"

namespace nmpc {

struct MmpBlock3HParams {
    int M, Cin, H, W, H2, W2, tx, ty;                // as MmpBlock3Params
    const float *x;                                  // [M][Cin][H][W]
    const uint16_t *w1;                              // packed [9][ceil(Cin / 32)][4][64][8] binary16
    const float *s1, *b1;                            // [64], [64]
    const uint16_t *w2;                              // packed [9][2][4][64][8]
    const float *s2, *b2;                            // [64], [64]
    const uint16_t *wd;                              // packed [ceil(Cin / 32)][4][64][8] (kernel <., true>) or unused
    const float *sd, *bd;                            // [64], [64] or unused
    float slope_mid, slope_out;
    float* out;                                      // [M][64][H2][W2]
};

constexpr int kB3HPL = 288;                          // positions (of 16 bytes) per plane in LDS
static_assert(kB3HPL * 16 % 256 == 0, "the plane stride must keep a lane group's two runs on distinct 16-byte slots");
static_assert(kB3M0 + 16 * kB3GM + kB3S + 1 <= kB3HPL && kB3M0 - kB3S - 1 >= 0, "a tap leaves the plane");

// layer3's geometry of mmp_blkh_kernel (nmpc_mmp_block_f16.h): the sibling's waves -- wave = 2 pw + hw takes the pixel groups of
// parity pw (7 of m, its first 6 of out, in the sibling's order) and the A groups 2 hw, 2 hw + 1
struct MmpBlock3HGeom : MmpBlock3Waves {
    using Params = MmpBlock3HParams;
    static constexpr int C = kB3C, Threads = kB3Threads, S = kB3S, Q = kB3Q, TH = kB3TH, TW = kB3TW;
    static constexpr int PL = kB3HPL, SH = 0;
    static constexpr int NI = kB3NI, NO = kB3NO, NH = kB3NH;
    static constexpr int Unroll = 3;
    static constexpr bool Fitted = false, RegTight = false;
    static constexpr int ck(int stride) { return stride == 2 ? 32 : 64; }
    static constexpr int min_wg(int stride) { return stride == 2 ? 2 : 4; }
};

} // namespace nmpc
