// nmpc_mmp_block2_f16.h -- layer2's geometry of the one residual-block kernel on binary16 MFMA operands, mmp_blkh_kernel of
// nmpc_mmp_block_f16.h: the block of nmpc_mmp_block2.h (resnet34.layer2 of the multi-hypothesis predictor's network: 32 output
// channels, stride 1 or 2 on the first convolution and the projection, projection or identity; predictor `mmp`, opt-in on top of
// the opt-in fused layer2: MmpFrontEnd(operands={"layer2": "f16"})). The rounding rule, the MFMA fragments, the octet-plane LDS
// layout with its bank argument, the packed-weight order, the four steps and the fixed summation order are stated there; here is
// what is layer2's own. The 32 channels of m and of a 32 -> 32 block's x are exactly ONE K block per tap and two A groups.
//
// Kept from the sibling (proven there, with wrong-variant controls), whose constants this header includes: the flat domain of
// 12 x 48 = 576 positions of the OUTPUT plane around a tile of 8 x 44 outputs; the 30 pixel groups of m (rows 1 .. 10) and 24 of
// out (rows 2 .. 9) in the order of mmp_b2_group, group j on wave j & 3, so that a wave's first 6 groups of m are its groups of
// out; the flat-offset taps; the parity split of the strided input into four sub-planes on the same domain (tap ky reads row
// parity ky != 1 at offset -48 for ky = 0, likewise kx); m exactly zero outside the plane; m written over the dead input; the
// projection in the epilogue on x read again; 256 threads = 4 waves; one workgroup per [row][tile row][tile column].
//
// Decision 1 -- wave mapping: the sibling's. Every wave holds BOTH A groups (h = 0, 1) of a tap and takes the pixel groups
// j & 3 == wave: 8 groups of m (two waves 7 and a recomputed copy, discarded), 6 of out, and ONE ds_read_b128 feeds TWO MFMAs.
// Layer3's alternative (wave = pixel parity x channel half) would here leave one A group per wave: one LDS read per MFMA, 15
// groups of m per wave, the same 64 accumulators -- twice the LDS traffic for nothing. Accumulators: 8 x 2 x 4 = 64 per lane.
// Decision 2 -- LDS layout: the shared octet planes, of kB2P = 592 slots = 9 472 B = 37 x 256 B (the sibling's stride, now counted
// in 16-byte slots), with position q at slot q + 1 for x and for m alike, so the position -1 that the first group of m reaches
// (48 - 49) and the position 576 that the last one reaches (527 + 49) are slots 0 and 577 of the same plane: inside it, never
// written, and read for wrapped columns only. The shift by one slot keeps the bank argument: it holds for every first slot.
// Decision 3 -- LDS size and occupancy. m is 4 planes = 37 888 B. A 32 -> 32 block (three of the four) stages its 4 planes of x
// at once and writes m over them: ONE chunk, three barriers in all (staged, conv1 read, m written), 37 888 B static, FOUR
// workgroups per CU by LDS (151 552 of 163 840 B) and, at __launch_bounds__(256, 4), at most 128 registers per lane; whether the 64
// accumulators, the staged octets and the A fragments fit those without scratch is for the compiler to show (below).
// Decision 4 -- the strided first block (Cin = 16, half a K block). Counted per wave and tile:
//   (a) zeros: stage the chunk's 2 octets x 4 sub-planes = 8 planes = 75 776 B (two workgroups per CU, as the sibling), the lanes
//       l >> 4 in {2, 3} feed B = 0 against the packed zeros of A: 9 x 8 x 2 = 144 MFMAs of conv1, 264 for the block with its
//       12 of the projection and 108 of conv2;
//   (b) tap pairing: lanes l >> 4 in {0, 1} read tap 2 p, lanes {2, 3} tap 2 p + 1 (the B address is per lane): 5 x 8 x 2 = 80
//       MFMAs of conv1, 200 for the block; w1p becomes [5][..] for strided blocks only, with a tenth, zero tap, and the packing,
//       its inverse and the model would depend on the stride.
// (b) saves 64 of the 1 020 MFMAs of a tile of all four blocks = 0.17 ms of a 2.7 ms floor that the kernel is not expected to come
// near (below). Taken: (a). One packing for both strides. A strided chunk is 16 channels: the half
// (c0 >> 4) & 1 of K block c0 >> 5, the lanes of the other half feed zeros; a longer strided Cin (32, 64: tests only) issues
// conv1's MFMAs twice per K block.
// Decision 5 -- Cin = 64 at stride 1 (tests only, with projection): chunks of 32 channels, one behind the other behind a barrier;
// no register prefetch of the next chunk, as in layer3's f16 kernel: the network's blocks are one chunk.
// Decision 6 -- MFMA-to-load ratio: per wave one ds_read_b128 (1 KB) feeds two MFMAs = 32 cycles; the CU's four waves read
// (72 + 54) x 4 KB = 504 KB per 32 -> 32 tile = 2 016 clocks of the LDS array at 256 B / clock against 252 x 16 = 4 032 of MFMA.
// The weights: two 16-byte loads per lane per tap = per 16 or 12 MFMAs (36 864 B of w1 / w2 in all: L1 / L2 hits).
//
// Step counts per wave: 1. 9 taps x 8 pixel groups x 2 A groups of MFMA per chunk; 3. 9 taps x 6 groups x 2 A groups on m.
//
// Modelled before the device run, instruction counts only. Per wave and tile: a 32 -> 32 block 9 x 8 x 2 + 9 x 6 x 2 = 144 + 108 =
// 252 MFMA, the strided block 144 + 12 + 108 = 264: 1 020 for a tile of all four, of 16 cycles each = 16 320 cycles (the f32
// kernel: 7 536 x 32 = 241 152). At B = 256, 4 pedestrians, N_hor = 20 (20 480 rows x 5 tiles over 256 CUs at 2.4 GHz): 102 400 x
// 16 320 / (256 x 2.4e9) = 2.7 ms per lock-step if the MFMA pipe never waits (f32: 40 ms); 5.8 ms for the 36.6 GB at the 6.29 TB/s
// copy rate, unchanged. Neither floor is expected: per 32 -> 32 tile a thread issues 72 loads of x a plane apart, waits, converts,
// and at the end stores 48 dwords (runs of 16 floats), none of it under MFMAs of its own workgroup; only the other three
// workgroups of the CU fill that. Layer3's f16 kernel, built the same way, reached 17 % of the copy rate; at that rate layer2
// would take 35 ms. Expected: bound by the staging loads and the final stores, not by the pipe; several times 5.8 ms, under the
// f32 kernel's 71.5 ms.
// Measured (profiles/mmp_layer2_f16_evaluate.json; both kernels in one process, layer3 and layer4 on binary16
// in both arms, three runs each): the four launches on 440 rows 0.513 ms (0.511-0.513) against the f32 kernel's 1.536 (1.534-1.537):
// 0.334 x (the target was 0.56 x); 23.9 ms per lock-step against 71.5, 92.8 T useful fma/s, 1.53 TB/s = 24 % of the copy rate; the
// strided block 0.198 ms (f32: 0.432), each 32 -> 32 block 0.105-0.106 (0.374-0.393). 8.8 x the MFMA floor, 4.1 x the traffic floor:
// what waits is, from the code and not from counters (no counter run was made), the staging loads in front of the first barrier
// and the stores behind the last MFMA, as expected. The strided block runs at half the others' rate: 144 loads per thread (18
// octets, two floats apart along x), two workgroups per CU to cover them where the others have four, and its projection's 8
// loads per pixel group in the epilogue. Not built: tap pairing (decision 4), a register prefetch of the next tile. Built since:
// binary16 activations in memory (nmpc_mmp_block_f16.h, MmpBlkhIo): the 32 -> 32 blocks 0.105-0.107 -> 0.069-0.070 ms, the strided
// block, whose x stays layer1's float32 output, 0.193 -> 0.175 ms (profiles/mmp_f16_activations_evaluate.json).
//
// Compiler (hipcc -O3 --offload-arch=gfx950; tools/kernel_resources.py on the shipped code object): mmp_blkh_kernel<MmpBlock2HGeom, 2, true>
// 126 VGPRs, 80 SGPRs, 75 776 B LDS; <1, true> 126 VGPRs, 80 SGPRs, 37 888 B; <1, false> 122 VGPRs, 70 SGPRs, 37 888 B; 0 AGPRs, no
// spills, scratch 0, code 21-32 KB: four workgroups per CU compile clean. tests/test_mmp_block2_f16_cpu.py holds the three
// kernels to: scratch 0, no spills, the LDS of 4 (8 at stride 2) planes, 160 KB / LDS = the 4 (2) workgroups per CU that
// __launch_bounds__ claims, and registers that allow as many waves per SIMD.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmpc_mmp_block2.h"
#include "nmpc_mmp_block_f16.h"

namespace nmpc {

struct MmpBlock2HParams {
    int M, Cin, H, W, H2, W2, tx, ty;                // as MmpBlock2Params
    const float *x;                                  // [M][Cin][H][W]
    const uint16_t *w1;                              // packed [9][ceil(Cin / 32)][2][64][8] binary16
    const float *s1, *b1;                            // [32], [32]
    const uint16_t *w2;                              // packed [9][1][2][64][8]
    const float *s2, *b2;                            // [32], [32]
    const uint16_t *wd;                              // packed [ceil(Cin / 32)][2][64][8] (kernel <., true>) or unused
    const float *sd, *bd;                            // [32], [32] or unused
    float slope_mid, slope_out;
    float* out;                                      // [M][32][H2][W2]
};

constexpr int kB2HMP = kB2C / 8;                     // planes of m: 4 octets of channels
constexpr int kB2HPB = kB2P * 16;                    // bytes of a plane in LDS: 9 472
static_assert(kB2C == 32, "m is one K block");
static_assert(kB2HPB % 256 == 0, "the plane stride must keep a lane group's two runs on distinct 16-byte slots");
// m's groups cover the positions kB2S (row 1) .. (kB2R - 1) kB2S - 1 (row 10); a tap reaches kB2S + 1 further, a slot is position + 1
static_assert(kB2S - (kB2S + 1) + 1 >= 0 && (kB2R - 1) * kB2S - 1 + (kB2S + 1) + 1 < kB2P, "a tap leaves the plane");
static_assert(kB2HMP * kB2HPB * 4 <= 160 * 1024, "four workgroups do not fit a CU's LDS");

// layer2's geometry of mmp_blkh_kernel (nmpc_mmp_block_f16.h): the sibling's waves -- every wave holds both A groups and takes the
// pixel groups j & 3 == wave in the sibling's order (decision 1) --; position q sits at slot q + 1 (decision 2)
struct MmpBlock2HGeom : MmpBlock2Waves {
    using Params = MmpBlock2HParams;
    static constexpr int C = kB2C, Threads = kB2Threads, S = kB2S, Q = kB2Q, TH = kB2TH, TW = kB2TW;
    static constexpr int PL = kB2P, SH = 1;
    static constexpr int NI = kB2NI, NO = kB2NO, NH = kB2NH;
    static constexpr int Unroll = 3;
    static constexpr bool Fitted = false, RegTight = false;
    static constexpr int ck(int stride) { return stride == 2 ? 16 : 32; } // (decision 4: half a K block, with zeros)
    static constexpr int min_wg(int stride) { return stride == 2 ? 2 : 4; }
};

} // namespace nmpc
