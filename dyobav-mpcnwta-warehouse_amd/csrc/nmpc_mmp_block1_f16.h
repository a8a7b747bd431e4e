// nmpc_mmp_block1_f16.h -- layer1's geometry of the one residual-block kernel on binary16 MFMA operands, mmp_blkh_kernel of
// nmpc_mmp_block_f16.h: the block of nmpc_mmp_block.h (resnet34.layer1 of the multi-hypothesis predictor's network: 16 output
// channels, stride 1 only, projection or identity; the network's blocks are 64 -> 16 with projection, then two 16 -> 16; predictor
// `mmp`, opt-in for the whole network: MmpFrontEnd(precision="f16")). The rounding rule, the MFMA fragments, the octet-plane LDS
// layout with its bank argument, the packed-weight order, the four steps and the fixed summation order are stated there and hold
// here word for word; here is what is layer1's own.
//
// Which of the two forms this is: a GEOMETRY of the shared kernel, not a kernel of its own. What layer1 needed from the shared
// body and did not find there is derived from the numbers, three lines:
//   - C = 16 is ONE A group (NA = 1) and m is 2 octet planes, half a K block: the second convolution has KB2 = ceil(C / 32) = 1 K
//     block per tap (the body divided, C / 32 = 0), and where C % 32 != 0 its lane groups l >> 4 in {2, 3} feed zeros against the
//     packed zeros of w2 (they would otherwise read planes 2 and 3, which a 16 -> 16 block does not have);
//   - the 30 pixel groups of out do not fill the four waves' 4 x 8 slots, so the epilogue's "a group of out has no row outside
//     the tile" holds only where TH x S / 16 equals the slots; otherwise the row test that layer3 and layer4 use applies;
//   - Cin = 16 is a half-chunk as layer2's strided block already is; Cin = 8 (tests only) a quarter, its second octet staged as
//     zeros by the test ch < Cin that every chunk already makes.
// For C = 32, 64, 128 each of the three is the constant it was: the 36 kernels the code object had keep their bytes under their
// names (profiles/mmp_layer1_f16_code_object_identity.txt, tools/code_object_hash.py on both builds).
//
// Kept from the float32 sibling nmpc_mmp_block.h, whose constants this header includes: the flat domain of 19 x 32 = 608 positions
// around a tile of 15 x 28 outputs, S = 32 so that a pixel group is half a row; the 34 pixel groups of m (rows 1 .. 17) and 30 of
// out (rows 2 .. 16), group j on wave j & 3: 9 and 8 slots per wave; m exactly zero outside the plane; the wrapped columns (0, 1,
// 30, 31 of out, 0 and 31 of m) computed and never stored; 256 threads, one workgroup per [row][tile row][tile column]. The
// shared body takes a wave's groups of out to be its first NO groups of m, so the groups are ordered as mmp_b2_group orders
// layer2's: the 30 of out first, then row 1, then row 17 (mmp_b1h_group). Waves 2 and 3 then hold a group of row 1 in their
// eighth slot (computed through the second convolution on a row of m that nobody wrote, dropped by the row test) and a
// recomputed copy of the last group in their ninth (not stored).
//
// LDS: the octet planes of the shared layout, PL = 624 slots = 9 984 B = 39 x 256 B (the sibling's stride, in 16-byte slots), with
// position q at slot q + 1: the positions -1 (32 - 33) and 608 (575 + 33) that the first and last group of m reach are slots 0
// and 609 of the same plane -- inside it, never written, read for wrapped columns only.
//
// Decision 1 -- K packing of the 16-channel convolutions (five of the stage's six). Counted per wave and tile:
//   (a) zeros in half of each K block: 9 MFMAs per pixel group and tap set. First block (64 -> 16, chunks of 32) 2 x 9 x 9 conv1
//       + 2 x 8 projection + 9 x 8 conv2 = 250, each 16 -> 16 block 81 + 72 = 153: 556 MFMAs of 16 cycles = 8 896 cycles (the
//       float32 kernel: 2 936 x 32 = 93 952). 307 200 tiles over 256 CUs at 2.4 GHz: 4.4 ms per lock-step if the pipe never waits.
//   (b) tap pairing (lane groups {0, 1} read tap 2 p, {2, 3} tap 2 p + 1): 5 MFMAs, a tenth zero tap, a packing of its own:
//       162 + 16 + 40 = 218 and 2 x (45 + 40) = 170: 388 MFMAs = 3.1 ms.
//   The three f16 siblings run 4-9 x over their MFMA floors, bound by staging loads and final stores; 1.3 ms of a floor that is
//   not expected to be reached does not pay for a second packing. Taken: (a), mmp_stem._pack_f16 as it is with C // 16 = 1. (b) is
//   counted and not built.
// Decision 2 -- chunk and occupancy. A 16 -> 16 block stages its 2 planes (19 968 B) in one chunk, a half K block. The 64 -> 16
//   block could take chunks of 16 (four half-filled passes: 324 MFMAs of conv1 instead of 162, four barrier pairs), of 32 (4
//   planes = 39 936 B: FOUR workgroups per CU, 159 744 of 163 840 B) or of 64 (8 planes = 79 872 B: two). Taken: 32 with a
//   projection, 16 without -- the two cases differ by PROJ, not by stride, so the chunk travels in the geometry's template
//   argument (MmpBlock1HGeom<PROJ>; the launch pairs it with the kernel's PROJ) and ck(stride) stays the body's one question.
//   Four workgroups per CU at __launch_bounds__(256, 4) need <= 128 registers; the accumulators are 9 x 4 = 36 (compiler below).
// Decision 3 -- instantiations: <MmpBlock1HGeom<true>, 1, true> and <MmpBlock1HGeom<false>, 1, false>, each in the four memory
//   forms of MmpBlkhIo: 8 kernels, no stride 2.
//
// Modelled before the device run, from the code only. Global memory instructions per thread and tile (float32 form -> octet form):
//   64 -> 16   staging 2 chunks x 9.5 items x 8 = 152 dwords -> 19 of 16 B; projection 8 groups x 2 K blocks x 8 = 128 -> 16 of
//              16 B; stores 8 groups x 4 = 32 dwords -> 8 of 8 B
//   16 -> 16   staging 4.75 x 8 = 38 dwords -> 4.75 of 16 B; identity 32 dwords -> 8 of 8 B; stores 32 -> 8 of 8 B
// In the network the first block reads the fill's float32 output (280 dword loads per thread and tile, the projection's in the
// epilogue behind the last MFMA) and is expected to take several times as long as each of the other two, which move 4 + 1 + 1
// bytes per output value less than the float32 kernel's 12. Traffic: 64 ch x 4 B x 1.45 (halo) + 64 x 4 (projection) in, 16 x 2
// out for the first block, 16 x 2 x 1.45 + 16 x 2 in and 16 x 2 out (16 x 4 for the last) for the others, per output pixel: about
// 0.85 kB against the float32 stage's 1.1 kB + re-read halos -- the copy-rate floor stays near 8-10 ms per lock-step. Expected
// wait: the staging loads in front of the first barrier and, in the first block, the projection's loads in the epilogue, covered
// only by the other three workgroups of the CU; not the MFMA pipe. Expected: the stage well under half the float32 kernel's 86
// ms, several times the 4.4 ms floor; the first block more than half of it.
// Measured (profiles/mmp_layer1_f16_evaluate.json; tools/mmp_evaluate_profile.py --half-layer1: B = 256, 4
// pedestrians, N_hor = 20, fp32; both arms in one process, three alternated runs each; the parent arm is layer2 .. layer4 on
// binary16 operands with binary16 activations and layer1 on the float32 kernel): layer1's three launches on 440 rows 0.766 /
// 0.772 / 0.771 ms against 1.955 / 1.878 / 1.903: 0.39 / 0.41 / 0.41 x (spreads 0.8 % and 4.0 %: faster by far more than the
// larger one in every run); in the loop 35.5 ms per lock-step against 87.0, the stage 130.2 ms against 182.4 = 0.714 x (single
// runs 130.2 / 130.2 / 130.2 against 182.2 / 182.5 / 182.4). Both merge conditions hold in each run. Per block: 64 -> 16 0.504 ms
// (float32 kernel 0.967), each 16 -> 16 0.133-0.134 (0.464-0.465); layer2's strided block, which now reads the octet form,
// 0.119 against 0.167 -- it gained as the earlier record expected (0.71 x, where binary16 stores alone had given 0.91 x).
// Against the model: 76 T useful fma/s over the three launches (the float32 kernel 31), the first block 67 T and 1.54 TB/s = 25 %
// of the copy rate, the 16 -> 16 blocks 93 T and 1.29-1.31 TB/s = 21 %; 35.9 ms per lock-step is 8.2 x the MFMA floor of 4.4 ms and
// 3.6 x the traffic floor: where the model said, under half the float32 kernel, the first block 65 % of the three, the pipe not
// what waits. Where it was wrong: nothing it stated -- but it gave no figure for the 16 -> 16 blocks, which with half the MFMAs
// per byte of layer2's 32 -> 32 blocks run at the same 1.3 TB/s: staging loads in front of the first barrier and stores behind
// the last MFMA, read from the code, not from counters (no counter run was made).
//
// Compiler (hipcc -O3 --offload-arch=gfx950; tools/kernel_resources.py on the shipped code object), VGPRs / SGPRs on float32 memory,
// binary16 out, binary16 x, both: <true> 95 / 96, 95 / 94, 94 / 94, 94 / 93 with 39 936 B of LDS; <false> 98 / 92, 98 / 92, 96 / 78,
// 96 / 77 with 19 968 B; 0 AGPRs, no spills, scratch 0, code 18-30 KB: four workgroups per CU compile clean (bound 128).
// tests/test_mmp_block1_f16_cpu.py holds the eight kernels to scratch 0, no spills, 39 936 B (projection) or 19 968 B (identity)
// of LDS, and registers that allow the four workgroups per CU that __launch_bounds__ claims.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmpc_mmp_block.h"
#include "nmpc_mmp_block_f16.h"

namespace nmpc {

struct MmpBlock1HParams {
    int M, Cin, H, W, H2, W2, tx, ty;                // as MmpBlock2HParams; stride 1: H2 = H, W2 = W
    const float *x;                                  // [M][Cin][H][W]
    const uint16_t *w1;                              // packed [9][ceil(Cin / 32)][1][64][8] binary16
    const float *s1, *b1;                            // [16], [16]
    const uint16_t *w2;                              // packed [9][1][1][64][8], zero for the channels >= 16
    const float *s2, *b2;                            // [16], [16]
    const uint16_t *wd;                              // packed [ceil(Cin / 32)][1][64][8] (kernel <., true>) or unused
    const float *sd, *bd;                            // [16], [16] or unused
    float slope_mid, slope_out;
    float* out;                                      // [M][16][H][W]
};

constexpr int kB1HR = kBlkTH + 4;                    // rows of the flat domain: 19
constexpr int kB1HGR = kBlkS / 16;                   // pixel groups per row: 2
constexpr int kB1HGO = kBlkTH * kB1HGR;              // pixel groups of out: 30
constexpr int kB1HMP = kBlkC / 8;                    // planes of m: 2 octets of channels
constexpr int kB1HPB = kBlkP * 16;                   // bytes of a plane in LDS: 9 984
static_assert(kBlkC == 16, "m is half a K block and one A group");
static_assert(kBlkS % 16 == 0 && kBlkQ == kB1HR * kBlkS, "a pixel group lies in one row of the domain");
static_assert(kBlkGM == kB1HGO + 2 * kB1HGR && kBlkNI * 4 >= kBlkGM && kBlkNO * 4 >= kB1HGO, "the groups do not fit the waves' slots");
static_assert(kB1HPB % 256 == 0, "the plane stride must keep a lane group's two runs on distinct 16-byte slots");
// m's groups cover the positions kBlkS (row 1) .. (kB1HR - 1) kBlkS - 1 (row 17); a tap reaches kBlkS + 1 further, a slot is position + 1
static_assert(kBlkS - (kBlkS + 1) + 1 >= 0 && (kB1HR - 1) * kBlkS - 1 + (kBlkS + 1) + 1 < kBlkP, "a tap leaves the plane");
static_assert(4 * kB1HPB * 4 <= 160 * 1024, "four workgroups with a chunk of 32 channels do not fit a CU's LDS");

// first position of m's pixel group j: rows 2 .. 16 (the groups of out) first, then row 1, then row 17
__device__ __forceinline__ constexpr int mmp_b1h_group(int j)
{
    return j < kB1HGO ? 2 * kBlkS + 16 * j : j < kB1HGO + kB1HGR ? kBlkS + 16 * (j - kB1HGO) : (kB1HR - 2) * kBlkS + 16 * (j - kB1HGO - kB1HGR);
}

// layer1's geometry of mmp_blkh_kernel (nmpc_mmp_block_f16.h): every wave holds the one A group and takes the pixel groups
// j & 3 == wave in the order of mmp_b1h_group; position q sits at slot q + 1; PROJ (the kernel's own) chooses the chunk (decision 2)
template <bool PROJ>
struct MmpBlock1HGeom {
    using Params = MmpBlock1HParams;
    static constexpr int C = kBlkC, Threads = kBlkThreads, S = kBlkS, Q = kBlkQ, TH = kBlkTH, TW = kBlkTW;
    static constexpr int PL = kBlkP, SH = 1;
    static constexpr int NI = kBlkNI, NO = kBlkNO, NH = 1;
    // (of the 10 / 5 items a thread stages; the identity kernels' whole loop, 5, cost 2 to 9 SGPR spills at 106 SGPRs, 4 none at 92)
    static constexpr int Unroll = PROJ ? 5 : 4;
    static constexpr bool Fitted = false, RegTight = false;
    static constexpr int ck(int) { return PROJ ? 32 : 16; } // (a whole K block, or the half that Cin = 16 is)
    static constexpr int min_wg(int) { return 4; }
    static __device__ __forceinline__ int pixel_wave(int wave) { return wave; }
    // waves 2 and 3 have 8 groups of m: their ninth slot computes the last group again and stores nothing
    static __device__ __forceinline__ int group(int wave, int i) { return mmp_b1h_group(wave + 4 * i < kBlkGM ? wave + 4 * i : kBlkGM - 1); }
    static __device__ __forceinline__ int first_a(int) { return 0; }
    static __device__ __forceinline__ bool live(int wave, int i) { return wave + 4 * i < kBlkGM; }
};

} // namespace nmpc
