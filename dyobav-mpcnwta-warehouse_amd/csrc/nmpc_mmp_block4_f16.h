// nmpc_mmp_block4_f16.h -- the residual block of nmpc_mmp_block4.h (resnet34.layer4 of the multi-hypothesis predictor's network:
// 128 output channels, stride 1 or 2, projection or identity) with binary16 MFMA OPERANDS and float32 everything else (predictor
// `mmp`, opt-in on top of the opt-in fused layer4: MmpFrontEnd(half=("layer4",))). The block, its strides, its padding and the
// zero ring of m are defined there; x [M][Cin][H][W] and out [M][128][H2][W2] stay float32 in memory. The sibling of
// nmpc_mmp_block3_f16.h (64 channels), whose rule, fragments and LDS layout it keeps.
//
// The rounding rule -- whatever an MFMA reads is f16, nothing else is:
//   - the weights w1, w2, wd are rounded ONCE on the host (mmp_stem.pack_block4_f16) and arrive packed in fragment order (below);
//   - x is rounded when it is staged into LDS (the first convolution's operand; the projection reads it again from memory and
//     rounds it the same way);
//   - m = leaky(fma(s1, acc, b1), slope_mid) is rounded when it is written to LDS;
//   - rounding is to nearest even; a value beyond +-65504 saturates to +-65504 (mmp_b3h_round clips, then converts: the
//     infinities saturate with the finite values), NaN stays NaN, subnormals are kept (the kernel runs with f16 denormals on, and
//     the gfx950 MFMA does not flush them: tests/test_gpu_mmp_block4_f16.py pins that on the device);
//   - float32, as in the sibling: the accumulation (the MFMA's), the two affines and both LeakyReLUs, the addition z + id, x as
//     the identity when there is no projection (read again UNROUNDED), x and out in memory.
// tests/mmp_block4_f16_reference.py states the same rule in float64 with a derived bound.
//
// Instruction: v_mfma_f32_16x16x32_f16, K = 32 per instruction against the f32 kernel's 4 at half its cycles (16 against 32):
//   A: lane l holds w[co = 16 g + (l & 15)][ci = 32 kb + 8 (l >> 4) + j], j = 0 .. 7, of one tap         (4 VGPRs, one 16-byte load)
//   B: lane l holds tile[ci = 32 kb + 8 (l >> 4) + j][q + off(tap)], q = q0 + (l & 15)                   (4 VGPRs, one ds_read_b128)
//   D: 4 VGPRs: channel 16 g + 4 (l >> 4) + r in register r, pixel q0 + (l & 15)                         (as the f32 form)
// 128 output channels are eight A groups g; 128 input channels are four K blocks per tap, the strided block's 64 two; a Cin that
// is no multiple of 32 has zeros in the last K block (staged zeros in B, packed zeros in A).
//
// Ported unchanged from nmpc_mmp_block4.h (proven there, with wrong-variant controls): the flat domain of 12 x 13 = 156
// positions of the OUTPUT plane, m and out on the SAME eight pixel groups from position 14 when the plane fits 10 x 11 and tiles
// of 8 x 9 with a halo of one along a longer side (oy, ox = 1 or 2), the flat-offset taps, the parity split of the strided input
// into four sub-planes on the same domain (tap ky reads row parity ky != 1 at offset -13 for ky = 0), m zero outside the plane
// and zeros on the 28 positions of the ring that no group covers, m written over the dead input, the projection in the epilogue.
//
// LDS layout, the sibling's: channels innermost, in OCTETS: [plane = sub-plane x octet][position q][8 halves], 16 bytes per
// position, planes of kB4HPL = 160 positions = 2 560 B = 10 x 256 B (the domain's 156 padded by 4). A B fragment is one aligned
// ds_read_b128; because the plane stride is a multiple of 256 B the sixteen 16-byte slots of a lane group (positions q0 + {0 ..
// 3, 12 .. 15} of one plane and q0 + {4 .. 11} of the plane behind it; nmpc_mmp_block3_f16.h counts the banks) are q0 + 0 .. 15
// mod 16: conflict-free for every q0 and every tap offset. The m store is one ds_write_b64 per pixel group and A group (the 4
// consecutive channels of a D fragment are half an octet). m is 16 planes = 40 960 B.
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
// The packed weights (uint16 = binary16 bits, 16-byte aligned, mmp_stem.pack_block4_f16; include/nmpc_hip.h):
//   w1p[tap t = 3 ky + kx][K block kb < ceil(Cin / 32)][group g < 8][lane l < 64][j < 8] = f16(w1[16 g + (l & 15)][32 kb + 8 (l >> 4) + j][ky][kx])
//   w2p the same with Cin = 128;  wdp[kb][g][l][j] = f16(wd[16 g + (l & 15)][32 kb + 8 (l >> 4) + j]);   0 where the channel is >= Cin.
//
// Steps: workgroup = [row of the batch][tile row][tile column] flattened in x. 1. per chunk: x global -> f16 -> LDS (8 channels
// of a position per 16-byte store, zero outside the plane and for channels >= Cin), barrier, per K block 9 taps x 4 pixel
// groups x 4 A groups of MFMA; 2. barrier; m -> LDS, zeros to the ring; barrier; 3. 4 K blocks x 9 taps x 4 x 4 on m; 4. per
// pixel group of out: the projection (x read again and rounded, one MFMA per K block and A group), the affines, the identity,
// the activation, one dword store per value. No atomics, no scratch. Every word of LDS that is read has been written: a plane
// of x on 0 .. 155 by the staging, a plane of m on 14 .. 141 by the groups and on the rest of 0 .. 155 by the zeros; the
// positions 156 .. 159 are never read (a tap reaches 141 + 14).
//
// Summation order (fixed): per convolution K blocks ascending, per K block the taps ky-major, per tap the instruction's own
// order over its 32 channels; then one fma per affine and one addition. A row's bits depend on that row of x and the weights
// only: not on M, the row's position, the launch or the alignment of out.
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
// Compiler (hipcc -O3 --offload-arch=gfx950; tools/kernel_resources.py on the shipped code object): mmp_blk4h_kernel<2, true>
// 162 VGPRs, 82 SGPRs; <1, true> 142 VGPRs, 82 SGPRs; <1, false> 146 VGPRs, 70 SGPRs; all 40 960 B LDS, no spills, scratch 0,
// code 19-25 KB. tests/test_mmp_block4_f16_cpu.py holds the three kernels to: scratch 0, no spills, 40 960 B and at most 168
// registers (3 waves per SIMD, three workgroups per CU).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmpc_mmp_block3_f16.h"
#include "nmpc_mmp_block4.h"

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

template <int STRIDE, bool PROJ>
__global__ __launch_bounds__(kB4HThreads, 3) void mmp_blk4h_kernel(MmpBlock4HParams p)
{
    static_assert(STRIDE == 1 || STRIDE == 2, "stride");
    constexpr int CK = STRIDE == 2 ? 32 : 128;         // input channels per chunk
    constexpr int NO = CK / 8;                         // octets of channels per chunk
    constexpr int NPL = NO * STRIDE * STRIDE;          // planes per chunk: [sub-plane][octet]
    constexpr int NI = NPL * kB4Q;                     // 16-byte items per chunk
    constexpr int PRE = (NI + kB4HThreads - 1) / kB4HThreads; // items a thread stages per chunk: 10
    static_assert(NPL == kB4HMP, "m goes exactly over the chunk");
    __shared__ __attribute__((aligned(16))) _Float16 lds[NPL * kB4HPL * 8]; // [plane][position][8]; m over the last chunk

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pw = wave >> 1, hb = kB4HNH * (wave & 1); // the wave's parity of pixel groups; its first A group
    const int lane = tid & 63, col = tid & 15, k4 = (tid >> 4) & 3;
    const int tiles = p.tx * p.ty;
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    if (n >= p.M) return; // (workgroup-uniform, in front of every barrier)
    const int tyi = tile / p.tx, txi = tile - tyi * p.tx;
    const int gy0 = tyi * kB4TH - p.oy, gx0 = txi * kB4TW - p.ox; // the output pixel of position 0 (one tile: -1)
    const size_t plane = (size_t)p.H * p.W, plane2 = (size_t)p.H2 * p.W2;
    const float* xn = p.x + (size_t)n * p.Cin * plane;
    const int KB1 = (p.Cin + 31) >> 5;               // K blocks of the first convolution and the projection

    const mmp_b4_f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    mmp_b4_f4 acc[kB4NI][kB4HNH];
    int gq[kB4NI]; // the wave's pixel groups: first position + col
#pragma unroll
    for (int i = 0; i < kB4NI; ++i) {
        gq[i] = kB4M0 + 16 * (pw + 2 * i) + col;
#pragma unroll
        for (int h = 0; h < kB4HNH; ++h) acc[i][h] = zero;
    }

    // ---- 1. the first convolution, the input staged in chunks of CK channels, rounded on the way
    for (int c0 = 0; c0 < p.Cin; c0 += CK) {
        if (c0) __syncthreads(); // the previous chunk has been read
#pragma unroll 1
        for (int e = 0; e < PRE; ++e) {
            const int i = tid + e * kB4HThreads;
            if (i < NI) {
                const int pl = i / kB4Q, q = i - pl * kB4Q;
                const int sub = pl / NO, o = pl - sub * NO;
                const int y = STRIDE * (gy0 + q / kB4S) + sub / 2, xx = STRIDE * (gx0 + q % kB4S) + sub % 2;
                const int ch = c0 + 8 * o;               // (Cin is a multiple of 8: an octet is inside or outside)
                const bool in = ch < p.Cin && y >= 0 && y < p.H && xx >= 0 && xx < p.W;
                const size_t at = in ? (size_t)ch * plane + (size_t)y * p.W + xx : (size_t)0;
                mmp_b3h_h8 v;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = mmp_b3h_round(in ? xn[at + (size_t)j * plane] : 0.0f);
                *reinterpret_cast<mmp_b3h_h8*>(lds + 8 * (pl * kB4HPL + q)) = v;
            }
        }
        __syncthreads();
        for (int kb = 0; kb < CK / 32; ++kb) {
            if (c0 + 32 * kb >= p.Cin) break; // (uniform)
            const uint16_t* wk = p.w1 + ((size_t)((c0 >> 5) + kb) * 8 + hb) * 512 + lane * 8;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ky = t / 3, kx = t % 3;
                const int sub = STRIDE == 2 ? 2 * (ky != 1) + (kx != 1) : 0;
                const int off = STRIDE == 2 ? (ky == 0 ? -kB4S : 0) + (kx == 0 ? -1 : 0) : (ky - 1) * kB4S + (kx - 1);
                mmp_b3h_h8 a[kB4HNH];
#pragma unroll
                for (int h = 0; h < kB4HNH; ++h) a[h] = *reinterpret_cast<const mmp_b3h_h8*>(wk + ((size_t)t * KB1 * 8 + h) * 512);
                const _Float16* xb = lds + 8 * ((sub * NO + 4 * kb + k4) * kB4HPL + off);
#pragma unroll
                for (int i = 0; i < kB4NI; ++i) {
                    const mmp_b3h_h8 b = *reinterpret_cast<const mmp_b3h_h8*>(xb + 8 * gq[i]);
#pragma unroll
                    for (int h = 0; h < kB4HNH; ++h) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[h], b, acc[i][h], 0, 0, 0);
                }
            }
        }
    }

    // ---- 2. m -> LDS over the last chunk, rounded, zero outside the plane; zeros to what no group covers
    __syncthreads(); // the last chunk has been read
    unsigned inm = 0; // bit i: the wave's pixel group i has a pixel of the plane in this lane
#pragma unroll
    for (int i = 0; i < kB4NI; ++i) {
        const int y = gy0 + gq[i] / kB4S, xx = gx0 + gq[i] % kB4S;
        inm |= (unsigned)(y >= 0 && y < p.H2 && xx >= 0 && xx < p.W2) << i;
    }
#pragma unroll
    for (int h = 0; h < kB4HNH; ++h) {
        __builtin_amdgcn_sched_barrier(0); // (one A group's affine at a time: the registers hold no more beside the accumulators)
        float s[4], sh[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] = p.s1[16 * (hb + h) + 4 * k4 + r], sh[r] = p.b1[16 * (hb + h) + 4 * k4 + r];
        // channels 16 (hb + h) + 4 k4 + r, r = 0 .. 3: half of octet 2 (hb + h) + (k4 >> 1)
        _Float16* mo = lds + 8 * ((2 * (hb + h) + (k4 >> 1)) * kB4HPL) + 4 * (k4 & 1);
#pragma unroll
        for (int i = 0; i < kB4NI; ++i) {
            const int q = gq[i];
            const bool in = (inm >> i) & 1;
            mmp_b3h_h4 mv;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = fmaf(s[r], acc[i][h][r], sh[r]);
                mv[r] = mmp_b3h_round(in ? (v > 0.0f ? v : v * p.slope_mid) : 0.0f);
            }
            *reinterpret_cast<mmp_b3h_h4*>(mo + 8 * q) = mv;
        }
    }
    for (int i = tid; i < kB4HMP * kB4Ring; i += kB4HThreads) {
        const int pl = i / kB4Ring, j = i - pl * kB4Ring;
        const mmp_b3h_h8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
        *reinterpret_cast<mmp_b3h_h8*>(lds + 8 * (pl * kB4HPL + (j < kB4M0 ? j : kB4M1 - kB4M0 + j))) = z8;
    }
    __syncthreads();

    // ---- 3. the second convolution on the m tile (the groups of out are the groups of m)
#pragma unroll
    for (int i = 0; i < kB4NI; ++i)
#pragma unroll
        for (int h = 0; h < kB4HNH; ++h) acc[i][h] = zero;
    for (int kb = 0; kb < kB4C / 32; ++kb) {
        const uint16_t* wk = p.w2 + ((size_t)kb * 8 + hb) * 512 + lane * 8;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int off = (t / 3 - 1) * kB4S + (t % 3 - 1);
            mmp_b3h_h8 a[kB4HNH];
#pragma unroll
            for (int h = 0; h < kB4HNH; ++h) a[h] = *reinterpret_cast<const mmp_b3h_h8*>(wk + ((size_t)t * (kB4C / 32) * 8 + h) * 512);
            const _Float16* mb = lds + 8 * ((4 * kb + k4) * kB4HPL + off);
#pragma unroll
            for (int i = 0; i < kB4NI; ++i) {
                const mmp_b3h_h8 b = *reinterpret_cast<const mmp_b3h_h8*>(mb + 8 * gq[i]);
#pragma unroll
                for (int h = 0; h < kB4HNH; ++h) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[h], b, acc[i][h], 0, 0, 0);
            }
        }
    }

    // ---- 4. the projection, the affine, the identity, the activation and the store
    float* on = p.out + (size_t)n * kB4C * plane2;
#pragma unroll
    for (int i = 0; i < kB4NI; ++i) {
        __builtin_amdgcn_sched_barrier(0); // (the loads of one pixel group at a time: all four at once do not fit the registers)
        int q = gq[i];
        asm volatile("" : "+v"(q)); // (the pixel is worked out again here, not kept in registers across the second convolution)
        const int r0 = q / kB4S, c = q - r0 * kB4S;
        const int y = gy0 + r0, xx = gx0 + c;
        const bool valid = r0 >= p.oy && r0 < kB4R - p.oy && c >= p.ox && c < kB4S - p.ox && y < p.H2 && xx < p.W2; // (then y, xx >= 0)
        mmp_b4_f4 idacc[kB4HNH] = {zero, zero, zero, zero};
        if (PROJ) { // (every lane takes part in the MFMAs; a lane without a pixel, or with channels >= Cin, feeds zeros)
            const float* xc = xn + (valid ? (size_t)(STRIDE * y) * p.W + STRIDE * xx : (size_t)0);
            for (int kb = 0; kb < KB1; ++kb) {
                const int ch = 32 * kb + 8 * k4;
                const bool ld = valid && ch < p.Cin;
                mmp_b3h_h8 b;
#pragma unroll
                for (int j = 0; j < 8; ++j) b[j] = mmp_b3h_round(ld ? xc[(size_t)(ch + j) * plane] : 0.0f);
#pragma unroll
                for (int h = 0; h < kB4HNH; ++h)
                    idacc[h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                        *reinterpret_cast<const mmp_b3h_h8*>(p.wd + ((size_t)kb * 8 + hb + h) * 512 + lane * 8), b, idacc[h], 0, 0, 0);
            }
        }
        if (!valid) continue;
        const size_t pix = (size_t)y * p.W2 + xx;
#pragma unroll
        for (int h = 0; h < kB4HNH; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = 16 * (hb + h) + 4 * k4 + r;
                const size_t o = (size_t)co * plane2 + pix;
                const float z = fmaf(p.s2[co], acc[i][h][r], p.b2[co]);
                const float id = PROJ ? fmaf(p.sd[co], idacc[h][r], p.bd[co]) : xn[o]; // (no projection: plane2 == plane)
                const float v = z + id;
                on[o] = v > 0.0f ? v : v * p.slope_out;
            }
    }
}

} // namespace nmpc
