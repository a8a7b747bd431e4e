// nmpc_mmp_block2_f16.h -- the residual block of nmpc_mmp_block2.h (resnet34.layer2 of the multi-hypothesis predictor's network:
// 32 output channels, stride 1 or 2 on the first convolution and the projection, projection or identity) with binary16 MFMA
// OPERANDS and float32 everything else (predictor `mmp`, opt-in on top of the opt-in fused layer2:
// MmpFrontEnd(operands={"layer2": "f16"})). The block, its strides, its padding and the zero ring of m are defined there;
// x [M][Cin][H][W] and out [M][32][H2][W2] stay float32 in memory.
//
// The rounding rule (layer3's, nmpc_mmp_block3_f16.h, stated again) -- whatever an MFMA reads is f16, nothing else is:
//   - the weights w1, w2, wd are rounded ONCE on the host (mmp_stem.pack_block2_f16) and arrive packed in fragment order (below);
//   - x is rounded when it is staged into LDS (the first convolution's operand); the projection reads it again from memory and
//     rounds it the same way;
//   - m = leaky(fma(s1, acc, b1), slope_mid) is rounded when it is written to LDS;
//   - rounding is to nearest even; a value beyond +-65504 saturates to +-65504 (mmp_b2h_round clips, then converts: the
//     infinities saturate with the finite values), NaN stays NaN, subnormals are kept (f16 denormals are on, and the gfx950 MFMA
//     does not flush them: tests/test_gpu_mmp_block2_f16.py pins that on the device);
//   - float32, as in the sibling: the accumulation (the MFMA's), the two affines and both LeakyReLUs, the addition z + id, x as
//     the identity when there is no projection (read again UNROUNDED), x and out in memory.
// tests/mmp_block2_f16_reference.py states the same rule in float64 with a derived bound.
//
// Instruction: v_mfma_f32_16x16x32_f16, K = 32 per instruction against the sibling's 4 at half its cycles (16 against 32 per SIMD):
//   A: lane l holds w[co = 16 h + (l & 15)][ci = 32 kb + 8 (l >> 4) + j], j = 0 .. 7, of one tap         (4 VGPRs, one 16-byte load)
//   B: lane l holds tile[ci = 32 kb + 8 (l >> 4) + j][q + off(tap)], q = q0 + (l & 15)                   (4 VGPRs, one ds_read_b128)
//   D: 4 VGPRs: channel 16 h + 4 (l >> 4) + r in register r, pixel q0 + (l & 15)                         (as the f32 form)
// The 32 channels of m and of a 32 -> 32 block's x are exactly ONE K block per tap; a Cin that is no multiple of 32 has zeros in
// the last K block (staged zeros in B, packed zeros in A).
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
// Decision 2 -- LDS layout: channels innermost, in OCTETS: [plane = sub-plane x octet][slot = position q + 1][8 halves], 16 bytes
// per slot, planes of kB2P = 592 slots = 9 472 B = 37 x 256 B (the sibling's stride, now counted in 16-byte slots). Position q
// sits at slot q + 1 for x and for m alike, so the position -1 that the first group of m reaches (48 - 49) and the position 576
// that the last one reaches (527 + 49) are slots 0 and 577 of the same plane: inside it, never written, and read for wrapped
// columns only. A B fragment is one aligned ds_read_b128. Banks (b128: bank = (byte / 4) mod 64, four groups of 16 lanes, each
// two runs of lanes: l & 15 in {0 .. 3, 12 .. 15} of one l >> 4 and {4 .. 11} of the next): a group reads slots s0 + {0 .. 3,
// 12 .. 15} of one plane and s0 + {4 .. 11} of the plane behind it; because the plane stride is a multiple of 256 B (static_assert
// below) the sixteen 16-byte slots are s0 + 0 .. 15 mod 16: all distinct, conflict-free for every group, every tap offset and
// the shift by one slot. The m store is one ds_write_b64 per pixel group and A group (4 consecutive channels of a D fragment
// are half an octet).
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
// near (below). Taken: (a). One packing for both strides, w1p as stated in the issue. A strided chunk is 16 channels: the half
// (c0 >> 4) & 1 of K block c0 >> 5, the lanes of the other half feed zeros; a longer strided Cin (32, 64: tests only) issues
// conv1's MFMAs twice per K block.
// Decision 5 -- Cin = 64 at stride 1 (tests only, with projection): chunks of 32 channels, one behind the other behind a barrier;
// no register prefetch of the next chunk, as in layer3's f16 kernel: the network's blocks are one chunk.
// Decision 6 -- MFMA-to-load ratio: per wave one ds_read_b128 (1 KB) feeds two MFMAs = 32 cycles; the CU's four waves read
// (72 + 54) x 4 KB = 504 KB per 32 -> 32 tile = 2 016 clocks of the LDS array at 256 B / clock against 252 x 16 = 4 032 of MFMA.
// The weights: two 16-byte loads per lane per tap = per 16 or 12 MFMAs (36 864 B of w1 / w2 in all: L1 / L2 hits).
//
// The packed weights (uint16 = binary16 bits, 16-byte aligned, mmp_stem.pack_block2_f16; include/nmpc_hip.h):
//   w1p[tap t = 3 ky + kx][K block kb < ceil(Cin / 32)][group h < 2][lane l < 64][j < 8] = f16(w1[16 h + (l & 15)][32 kb + 8 (l >> 4) + j][ky][kx])
//   w2p the same with Cin = 32 (kb = 0);   wdp[kb][h][l][j] = f16(wd[16 h + (l & 15)][32 kb + 8 (l >> 4) + j]);   0 where the channel is >= Cin.
//
// Steps: 1. per chunk: x global -> f16 -> LDS (8 channels of a position per 16-byte store, zero outside the plane and for
// channels >= Cin), barrier, 9 taps x 8 pixel groups x 2 A groups of MFMA; 2. barrier; m -> LDS; barrier; 3. 9 taps x 6 groups
// x 2 A groups on m; 4. per pixel group of out: the projection (x read again and rounded, one MFMA per K block and A group), the
// affines, the identity, the activation, one dword store per value. No atomics, no scratch.
//
// Summation order (fixed): per convolution chunks ascending, per chunk the taps ky-major, per tap the instruction's own order
// over its 32 channels; then one fma per affine and one addition. A row's bits depend on that row of x and the weights only: not
// on M, the row's position, the launch or the alignment of out.
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
// loads per pixel group in the epilogue. Not built: tap pairing (decision 4), a register prefetch of the next tile, f16
// activations in memory.
//
// Compiler (hipcc -O3 --offload-arch=gfx950; tools/kernel_resources.py on the shipped code object): mmp_blk2h_kernel<2, true>
// 126 VGPRs, 80 SGPRs, 75 776 B LDS; <1, true> 126 VGPRs, 80 SGPRs, 37 888 B; <1, false> 122 VGPRs, 70 SGPRs, 37 888 B; 0 AGPRs, no
// spills, scratch 0, code 21-32 KB: four workgroups per CU compile clean. tests/test_mmp_block2_f16_cpu.py holds the three
// kernels to: scratch 0, no spills, the LDS of 4 (8 at stride 2) planes, 160 KB / LDS = the 4 (2) workgroups per CU that
// __launch_bounds__ claims, and registers that allow as many waves per SIMD.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmpc_mmp_block2.h"

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

typedef _Float16 mmp_b2h_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 mmp_b2h_h4 __attribute__((ext_vector_type(4)));

// float32 -> binary16 of the rule: clipped to +-65504 (NaN passes both comparisons), then rounded to nearest even
__device__ __forceinline__ _Float16 mmp_b2h_round(float v)
{
    v = v > 65504.0f ? 65504.0f : v;
    v = v < -65504.0f ? -65504.0f : v;
    return (_Float16)v;
}

template <int STRIDE, bool PROJ>
__global__ __launch_bounds__(kB2Threads, STRIDE == 2 ? 2 : 4) void mmp_blk2h_kernel(MmpBlock2HParams p)
{
    static_assert(STRIDE == 1 || STRIDE == 2, "stride");
    constexpr int CK = STRIDE == 2 ? 16 : 32;          // input channels per chunk: half a K block, or one
    constexpr int NO = CK / 8;                         // octets of channels per chunk
    constexpr int NPL = NO * STRIDE * STRIDE;          // planes per chunk: [sub-plane][octet]
    constexpr int NI = NPL * kB2Q;                     // 16-byte items per chunk
    constexpr int PRE = NI / kB2Threads;               // items a thread stages per chunk: 9 / 18
    static_assert(NI % kB2Threads == 0 && NPL >= kB2HMP, "the chunk does not fit the workgroup, or m does not fit over it");
    __shared__ __attribute__((aligned(16))) _Float16 lds[NPL * kB2P * 8]; // [plane][slot = position + 1][8]; m over the last chunk

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, col = tid & 15, k4 = (tid >> 4) & 3;
    const int tiles = p.tx * p.ty;
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    if (n >= p.M) return; // (workgroup-uniform, in front of every barrier)
    const int tyi = tile / p.tx, txi = tile - tyi * p.tx;
    const int gy0 = tyi * kB2TH - 2, gx0 = txi * kB2TW - 2; // the output pixel of position 0
    const size_t plane = (size_t)p.H * p.W, plane2 = (size_t)p.H2 * p.W2;
    const float* xn = p.x + (size_t)n * p.Cin * plane;
    const int KB1 = (p.Cin + 31) >> 5;               // K blocks of the first convolution and the projection

    const mmp_b2_f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    const mmp_b2h_h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    mmp_b2_f4 acc[kB2NI][kB2NH];
    int gq[kB2NI]; // the wave's pixel groups: first position + col
#pragma unroll
    for (int i = 0; i < kB2NI; ++i) {
        const int j = wave + 4 * i;
        gq[i] = mmp_b2_group(j < kB2GM ? j : kB2GM - 1) + col;
#pragma unroll
        for (int h = 0; h < kB2NH; ++h) acc[i][h] = zero;
    }

    // ---- 1. the first convolution, the input staged in chunks of CK channels, rounded on the way
    for (int c0 = 0; c0 < p.Cin; c0 += CK) {
        if (c0) __syncthreads(); // the previous chunk has been read
#pragma unroll 3
        for (int e = 0; e < PRE; ++e) {
            const int i = tid + e * kB2Threads;
            const int pl = i / kB2Q, q = i - pl * kB2Q;
            const int sub = pl / NO, o = pl - sub * NO;
            const int y = STRIDE * (gy0 + q / kB2S) + sub / 2, xx = STRIDE * (gx0 + q % kB2S) + sub % 2;
            const int ch = c0 + 8 * o;                   // (Cin is a multiple of 8: an octet is inside or outside)
            const bool in = ch < p.Cin && y >= 0 && y < p.H && xx >= 0 && xx < p.W;
            const size_t at = in ? (size_t)ch * plane + (size_t)y * p.W + xx : (size_t)0;
            mmp_b2h_h8 v;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = mmp_b2h_round(in ? xn[at + (size_t)j * plane] : 0.0f);
            *reinterpret_cast<mmp_b2h_h8*>(lds + 8 * (pl * kB2P + q + 1)) = v;
        }
        __syncthreads();
        // stride 1: the chunk is K block c0 / 32, lane group k4 reads octet k4. Stride 2: the chunk is half (c0 / 16) & 1 of K
        // block c0 / 32: the lane groups of that half read octets 0, 1, the other two feed zeros
        const bool feeds = STRIDE == 1 || (k4 >> 1) == ((c0 >> 4) & 1);
        const int oct = STRIDE == 1 ? k4 : (k4 & 1);
        const uint16_t* wk = p.w1 + (size_t)(c0 >> 5) * 2 * 512 + lane * 8;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int ky = t / 3, kx = t % 3;
            const int sub = STRIDE == 2 ? 2 * (ky != 1) + (kx != 1) : 0;
            const int off = STRIDE == 2 ? (ky == 0 ? -kB2S : 0) + (kx == 0 ? -1 : 0) : (ky - 1) * kB2S + (kx - 1);
            mmp_b2h_h8 a[kB2NH];
#pragma unroll
            for (int h = 0; h < kB2NH; ++h) a[h] = *reinterpret_cast<const mmp_b2h_h8*>(wk + ((size_t)t * KB1 * 2 + h) * 512);
            const _Float16* xb = lds + 8 * ((sub * NO + oct) * kB2P + off + 1);
#pragma unroll
            for (int i = 0; i < kB2NI; ++i) {
                const mmp_b2h_h8 b = feeds ? *reinterpret_cast<const mmp_b2h_h8*>(xb + 8 * gq[i]) : zero8;
#pragma unroll
                for (int h = 0; h < kB2NH; ++h) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[h], b, acc[i][h], 0, 0, 0);
            }
        }
    }

    // ---- 2. m -> LDS over the last chunk, rounded, zero outside the plane
    __syncthreads(); // the last chunk has been read
#pragma unroll
    for (int h = 0; h < kB2NH; ++h) {
        float s[4], sh[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] = p.s1[16 * h + 4 * k4 + r], sh[r] = p.b1[16 * h + 4 * k4 + r];
        // channels 16 h + 4 k4 + r, r = 0 .. 3: half of octet 2 h + (k4 >> 1)
        _Float16* mo = lds + 8 * ((2 * h + (k4 >> 1)) * kB2P + 1) + 4 * (k4 & 1);
#pragma unroll
        for (int i = 0; i < kB2NI; ++i) {
            if (wave + 4 * i >= kB2GM) continue; // (a recomputed copy)
            const int q = gq[i];
            const int y = gy0 + q / kB2S, xx = gx0 + q % kB2S;
            const bool in = y >= 0 && y < p.H2 && xx >= 0 && xx < p.W2;
            mmp_b2h_h4 mv;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = fmaf(s[r], acc[i][h][r], sh[r]);
                mv[r] = mmp_b2h_round(in ? (v > 0.0f ? v : v * p.slope_mid) : 0.0f);
            }
            *reinterpret_cast<mmp_b2h_h4*>(mo + 8 * q) = mv;
        }
    }
    __syncthreads();

    // ---- 3. the second convolution on the m tile: one K block (the wave's groups of out are its first kB2NO groups of m)
#pragma unroll
    for (int i = 0; i < kB2NO; ++i)
#pragma unroll
        for (int h = 0; h < kB2NH; ++h) acc[i][h] = zero;
    {
        const uint16_t* wk = p.w2 + lane * 8;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int off = (t / 3 - 1) * kB2S + (t % 3 - 1);
            mmp_b2h_h8 a[kB2NH];
#pragma unroll
            for (int h = 0; h < kB2NH; ++h) a[h] = *reinterpret_cast<const mmp_b2h_h8*>(wk + ((size_t)t * 2 + h) * 512);
            const _Float16* mb = lds + 8 * (k4 * kB2P + off + 1);
#pragma unroll
            for (int i = 0; i < kB2NO; ++i) {
                const mmp_b2h_h8 b = *reinterpret_cast<const mmp_b2h_h8*>(mb + 8 * gq[i]);
#pragma unroll
                for (int h = 0; h < kB2NH; ++h) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[h], b, acc[i][h], 0, 0, 0);
            }
        }
    }

    // ---- 4. the projection, the affine, the identity, the activation and the store
    float* on = p.out + (size_t)n * kB2C * plane2;
#pragma unroll
    for (int i = 0; i < kB2NO; ++i) {
        const int q = gq[i];
        const int c = q % kB2S;
        const int y = gy0 + q / kB2S, xx = gx0 + c; // rows 2 .. 9 of the domain: y >= 0; c >= 2: xx >= 0
        const bool valid = c >= 2 && c < 2 + kB2TW && y < p.H2 && xx < p.W2;
        mmp_b2_f4 idacc[kB2NH] = {zero, zero};
        if (PROJ) { // (every lane takes part in the MFMAs; a lane without a pixel, or with channels >= Cin, feeds zeros)
            const float* xc = xn + (valid ? (size_t)(STRIDE * y) * p.W + STRIDE * xx : (size_t)0);
            for (int kb = 0; kb < KB1; ++kb) {
                const int ch = 32 * kb + 8 * k4;
                const bool ld = valid && ch < p.Cin;
                mmp_b2h_h8 b;
#pragma unroll
                for (int j = 0; j < 8; ++j) b[j] = mmp_b2h_round(ld ? xc[(size_t)(ch + j) * plane] : 0.0f);
#pragma unroll
                for (int h = 0; h < kB2NH; ++h)
                    idacc[h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                        *reinterpret_cast<const mmp_b2h_h8*>(p.wd + ((size_t)kb * 2 + h) * 512 + lane * 8), b, idacc[h], 0, 0, 0);
            }
        }
        if (!valid) continue;
        const size_t pix = (size_t)y * p.W2 + xx;
#pragma unroll
        for (int h = 0; h < kB2NH; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = 16 * h + 4 * k4 + r;
                const size_t o = (size_t)co * plane2 + pix;
                const float z = fmaf(p.s2[co], acc[i][h][r], p.b2[co]);
                const float id = PROJ ? fmaf(p.sd[co], idacc[h][r], p.bd[co]) : xn[o]; // (no projection: plane2 == plane)
                const float v = z + id;
                on[o] = v > 0.0f ? v : v * p.slope_out;
            }
    }
}

} // namespace nmpc
