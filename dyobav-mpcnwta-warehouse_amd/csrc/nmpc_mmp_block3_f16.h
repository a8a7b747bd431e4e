// nmpc_mmp_block3_f16.h -- the residual block of nmpc_mmp_block3.h (resnet34.layer3 of the multi-hypothesis predictor's network:
// 64 output channels, stride 1 or 2, projection or identity) with binary16 MFMA OPERANDS and float32 everything else (predictor
// `mmp`, opt-in on top of the opt-in fused layer3: MmpFrontEnd(half=("layer3",))). The block, its strides, its padding and the
// zero ring of m are defined there; x [M][Cin][H][W] and out [M][64][H2][W2] stay float32 in memory.
//
// The rounding rule -- whatever an MFMA reads is f16, nothing else is:
//   - the weights w1, w2, wd are rounded ONCE on the host (mmp_stem.pack_block3_f16) and arrive packed in fragment order (below);
//   - x is rounded when it is staged into LDS (both convolutions' and the projection's operand; the projection reads it again
//     from memory and rounds it the same way);
//   - m = leaky(fma(s1, acc, b1), slope_mid) is rounded when it is written to LDS;
//   - rounding is to nearest even; a value beyond +-65504 saturates to +-65504 (mmp_b3h_round clips, then converts: the
//     infinities saturate with the finite values), NaN stays NaN, subnormals are kept (the kernel runs with f16 denormals on, and
//     the gfx950 MFMA does not flush them: tests/test_gpu_mmp_block3_f16.py pins that on the device);
//   - float32, as in the sibling: the accumulation (the MFMA's), the two affines and both LeakyReLUs, the addition z + id, x as
//     the identity when there is no projection (read again UNROUNDED), x and out in memory.
// tests/mmp_block3_f16_reference.py states the same rule in float64 with a derived bound.
//
// Instruction: v_mfma_f32_16x16x32_f16, K = 32 per instruction against the sibling's 4 at half its cycles (16 against 32 per SIMD):
//   A: lane l holds w[co = 16 g + (l & 15)][ci = 32 kb + 8 (l >> 4) + j], j = 0 .. 7, of one tap         (4 VGPRs, one 16-byte load)
//   B: lane l holds tile[ci = 32 kb + 8 (l >> 4) + j][q + off(tap)], q = q0 + (l & 15)                   (4 VGPRs, one ds_read_b128)
//   D: 4 VGPRs: channel 16 g + 4 (l >> 4) + r in register r, pixel q0 + (l & 15)                         (as the f32 form)
// 64 channels are two K blocks per tap, the strided block's 32 input channels one; a Cin that is no multiple of 32 has zeros in
// the last K block (staged zeros in B, packed zeros in A).
//
// Ported unchanged from the sibling (proven there, with wrong-variant controls): the flat domain of 11 x 25 = 275 positions of
// the OUTPUT plane around a tile of 7 x 21 outputs, its 14 pixel groups of m from position 26 and 12 of out, the flat-offset
// taps, the parity split of the strided input into four sub-planes on the same domain (tap ky reads row parity ky != 1 at
// offset -25 for ky = 0), m zero outside the plane, m written over the dead input, the projection in the epilogue, 256
// threads = 2 x 2 waves (wave = 2 pw + hw: pixel groups of parity pw, channel halves 2 hw, 2 hw + 1: 7 + 6 groups and TWO A
// operands per B read each), one workgroup per [row][tile row][tile column].
//
// Decision 1 -- LDS layout: channels innermost, in OCTETS: [plane = sub-plane x octet][position q][8 halves], 16 bytes per
// position, planes of kB3HPL = 288 positions = 4 608 B = 18 x 256 B. A B fragment is one aligned ds_read_b128. Banks (b128: bank =
// (byte / 4) mod 64, four groups of 16 lanes, each two runs of lanes: l & 15 in {0 .. 3, 12 .. 15} of one l >> 4 and {4 .. 11}
// of the next): a group reads positions q0 + {0 .. 3, 12 .. 15} of one plane and q0 + {4 .. 11} of the plane behind it; because
// the plane stride is a multiple of 256 B the sixteen 16-byte slots are q0 + 0 .. 15 mod 16: all distinct, conflict-free for
// every q0 and every tap offset. The alternative [position][64 channels] (128 B or 144 B per position) was counted and is
// 2-way conflicted for every stride of 16 a bytes, a odd, 128 .. 240: the two runs of a lane group land on the same slots.
// The m store is one ds_write_b64 per pixel group and channel half (4 consecutive channels of a D fragment are half an octet).
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
// The packed weights (uint16 = binary16 bits, 16-byte aligned, mmp_stem.pack_block3_f16; include/nmpc_hip.h):
//   w1p[tap t = 3 ky + kx][K block kb < ceil(Cin / 32)][group g < 4][lane l < 64][j < 8] = f16(w1[16 g + (l & 15)][32 kb + 8 (l >> 4) + j][ky][kx])
//   w2p the same with Cin = 64;   wdp[kb][g][l][j] = f16(wd[16 g + (l & 15)][32 kb + 8 (l >> 4) + j]);   0 where the channel is >= Cin.
//
// Steps: 1. per chunk: x global -> f16 -> LDS (8 channels of a position per 16-byte store, zero outside the plane and for
// channels >= Cin), barrier, per K block 9 taps x 7 pixel groups x 2 halves of MFMA; 2. barrier; m -> LDS; barrier; 3. 2 K
// blocks x 9 taps x 6 groups x 2 halves on m; 4. per pixel group of out: the projection (x read again and rounded, one MFMA per
// K block and half), the affines, the identity, the activation, one dword store per value. No atomics, no scratch.
// Words of LDS read without being written (position 275 .. 287 of a plane, 16 .. 25 and 250 .. 259 of m) feed wrapped columns
// and the unused ends of the first and last group only, as in the sibling.
//
// Summation order (fixed): per convolution K blocks ascending, per K block the taps ky-major, per tap the instruction's own
// order over its 32 channels; then one fma per affine and one addition. A row's bits depend on that row of x and the weights
// only: not on M, the row's position, the launch or the alignment of out.
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
// Compiler (hipcc -O3 --offload-arch=gfx950; tools/kernel_resources.py on the shipped code object): mmp_blk3h_kernel<2, true>
// 165 VGPRs, 86 SGPRs, 73 728 B LDS; <1, true> 124 VGPRs, 86 SGPRs, 36 864 B; <1, false> 124 VGPRs, 74 SGPRs, 36 864 B; no
// spills, scratch 0. tests/test_mmp_block3_f16_cpu.py holds them to: scratch 0, no spills, 36 864 B and at most 128 registers
// (4 waves per SIMD) at stride 1, 73 728 B and at most 256 (2 waves per SIMD) at stride 2.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nmpc_mmp_block3.h"

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
constexpr int kB3HMP = kB3C / 8;                     // planes of m: 8 octets of channels
static_assert(kB3HPL * 16 % 256 == 0, "the plane stride must keep a lane group's two runs on distinct 16-byte slots");
static_assert(kB3M0 + 16 * kB3GM + kB3S + 1 <= kB3HPL && kB3M0 - kB3S - 1 >= 0, "a tap leaves the plane");

typedef _Float16 mmp_b3h_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 mmp_b3h_h4 __attribute__((ext_vector_type(4)));

// float32 -> binary16 of the rule: clipped to +-65504 (NaN passes both comparisons), then rounded to nearest even
__device__ __forceinline__ _Float16 mmp_b3h_round(float v)
{
    v = v > 65504.0f ? 65504.0f : v;
    v = v < -65504.0f ? -65504.0f : v;
    return (_Float16)v;
}

template <int STRIDE, bool PROJ>
__global__ __launch_bounds__(kB3Threads, STRIDE == 2 ? 2 : 4) void mmp_blk3h_kernel(MmpBlock3HParams p)
{
    static_assert(STRIDE == 1 || STRIDE == 2, "stride");
    constexpr int CK = STRIDE == 2 ? 32 : 64;          // input channels per chunk
    constexpr int NO = CK / 8;                         // octets of channels per chunk
    constexpr int NPL = NO * STRIDE * STRIDE;          // planes per chunk: [sub-plane][octet]
    constexpr int NI = NPL * kB3Q;                     // 16-byte items per chunk
    constexpr int PRE = (NI + kB3Threads - 1) / kB3Threads; // items a thread stages per chunk: 9 / 18
    static_assert(NPL >= kB3HMP, "m does not fit over the chunk");
    __shared__ __attribute__((aligned(16))) _Float16 lds[NPL * kB3HPL * 8]; // [plane][position][8]; m over the last chunk

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pw = wave >> 1, hb = 2 * (wave & 1);   // the wave's parity of pixel groups; its first channel half
    const int lane = tid & 63, col = tid & 15, k4 = (tid >> 4) & 3;
    const int tiles = p.tx * p.ty;
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    if (n >= p.M) return; // (workgroup-uniform, in front of every barrier)
    const int tyi = tile / p.tx, txi = tile - tyi * p.tx;
    const int gy0 = tyi * kB3TH - 2, gx0 = txi * kB3TW - 2; // the output pixel of position 0
    const size_t plane = (size_t)p.H * p.W, plane2 = (size_t)p.H2 * p.W2;
    const float* xn = p.x + (size_t)n * p.Cin * plane;
    const int KB1 = (p.Cin + 31) >> 5;               // K blocks of the first convolution and the projection

    const mmp_b3_f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    mmp_b3_f4 acc[kB3NI][kB3NH];
    int gq[kB3NI]; // the wave's pixel groups: first position + col
#pragma unroll
    for (int i = 0; i < kB3NI; ++i) {
        gq[i] = mmp_b3_group(pw + 2 * i) + col;
#pragma unroll
        for (int h = 0; h < kB3NH; ++h) acc[i][h] = zero;
    }

    // ---- 1. the first convolution, the input staged in chunks of CK channels, rounded on the way
    for (int c0 = 0; c0 < p.Cin; c0 += CK) {
        if (c0) __syncthreads(); // the previous chunk has been read
#pragma unroll 3
        for (int e = 0; e < PRE; ++e) {
            const int i = tid + e * kB3Threads;
            if (i < NI) {
                const int pl = i / kB3Q, q = i - pl * kB3Q;
                const int sub = pl / NO, o = pl - sub * NO;
                const int y = STRIDE * (gy0 + q / kB3S) + sub / 2, xx = STRIDE * (gx0 + q % kB3S) + sub % 2;
                const int ch = c0 + 8 * o;               // (Cin is a multiple of 8: an octet is inside or outside)
                const bool in = ch < p.Cin && y >= 0 && y < p.H && xx >= 0 && xx < p.W;
                const size_t at = in ? (size_t)ch * plane + (size_t)y * p.W + xx : (size_t)0;
                mmp_b3h_h8 v;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = mmp_b3h_round(in ? xn[at + (size_t)j * plane] : 0.0f);
                *reinterpret_cast<mmp_b3h_h8*>(lds + 8 * (pl * kB3HPL + q)) = v;
            }
        }
        __syncthreads();
        for (int kb = 0; kb < CK / 32; ++kb) {
            if (c0 + 32 * kb >= p.Cin) break; // (uniform)
            const uint16_t* wk = p.w1 + ((size_t)((c0 >> 5) + kb) * 4 + hb) * 512 + lane * 8;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ky = t / 3, kx = t % 3;
                const int sub = STRIDE == 2 ? 2 * (ky != 1) + (kx != 1) : 0;
                const int off = STRIDE == 2 ? (ky == 0 ? -kB3S : 0) + (kx == 0 ? -1 : 0) : (ky - 1) * kB3S + (kx - 1);
                mmp_b3h_h8 a[kB3NH];
#pragma unroll
                for (int h = 0; h < kB3NH; ++h) a[h] = *reinterpret_cast<const mmp_b3h_h8*>(wk + ((size_t)t * KB1 * 4 + h) * 512);
                const _Float16* xb = lds + 8 * ((sub * NO + 4 * kb + k4) * kB3HPL + off);
#pragma unroll
                for (int i = 0; i < kB3NI; ++i) {
                    const mmp_b3h_h8 b = *reinterpret_cast<const mmp_b3h_h8*>(xb + 8 * gq[i]);
#pragma unroll
                    for (int h = 0; h < kB3NH; ++h) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[h], b, acc[i][h], 0, 0, 0);
                }
            }
        }
    }

    // ---- 2. m -> LDS over the last chunk, rounded, zero outside the plane
    __syncthreads(); // the last chunk has been read
#pragma unroll
    for (int h = 0; h < kB3NH; ++h) {
        float s[4], sh[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] = p.s1[16 * (hb + h) + 4 * k4 + r], sh[r] = p.b1[16 * (hb + h) + 4 * k4 + r];
        // channels 16 (hb + h) + 4 k4 + r, r = 0 .. 3: half of octet 2 (hb + h) + (k4 >> 1)
        _Float16* mo = lds + 8 * ((2 * (hb + h) + (k4 >> 1)) * kB3HPL) + 4 * (k4 & 1);
#pragma unroll
        for (int i = 0; i < kB3NI; ++i) {
            const int q = gq[i];
            const int y = gy0 + q / kB3S, xx = gx0 + q % kB3S;
            const bool in = y >= 0 && y < p.H2 && xx >= 0 && xx < p.W2;
            mmp_b3h_h4 mv;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = fmaf(s[r], acc[i][h][r], sh[r]);
                mv[r] = mmp_b3h_round(in ? (v > 0.0f ? v : v * p.slope_mid) : 0.0f);
            }
            *reinterpret_cast<mmp_b3h_h4*>(mo + 8 * q) = mv;
        }
    }
    __syncthreads();

    // ---- 3. the second convolution on the m tile (the wave's groups of out are its first kB3NO groups of m)
#pragma unroll
    for (int i = 0; i < kB3NO; ++i)
#pragma unroll
        for (int h = 0; h < kB3NH; ++h) acc[i][h] = zero;
    for (int kb = 0; kb < kB3C / 32; ++kb) {
        const uint16_t* wk = p.w2 + ((size_t)kb * 4 + hb) * 512 + lane * 8;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int off = (t / 3 - 1) * kB3S + (t % 3 - 1);
            mmp_b3h_h8 a[kB3NH];
#pragma unroll
            for (int h = 0; h < kB3NH; ++h) a[h] = *reinterpret_cast<const mmp_b3h_h8*>(wk + ((size_t)t * (kB3C / 32) * 4 + h) * 512);
            const _Float16* mb = lds + 8 * ((4 * kb + k4) * kB3HPL + off);
#pragma unroll
            for (int i = 0; i < kB3NO; ++i) {
                const mmp_b3h_h8 b = *reinterpret_cast<const mmp_b3h_h8*>(mb + 8 * gq[i]);
#pragma unroll
                for (int h = 0; h < kB3NH; ++h) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[h], b, acc[i][h], 0, 0, 0);
            }
        }
    }

    // ---- 4. the projection, the affine, the identity, the activation and the store
    float* on = p.out + (size_t)n * kB3C * plane2;
#pragma unroll
    for (int i = 0; i < kB3NO; ++i) {
        const int q = gq[i];
        const int r0 = q / kB3S, c = q - r0 * kB3S;
        const int y = gy0 + r0, xx = gx0 + c;
        const bool valid = r0 >= 2 && r0 < 2 + kB3TH && c >= 2 && c < 2 + kB3TW && y < p.H2 && xx < p.W2; // (then y, xx >= 0)
        mmp_b3_f4 idacc[kB3NH] = {zero, zero};
        if (PROJ) { // (every lane takes part in the MFMAs; a lane without a pixel, or with channels >= Cin, feeds zeros)
            const float* xc = xn + (valid ? (size_t)(STRIDE * y) * p.W + STRIDE * xx : (size_t)0);
            for (int kb = 0; kb < KB1; ++kb) {
                const int ch = 32 * kb + 8 * k4;
                const bool ld = valid && ch < p.Cin;
                mmp_b3h_h8 b;
#pragma unroll
                for (int j = 0; j < 8; ++j) b[j] = mmp_b3h_round(ld ? xc[(size_t)(ch + j) * plane] : 0.0f);
#pragma unroll
                for (int h = 0; h < kB3NH; ++h)
                    idacc[h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                        *reinterpret_cast<const mmp_b3h_h8*>(p.wd + ((size_t)kb * 4 + hb + h) * 512 + lane * 8), b, idacc[h], 0, 0, 0);
            }
        }
        if (!valid) continue;
        const size_t pix = (size_t)y * p.W2 + xx;
#pragma unroll
        for (int h = 0; h < kB3NH; ++h)
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
