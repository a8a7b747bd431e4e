// nmpc_mmp_block_f32.h -- the residual block of the multi-hypothesis predictor's network (resnet34.layer2 .. layer4 of the
// reference's ConvMultiHypoNet(lite=True), net_module/net.py:45-82, submodules.py:21-40), fused, float32 in and out, stated ONCE
// for every stage (predictor `mmp`, opt-in). A stage is a GEOMETRY G: nmpc_mmp_block2.h (C = 32 output channels),
// nmpc_mmp_block3.h (64) and nmpc_mmp_block4.h (128) hold one each, with the stage's Params, its constants, its decisions, its
// model and its measured figures. nmpc_mmp_block_f16.h is the same block on binary16 MFMA operands. The stride s in {1, 2}
// applies to the first convolution and to the projection only:
//   m   = leaky( s1 * conv3x3(x, w1; stride s, zero padding 1) + b1 , slope_mid )        Cin -> C, plane H x W -> H2 x W2
//   z   =        s2 * conv3x3(m, w2; stride 1, zero padding 1) + b2                      C -> C
//   id  = x  (wd == nullptr: s == 1 and Cin == C)  |  sd * conv1x1(x, wd; stride s) + bd
//   out = leaky( z + id , slope_out )
// x [M][Cin][H][W] -> out [M][C][H2][W2], H2 = (H - 1) / s + 1, W2 = (W - 1) / s + 1; m, z and id never exist in memory. The
// norms are folded into (s, b) on the host (mmp_stem.fold_block2 .. fold_block4). m outside the H2 x W2 plane is ZERO (the
// second convolution's padding), not leaky(b1).
//
// Instruction: v_mfma_f32_16x16x4_f32 as an implicit GEMM. The C output channels are C / 16 A operands per tap, of which a wave
// holds G::NH = 2 from G::first_a(wave) on:
//   A_h = w[co = 16 h + (lane & 15)][ci = 4 g + (lane >> 4)][ky][kx]                 one VGPR each, held for all pixel groups
//   B   = tile[ci = 4 g + (lane >> 4)][q + off(ky, kx)], q = q0 + (lane & 15)        ONE ds_read_b32 for both
//   D_h = 4 VGPRs: channel 16 h + 4 (lane >> 4) + r in register r, pixel q0 + (lane & 15)
// so one LDS instruction per 2 048 fma, and a group of 16 positions is 4 accumulator VGPRs per lane and A operand.
//
// The flat domain. Everything lives on ONE flat domain of the OUTPUT plane: G::Q positions in rows of G::S, a tile of outputs
// with its halo; position q = S r + c is the output pixel (gy0 + r, gx0 + c). A PIXEL GROUP is 16 consecutive positions from a
// first position G::group(pg, i): where S is no multiple of 16 it runs across row ends, and every lane works out its own row
// and column; a tap is a flat offset (ky - 1) S + (kx - 1) whatever the group. A wave's groups of out are its first G::NO groups
// of m, so out, and the identity added to it, sit in the lane and register that held m of the same pixel. Positions in the
// halo columns are computed from wrapped neighbours and never stored or used (a column of D depends on the same column of B
// only).
// The parity split. The strided block's input tile is stored split by row and column parity, four sub-planes per channel, each
// on the same domain: sub-plane (py, px) at position (r, c) holds x[2 (gy0 + r) + py][2 (gx0 + c) + px]. The tap ky reads row
// parity py = (ky != 1) at the flat offset -S for ky = 0 and 0 otherwise (2 Y - 1 = 2 (Y - 1) + 1), likewise kx: a tap is ONE
// flat offset into ONE sub-plane again, and the projection reads the (even, even) sub-plane at the centre tap's position.
// Layout in LDS [sub-plane][channel][G::P]: the four channels of a B read are one plane stride apart.
// Banks (ds_read_b32 / ds_write_b32: two groups of 32 lanes, bank = word mod 32): the plane stride G::P is 16 mod 32 (each
// stage's static_assert), a B read takes 16 consecutive words of each of two planes per lane group -- 32 distinct banks
// wherever the group starts, conflict-free, at either stride. The m store writes, per register r and A operand h, channel
// 16 h + 4 k + r to slot 16 h + 4 r + k: the lanes of a store are 16 consecutive words of planes one stride apart --
// conflict-free as well; the second convolution's group g then holds the channels 16 (g / 4) + (g % 4) + {0, 4, 8, 12}.
// m over the input. The input chunk (G::cc(STRIDE) channels, at stride 2 four sub-planes each) is dead when m is written, so m
// is written OVER it behind one more barrier: G::Lds words of static LDS hold either.
// The projection is computed in the epilogue, per pixel group of out: Cin / 4 MFMA pairs whose B is x[4 g + k][s y][s x] read
// again from global memory (L2; 1 / 9 of what conv1 read), into 8 transient registers. The same instructions in the same order
// as resident accumulators would see; what is lost is their overlap with conv1's MFMAs (nmpc_mmp_block2.h, decision 4).
//
// Steps: workgroup = [row of the batch][tile row][tile column] flattened in x.
//   1. per chunk of input channels: the chunk's planes global -> registers (issued one chunk ahead, behind the barrier) ->
//      LDS, zero outside the plane and for channels >= Cin; then per group of 4 channels 9 taps x G::NI pixel groups x 2 A
//      operands of MFMA into the resident accumulators of m
//   2. barrier; m = leaky(fma(s1, acc, b1)), zero outside the plane -> LDS [C slots][G::P]; a fitted domain's ring -> zeros; barrier
//   3. per group of 4 slots 9 taps x G::NO pixel groups x 2 A operands of MFMA on the m tile
//   4. per pixel group of out: with a projection Cin / 4 x 2 MFMA on x read again (a lane without a pixel feeds zeros); then
//      out = leaky(fma(s2, acc, b2) + id), id = fma(sd, idacc, bd) or x read again (L2), one dword store per value: any
//      float-aligned out gives the same bits. No atomics.
//
// Summation order (fixed): conv1 -- input channels in groups of four ascending, per group the nine taps ky-major, per tap
// the four channels ascending (the instruction's k order); the projection -- input channels ascending; conv2 -- channel
// groups 16 (g / 4) + (g % 4) + {0, 4, 8, 12}, g = 0 .. C / 4 - 1 ascending, per group the taps ky-major, per tap the four
// channels ascending; then one fma per affine and one addition z + id. A row's bits depend on that row of x and the weights
// only: not on M, the row's position, the launch or the alignment of out.
//
// The nine kernels are byte for byte those of the three bodies this one replaced (profiles/mmp_f32_one_kernel_code_object_identity.txt).
//
// A geometry G holds (nmpc_mmp_block3.h is the plainest to read):
//   Params                   the kernel's argument, a true __global__ argument (handed on to a helper it cost the binary16
//                            kernel registers and spills: nmpc_mmp_block_f16.h)
//   C, Threads, min_wg       output channels; threads per workgroup; workgroups per CU of __launch_bounds__
//   S, Q, TH, TW             the flat domain: row stride, positions, outputs per tile
//   P, SH, Lds               words of an LDS plane; the word of position 0 in a plane of x (m: 0); words of static LDS
//   NI, NO, NH               pixel groups of m and of out per wave; A operands per wave
//   cc(STRIDE)               input channels per chunk
//   pixel_wave(wave)         pg: which share of the pixel groups the wave takes;   first_a(wave)   its first A operand
//   group(pg, i)             first position of the wave's pixel group i
//   live(pg, i)              whether slot i is a group of its own (false: a recomputed copy, not stored)
//   Fitted                   the domain is fitted to the plane of m (layer4): Params carry the origin oy, ox of out in the domain
//                            (otherwise 2, 2), and the Ring positions ring(j) of a plane that no group covers get zeros
//   again(STRIDE)            the staging addresses and masks are worked out again per chunk, behind an opaque thread index, not
//                            kept across the MFMAs as loop invariants (layer2 at stride 2: 73 VGPRs spilled otherwise). All but
//                            layer2 at stride 1; there it would change the bytes (244 -> 202 / 204 VGPRs, 2 KB more code; not timed)
//   MaskedXc                 the projection's address of x is formed for a lane with a pixel only (layer3, layer4), not for every
//                            lane and only loaded under the test (layer2). Masked everywhere: layer2's two projection kernels +100 /
//                            -152 B of code on the same VGPRs; unmasked everywhere: layer3's and layer4's four +48 .. +108 B
// pixel_wave, group, first_a and live of layer2 and of layer3 are a struct of their own (MmpBlock2Waves, MmpBlock3Waves) that the
// geometries of nmpc_mmp_block_f16.h share.
// What follows from the numbers is derived in the body: EVEN, WHOLE and ROWS below.
#pragma once

#include <hip/hip_runtime.h>

namespace nmpc {

typedef float mmp_blkf_f4 __attribute__((ext_vector_type(4)));

template <typename G, int STRIDE, bool PROJ>
__global__ __launch_bounds__(G::Threads, G::min_wg) void mmp_blkf_kernel(typename G::Params p)
{
    static_assert(STRIDE == 1 || STRIDE == 2, "stride");
    constexpr int CC = G::cc(STRIDE);                  // input channels per chunk
    constexpr int NPL = CC * STRIDE * STRIDE;          // planes per chunk: [sub-plane][channel]
    constexpr int NV = NPL * G::Q;                     // values per chunk
    constexpr int PRE = (NV + G::Threads - 1) / G::Threads; // tile values a thread stages per chunk
    constexpr int C = G::C, S = G::S, P = G::P, NH = G::NH;
    constexpr bool EVEN = NV % G::Threads == 0;        // every thread stages PRE values: no test of i < NV
    // Cin is a multiple of 8: a stage whose chunks hold 8 channels at the most has all the channels of a chunk, and none is tested
    // (judged by the stage's larger chunk: layer3's strided chunk of 8 keeps the tests its stride-1 kernels need, and its bytes)
    constexpr bool WHOLE = G::cc(1) <= 8;
    constexpr bool ROWS = S % 16 == 0;                 // a pixel group lies in ONE row of the domain: a group of out has no row outside the tile
    static_assert(NPL <= C, "the chunk does not fit under m");
    __shared__ float lds[G::Lds];
    float* const xs = lds + G::SH; // [NPL][P]: position q of a plane at SH + q (SH = 1: the first tap of a group may be q = -1)
    float* const ms = lds;         // [C slots][P]: position q at q; written over the last chunk

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pg = G::pixel_wave(wave), hb = G::first_a(wave); // the wave's share of the pixel groups; its first A operand
    const int col = tid & 15, k = (tid >> 4) & 3;
    const int tiles = p.tx * p.ty;
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    if (n >= p.M) return; // (workgroup-uniform, in front of every barrier)
    const int tyi = tile / p.tx, txi = tile - tyi * p.tx;
    int oy = 2, ox = 2; // the first row / column of out in the domain
    if constexpr (G::Fitted) oy = p.oy, ox = p.ox;
    const int gy0 = tyi * G::TH - oy, gx0 = txi * G::TW - ox; // the output pixel of position 0
    const size_t plane = (size_t)p.H * p.W, plane2 = (size_t)p.H2 * p.W2;
    const float* xn = p.x + (size_t)n * p.Cin * plane;

    float pre[PRE];
    auto fetch = [&](int c0) {
        int t0 = tid;
        if (G::again(STRIDE)) asm volatile("" : "+v"(t0));
#pragma unroll
        for (int e = 0; e < PRE; ++e) {
            const int i = t0 + e * G::Threads;
            const int pl = i / G::Q, q = i - pl * G::Q;
            const int sub = pl / CC, ch = pl - sub * CC;
            const int y = STRIDE * (gy0 + q / S) + sub / 2, xx = STRIDE * (gx0 + q % S) + sub % 2;
            const bool in = (EVEN || i < NV) && (WHOLE || c0 + ch < p.Cin) && y >= 0 && y < p.H && xx >= 0 && xx < p.W;
            pre[e] = in ? xn[(size_t)(c0 + ch) * plane + (size_t)y * p.W + xx] : 0.0f;
        }
    };

    const mmp_blkf_f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    mmp_blkf_f4 acc[G::NI][NH];
    int gq[G::NI]; // the wave's pixel groups: first position + col
#pragma unroll
    for (int i = 0; i < G::NI; ++i) {
        gq[i] = G::group(pg, i) + col;
#pragma unroll
        for (int h = 0; h < NH; ++h) acc[i][h] = zero;
    }

    // ---- 1. the first convolution, the input streamed in chunks
    fetch(0);
    for (int c0 = 0; c0 < p.Cin; c0 += CC) {
        __syncthreads(); // the previous chunk has been read
#pragma unroll
        for (int e = 0; e < PRE; ++e) {
            const int i = tid + e * G::Threads;
            const int pl = i / G::Q, q = i - pl * G::Q;
            if (EVEN || i < NV) xs[pl * P + q] = pre[e];
        }
        __syncthreads();
        if (c0 + CC < p.Cin) fetch(c0 + CC);
        for (int cg = 0; cg < CC / 4; ++cg) {
            if (!WHOLE && c0 + 4 * cg >= p.Cin) break; // (Cin is a multiple of 8: uniform)
            const int ci = c0 + 4 * cg + k;
            float a[NH][9];
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                const float* wp = p.w1 + ((size_t)(16 * (hb + h) + col) * p.Cin + ci) * 9;
#pragma unroll
                for (int t = 0; t < 9; ++t) a[h][t] = wp[t];
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ky = t / 3, kx = t % 3;
                const int sub = STRIDE == 2 ? 2 * (ky != 1) + (kx != 1) : 0;
                const int off = STRIDE == 2 ? (ky == 0 ? -S : 0) + (kx == 0 ? -1 : 0) : (ky - 1) * S + (kx - 1);
                const float* xb = xs + (sub * CC + 4 * cg + k) * P + off;
#pragma unroll
                for (int i = 0; i < G::NI; ++i) {
                    const float b = xb[gq[i]];
#pragma unroll
                    for (int h = 0; h < NH; ++h) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h][t], b, acc[i][h], 0, 0, 0);
                }
            }
        }
    }

    // ---- 2. m -> LDS over the last chunk, zero outside the plane; zeros to what no group covers
    __syncthreads(); // the last chunk has been read
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        float s[4], sh[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] = p.s1[16 * (hb + h) + 4 * k + r], sh[r] = p.b1[16 * (hb + h) + 4 * k + r];
#pragma unroll
        for (int i = 0; i < G::NI; ++i) {
            if (!G::live(pg, i)) continue;
            const int q = gq[i];
            const int y = gy0 + q / S, xx = gx0 + q % S;
            const bool in = y >= 0 && y < p.H2 && xx >= 0 && xx < p.W2;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = fmaf(s[r], acc[i][h][r], sh[r]);
                ms[(16 * (hb + h) + 4 * r + k) * P + q] = in ? (v > 0.0f ? v : v * p.slope_mid) : 0.0f;
            }
        }
    }
    if constexpr (G::Fitted) {
        for (int i = tid; i < C * G::Ring; i += G::Threads) {
            const int slot = i / G::Ring, j = i - slot * G::Ring;
            ms[slot * P + G::ring(j)] = 0.0f;
        }
    }
    __syncthreads();

    // ---- 3. the second convolution on the m tile (the wave's groups of out are its first G::NO groups of m)
#pragma unroll
    for (int i = 0; i < G::NO; ++i)
#pragma unroll
        for (int h = 0; h < NH; ++h) acc[i][h] = zero;
    for (int g = 0; g < C / 4; ++g) {
        const int ch = 16 * (g / 4) + 4 * k + (g % 4); // slot 4 g + k holds this channel
        float a[NH][9];
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            const float* wp = p.w2 + ((16 * (hb + h) + col) * C + ch) * 9;
#pragma unroll
            for (int t = 0; t < 9; ++t) a[h][t] = wp[t];
        }
        const float* mb = ms + (4 * g + k) * P;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int off = (t / 3 - 1) * S + (t % 3 - 1);
#pragma unroll
            for (int i = 0; i < G::NO; ++i) {
                const float b = mb[gq[i] + off];
#pragma unroll
                for (int h = 0; h < NH; ++h) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h][t], b, acc[i][h], 0, 0, 0);
            }
        }
    }

    // ---- 4. the projection, the affine, the identity, the activation and the store
    float* on = p.out + (size_t)n * C * plane2;
#pragma unroll
    for (int i = 0; i < G::NO; ++i) {
        const int q = gq[i];
        const int r0 = q / S, c = ROWS ? q % S : q - r0 * S;
        const int y = gy0 + r0, xx = gx0 + c;
        // inside the tile and the plane (then y, xx >= 0). A fitted domain reads its origin from the argument again: on the two
        // variables the compiler orders layer4's six tests differently (20 .. 172 B of code per kernel)
        bool valid;
        if constexpr (G::Fitted) valid = r0 >= p.oy && r0 < G::Q / S - p.oy && c >= p.ox && c < S - p.ox && y < p.H2 && xx < p.W2;
        else valid = (ROWS || (r0 >= oy && r0 < G::Q / S - oy)) && c >= ox && c < S - ox && y < p.H2 && xx < p.W2;
        mmp_blkf_f4 idacc[NH] = {};
        if (PROJ) { // (every lane takes part in the MFMAs; a lane without a pixel feeds zeros)
            const float* xc = xn + (size_t)k * plane; // x[k][s y][s x], formed for every lane or for a lane with a pixel only
            if constexpr (G::MaskedXc) xc += valid ? (size_t)(STRIDE * y) * p.W + STRIDE * xx : (size_t)0;
            else xc = xc + (size_t)(STRIDE * y) * p.W + STRIDE * xx;
            for (int c0 = 0; c0 < p.Cin; c0 += 4) {
                const float b = valid ? xc[(size_t)c0 * plane] : 0.0f;
#pragma unroll
                for (int h = 0; h < NH; ++h)
                    idacc[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(p.wd[(16 * (hb + h) + col) * p.Cin + c0 + k], b, idacc[h], 0, 0, 0);
            }
        }
        if (!valid) continue;
        const size_t pix = (size_t)y * p.W2 + xx;
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = 16 * (hb + h) + 4 * k + r;
                const size_t o = (size_t)co * plane2 + pix;
                const float z = fmaf(p.s2[co], acc[i][h][r], p.b2[co]);
                const float id = PROJ ? fmaf(p.sd[co], idacc[h][r], p.bd[co]) : xn[o]; // (no projection: plane2 == plane)
                const float v = z + id;
                on[o] = v > 0.0f ? v : v * p.slope_out;
            }
    }
}

} // namespace nmpc
