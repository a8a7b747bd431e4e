// nmpc_mmp_block2.h -- one residual block of the multi-hypothesis predictor's second residual stage (resnet34.layer2 of the
// reference's ConvMultiHypoNet(lite=True), net_module/net.py:45-61, submodules.py:21-40: four BasicBlocks at 32 channels, the
// first 16 -> 32 at stride 2 with a 1 x 1, stride-2 projection), fused ("next" row f3, predictor `mmp`, opt-in), float32 in
// and out. The stride s in {1, 2} applies to the first convolution and to the projection only:
//   m   = leaky( s1 * conv3x3(x, w1; stride s, zero padding 1) + b1 , slope_mid )        Cin -> 32, plane H x W -> H2 x W2
//   z   =        s2 * conv3x3(m, w2; stride 1, zero padding 1) + b2                      32 -> 32
//   id  = x  (wd == nullptr: s == 1 and Cin == 32)  |  sd * conv1x1(x, wd; stride s) + bd
//   out = leaky( z + id , slope_out )
// x [M][Cin][H][W] -> out [M][32][H2][W2], H2 = (H - 1) / s + 1, W2 = (W - 1) / s + 1; m, z and id never exist in memory. The
// norms are folded into (s, b) on the host (mmp_stem.fold_block2). m outside the H2 x W2 plane is ZERO (the second
// convolution's padding), not leaky(b1). The sibling of nmpc_mmp_block.h (16 channels, stride 1), whose building blocks it keeps.
//
// Instructions: v_mfma_f32_16x16x4_f32 as an implicit GEMM, as there. The 32 output channels are TWO A operands per tap
//   A_h = w[co = 16 h + (lane & 15)][ci = 4 g + (lane >> 4)][ky][kx], h = 0, 1       two VGPRs, held for all pixel groups
//   B   = tile[ci = 4 g + (lane >> 4)][q + off(ky, kx)], q = q0 + (lane & 15)        ONE ds_read_b32 for both
//   D_h = 4 VGPRs: channel 16 h + 4 (lane >> 4) + r in register r, pixel q0 + (lane & 15)
// so one LDS instruction per 2 048 fma: half the LDS reads per fma of the 16-channel kernel.
//
// Decision 1 -- tile geometry. Everything lives on ONE flat domain of the OUTPUT plane: kB2R x kB2S = 12 x 48 positions, the
// tile of 8 x 44 outputs with a halo of two; position q = 48 r + c is the output pixel (8 ty - 2 + r, 44 tx - 2 + c). The
// 37 x 42 plane of layer2 is one tile wide and five high: 5 tiles of 352 cover 1 554 pixels, 88 % filled (the 15 x 28 tile on a
// stride of 32 would take 3 x 2 = 6 tiles of 420: 62 %). m is computed on rows 1 .. 10 (30 groups of 16 positions), out on rows
// 2 .. 9 (24 groups), all 48 columns; columns 0, 1, 46, 47 of out and 0, 47 of m are computed from wrapped neighbours and never
// stored or used (a column of D depends on the same column of B only). Group j of m belongs to wave j & 3 in the order
// rows 2 .. 9, then row 1, then row 10: the wave's first 6 groups are exactly its groups of out (24 = 4 x 6, no copies
// there), so out, and the identity added to it, sit in the lane and register that held m of the same pixel; of the 8 groups
// per wave of m, two waves have 7 and recompute a neighbour (discarded). Of the issued MFMAs of a 32 -> 32 block 79 % are useful work on a full tile
// (halo rows of m, four wrapped columns of 48, the two recomputed copies), 83 % of the strided 16 -> 32 block.
// Decision 2 -- stride-2 taps. The strided block's input tile is stored split by row and column parity, four sub-planes per
// channel, each on the same 12 x 48 domain: sub-plane (py, px) at position (r, c) holds x[2 (8 ty - 2 + r) + py][2 (44 tx - 2 +
// c) + px]. The tap ky reads row parity py = (ky != 1) at the flat offset -48 for ky = 0 and 0 otherwise (2 Y - 1 = 2 (Y - 1) + 1),
// likewise kx: a tap is ONE flat offset into ONE sub-plane again, and the projection reads the (even, even) sub-plane at the
// centre tap's position (see decision 4 for where it is read). Layout in LDS [sub-plane][channel][592]: the four channels of a B read are
// one plane stride apart.
// Bank behaviour (ds_read_b32 / ds_write_b32: two groups of 32 lanes, bank = word mod 32): the plane stride is kB2P = 592 =
// 16 mod 32, a B read takes 16 consecutive words of each of two planes per lane group -- 32 distinct banks, conflict-free, at
// either stride. The m store writes, per register r and half h, channel 16 h + 4 k + r to slot 16 h + 4 r + k: the lanes of a
// store are 16 consecutive words of planes one stride apart -- conflict-free as well; the second convolution's group g then
// holds the channels 16 (g / 4) + (g % 4) + {0, 4, 8, 12}.
// Decision 3 -- LDS and occupancy. 32 channels of m on 592 words are 75 776 B; the input chunk (8 channels at stride 1 = 8
// planes, 4 channels at stride 2 = 16 planes: a strided chunk of 8 would stage 72 registers per thread next to 112
// accumulators) is dead when m is written, so m is written OVER it behind one more barrier: 75 792 B static, two workgroups
// per CU (160 KB), which is what feeds the MFMA pipe in the 16-channel kernel. __launch_bounds__(256, 2) states it: 256
// registers per lane, VGPRs + AGPRs.
// Decision 4 -- the accumulators of id are NOT resident. 8 x 2 x 4 = 64 registers of m next to 6 x 2 x 4 = 48 of id, the staged
// chunk (18 / 36) and 18 weights compiled to 25 (stride 1) and 126 (stride 2) spilled VGPRs under the bound of 256. The
// projection is therefore computed in the epilogue, per pixel group of out: Cin / 4 MFMA pairs whose B is x[4 g + k][s y][s x]
// read again from global memory (L2; 1 / 9 of what conv1 read -- at stride 2 the (even, even) sub-plane), into 8 transient
// registers. The same instructions in the same order as resident accumulators would see; what is lost is their overlap with
// conv1's MFMAs. Likewise at stride 2 the 36 addresses and masks of the staged chunk are recomputed per chunk instead of kept
// across the MFMAs as loop invariants (73 spilled VGPRs otherwise).
//
// Steps: 256 threads = 4 waves per workgroup; workgroup = [row of the batch][tile row][tile column] flattened in x.
//   1. per chunk of input channels: the chunk's planes global -> registers (issued one chunk ahead, behind the barrier) ->
//      LDS, zero outside the plane; then per group of 4 channels 9 taps x 8 pixel groups x 2 halves of MFMA into the resident
//      accumulators of m
//   2. barrier; m = leaky(fma(s1, acc, b1)), zero outside the plane -> LDS [32 slots][592]; barrier
//   3. per group of 4 slots 9 taps x 6 pixel groups x 2 halves of MFMA on the m tile
//   4. per pixel group of out: with a projection Cin / 4 x 2 MFMA on x read again (a lane without a pixel feeds zeros); then
//      out = leaky(fma(s2, acc, b2) + id), id = fma(sd, idacc, bd) or x read again (L2), one dword store per value: runs of
//      16 (14, 12 at a tile's edges) consecutive floats, any float-aligned out gives the same bits. No atomics.
// Words of LDS read without being written (positions -1 and 576 of a plane, 47 and 528 of an m plane) are neighbours of
// wrapped columns only; what they hold is discarded.
//
// Summation order (fixed): conv1 -- input channels in groups of four ascending, per group the nine taps ky-major, per tap
// the four channels ascending (the instruction's k order); the projection -- input channels ascending; conv2 -- channel
// groups 16 (g / 4) + (g % 4) + {0, 4, 8, 12}, g = 0 .. 7 ascending, per group the taps ky-major, per tap the four channels
// ascending; then one fma per affine and one addition z + id. A row's bits depend on that row of x and the weights only: not
// on M, the row's position, the launch or the alignment of out.
//
// Modelled before the device run, from the instruction count (four waves on the four SIMDs of a CU: a tile takes as long as
// one wave's MFMAs). Per wave and tile: the strided first block (Cin = 16) 4 channel groups x (9 x 8 x 2 + 6 x 2 of the
// projection) + 8 x 9 x 6 x 2 = 624 + 864 = 1 488 MFMA; each of the other three 8 x 144 + 864 = 2 016: 7 536 for a tile of all
// four, of 32 cycles each, for 352 x 69 632 useful fma = 5 984 MFMA-equivalents per wave: 79 % useful. At B = 256, 4 pedestrians,
// N_hor = 20 (20 480 rows x 5 tiles over 256 CUs at 2.4 GHz) that is 102 400 x 7 536 x 32 / (256 x 2.4e9) = 40 ms per lock-step if
// the MFMA pipe never waits; 28 ms at the 78.6 T fma/s fp32 peak for the 2.22e12 useful fma alone; 5.8 ms for the 36.6 GB
// (x of the first block once, three reads and four writes of [32][37][42]) at the 6.29 TB/s copy rate.
// Measured (profiles/mmp_layer2_evaluate.json): 71.5 ms, 31.0 T useful fma/s = 39 % of the fp32 peak,
// 0.51 TB/s; torch's own layer2, eager, on the same rows: 128.8 ms. The model is short by 1.78 x (the 16-channel kernel: 1.8 x).
// What is believed to cost the rest, from the code, not from counters: as there, two waves per SIMD that stop at two barriers
// per chunk (288 MFMA between them at stride 1, 144 at stride 2) and at the third in front of the m store; epilogues without
// conv MFMAs; the strided block (22.7 T fma/s against 32-33 T of the others) also recomputes its staging addresses, reads x
// two floats apart and runs its projection in the epilogue. Not built: a third workgroup per CU, a double-buffered chunk,
// resident id accumulators in AGPRs.
//
// Compiler (hipcc -O3 --offload-arch=gfx950; tools/kernel_resources.py on the shipped code object): mmp_blk2_kernel<2, true>
// 212 VGPRs, 74 SGPRs, no SGPR spills; <1, true> 244 VGPRs, 106 SGPRs and 33 SGPR spills; <1, false> 244 VGPRs, 106 SGPRs and 28
// SGPR spills (to VGPR lanes: no memory); all 0 AGPRs, no VGPR spills, scratch 0, 75 792 B LDS, occupancy 2 waves per SIMD
// (registers and LDS agree). tests/test_mmp_block2_cpu.py holds every kernel of this family to that.
#pragma once

#include <hip/hip_runtime.h>

namespace nmpc {

struct MmpBlock2Params {
    int M, Cin, H, W, H2, W2, tx, ty;                // H, W: the input plane; H2, W2: the output plane; tiles along x, y
    const float *x;                                  // [M][Cin][H][W]
    const float *w1, *s1, *b1;                       // [32][Cin][3][3], [32], [32]
    const float *w2, *s2, *b2;                       // [32][32][3][3], [32], [32]
    const float *wd, *sd, *bd;                       // [32][Cin], [32], [32] (kernel <., true>) or unused
    float slope_mid, slope_out;
    float* out;                                      // [M][32][H2][W2]
};

constexpr int kB2Threads = 256;
constexpr int kB2C = 32;                             // output channels
constexpr int kB2NH = kB2C / 16;                     // A operands per tap
constexpr int kB2TH = 8, kB2TW = 44;                 // outputs per tile
constexpr int kB2S = kB2TW + 4;                      // row stride of the flat domain: 48
constexpr int kB2R = kB2TH + 4;                      // rows of the flat domain: 12
constexpr int kB2Q = kB2R * kB2S;                    // positions of the flat domain: 576
constexpr int kB2P = 592;                            // plane stride in LDS
constexpr int kB2GR = kB2S / 16;                     // pixel groups per row: 3
constexpr int kB2GO = kB2TH * kB2GR;                 // pixel groups of out: 24
constexpr int kB2GM = (kB2TH + 2) * kB2GR;           // pixel groups of m: 30
constexpr int kB2NO = kB2GO / 4;                     // pixel groups of out per wave: 6
constexpr int kB2NI = (kB2GM + 3) / 4;               // pixel groups of m per wave: 8
constexpr int kB2Lds = kB2C * kB2P + 4;              // words of static LDS
static_assert(kB2S % 16 == 0 && kB2GO % 4 == 0, "the flat domain does not fit the waves");
static_assert(kB2P % 32 == 16 && kB2P >= kB2Q + 2, "plane stride: bank spread, and the taps of the last group stay inside");
static_assert(kB2Lds * 4 <= 80 * 1024, "static LDS over half a CU's");

// first position of m's pixel group j: rows 2 .. 9 (the groups of out) first, then row 1, then row 10
__device__ __forceinline__ constexpr int mmp_b2_group(int j)
{
    return j < kB2GO ? 2 * kB2S + 16 * j : j < kB2GO + kB2GR ? kB2S + 16 * (j - kB2GO) : (kB2R - 2) * kB2S + 16 * (j - kB2GO - kB2GR);
}

typedef float mmp_b2_f4 __attribute__((ext_vector_type(4)));

template <int STRIDE, bool PROJ>
__global__ __launch_bounds__(kB2Threads, 2) void mmp_blk2_kernel(MmpBlock2Params p)
{
    static_assert(STRIDE == 1 || STRIDE == 2, "stride");
    constexpr int CC = STRIDE == 2 ? 4 : 8;            // input channels per chunk
    constexpr int NPL = CC * STRIDE * STRIDE;          // planes per chunk: [sub-plane][channel]
    constexpr int PRE = NPL * kB2Q / kB2Threads;       // tile values a thread stages per chunk: 18 / 36
    static_assert(NPL * kB2Q % kB2Threads == 0 && NPL <= kB2C, "the chunk does not fit the workgroup");
    __shared__ float lds[kB2Lds];
    float* const xs = lds + 1;   // [NPL][592]: position q of a plane at 1 + q (the first tap of position 48 is q = -1)
    float* const ms = lds;       // [32 slots][592]: position q at q; written over the last chunk

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = tid & 15, k = (tid >> 4) & 3;
    const int tiles = p.tx * p.ty;
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    if (n >= p.M) return; // (workgroup-uniform, in front of every barrier)
    const int tyi = tile / p.tx, txi = tile - tyi * p.tx;
    const int gy0 = tyi * kB2TH - 2, gx0 = txi * kB2TW - 2; // the output pixel of position 0
    const size_t plane = (size_t)p.H * p.W, plane2 = (size_t)p.H2 * p.W2;
    const float* xn = p.x + (size_t)n * p.Cin * plane;

    float pre[PRE];
    auto fetch = [&](int c0) {
        int t0 = tid;
        // (stride 2: the 36 addresses and masks are worked out again per chunk; kept across the MFMAs as loop invariants they
        // spill -- 73 VGPRs to scratch)
        if (STRIDE == 2) asm volatile("" : "+v"(t0));
#pragma unroll
        for (int e = 0; e < PRE; ++e) {
            const int i = t0 + e * kB2Threads;
            const int pl = i / kB2Q, q = i - pl * kB2Q;
            const int sub = pl / CC, ch = pl - sub * CC;
            const int y = STRIDE * (gy0 + q / kB2S) + sub / 2, xx = STRIDE * (gx0 + q % kB2S) + sub % 2;
            const bool in = y >= 0 && y < p.H && xx >= 0 && xx < p.W;
            pre[e] = in ? xn[(size_t)(c0 + ch) * plane + (size_t)y * p.W + xx] : 0.0f;
        }
    };

    const mmp_b2_f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    mmp_b2_f4 acc[kB2NI][kB2NH];
    int gq[kB2NI]; // the wave's pixel groups: first position + col
#pragma unroll
    for (int i = 0; i < kB2NI; ++i) {
        const int j = wave + 4 * i;
        gq[i] = mmp_b2_group(j < kB2GM ? j : kB2GM - 1) + col;
#pragma unroll
        for (int h = 0; h < kB2NH; ++h) acc[i][h] = zero;
    }

    // ---- 1. the first convolution (and the projection), the input streamed in chunks
    fetch(0);
    for (int c0 = 0; c0 < p.Cin; c0 += CC) {
        __syncthreads(); // the previous chunk has been read
#pragma unroll
        for (int e = 0; e < PRE; ++e) {
            const int i = tid + e * kB2Threads;
            const int pl = i / kB2Q, q = i - pl * kB2Q;
            xs[pl * kB2P + q] = pre[e];
        }
        __syncthreads();
        if (c0 + CC < p.Cin) fetch(c0 + CC);
#pragma unroll
        for (int cg = 0; cg < CC / 4; ++cg) {
            const int ci = c0 + 4 * cg + k;
            float a[kB2NH][9];
#pragma unroll
            for (int h = 0; h < kB2NH; ++h) {
                const float* wp = p.w1 + ((size_t)(16 * h + col) * p.Cin + ci) * 9;
#pragma unroll
                for (int t = 0; t < 9; ++t) a[h][t] = wp[t];
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ky = t / 3, kx = t % 3;
                const int sub = STRIDE == 2 ? 2 * (ky != 1) + (kx != 1) : 0;
                const int off = STRIDE == 2 ? (ky == 0 ? -kB2S : 0) + (kx == 0 ? -1 : 0) : (ky - 1) * kB2S + (kx - 1);
                const float* xb = xs + (sub * CC + 4 * cg + k) * kB2P + off;
#pragma unroll
                for (int i = 0; i < kB2NI; ++i) {
                    const float b = xb[gq[i]];
#pragma unroll
                    for (int h = 0; h < kB2NH; ++h) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h][t], b, acc[i][h], 0, 0, 0);
                }
            }
        }
    }

    // ---- 2. m -> LDS over the last chunk, zero outside the plane
    __syncthreads(); // the last chunk has been read
#pragma unroll
    for (int h = 0; h < kB2NH; ++h) {
        float s[4], sh[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] = p.s1[16 * h + 4 * k + r], sh[r] = p.b1[16 * h + 4 * k + r];
#pragma unroll
        for (int i = 0; i < kB2NI; ++i) {
            if (wave + 4 * i >= kB2GM) continue; // (a recomputed copy)
            const int q = gq[i];
            const int y = gy0 + q / kB2S, xx = gx0 + q % kB2S;
            const bool in = y >= 0 && y < p.H2 && xx >= 0 && xx < p.W2;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = fmaf(s[r], acc[i][h][r], sh[r]);
                ms[(16 * h + 4 * r + k) * kB2P + q] = in ? (v > 0.0f ? v : v * p.slope_mid) : 0.0f;
            }
        }
    }
    __syncthreads();

    // ---- 3. the second convolution on the m tile (the wave's groups of out are its first kB2NO groups of m)
#pragma unroll
    for (int i = 0; i < kB2NO; ++i)
#pragma unroll
        for (int h = 0; h < kB2NH; ++h) acc[i][h] = zero;
    for (int g = 0; g < kB2C / 4; ++g) {
        const int ch = 16 * (g / 4) + 4 * k + (g % 4); // slot 4 g + k holds this channel
        float a[kB2NH][9];
#pragma unroll
        for (int h = 0; h < kB2NH; ++h) {
            const float* wp = p.w2 + ((16 * h + col) * kB2C + ch) * 9;
#pragma unroll
            for (int t = 0; t < 9; ++t) a[h][t] = wp[t];
        }
        const float* mb = ms + (4 * g + k) * kB2P;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int off = (t / 3 - 1) * kB2S + (t % 3 - 1);
#pragma unroll
            for (int i = 0; i < kB2NO; ++i) {
                const float b = mb[gq[i] + off];
#pragma unroll
                for (int h = 0; h < kB2NH; ++h) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h][t], b, acc[i][h], 0, 0, 0);
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
        if (PROJ) { // (every lane takes part in the MFMAs; a lane without a pixel feeds zeros)
            const float* xc = xn + (size_t)k * plane + (size_t)(STRIDE * y) * p.W + STRIDE * xx;
            for (int c0 = 0; c0 < p.Cin; c0 += 4) {
                const float b = valid ? xc[(size_t)c0 * plane] : 0.0f;
#pragma unroll
                for (int h = 0; h < kB2NH; ++h)
                    idacc[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(p.wd[(16 * h + col) * p.Cin + c0 + k], b, idacc[h], 0, 0, 0);
            }
        }
        if (!valid) continue;
        const size_t pix = (size_t)y * p.W2 + xx;
#pragma unroll
        for (int h = 0; h < kB2NH; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = 16 * h + 4 * k + r;
                const size_t o = (size_t)co * plane2 + pix;
                const float z = fmaf(p.s2[co], acc[i][h][r], p.b2[co]);
                const float id = PROJ ? fmaf(p.sd[co], idacc[h][r], p.bd[co]) : xn[o]; // (no projection: plane2 == plane)
                const float v = z + id;
                on[o] = v > 0.0f ? v : v * p.slope_out;
            }
    }
}

} // namespace nmpc
