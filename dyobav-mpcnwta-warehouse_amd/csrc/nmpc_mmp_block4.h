// nmpc_mmp_block4.h -- one residual block of the multi-hypothesis predictor's fourth residual stage (resnet34.layer4 of the
// reference's ConvMultiHypoNet(lite=True), net_module/net.py:63-82, submodules.py:21-40: three BasicBlocks at 128 channels, the
// first 64 -> 128 at stride 2 with a 1 x 1, stride-2 projection), fused ("next" row f4, predictor `mmp`, opt-in), float32 in
// and out. The stride s in {1, 2} applies to the first convolution and to the projection only:
//   m   = leaky( s1 * conv3x3(x, w1; stride s, zero padding 1) + b1 , slope_mid )        Cin -> 128, plane H x W -> H2 x W2
//   z   =        s2 * conv3x3(m, w2; stride 1, zero padding 1) + b2                      128 -> 128
//   id  = x  (wd == nullptr: s == 1 and Cin == 128)  |  sd * conv1x1(x, wd; stride s) + bd
//   out = leaky( z + id , slope_out )
// x [M][Cin][H][W] -> out [M][128][H2][W2], H2 = (H - 1) / s + 1, W2 = (W - 1) / s + 1; m, z and id never exist in memory. The
// norms are folded into (s, b) on the host (mmp_stem.fold_block4). m outside the H2 x W2 plane is ZERO (the second
// convolution's padding), not leaky(b1). The sibling of nmpc_mmp_block3.h (64 channels), whose building blocks it keeps: the
// flat domain with pixel groups across row ends, the parity split of the strided input tile, m written over the dead input
// chunk, the projection in the epilogue. What it does not keep is the tile.
//
// Instructions: v_mfma_f32_16x16x4_f32 as an implicit GEMM, as there. The 128 output channels are EIGHT A operands per tap,
//   A_h = w[co = 16 h + (lane & 15)][ci = 4 g + (lane >> 4)][ky][kx], h = 0 .. 7
//   B   = tile[ci = 4 g + (lane >> 4)][q + off(ky, kx)], q = q0 + (lane & 15)
//   D_h = 4 VGPRs: channel 16 h + 4 (lane >> 4) + r in register r, pixel q0 + (lane & 15)
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
// Decision 3 -- stride-2 taps, as in the sibling: the strided block's input tile is stored split by row and column parity,
// four sub-planes per channel on the same 12 x 13 domain: sub-plane (py, px) at (r, c) holds x[2 (y0 + r) + py][2 (x0 + c) +
// px]. The tap ky reads row parity py = (ky != 1) at the flat offset -13 for ky = 0 and 0 otherwise, likewise kx: ONE flat
// offset into ONE sub-plane. Layout in LDS [sub-plane][channel][176].
// Bank behaviour (ds_read_b32 / ds_write_b32: two groups of 32 lanes, bank = word mod 32): the plane stride kB4P = 176 = 16
// mod 32; a B read takes 16 consecutive words of each of two planes per lane group -- 32 distinct banks wherever the group
// starts, conflict-free. The m store writes, per register r and sixteenth h, channel 16 h + 4 k + r to slot 16 h + 4 r + k: 16
// consecutive words of planes one stride apart -- conflict-free; the second convolution's group g (0 .. 31) then holds the
// channels 16 (g / 4) + (g % 4) + {0, 4, 8, 12}.
// Decision 4 -- LDS and occupancy. 128 slots of m on 176 words are 90 112 B static; the input chunk (32 channels at stride 1 =
// 32 planes, 16 channels at stride 2 = 64 planes; a thread stages 10 / 20 values) is dead when m is written, so m is written
// OVER it behind one more barrier. __launch_bounds__(512, 1): one workgroup per CU, two waves per SIMD, 256 registers per lane.
// A chunk of 32 channels (stride 1) puts 8 x 9 x 4 x 2 = 576 MFMA per wave between two barrier pairs (the sibling: 504); a Cin
// that is no multiple of the chunk stages zeros for the missing channels and skips their MFMAs.
// Decision 5 -- the projection runs in the epilogue on x read again (L2), per pixel group of out, as in the siblings (1 % of
// layer4's fma).
//
// Steps: 512 threads = 8 waves per workgroup; workgroup = [row of the batch][tile row][tile column] flattened in x.
//   1. per chunk of input channels: the chunk's planes global -> registers (issued one chunk ahead, behind the barrier) ->
//      LDS, zero outside the plane; then per group of 4 channels 9 taps x 4 pixel groups x 2 sixteenths of MFMA into the
//      resident accumulators of m
//   2. barrier; m = leaky(fma(s1, acc, b1)), zero outside the plane -> LDS [128 slots][176], and zeros to the positions 0 ..
//      13 and 142 .. 155 of every slot (the ring that no group covers: outside the plane wherever a valid out reads it); barrier
//   3. per group of 4 slots 9 taps x 4 pixel groups x 2 sixteenths of MFMA on the m tile
//   4. per pixel group of out: with a projection Cin / 4 x 2 MFMA on x read again (a lane without a pixel feeds zeros); then
//      out = leaky(fma(s2, acc, b2) + id), id = fma(sd, idacc, bd) or x read again (L2), one dword store per value. No atomics.
// Every word of LDS that is read has been written: an x plane on 0 .. 155 by the staging, an m plane on 14 .. 141 by the
// groups and on the rest of 0 .. 155 by the zeros.
//
// Summation order (fixed): conv1 -- input channels in groups of four ascending, per group the nine taps ky-major, per tap
// the four channels ascending (the instruction's k order); the projection -- input channels ascending; conv2 -- channel
// groups 16 (g / 4) + (g % 4) + {0, 4, 8, 12}, g = 0 .. 31 ascending, per group the taps ky-major, per tap the four channels
// ascending; then one fma per affine and one addition z + id. A row's bits depend on that row of x and the weights only: not
// on M, the row's position, the launch or the alignment of out.
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
// Compiler (hipcc -O3 --offload-arch=gfx950; tools/kernel_resources.py on the shipped code object): mmp_blk4_kernel<2, true>
// 124 VGPRs, 94 SGPRs; <1, true> 102 VGPRs, 84 SGPRs; <1, false> 102 VGPRs, 71 SGPRs; all 0 AGPRs, no VGPR or SGPR spills,
// scratch 0, 90 112 B LDS, code 16-28 KB, occupancy one workgroup = 2 waves per SIMD (LDS decides; registers would allow more).
// tests/test_mmp_block4_cpu.py holds every kernel of this family to that.
#pragma once

#include <hip/hip_runtime.h>

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

typedef float mmp_b4_f4 __attribute__((ext_vector_type(4)));

// tiles along a side of n outputs that holds m of them in one tile and t = m - 2 per tile otherwise (host and tests)
__host__ __device__ constexpr long long mmp_b4_tiles(long long n, int m) { return n <= m ? 1 : (n + m - 3) / (m - 2); }

template <int STRIDE, bool PROJ>
__global__ __launch_bounds__(kB4Threads, 1) void mmp_blk4_kernel(MmpBlock4Params p)
{
    static_assert(STRIDE == 1 || STRIDE == 2, "stride");
    constexpr int CC = STRIDE == 2 ? 16 : 32;          // input channels per chunk
    constexpr int NPL = CC * STRIDE * STRIDE;          // planes per chunk: [sub-plane][channel]
    constexpr int NV = NPL * kB4Q;                     // values per chunk
    constexpr int PRE = (NV + kB4Threads - 1) / kB4Threads; // tile values a thread stages per chunk: 10 / 20
    static_assert(NPL <= kB4C, "the chunk does not fit under m");
    __shared__ float lds[kB4Lds];
    float* const xs = lds;       // [NPL][176]: position q of a plane at q
    float* const ms = lds;       // [128 slots][176]; written over the last chunk

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pw = wave >> 2, hb = 2 * (wave & 3);   // the wave's parity of pixel groups; its first channel sixteenth
    const int col = tid & 15, k = (tid >> 4) & 3;
    const int tiles = p.tx * p.ty;
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    if (n >= p.M) return; // (workgroup-uniform, in front of every barrier)
    const int tyi = tile / p.tx, txi = tile - tyi * p.tx;
    const int gy0 = tyi * kB4TH - p.oy, gx0 = txi * kB4TW - p.ox; // the output pixel of position 0 (one tile: -1)
    const size_t plane = (size_t)p.H * p.W, plane2 = (size_t)p.H2 * p.W2;
    const float* xn = p.x + (size_t)n * p.Cin * plane;

    float pre[PRE];
    auto fetch = [&](int c0) {
        int t0 = tid;
        // (the addresses and masks are worked out again per chunk, not kept across the MFMAs as loop invariants)
        asm volatile("" : "+v"(t0));
#pragma unroll
        for (int e = 0; e < PRE; ++e) {
            const int i = t0 + e * kB4Threads;
            const int pl = i / kB4Q, q = i - pl * kB4Q;
            const int sub = pl / CC, ch = pl - sub * CC;
            const int y = STRIDE * (gy0 + q / kB4S) + sub / 2, xx = STRIDE * (gx0 + q % kB4S) + sub % 2;
            const bool in = i < NV && c0 + ch < p.Cin && y >= 0 && y < p.H && xx >= 0 && xx < p.W;
            pre[e] = in ? xn[(size_t)(c0 + ch) * plane + (size_t)y * p.W + xx] : 0.0f;
        }
    };

    const mmp_b4_f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    mmp_b4_f4 acc[kB4NI][kB4NH];
    int gq[kB4NI]; // the wave's pixel groups: first position + col
#pragma unroll
    for (int i = 0; i < kB4NI; ++i) {
        gq[i] = kB4M0 + 16 * (pw + 2 * i) + col;
#pragma unroll
        for (int h = 0; h < kB4NH; ++h) acc[i][h] = zero;
    }

    // ---- 1. the first convolution, the input streamed in chunks
    fetch(0);
    for (int c0 = 0; c0 < p.Cin; c0 += CC) {
        __syncthreads(); // the previous chunk has been read
#pragma unroll
        for (int e = 0; e < PRE; ++e) {
            const int i = tid + e * kB4Threads;
            const int pl = i / kB4Q, q = i - pl * kB4Q;
            if (i < NV) xs[pl * kB4P + q] = pre[e];
        }
        __syncthreads();
        if (c0 + CC < p.Cin) fetch(c0 + CC);
        for (int cg = 0; cg < CC / 4; ++cg) {
            if (c0 + 4 * cg >= p.Cin) break; // (Cin is a multiple of 8, a chunk holds 16 or 32: uniform)
            const int ci = c0 + 4 * cg + k;
            float a[kB4NH][9];
#pragma unroll
            for (int h = 0; h < kB4NH; ++h) {
                const float* wp = p.w1 + ((size_t)(16 * (hb + h) + col) * p.Cin + ci) * 9;
#pragma unroll
                for (int t = 0; t < 9; ++t) a[h][t] = wp[t];
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ky = t / 3, kx = t % 3;
                const int sub = STRIDE == 2 ? 2 * (ky != 1) + (kx != 1) : 0;
                const int off = STRIDE == 2 ? (ky == 0 ? -kB4S : 0) + (kx == 0 ? -1 : 0) : (ky - 1) * kB4S + (kx - 1);
                const float* xb = xs + (sub * CC + 4 * cg + k) * kB4P + off;
#pragma unroll
                for (int i = 0; i < kB4NI; ++i) {
                    const float b = xb[gq[i]];
#pragma unroll
                    for (int h = 0; h < kB4NH; ++h) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h][t], b, acc[i][h], 0, 0, 0);
                }
            }
        }
    }

    // ---- 2. m -> LDS over the last chunk, zero outside the plane; zeros to what no group covers
    __syncthreads(); // the last chunk has been read
#pragma unroll
    for (int h = 0; h < kB4NH; ++h) {
        float s[4], sh[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] = p.s1[16 * (hb + h) + 4 * k + r], sh[r] = p.b1[16 * (hb + h) + 4 * k + r];
#pragma unroll
        for (int i = 0; i < kB4NI; ++i) {
            const int q = gq[i];
            const int y = gy0 + q / kB4S, xx = gx0 + q % kB4S;
            const bool in = y >= 0 && y < p.H2 && xx >= 0 && xx < p.W2;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = fmaf(s[r], acc[i][h][r], sh[r]);
                ms[(16 * (hb + h) + 4 * r + k) * kB4P + q] = in ? (v > 0.0f ? v : v * p.slope_mid) : 0.0f;
            }
        }
    }
    for (int i = tid; i < kB4C * kB4Ring; i += kB4Threads) {
        const int slot = i / kB4Ring, j = i - slot * kB4Ring;
        ms[slot * kB4P + (j < kB4M0 ? j : kB4M1 - kB4M0 + j)] = 0.0f;
    }
    __syncthreads();

    // ---- 3. the second convolution on the m tile (the groups of out are the groups of m)
#pragma unroll
    for (int i = 0; i < kB4NI; ++i)
#pragma unroll
        for (int h = 0; h < kB4NH; ++h) acc[i][h] = zero;
    for (int g = 0; g < kB4C / 4; ++g) {
        const int ch = 16 * (g / 4) + 4 * k + (g % 4); // slot 4 g + k holds this channel
        float a[kB4NH][9];
#pragma unroll
        for (int h = 0; h < kB4NH; ++h) {
            const float* wp = p.w2 + ((16 * (hb + h) + col) * kB4C + ch) * 9;
#pragma unroll
            for (int t = 0; t < 9; ++t) a[h][t] = wp[t];
        }
        const float* mb = ms + (4 * g + k) * kB4P;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int off = (t / 3 - 1) * kB4S + (t % 3 - 1);
#pragma unroll
            for (int i = 0; i < kB4NI; ++i) {
                const float b = mb[gq[i] + off];
#pragma unroll
                for (int h = 0; h < kB4NH; ++h) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h][t], b, acc[i][h], 0, 0, 0);
            }
        }
    }

    // ---- 4. the projection, the affine, the identity, the activation and the store
    float* on = p.out + (size_t)n * kB4C * plane2;
#pragma unroll
    for (int i = 0; i < kB4NI; ++i) {
        const int q = gq[i];
        const int r0 = q / kB4S, c = q - r0 * kB4S;
        const int y = gy0 + r0, xx = gx0 + c;
        const bool valid = r0 >= p.oy && r0 < kB4R - p.oy && c >= p.ox && c < kB4S - p.ox && y < p.H2 && xx < p.W2; // (then y, xx >= 0)
        mmp_b4_f4 idacc[kB4NH] = {zero, zero};
        if (PROJ) { // (every lane takes part in the MFMAs; a lane without a pixel feeds zeros)
            const float* xc = xn + (size_t)k * plane + (valid ? (size_t)(STRIDE * y) * p.W + STRIDE * xx : (size_t)0);
            for (int c0 = 0; c0 < p.Cin; c0 += 4) {
                const float b = valid ? xc[(size_t)c0 * plane] : 0.0f;
#pragma unroll
                for (int h = 0; h < kB4NH; ++h)
                    idacc[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(p.wd[(16 * (hb + h) + col) * p.Cin + c0 + k], b, idacc[h], 0, 0, 0);
            }
        }
        if (!valid) continue;
        const size_t pix = (size_t)y * p.W2 + xx;
#pragma unroll
        for (int h = 0; h < kB4NH; ++h)
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
