// nmpc_mmp_block3.h -- one residual block of the multi-hypothesis predictor's third residual stage (resnet34.layer3 of the
// reference's ConvMultiHypoNet(lite=True), net_module/net.py:45-61, submodules.py:21-40: six BasicBlocks at 64 channels, the
// first 32 -> 64 at stride 2 with a 1 x 1, stride-2 projection), fused ("next" row f3, predictor `mmp`, opt-in), float32 in
// and out. The stride s in {1, 2} applies to the first convolution and to the projection only:
//   m   = leaky( s1 * conv3x3(x, w1; stride s, zero padding 1) + b1 , slope_mid )        Cin -> 64, plane H x W -> H2 x W2
//   z   =        s2 * conv3x3(m, w2; stride 1, zero padding 1) + b2                      64 -> 64
//   id  = x  (wd == nullptr: s == 1 and Cin == 64)  |  sd * conv1x1(x, wd; stride s) + bd
//   out = leaky( z + id , slope_out )
// x [M][Cin][H][W] -> out [M][64][H2][W2], H2 = (H - 1) / s + 1, W2 = (W - 1) / s + 1; m, z and id never exist in memory. The
// norms are folded into (s, b) on the host (mmp_stem.fold_block3). m outside the H2 x W2 plane is ZERO (the second
// convolution's padding), not leaky(b1). The sibling of nmpc_mmp_block2.h (32 channels), whose building blocks it keeps: the
// flat domain, the parity split of the strided input tile, m written over the dead input chunk, the projection in the epilogue.
//
// Instructions: v_mfma_f32_16x16x4_f32 as an implicit GEMM, as there. The 64 output channels are FOUR A operands per tap,
//   A_h = w[co = 16 h + (lane & 15)][ci = 4 g + (lane >> 4)][ky][kx], h = 0 .. 3
//   B   = tile[ci = 4 g + (lane >> 4)][q + off(ky, kx)], q = q0 + (lane & 15)
//   D_h = 4 VGPRs: channel 16 h + 4 (lane >> 4) + r in register r, pixel q0 + (lane & 15)
// and a group of 16 positions is 16 accumulator VGPRs per lane.
//
// Decision 1 -- tile geometry. ONE flat domain of the OUTPUT plane: kB3R x kB3S = 11 x 25 = 275 positions, the tile of 7 x 21
// outputs with a halo of two; position q = 25 r + c is the output pixel (7 ty - 2 + r, 21 tx - 2 + c). The 19 x 21 plane of
// layer3 is one tile wide and three high. The row stride 25 is no multiple of 16: a pixel group is 16 consecutive POSITIONS
// and runs across row ends (every lane works out its own row and column); nothing in the flat-offset taps needs more.
//   m is needed on rows 1 .. 9, columns 1 .. 23: positions 26 .. 248, kB3GM = 14 groups from position 26 (26 + 16 a, a = 0 .. 13);
//   out on rows 2 .. 8, columns 2 .. 22: positions 52 .. 222, covered by the kB3GO = 12 groups a = 1 .. 12 (42 .. 233) of the same grid,
// so a group of out is a group of m and out, and the identity added to it, sit in the lane and register that held m of the
// same pixel. Positions in the two halo columns on either side (0, 1, 23, 24 for out; 0, 24 for m) are computed from wrapped
// neighbours and never stored or used (a column of D depends on the same column of B only).
// The alternatives, for the 19 x 21 plane and a 64 -> 64 block (useful = 2 x 399 / 16 = 49.9 group-convolutions per row):
//   - the whole plane in one workgroup of 512 threads: 23 x 25 = 575 positions, m 33 groups + out 30; 8 waves take 5 + 4 each:
//     72 issued, 69 % useful -- but m is 147 456 B, ONE workgroup per CU, and every barrier (two per chunk, one in front of
//     the m store) and every epilogue then stops the whole CU's MFMA pipes. The siblings' 1.8 x over their models is
//     believed to be exactly such stops with TWO workgroups per CU; with one there is nothing to fill them.
//   - three tiles of 7 rows, 256 threads, two workgroups per CU (m 77 824 B): 14 + 12 = 26 groups per tile, 78 issued, 64 %
//     useful. BUILT: 8 % more MFMAs issued than the whole plane, and a second workgroup to run while one waits.
// Decision 2 -- the waves. 14 and 12 groups do not divide by four waves, and four A operands per B read in every wave would
// round them to 16 + 12 (59 %). So the workgroup's four waves are 2 x 2: wave = 2 pw + hw computes the channel halves
// 2 hw, 2 hw + 1 (32 channels: TWO A operands per ds_read_b32, as in the 32-channel kernel -- one LDS instruction per 2 048
// fma, which is what that kernel runs at) for the groups of parity pw: 7 groups of m and 6 of out each, exactly. Group j of m
// (wave parity j & 1, index j >> 1) is a = j + 1 for j < 12 (the groups of out first), a = 0 for j = 12, a = 13 for j = 13.
// 7 x 2 x 4 = 56 accumulator VGPRs per lane.
// Decision 3 -- stride-2 taps, as in the sibling: the strided block's input tile is stored split by row and column parity,
// four sub-planes per channel on the same 11 x 25 domain: sub-plane (py, px) at (r, c) holds x[2 (7 ty - 2 + r) + py][2 (21 tx
// - 2 + c) + px]. The tap ky reads row parity py = (ky != 1) at the flat offset -25 for ky = 0 and 0 otherwise, likewise kx:
// ONE flat offset into ONE sub-plane. Layout in LDS [sub-plane][channel][304].
// Bank behaviour (ds_read_b32 / ds_write_b32: two groups of 32 lanes, bank = word mod 32): the plane stride kB3P = 304 = 16
// mod 32; a B read takes 16 consecutive words of each of two planes per lane group -- 32 distinct banks wherever the group
// starts, conflict-free. The m store writes, per register r and half h, channel 16 h + 4 k + r to slot 16 h + 4 r + k: 16
// consecutive words of planes one stride apart -- conflict-free; the second convolution's group g (0 .. 15) then holds the
// channels 16 (g / 4) + (g % 4) + {0, 4, 8, 12}.
// Decision 4 -- LDS and occupancy. 64 channels of m on 304 words are 77 824 B; the input chunk (16 channels at stride 1 = 16
// planes, 8 channels at stride 2 = 32 planes; a thread stages 18 / 35 values) is dead when m is written, so m is written OVER
// it behind one more barrier: 77 840 B static, two workgroups per CU. __launch_bounds__(256, 2) states it: two waves per SIMD,
// 256 registers per lane. A chunk of 16 channels (stride 1) puts 4 x 9 x 7 x 2 = 504 MFMA per wave between two barrier pairs
// (the sibling: 288); a Cin that is no multiple of 16 stages zeros for the missing channels and skips their MFMAs.
// Decision 5 -- the projection runs in the epilogue on x read again (L2), per pixel group of out, as in the sibling (there
// resident accumulators spilled; here they would fit, and are not built: the projection is 0.5 % of layer3's fma).
//
// Steps: 256 threads = 4 waves per workgroup; workgroup = [row of the batch][tile row][tile column] flattened in x.
//   1. per chunk of input channels: the chunk's planes global -> registers (issued one chunk ahead, behind the barrier) ->
//      LDS, zero outside the plane; then per group of 4 channels 9 taps x 7 pixel groups x 2 halves of MFMA into the resident
//      accumulators of m
//   2. barrier; m = leaky(fma(s1, acc, b1)), zero outside the plane -> LDS [64 slots][304]; barrier
//   3. per group of 4 slots 9 taps x 6 pixel groups x 2 halves of MFMA on the m tile
//   4. per pixel group of out: with a projection Cin / 4 x 2 MFMA on x read again (a lane without a pixel feeds zeros); then
//      out = leaky(fma(s2, acc, b2) + id), id = fma(sd, idacc, bd) or x read again (L2), one dword store per value. No atomics.
// Words of LDS read without being written (positions 16 .. 25 and 250 .. 259 of an m plane, 275 of an x plane) feed wrapped
// columns and the unused ends of the first and last group only; what they hold is discarded.
//
// Summation order (fixed): conv1 -- input channels in groups of four ascending, per group the nine taps ky-major, per tap
// the four channels ascending (the instruction's k order); the projection -- input channels ascending; conv2 -- channel
// groups 16 (g / 4) + (g % 4) + {0, 4, 8, 12}, g = 0 .. 15 ascending, per group the taps ky-major, per tap the four channels
// ascending; then one fma per affine and one addition z + id. A row's bits depend on that row of x and the weights only: not
// on M, the row's position, the launch or the alignment of out.
//
// Modelled before the device run, from the instruction count (four waves on the four SIMDs of a CU: a tile takes as long as
// one wave's MFMAs). Per wave and tile: the strided first block (Cin = 32) 8 channel groups x 9 x 7 x 2 + 6 x 8 x 2 of the
// projection + 16 x 9 x 6 x 2 = 1 008 + 96 + 1 728 = 2 832 MFMA; each of the other five 16 x 126 + 1 728 = 3 744: 21 552 for a tile
// of all six, of 32 cycles each, for 133 (a third of the 399 pixels) x 426 112 useful fma = 13 837 MFMA-equivalents per wave: 64 % useful.
// At B = 256, 4 pedestrians, N_hor = 20 (20 480 rows x 3 tiles over 256 CUs at 2.4 GHz) that is 61 440 x 21 552 x 32 / (256 x
// 2.4e9) = 69 ms per lock-step if the MFMA pipe never waits; 44 ms at the 78.6 T fma/s fp32 peak for the 3.48e12 useful fma
// alone; 4.3 ms for the 27.1 GB (x of the first block once, five reads and six writes of [64][19][21]) at the 6.29 TB/s copy rate.
// Measured (profiles/mmp_layer3_evaluate.json): 121.8 ms, 28.6 T useful fma/s = 36 % of the fp32 peak,
// 0.22 TB/s; torch's own layer3, eager, on the same rows in the same process: 170.4 ms (169-174 over three runs; the kernels
// 121-122). The model is short by 1.77 x (the 32-channel kernel: 1.78 x, the 16-channel one: 1.8 x). The strided block runs at 22.3 T
// fma/s (28 %), the five others at 28.2-29.3 T (36-37 %): with 64 % of the issued MFMAs useful the pipe is busy 56-58 % of the
// time (the 32-channel kernel: 40-43 % at 79 % useful, busy 51-54 %). What is believed to cost the rest, from the code, not from counters: as in the siblings two waves
// per SIMD that stop at two barriers per chunk and at a third in front of the m store, and epilogues without conv MFMAs (here
// 48 dword stores per lane). One experiment: the next channel group's 18 weights loaded under the MFMAs of the group at work,
// in both convolutions (200 / 220 VGPRs): 2.594 ms against 2.618 ms for the six launches on 440 rows, 1 %, the spread between
// runs -- the weight loads are not what waits; not kept. Not built: resident id accumulators (registers are there: 0.5 % of
// the fma), a double-buffered chunk (LDS is not there beside m at two workgroups per CU), the whole-plane workgroup.
//
// Compiler (hipcc -O3 --offload-arch=gfx950; tools/kernel_resources.py on the shipped code object): mmp_blk3_kernel<2, true>
// 196 VGPRs, 105 SGPRs; <1, true> 177 VGPRs, 99 SGPRs; <1, false> 177 VGPRs, 86 SGPRs; all 0 AGPRs, no VGPR or SGPR spills,
// scratch 0, 77 840 B LDS, occupancy 2 waves per SIMD (registers -- at most 256 -- and LDS agree).
// tests/test_mmp_block3_cpu.py holds every kernel of this family to that.
#pragma once

#include <hip/hip_runtime.h>

namespace nmpc {

struct MmpBlock3Params {
    int M, Cin, H, W, H2, W2, tx, ty;                // H, W: the input plane; H2, W2: the output plane; tiles along x, y
    const float *x;                                  // [M][Cin][H][W]
    const float *w1, *s1, *b1;                       // [64][Cin][3][3], [64], [64]
    const float *w2, *s2, *b2;                       // [64][64][3][3], [64], [64]
    const float *wd, *sd, *bd;                       // [64][Cin], [64], [64] (kernel <., true>) or unused
    float slope_mid, slope_out;
    float* out;                                      // [M][64][H2][W2]
};

constexpr int kB3Threads = 256;
constexpr int kB3C = 64;                             // output channels
constexpr int kB3NH = 2;                             // A operands per tap and wave: the wave's two channel halves of four
constexpr int kB3TH = 7, kB3TW = 21;                 // outputs per tile
constexpr int kB3S = kB3TW + 4;                      // row stride of the flat domain: 25
constexpr int kB3R = kB3TH + 4;                      // rows of the flat domain: 11
constexpr int kB3Q = kB3R * kB3S;                    // positions of the flat domain: 275
constexpr int kB3P = 304;                            // plane stride in LDS
constexpr int kB3M0 = kB3S + 1;                      // first position of m: 26
constexpr int kB3GM = ((kB3TH + 2) * kB3S - 2 + 15) / 16; // pixel groups of m: positions 26 .. 248 -> 14
constexpr int kB3GO = kB3GM - 2;                     // pixel groups of out: 12 (all of m's but the first and the last)
constexpr int kB3NO = kB3GO / 2;                     // pixel groups of out per wave: 6
constexpr int kB3NI = kB3GM / 2;                     // pixel groups of m per wave: 7
constexpr int kB3Lds = kB3C * kB3P + 4;              // words of static LDS
static_assert(kB3GM % 2 == 0, "the groups do not fit the two wave parities");
static_assert(kB3M0 + 16 <= 2 * kB3S + 2 && kB3M0 + 16 * (kB3GO + 1) >= (kB3TH + 1) * kB3S + kB3TW + 2, "the groups of out do not cover the tile");
static_assert(kB3M0 + 16 * kB3GM + kB3S + 1 <= kB3Q + 1 && kB3M0 + 16 * kB3GM <= kB3Q, "a tap of the last group of m leaves the plane");
static_assert(kB3P % 32 == 16 && kB3P >= kB3Q + 2, "plane stride: bank spread, and the taps of the last group stay inside");
static_assert(kB3Lds * 4 <= 80 * 1024, "static LDS over half a CU's");

// first position of m's pixel group j: the groups of out first (a = 1 .. 12), then the first (a = 0), then the last (a = 13)
__device__ __forceinline__ constexpr int mmp_b3_group(int j) { return kB3M0 + 16 * (j < kB3GO ? j + 1 : j == kB3GO ? 0 : kB3GM - 1); }

typedef float mmp_b3_f4 __attribute__((ext_vector_type(4)));

template <int STRIDE, bool PROJ>
__global__ __launch_bounds__(kB3Threads, 2) void mmp_blk3_kernel(MmpBlock3Params p)
{
    static_assert(STRIDE == 1 || STRIDE == 2, "stride");
    constexpr int CC = STRIDE == 2 ? 8 : 16;           // input channels per chunk
    constexpr int NPL = CC * STRIDE * STRIDE;          // planes per chunk: [sub-plane][channel]
    constexpr int NV = NPL * kB3Q;                     // values per chunk
    constexpr int PRE = (NV + kB3Threads - 1) / kB3Threads; // tile values a thread stages per chunk: 18 / 35
    static_assert(NPL <= kB3C, "the chunk does not fit under m");
    __shared__ float lds[kB3Lds];
    float* const xs = lds + 1;   // [NPL][304]: position q of a plane at 1 + q
    float* const ms = lds;       // [64 slots][304]: position q at q; written over the last chunk

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pw = wave >> 1, hb = 2 * (wave & 1);   // the wave's parity of pixel groups; its first channel half
    const int col = tid & 15, k = (tid >> 4) & 3;
    const int tiles = p.tx * p.ty;
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    if (n >= p.M) return; // (workgroup-uniform, in front of every barrier)
    const int tyi = tile / p.tx, txi = tile - tyi * p.tx;
    const int gy0 = tyi * kB3TH - 2, gx0 = txi * kB3TW - 2; // the output pixel of position 0
    const size_t plane = (size_t)p.H * p.W, plane2 = (size_t)p.H2 * p.W2;
    const float* xn = p.x + (size_t)n * p.Cin * plane;

    float pre[PRE];
    auto fetch = [&](int c0) {
        int t0 = tid;
        // (the addresses and masks are worked out again per chunk, not kept across the MFMAs as loop invariants)
        asm volatile("" : "+v"(t0));
#pragma unroll
        for (int e = 0; e < PRE; ++e) {
            const int i = t0 + e * kB3Threads;
            const int pl = i / kB3Q, q = i - pl * kB3Q;
            const int sub = pl / CC, ch = pl - sub * CC;
            const int y = STRIDE * (gy0 + q / kB3S) + sub / 2, xx = STRIDE * (gx0 + q % kB3S) + sub % 2;
            const bool in = i < NV && c0 + ch < p.Cin && y >= 0 && y < p.H && xx >= 0 && xx < p.W;
            pre[e] = in ? xn[(size_t)(c0 + ch) * plane + (size_t)y * p.W + xx] : 0.0f;
        }
    };

    const mmp_b3_f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    mmp_b3_f4 acc[kB3NI][kB3NH];
    int gq[kB3NI]; // the wave's pixel groups: first position + col
#pragma unroll
    for (int i = 0; i < kB3NI; ++i) {
        gq[i] = mmp_b3_group(pw + 2 * i) + col;
#pragma unroll
        for (int h = 0; h < kB3NH; ++h) acc[i][h] = zero;
    }

    // ---- 1. the first convolution, the input streamed in chunks
    fetch(0);
    for (int c0 = 0; c0 < p.Cin; c0 += CC) {
        __syncthreads(); // the previous chunk has been read
#pragma unroll
        for (int e = 0; e < PRE; ++e) {
            const int i = tid + e * kB3Threads;
            const int pl = i / kB3Q, q = i - pl * kB3Q;
            if (i < NV) xs[pl * kB3P + q] = pre[e];
        }
        __syncthreads();
        if (c0 + CC < p.Cin) fetch(c0 + CC);
        for (int cg = 0; cg < CC / 4; ++cg) {
            if (c0 + 4 * cg >= p.Cin) break; // (Cin is a multiple of 8, a stride-1 chunk holds 16: uniform)
            const int ci = c0 + 4 * cg + k;
            float a[kB3NH][9];
#pragma unroll
            for (int h = 0; h < kB3NH; ++h) {
                const float* wp = p.w1 + ((size_t)(16 * (hb + h) + col) * p.Cin + ci) * 9;
#pragma unroll
                for (int t = 0; t < 9; ++t) a[h][t] = wp[t];
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ky = t / 3, kx = t % 3;
                const int sub = STRIDE == 2 ? 2 * (ky != 1) + (kx != 1) : 0;
                const int off = STRIDE == 2 ? (ky == 0 ? -kB3S : 0) + (kx == 0 ? -1 : 0) : (ky - 1) * kB3S + (kx - 1);
                const float* xb = xs + (sub * CC + 4 * cg + k) * kB3P + off;
#pragma unroll
                for (int i = 0; i < kB3NI; ++i) {
                    const float b = xb[gq[i]];
#pragma unroll
                    for (int h = 0; h < kB3NH; ++h) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h][t], b, acc[i][h], 0, 0, 0);
                }
            }
        }
    }

    // ---- 2. m -> LDS over the last chunk, zero outside the plane
    __syncthreads(); // the last chunk has been read
#pragma unroll
    for (int h = 0; h < kB3NH; ++h) {
        float s[4], sh[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] = p.s1[16 * (hb + h) + 4 * k + r], sh[r] = p.b1[16 * (hb + h) + 4 * k + r];
#pragma unroll
        for (int i = 0; i < kB3NI; ++i) {
            const int q = gq[i];
            const int y = gy0 + q / kB3S, xx = gx0 + q % kB3S;
            const bool in = y >= 0 && y < p.H2 && xx >= 0 && xx < p.W2;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = fmaf(s[r], acc[i][h][r], sh[r]);
                ms[(16 * (hb + h) + 4 * r + k) * kB3P + q] = in ? (v > 0.0f ? v : v * p.slope_mid) : 0.0f;
            }
        }
    }
    __syncthreads();

    // ---- 3. the second convolution on the m tile (the wave's groups of out are its first kB3NO groups of m)
#pragma unroll
    for (int i = 0; i < kB3NO; ++i)
#pragma unroll
        for (int h = 0; h < kB3NH; ++h) acc[i][h] = zero;
    for (int g = 0; g < kB3C / 4; ++g) {
        const int ch = 16 * (g / 4) + 4 * k + (g % 4); // slot 4 g + k holds this channel
        float a[kB3NH][9];
#pragma unroll
        for (int h = 0; h < kB3NH; ++h) {
            const float* wp = p.w2 + ((16 * (hb + h) + col) * kB3C + ch) * 9;
#pragma unroll
            for (int t = 0; t < 9; ++t) a[h][t] = wp[t];
        }
        const float* mb = ms + (4 * g + k) * kB3P;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int off = (t / 3 - 1) * kB3S + (t % 3 - 1);
#pragma unroll
            for (int i = 0; i < kB3NO; ++i) {
                const float b = mb[gq[i] + off];
#pragma unroll
                for (int h = 0; h < kB3NH; ++h) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h][t], b, acc[i][h], 0, 0, 0);
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
        if (PROJ) { // (every lane takes part in the MFMAs; a lane without a pixel feeds zeros)
            const float* xc = xn + (size_t)k * plane + (valid ? (size_t)(STRIDE * y) * p.W + STRIDE * xx : (size_t)0);
            for (int c0 = 0; c0 < p.Cin; c0 += 4) {
                const float b = valid ? xc[(size_t)c0 * plane] : 0.0f;
#pragma unroll
                for (int h = 0; h < kB3NH; ++h)
                    idacc[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(p.wd[(16 * (hb + h) + col) * p.Cin + c0 + k], b, idacc[h], 0, 0, 0);
            }
        }
        if (!valid) continue;
        const size_t pix = (size_t)y * p.W2 + xx;
#pragma unroll
        for (int h = 0; h < kB3NH; ++h)
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
