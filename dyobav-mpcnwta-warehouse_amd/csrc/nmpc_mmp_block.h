// nmpc_mmp_block.h -- one residual block of the multi-hypothesis predictor's first residual stage (resnet34.layer1 of the
// reference's ConvMultiHypoNet(lite=True), net_module/net.py:45-61, submodules.py:21-40), fused ("next" row f3, predictor
// `mmp`, opt-in), float32 in and out:
//   m   = leaky( s1 * conv3x3(x, w1; stride 1, zero padding 1) + b1 , slope_mid )        Cin -> 16
//   z   =        s2 * conv3x3(m, w2; stride 1, zero padding 1) + b2                      16 -> 16
//   id  = x  (wd == nullptr, Cin == 16)  |  sd * conv1x1(x, wd) + bd                     (the first block's `downsample`)
//   out = leaky( z + id , slope_out )
// x [M][Cin][H][W] -> out [M][16][H][W]; m, z and id never exist in memory. The norms are folded into (s, b) on the host
// (mmp_stem.fold_block). m outside the plane is ZERO (the second convolution's padding), not leaky(b1). The later stages share ONE
// kernel (nmpc_mmp_block_f32.h, which states the flat domain, the fragments and the summation order they have in common with this
// one); this kernel stays on its own: it keeps x and m in two LDS arrays, holds the projection's accumulators resident inside the
// conv1 loop, re-derives its groups of out and has no stride -- a flag each.
//
// Instructions: v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fmaf chain, one rounding per product; 1 024 fma per
// instruction, 32 cycles per SIMD = the vector fp32 rate, and the issue slots stay free for the LDS reads). An implicit
// GEMM: for one tap (ky, kx) and four input channels
//   A = w[co = lane & 15][ci = 4 g + (lane >> 4)][ky][kx]        one VGPR, held for all pixel groups of the wave
//   B = tile[ci = 4 g + (lane >> 4)][q + (ky - 1) S + (kx - 1)], q = q0 + (lane & 15): ONE ds_read_b32 straight from the tile
//   D = 4 VGPRs: channel 4 (lane >> 4) + r in register r, pixel q0 + (lane & 15)
// so one LDS instruction per 1 024 fma (the stem: one per 4). No im2col is built.
//
// Mapping: 256 threads = 4 waves per workgroup; workgroup = [row of the batch][tile row][tile column] flattened in x; a
// tile = 15 x 28 outputs. x, m and out live on ONE flat domain of 19 x 32 positions (the tile with a halo of two, row
// stride S = 32): position q = 32 r + c is the pixel (15 ty - 2 + r, 28 tx - 2 + c). A convolution is then the same flat
// offset (ky - 1) 32 + (kx - 1) at every position, a group of 16 consecutive positions is half a row, and the accumulators
// of m, id and out of one position sit in the same lane and register. m is computed on rows 1 .. 17 (34 groups), out on
// rows 2 .. 16 (30 groups), all 32 columns; columns 0, 1, 30, 31 of out (and 0, 31 of m) are computed from wrapped
// neighbours and never stored or used -- a column of D depends on the same column of B only, so they contaminate nothing.
// Four words of LDS are read without ever being written: index 0 and 609 of the chunk's first and last plane reach (the
// neighbours q = -1 and q = 608 of the first and last group of m) and positions 31 and 576 of every m plane (likewise for out).
// All four are neighbours of wrapped columns only (column 0's left, column 31's right), so whatever they hold is discarded.
// Group j (positions 32 + 16 j ..) belongs to wave j & 3: 9 groups of m, 8 of out per wave (a wave without a 9th / a first
// group recomputes a neighbouring one instead of idling in front of the barrier; the copy is discarded).
//   1. per chunk of 8 input channels (Cin / 8 chunks; the 64 channels of the first block do not fit LDS whole): the chunk's
//      19 x 32 x 8 tile global -> registers (issued one chunk ahead, behind the barrier) -> LDS, zero outside the plane;
//      then per group of 4 channels 9 taps x 9 pixel groups of MFMA into the resident accumulators of m, and with a
//      projection one more per pixel group into those of id (the 1 x 1 convolution reads the centre tap's B)
//   2. m = leaky(fma(s1, acc, b1)), zero outside the plane -> LDS [16][624], channel 4 a + r in slot 4 r + a (the lanes
//      of a store then fall on different banks; the second convolution's group g holds channels g, 4 + g, 8 + g, 12 + g)
//   3. per group of 4 slots 9 taps x 8 pixel groups of MFMA on the m tile
//   4. out = leaky(fma(s2, acc, b2) + id), id = fma(sd, idacc, bd) or x read again (L2), one dword store per value: runs of
//      16 (14 at a tile's edge) consecutive floats, any float-aligned out gives the same bits. No atomics.
// Planes in LDS have a stride of 624 floats (= 16 mod 32: the four channels of a ds_read_b32 fall on disjoint banks).
//
// Summation order (fixed): conv1 -- input channels in groups of four ascending, per group the nine taps ky-major, per tap
// the four channels ascending (the instruction's k order); the projection -- input channels ascending; conv2 -- channel
// groups {g, 4 + g, 8 + g, 12 + g}, g ascending, per group the taps ky-major, per tap the four channels ascending; then one
// fma per affine and one addition z + id. A row's bits depend on that row of x and the weights only: not on M, the row's
// position, the launch or the alignment of out.
//
// Modelled before the device run, from the instruction count: the four waves of a workgroup run on the four SIMDs of a CU, so
// a tile takes as long as one wave's MFMAs. Per wave and tile the first block (Cin = 64) issues 16 channel groups x (9 taps x 9
// pixel groups + 8 of the projection, which is needed on the groups of out only) + 4 x 9 x 8 = 1 712 MFMA, each of the other two 4 x 81 + 288 = 612: 2 936 for a tile of all
// three, of 32 cycles each, for 420 x 21 760 useful fma = 2 231 MFMA-equivalents: 76 % useful (halo rows of m, the four wrapped
// columns, the recomputed copies), and 97 % of a 74 x 83 plane's 15 tiles are filled. At B = 256, 4 pedestrians, N_hor = 20
// (20 480 rows x 15 tiles over 256 CUs at 2.4 GHz) that is 307 200 x 2 936 x 32 / (256 x 2.4e9) = 47 ms per lock-step if the
// MFMA pipe never waits (35 ms at the fp32 peak for the useful fma alone, 10 ms for the 64 GB at the copy rate).
// Measured (profiles/mmp_layer1_evaluate.json): 86 ms, 31.8 T useful fma/s = 40 % of the fp32 peak,
// 0.84 TB/s. The model is short by 1.8 x. What is believed to cost the rest, from the code and one experiment, not from
// counters: the MFMA pipe of a SIMD is fed by two waves (two workgroups per CU) which both stop at two barriers per chunk of
// 8 channels -- 180 MFMA = 5 760 cycles of work between barriers against a global-load latency of the order of 2 000 cycles
// for the chunk that is written to LDS behind the first of them -- and the epilogues (m through LDS, the dword stores) issue
// no MFMA at all. The experiment: the weights of a chunk issued ahead of the tile prefetch and all 36 weights of the second
// convolution loaded before the barrier in front of it -- 86.7 ms against 86.1 ms, no gain, not kept; so the weight loads are
// not what the pipe waits for. A third workgroup per CU (a 4-channel chunk: 50 KB of LDS, but 170 registers) and a
// double-buffered chunk with one barrier are not built.
//
// LDS (static): 8 x 624 x 4 = 19 968 B chunk + 16 x 624 x 4 = 39 936 B m tile = 59 904 B: two workgroups per CU.
// Compiler (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage; __launch_bounds__(256, 2) asks for two
// waves per SIMD, without it the projection kernel takes 189 VGPRs + 100 AGPRs and one): mmp_block_kernel<true> 233 VGPRs,
// 106 SGPRs and 17 SGPR spills; <false> 199 VGPRs, 106 SGPRs and 31 SGPR spills (SGPR spills go to VGPR lanes, v_writelane:
// no memory); both 0 AGPRs, no VGPR spills, scratch 0, 59 904 B LDS, occupancy 2 waves per SIMD (registers and LDS agree).
#pragma once

#include <hip/hip_runtime.h>

namespace nmpc {

struct MmpBlockParams {
    int M, Cin, H, W, tx, ty;                        // tx, ty: tiles per row of the batch along x, y
    const float *x;                                  // [M][Cin][H][W]
    const float *w1, *s1, *b1;                       // [16][Cin][3][3], [16], [16]
    const float *w2, *s2, *b2;                       // [16][16][3][3], [16], [16]
    const float *wd, *sd, *bd;                       // [16][Cin], [16], [16] (kernel <true>) or unused
    float slope_mid, slope_out;
    float* out;                                      // [M][16][H][W]
};

constexpr int kBlkThreads = 256;
constexpr int kBlkC = 16;                            // output channels
constexpr int kBlkTH = 15, kBlkTW = 28;              // outputs per tile
constexpr int kBlkS = kBlkTW + 4;                    // row stride of the flat domain: 32
constexpr int kBlkQ = (kBlkTH + 4) * kBlkS;          // positions of the flat domain: 608
constexpr int kBlkP = 624;                           // plane stride in LDS
constexpr int kBlkCC = 8;                            // input channels per chunk
constexpr int kBlkGM = (kBlkTH + 2) * kBlkS / 16;    // pixel groups of m, from position kBlkS: 34
constexpr int kBlkNI = (kBlkGM + 3) / 4;             // pixel groups of m per wave: 9
constexpr int kBlkGO0 = kBlkS / 16, kBlkGO1 = kBlkGO0 + kBlkTH * kBlkS / 16; // pixel groups of out: 2 .. 31
constexpr int kBlkNO = (kBlkGO1 + 3) / 4;            // pixel groups of out per wave: 8
constexpr int kBlkPre = kBlkCC * kBlkQ / kBlkThreads; // tile values a thread stages per chunk: 19
static_assert(kBlkS == 32 && kBlkCC * kBlkQ % kBlkThreads == 0, "the flat domain does not fit the workgroup");
static_assert(kBlkP % 32 == 16 && kBlkP >= kBlkQ + 2 + 1, "plane stride: bank spread, and the taps of the last group stay inside");
static_assert((kBlkCC + kBlkC) * kBlkP * 4 <= 64 * 1024, "static LDS over 64 KB");

typedef float mmp_blk_f4 __attribute__((ext_vector_type(4)));

template <bool PROJ>
__global__ __launch_bounds__(kBlkThreads, 2) void mmp_block_kernel(MmpBlockParams p)
{
    __shared__ float xs[kBlkCC * kBlkP];   // [8][624]: position q of a channel at 1 + q (the first tap of position 32 is q = -1)
    __shared__ float ms[kBlkC * kBlkP];    // [16 slots][624]: position q at q

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = tid & 15, k = (tid >> 4) & 3;
    const int tiles = p.tx * p.ty;
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    if (n >= p.M) return; // (workgroup-uniform, in front of every barrier)
    const int tyi = tile / p.tx, txi = tile - tyi * p.tx;
    const int gy0 = tyi * kBlkTH - 2, gx0 = txi * kBlkTW - 2; // the pixel of position 0
    const size_t plane = (size_t)p.H * p.W;
    const float* xn = p.x + (size_t)n * p.Cin * plane;

    float pre[kBlkPre];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int e = 0; e < kBlkPre; ++e) {
            const int i = tid + e * kBlkThreads;
            const int ch = i / kBlkQ, q = i - ch * kBlkQ;
            const int y = gy0 + q / kBlkS, xx = gx0 + q % kBlkS;
            const bool in = y >= 0 && y < p.H && xx >= 0 && xx < p.W;
            pre[e] = in ? xn[(size_t)(c0 + ch) * plane + (size_t)y * p.W + xx] : 0.0f;
        }
    };

    const mmp_blk_f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    mmp_blk_f4 acc[kBlkNI], idacc[kBlkNO]; // (id is needed where out is: the wave's first kBlkNO groups)
    int gq[kBlkNI]; // the wave's pixel groups: first position + col
#pragma unroll
    for (int i = 0; i < kBlkNI; ++i) {
        const int j = wave + 4 * i;
        gq[i] = kBlkS + 16 * (j < kBlkGM ? j : kBlkGM - 1) + col;
        acc[i] = zero;
        if (i < kBlkNO) idacc[i] = zero;
    }

    // ---- 1. the first convolution (and the projection), the input streamed in chunks of 8 channels
    fetch(0);
    for (int c0 = 0; c0 < p.Cin; c0 += kBlkCC) {
        __syncthreads(); // the previous chunk has been read
#pragma unroll
        for (int e = 0; e < kBlkPre; ++e) {
            const int i = tid + e * kBlkThreads;
            const int ch = i / kBlkQ, q = i - ch * kBlkQ;
            xs[ch * kBlkP + 1 + q] = pre[e];
        }
        __syncthreads();
        if (c0 + kBlkCC < p.Cin) fetch(c0 + kBlkCC);
#pragma unroll
        for (int cg = 0; cg < kBlkCC / 4; ++cg) {
            const int ci = c0 + 4 * cg + k;
            const float* wp = p.w1 + ((size_t)col * p.Cin + ci) * 9;
            float a[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) a[t] = wp[t];
            float ad = 0.0f;
            if (PROJ) ad = p.wd[col * p.Cin + ci];
            const float* xb = xs + (4 * cg + k) * kBlkP + 1;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int off = (t / 3 - 1) * kBlkS + (t % 3 - 1);
#pragma unroll
                for (int i = 0; i < kBlkNI; ++i) {
                    const float b = xb[gq[i] + off];
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b, acc[i], 0, 0, 0);
                    if (PROJ && t == 4 && i < kBlkNO) idacc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ad, b, idacc[i], 0, 0, 0);
                }
            }
        }
    }

    // ---- 2. m -> LDS, zero outside the plane
    {
        float s[4], sh[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] = p.s1[4 * k + r], sh[r] = p.b1[4 * k + r];
#pragma unroll
        for (int i = 0; i < kBlkNI; ++i) {
            if (wave + 4 * i >= kBlkGM) continue; // (a recomputed copy)
            const int q = gq[i];
            const int y = gy0 + q / kBlkS, xx = gx0 + q % kBlkS;
            const bool in = y >= 0 && y < p.H && xx >= 0 && xx < p.W;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = fmaf(s[r], acc[i][r], sh[r]);
                ms[(4 * r + k) * kBlkP + q] = in ? (v > 0.0f ? v : v * p.slope_mid) : 0.0f;
            }
        }
    }
    __syncthreads();

    // ---- 3. the second convolution on the m tile
#pragma unroll
    for (int i = 0; i < kBlkNO; ++i) {
        const int j = wave + 4 * i;
        gq[i] = kBlkS + 16 * (j < kBlkGO0 ? kBlkGO0 : j) + col;
        acc[i] = zero;
    }
    for (int g = 0; g < 4; ++g) {
        const float* wp = p.w2 + (col * kBlkC + 4 * k + g) * 9; // slot 4 g + k holds channel 4 k + g
        float a[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) a[t] = wp[t];
        const float* mb = ms + (4 * g + k) * kBlkP;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int off = (t / 3 - 1) * kBlkS + (t % 3 - 1);
#pragma unroll
            for (int i = 0; i < kBlkNO; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], mb[gq[i] + off], acc[i], 0, 0, 0);
        }
    }

    // ---- 4. the affine, the identity, the activation and the store
    {
        float s[4], sh[4], sp[4], shp[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[r] = p.s2[4 * k + r], sh[r] = p.b2[4 * k + r];
            sp[r] = PROJ ? p.sd[4 * k + r] : 0.0f, shp[r] = PROJ ? p.bd[4 * k + r] : 0.0f;
        }
        float* on = p.out + (size_t)n * kBlkC * plane;
#pragma unroll
        for (int i = 0; i < kBlkNO; ++i) {
            if (wave + 4 * i < kBlkGO0) continue; // (a recomputed copy)
            const int q = gq[i];
            const int c = q % kBlkS;
            const int y = gy0 + q / kBlkS, xx = gx0 + c; // rows 2 .. 16 of the domain: y >= 0; c >= 2: xx >= 0
            if (c < 2 || c >= 2 + kBlkTW || y >= p.H || xx >= p.W) continue;
            const size_t pix = (size_t)y * p.W + xx;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const size_t o = (size_t)(4 * k + r) * plane + pix;
                const float z = fmaf(s[r], acc[i][r], sh[r]);
                const float id = PROJ ? fmaf(sp[r], idacc[i][r], shp[r]) : xn[o];
                const float v = z + id;
                on[o] = v > 0.0f ? v : v * p.slope_out;
            }
        }
    }
}

} // namespace nmpc
