// nmpc_mmp_head.h -- the end of the multi-hypothesis predictor's network (the reference's ConvMultiHypoNet(lite=True),
// net_module/net.py:106-143, module_wta.py:18-48: AvgPool2d(2, 2), flatten, Linear(F, 128), LeakyReLU, Linear(128, 2 K)) in
// one launch ("next" row f5, predictor `mmp`, opt-in), float32 in and out:
//   p[c][i][j] = 0.25 * ((x[c][2i][2j] + x[c][2i][2j+1]) + (x[c][2i+1][2j] + x[c][2i+1][2j+1])),  i < H / 2, j < W / 2
//   f          = leaky( W1 * flat(p) + c1 , slope )          F = C (H / 2) (W / 2) -> 128, flat index (c (H / 2) + i) (W / 2) + j
//   out        = W2 * f + c2                                 128 -> O
// x [M][C][H][W] -> out [M][O]; p and f never exist in memory. An odd last row or column of x is NOT READ.
//
// Plainly: by operation count this is 0.5 % of the network (0.41 M multiply-adds per row), and what it moves is W1, 1.6 MB
// for F = 3 200. One workgroup takes kHeadRows = 16 rows of the batch, so W1 is read once per 16 rows (from L2, where it
// stays: 1 280 groups x 1.6 MB = 2.1 GB at B = 256, 4 pedestrians, N_hor = 20) and x once (1.15 GB from memory). The rows are
// the N side of v_mfma_f32_16x16x4_f32:
//   first layer:  A_h = W1[16 h + (lane & 15)][feature], B = p[row n0 + (lane & 15)][feature], four features per instruction (which
//                 four: below), p pooled from x into LDS;
//   f -> LDS, one barrier;
//   second layer: A = W2[16 t + (lane & 15)][4 g + (lane >> 4)], B = f from LDS (16 consecutive words of two features 16 words apart per
//                 32 lanes: conflict-free; the stores of the partial sums are two-way conflicts, 8 instructions per lane in all),
//                 wave w the output sixteenths t = w, w + 16, ...; rows o >= O of A are zeros and are not stored.
// What bounds it is not the traffic but how it is asked for, and how few workgroups a chunk gives: a default chunk of 22
// pedestrians is 440 rows = 28 workgroups on 256 CUs, one launch after the other. Two earlier shapes, both MEASURED (DESIGN.md
// section 7): (1) 256 threads, wave w the features 32 w .. 32 w + 31 over all F / 4 = 800 steps, every lane pooling its own B
// value from four dword loads of x and loading its A values as dwords: 0.386 ms per chunk = 18.0 ms per lock-step, 6.5 x
// torch's own pool and linear layers (2.75 ms); (2) the same loads from 16 waves with the first sum in four parts and eight
// steps' loads in flight: 24.1 ms -- slower, so it was not a chain of latencies. What both ask of a CU's one vector-memory
// path is cache lines: a load of x by 16 rows x 4 features touches some 16 lines, 800 steps x 4 loads x 4 feature quarters
// = 205 000 line requests per workgroup, and a dword load of W1 by 16 rows of it another 16 lines, 102 000 more: 307 000
// requests at about one a cycle are 0.13 ms per chunk whatever the waves do. Hence the shape here, 1 024 threads = 16 waves:
//   - x is pooled ONCE per workgroup into LDS in chunks of kHeadChunk = 512 features x 16 rows, consecutive lanes taking
//     consecutive features of a row (a load touches 5 to 6 lines): 3 200 loads, some 19 000 requests;
//   - the lane's A values are FOUR consecutive features in one 16-byte load, 16 t + 4 k + e for e = 0 .. 3, so the k side of
//     the MFMA of (t, e) is the features 16 t + e + {0, 4, 8, 12} (B is staged in that order: slot 16 t + 4 e + k): 1 600 loads,
//     25 600 requests; where F is no multiple of 4 or W1 is not 16-byte aligned the same values come in four dword loads;
//   - wave = 4 part + quarter: the features-out 32 quarter .. + 31 (two A operands) for the kHeadT = 8 groups of sixteen
//     features 8 part .. 8 part + 7 of every chunk; the four partial sums are added through LDS in a fixed order.
// Modelled from that count: 45 000 requests = 19 us per chunk, 0.9 ms per lock-step. MEASURED: 0.095 ms per chunk = 4.43 ms per
// lock-step (profiles/mmp_layer4_evaluate.json), a quarter of shape (1) and a fifth of (2), and still 1.50 x torch's 2.95 ms and
// 5 x this model: what the count leaves out, from the code and not from counters, is seven chunks of two barriers each on a
// workgroup of 16 waves, the 2 divisions per staged value, and a launch of 28 workgroups that ends with its slowest. LDS: a staged feature is 17 words (16
// rows and one of padding: the staging writes consecutive features, 17 words apart, conflict-free; a B read is 16 consecutive
// words of two slots 17 apart per 32 lanes, one bank shared by two lanes), 34 816 B, beside the 32 768 B of partial sums.
//
// Summation order (fixed): p as written above; the first sum in kHeadSplit = 4 parts, part q over the groups of sixteen
// features 16 t .. 16 t + 15 with (t mod 32) / 8 = q, t ascending, within a group four instructions e = 0 .. 3 that add the
// features 16 t + e, + 4, + 8, + 12 in that order (the instruction's k order), starting from 0; then ((part 0 + part 1) + part
// 2) + part 3, one addition of c1 and the slope; the second sum over the 128 features ascending in steps of four, starting
// from 0, then one addition of c2. Features f >= F are zeros on both sides. A row's bits depend on that row of x and the
// weights only (a column of D depends on the same column of B only): not on M, the row's position in its group of 16, or the
// alignment of out, x or the weights. No atomics.
#pragma once

#include <hip/hip_runtime.h>

namespace nmpc {

struct MmpHeadParams {
    int M, C, H, W, O, F;                            // F = C (H / 2) (W / 2)
    const float *x;                                  // [M][C][H][W]
    const float *w1, *c1;                            // [128][F], [128]
    const float *w2, *c2;                            // [O][128], [O]
    float slope;
    float* out;                                      // [M][O]
};

constexpr int kHeadThreads = 1024;
constexpr int kHeadRows = 16;                        // rows of the batch per workgroup: the N side of the MFMA
constexpr int kHeadFeatures = 128;                   // outputs of the first linear layer
constexpr int kHeadSplit = 4;                        // parts of the first sum: wave = 4 part + feature quarter
constexpr int kHeadChunk = 512;                      // pooled features staged in LDS at a time
constexpr int kHeadT = kHeadChunk / 16 / kHeadSplit; // groups of sixteen features per wave and chunk: 8
constexpr int kHeadPS = kHeadRows + 1;               // words per staged feature: 16 rows and one of padding (the staging's banks)

typedef float mmp_head_f4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kHeadThreads) void mmp_head_kernel(MmpHeadParams p)
{
    __shared__ float pl[kHeadChunk * kHeadPS];                  // the pooled chunk [slot][17]; feature 16 t + 4 k + e of it in slot 16 t + 4 e + k
    __shared__ float ps[kHeadSplit][kHeadFeatures * kHeadRows]; // the partial sums [part][feature][row]; f in ps[0] afterwards
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hq = wave & 3, part = wave >> 2;
    const int col = tid & 15, k = (tid >> 4) & 3;
    const int row0 = blockIdx.x * kHeadRows, row = row0 + col;
    const bool live = row < p.M;
    const int Hp = p.H / 2, Wp = p.W / 2, HW = Hp * Wp;
    const size_t xrow = (size_t)p.C * p.H * p.W;
    const mmp_head_f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};

    // ---- 1. the first linear layer, the pooled features staged in chunks
    mmp_head_f4 acc[2] = {zero, zero};
    const float* wa = p.w1 + (size_t)(32 * hq + col) * p.F;
    const float* wb = wa + (size_t)16 * p.F;
    // four weights in one load where every row of W1 allows it (the same values either way)
    const bool wide = p.F % 4 == 0 && reinterpret_cast<uintptr_t>(p.w1) % 16 == 0;
    for (int f0 = 0; f0 < p.F; f0 += kHeadChunk) {
        // the wave's weights of this chunk: lane (col, k) holds the features 16 t + 4 k + e, e = 0 .. 3 (issued in front of the staging)
        mmp_head_f4 a0[kHeadT], a1[kHeadT];
#pragma unroll
        for (int tt = 0; tt < kHeadT; ++tt) {
            const int f = f0 + 16 * (kHeadT * part + tt) + 4 * k;
            if (wide) {
                a0[tt] = f < p.F ? *reinterpret_cast<const mmp_head_f4*>(wa + f) : zero;
                a1[tt] = f < p.F ? *reinterpret_cast<const mmp_head_f4*>(wb + f) : zero;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) a0[tt][e] = f + e < p.F ? wa[f + e] : 0.0f, a1[tt][e] = f + e < p.F ? wb[f + e] : 0.0f;
            }
        }
        __syncthreads(); // the previous chunk has been read
        for (int e = tid; e < kHeadRows * kHeadChunk; e += kHeadThreads) {
            const int r = e / kHeadChunk, fl = e - r * kHeadChunk, f = f0 + fl; // (consecutive lanes: consecutive features of a row)
            float v = 0.0f;
            if (f < p.F && row0 + r < p.M) {
                const int c = f / HW, rem = f - c * HW, i = rem / Wp, j = rem - i * Wp;
                const float* xp = p.x + (size_t)(row0 + r) * xrow + ((size_t)(c * p.H + 2 * i) * p.W + 2 * j);
                v = 0.25f * ((xp[0] + xp[1]) + (xp[p.W] + xp[p.W + 1]));
            }
            pl[((fl & ~15) + 4 * (fl & 3) + ((fl >> 2) & 3)) * kHeadPS + r] = v;
        }
        __syncthreads();
#pragma unroll
        for (int tt = 0; tt < kHeadT; ++tt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float b = pl[(16 * (kHeadT * part + tt) + 4 * e + k) * kHeadPS + col];
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[tt][e], b, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[tt][e], b, acc[1], 0, 0, 0);
            }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) ps[part][(32 * hq + 16 * h + 4 * k + r) * kHeadRows + col] = acc[h][r];
    __syncthreads();
    for (int e = tid; e < kHeadFeatures * kHeadRows; e += kHeadThreads) {
        const float v = (((ps[0][e] + ps[1][e]) + ps[2][e]) + ps[3][e]) + p.c1[e / kHeadRows];
        ps[0][e] = v > 0.0f ? v : v * p.slope; // (each element is read and written by one thread)
    }
    __syncthreads();
    const float* fs = ps[0];

    // ---- 2. the second linear layer
    for (int t = wave; 16 * t < p.O; t += kHeadThreads / 64) {
        const int o = 16 * t + col;
        const float* w2 = p.w2 + (size_t)(o < p.O ? o : 0) * kHeadFeatures + k;
        mmp_head_f4 d = zero;
#pragma unroll 8
        for (int g = 0; g < kHeadFeatures / 4; ++g) {
            const float a = o < p.O ? w2[4 * g] : 0.0f;
            d = __builtin_amdgcn_mfma_f32_16x16x4f32(a, fs[(4 * g + k) * kHeadRows + col], d, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int oo = 16 * t + 4 * k + r;
            if (live && oo < p.O) p.out[(size_t)row * p.O + oo] = d[r] + p.c2[oo];
        }
    }
}

} // namespace nmpc
