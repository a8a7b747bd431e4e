// nmpc_mmp_stem.h -- the first layer of the multi-hypothesis predictor's network, fused with the input stack in front of it
// ("next" row f3, predictor `mmp`, opt-in): 7 x 7 / stride 2 / padding 3 convolution of the 7-channel stack -> per-channel
// affine (a folded BatchNorm2d) -> LeakyReLU -> 3 x 3 / stride 2 / padding 1 max-pool, for all n_off time offsets of a
// pedestrian, WITHOUT the stack [n_off][7][Hm][Wm] or the pre-pool activations ever being in memory. The shapes are those
// of the reference's ConvMultiHypoNet(lite=True) (net_module/net.py:24-43, submodules.py:21-27); the trunk behind the pool
// stays the caller's PyTorch.
//
// Identity: channels 0 .. 5 of the stack (nmpc_mmp.h) are the same in all n_off copies and channel 6 is the constant
// t = off + 1, and a convolution is linear, so
//   pre[off][c][oy][ox] = base[c][oy][ox] + t E[c][oy][ox]
//   base = the convolution of channels 0 .. 5 (zero outside the map), once per pedestrian instead of n_off times
//   E    = the sum of the channel-6 weights over the taps that fall inside the map (a constant away from the border)
//   out[off][c][py][px] = max over the pool window, clipped to the conv grid, of leaky(scale[c] pre + shift[c])
// evaluated as z = fma(t, B, A) with A = fma(scale, base, shift) and B = scale * E, both formed once per conv output. Where
// slope >= 0 leaky is non-decreasing, so max(leaky(z_i)) == leaky(max(z_i)) bit for bit and leaky is applied once per
// pooled output (MmpStemParams::mono, workgroup-uniform); a negative slope takes the element-wise form.
//
// The six planes are the float values nmpc_mmp_input_* writes: mmp_gauss / mmp_nearest / mmp_centre of nmpc_mmp.h, the same
// functions, in float64, rounded once to float, per pixel (no separable shortcut). fp32 accumulation in a fixed order (per
// output: input channel, then ky, then kx, one fma chain per output channel), so an item's bits depend on its own hist /
// hcount rows, the map and the weights only: not on the item list, the chunk, n_off or the alignment of out.
//
// Instructions: plain v_fma_f32. K = 294 per output and no reuse of an input value across more than 8 output channels per
// pass: v_mfma_f32_32x32x2_f32 runs at the vector fp32 rate on gfx950 (no gain in FLOP/s), would need the im2col operand
// built in LDS (one more write + read per tap), and packed v_pk_fma_f32 issues at half rate (build.py). So: one conv output
// per thread, 8 output channels per pass = 8 independent fma chains, the 8 weights of a tap read from LDS as two
// broadcast ds_read_b128, the input value as one ds_read_b32. (Tried and measured slower, 1.52 ms against 1.40 ms for 34
// pedestrians: the weights as scalar fma operands, s_load through the constant address space in stages of 28 with the next
// stage's loads issued behind each wait. Scalar loads return out of order, so every wait is for all of them.)
//
// Mapping: 256 threads per workgroup; workgroup = [item][tile row][tile column] flattened in x, a tile = 2 x 24 pooled
// outputs = 5 x 49 conv outputs (245 of 256 threads) = 15 x 103 input pixels.
//   1. threads 0 .. 4: centre and grid maximum of one Gaussian each (float64) -> LDS
//   2. all: the 15 x 103 x 6 input tile -> LDS, ONCE per workgroup, zero outside the map; even and odd columns in separate
//      halves of a row, so that the stride-2 taps of neighbouring lanes are consecutive dwords (no bank conflict)
//   3. per group of 8 output channels (C / 8 groups):
//      a. the group's 8 x 7 x 49 weights -> LDS, transposed to [input channel][ky][kx][8]
//      b. base and E of the thread's conv output for the 8 channels (294 + 49 taps x 8 fma; E from a 0 / 1 mask of the taps
//         inside the map), then A, B -> LDS over the weights (A = -inf, B = 0 outside the conv grid: what PyTorch's max-pool
//         pads with)
//      c. 2 x 24 x 8 = 384 pooled outputs over 256 threads: the 9 (A, B) pairs of the window -> registers, then the walk over
//         the n_off offsets: 9 fma, max, leaky, ONE dword store each -- compute once, store n_off times (mmp_input_kernel)
// Stores: a wave-instruction writes runs of 24 consecutive floats (96 bytes) along px, 2 2/3 runs per instruction; dword
// stores only, so any float-aligned out works and gives the same bits. No atomics.
// LDS (static): 37 440 B input tile + 15 680 B weights / (A, B) + 120 B centres = 53 240 B: three workgroups per CU.
// Compiler (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage): mmp_stem_kernel<float> and <double>
// 132 VGPRs, 0 AGPRs, 94 SGPRs, no spills, no scratch, 53 240 B LDS, occupancy 3 waves per SIMD (registers and LDS agree).
// Not at a hardware bound: 0.77 TB/s stored, 13.1 T fma/s; the halo makes a workgroup compute 1 545
// input pixels (five float64 exp and fifteen float64 divisions each) for 768 it owns.
//
// Binary16 out, opt-in (nmpc_mmp_stem_io_* with out_f16 = 1; MmpFrontEnd(fill="f16")): mmp_stem_kernel<MmpStemH<T>> writes
// out[n_item * n_off][C / 8][Hp][Wp][8], the octet form of nmpc_mmp_block_f16.h, uint16_t bit patterns, the base aligned to 16
// bytes; each value is mmp_blkh_round of exactly the float32 value mmp_stem_kernel<T> computes -- steps 1 .. 3b are the same
// text, and so are the fma order, the pool and the mono / element-wise choice. Only step 3c differs: who holds which outputs.
//   Mapping chosen: lane = [offset parity s < 2][pixel q < 48][half hf < 2], 192 of the 256 threads. A lane holds the 9 (A, B)
//   pairs of the FOUR channels 4 hf .. 4 hf + 3 of the pass's octet at one pooled pixel -- half an octet, as a D fragment of the
//   blocks -- and walks the offsets s, s + 2, ..: per offset 4 x (9 fma, max, leaky), four mmp_blkh_round, ONE 8-byte store.
//   Lanes 2 q and 2 q + 1 store the two halves of a 16-byte slot and consecutive px are consecutive slots, so a tile row is 384
//   contiguous bytes per offset and octet.
//   Counted against it:
//   - registers: 4 x 9 x 2 = 72 VGPRs of (A, B) per lane; a whole octet per lane (one 16-byte store, 48 lanes per parity) is 144
//     and does not fit 168 (three waves per SIMD) beside the rest; two channels per lane would be 4-byte stores.
//   - busy lanes: 192 of 256 for n_off >= 2 (wave 3 idles in 3c); per lane 4 channels x ceil(n_off / 2) offsets = 40 at n_off = 20,
//     what the parent's busiest lanes do (2 items x 20); in wave-instructions 3 x 40 against the parent's (2 + 2 + 1 + 1) x 20: equal.
//     Splitting the offsets by parity is what keeps the walk as short as the parent's with half as many (pixel, channel) owners.
//   - LDS: (A, B) stay [8][NP] as step 3b writes them (shared text), so the re-mapped reads are dwords at (4 hf + c) 245 + (2 pyl +
//     dy) 49 + 2 pxl + dx: bank (20 hf + 34 pyl + 2 pxl + const) mod 64, even offsets only -- 2-way as the parent's stride-2 reads,
//     3-way on the banks where the three ranges overlap (34 .. 46 of 0 .. 62); 72 reads per lane and pass (paired by the compiler
//     into ds_read2_b32 / ds_read_b64) against 343 x 3 in step 3b. A channel-innermost (A, B) would make them 16-byte reads but
//     changes step 3b and with it the float32 kernels' bytes.
//   - stores: 96 lanes x 8 B = 1.5 wave-instructions per tile, pass and offset against 6 of dwords.
//   - scalar registers: the float32 kernels use 94 of 102, and the compiler hoists every workgroup-uniform value of 3c out of the pass
//     loop into more (5 spilled to VGPR lanes when left alone). So the two strides, the weight pointer and the pass count are held
//     in VECTOR registers (mmp_stem_in_vgprs, an opaque v_mov), and the two lane masks (valid in 3b, "has offsets" in 3c) are made
//     pass by pass from a VGPR behind an empty asm instead of being carried as SGPR pairs: 160 VGPRs, 106 SGPRs with VCC, no spills,
//     no scratch, 53 240 B LDS, occupancy 3 (tools/kernel_resources.py; tests/test_mmp_fill_cpu.py). No atomics.
//   The float32 kernels keep their bytes (profiles/mmp_fill_f16_code_object_identity.txt: 292 of 292).
//   Measured (tools/mmp_evaluate_profile.py --fill-f16 -> profiles/mmp_fill_f16_evaluate.json; B = 256, 4 pedestrians, N_hor = 20,
//   both arms on precision = "f16", three runs each in one process): the launch alone 46.8 / 47.7 / 46.9 ms per lock-step ->
//   44.2 / 43.8 / 43.7 (0.92-0.94 x) at 0.37 TB/s stored against 0.68: half the bytes bought 7 %, so the stores were not what
//   bounds this kernel -- the float64 planes of the halo and the fma chains are. The gain is behind it: layer1's first block
//   22.5 -> 12.6 ms per lock-step, and a chunk of 34 pedestrians instead of 22; the stage 128.1 -> 107.7 ms.
#pragma once

#include <hip/hip_runtime.h>

#include "nmpc_mmp.h"
#include "nmpc_mmp_block_f16.h"

namespace nmpc {

struct MmpStemParams {
    int n_item, n_off, Hm, Wm, xr, yr, C, Ho, Wo, Hp, Wp, tx, ty, mono; // tx, ty: tiles per item along px, py
    long long n_ped;                                                  // B * H: rows of hist / hcount
    const long long* items;                                           // [n_item] or nullptr = 0 .. n_item - 1
    const void* hist;                                                 // [B][H][5][2]
    const long long* hcount;                                          // [B][H]
    double scale, offx, offy, xmax, ymax, rescale, s2, k;
    const float* ref;                                                 // [Hm][Wm]
    const float* weight;                                              // [C][7][7][7]
    const float* bn_scale;                                            // [C]
    const float* bn_shift;                                            // [C]
    float slope;
    float* out;                                                       // [n_item][n_off][C][Hp][Wp]; MmpStemH: the octet form
};

constexpr int kStemThreads = 256;
constexpr int kStemTPH = 2, kStemTPW = 24;                            // pooled tile
constexpr int kStemCH = 2 * kStemTPH + 1, kStemCW = 2 * kStemTPW + 1; // conv tile: 5 x 49
constexpr int kStemIH = 2 * kStemCH + 5, kStemIW = 2 * kStemCW + 5;   // input tile: 15 x 103
constexpr int kStemIW2 = (kStemIW + 1) / 2;                           // columns of one parity: 52
constexpr int kStemNP = kStemCH * kStemCW;                            // conv outputs per tile: 245
constexpr int kStemCG = 8;                                            // output channels per pass
constexpr int kStemTaps = 7 * 49;                                     // weights per output channel
constexpr int kStemXs = 6 * kStemIH * 2 * kStemIW2;                   // floats of the input tile
constexpr int kStemWab = 2 * kStemCG * kStemNP;                       // floats of (A, B); the weights (8 x 343) fit inside
constexpr int kStemHQ = 2 * kStemTPH * kStemTPW;                      // binary16 out: (pixel, half octet) pairs of a tile: 96
static_assert(kStemNP <= kStemThreads && kStemCG * kStemTaps <= kStemWab, "tile does not fit the workgroup");
static_assert(kStemCG == 8 && 2 * kStemHQ <= kStemThreads, "a pass is one octet; two offset parities fit the workgroup");
static_assert((kStemXs + kStemWab) * 4 + 5 * 3 * 8 <= 64 * 1024, "static LDS over 64 KB");

__host__ __device__ inline int mmp_stem_out(int n) { return (((n - 1) / 2 + 1) - 1) / 2 + 1; } // conv 7/2/3, then pool 3/2/1

// A workgroup-uniform value kept in vector registers (mmp_stem_kernel<MmpStemH<T>>: the scalar registers are the scarce ones
// there, 94 of 102 before step 3c adds its strides; left to itself the compiler holds them in SGPRs and spills five)
__device__ __forceinline__ size_t mmp_stem_in_vgprs(size_t v)
{
    unsigned lo, hi;
    asm("v_mov_b32 %0, %1" : "=v"(lo) : "s"((unsigned)v));
    asm("v_mov_b32 %0, %1" : "=v"(hi) : "s"((unsigned)(v >> 32)));
    return ((size_t)hi << 32) | lo;
}

// The form of out travels in the kernel's TYPE argument, as the blocks' MmpBlkhIo does: T = float / double is the element type of
// hist with float32 out, and those two kernels keep their names and their bytes; MmpStemH<T> is the same hist with out as
// binary16 in the octet form [n_item * n_off][C / 8][Hp][Wp][8], the base aligned to 16 bytes (step 3c alone differs). The
// params are a true __global__ argument: a body handed them by reference compiles to other bytes (tried: 11 300 B -> 11 256 B).
template <typename T>
struct MmpStemH {
};
template <typename T>
struct mmp_stem_io {
    typedef T Hist;
    static constexpr bool OH = false;
};
template <typename T>
struct mmp_stem_io<MmpStemH<T>> {
    typedef T Hist;
    static constexpr bool OH = true;
};

template <typename TT>
__global__ __launch_bounds__(kStemThreads) void mmp_stem_kernel(MmpStemParams p)
{
    typedef typename mmp_stem_io<TT>::Hist T;
    constexpr bool OH = mmp_stem_io<TT>::OH;
    __shared__ __attribute__((aligned(16))) float xs[kStemXs];   // [6][IH][parity][IW2]
    __shared__ __attribute__((aligned(16))) float wab[kStemWab]; // weights [7 * 49][8], then A [8][NP], B [8][NP]
    __shared__ double cen[5][3];                                 // cx, cy, zmax

    const int tid = threadIdx.x;
    const int tiles = p.tx * p.ty;
    const int item = blockIdx.x / tiles, tile = blockIdx.x - item * tiles;
    if (item >= p.n_item) return;
    const long long ped = p.items ? p.items[item] : item;
    if (ped < 0 || ped >= p.n_ped) return; // (workgroup-uniform, in front of every barrier)
    const int tyi = tile / p.tx, txi = tile - tyi * p.tx;
    const int py0 = tyi * kStemTPH, px0 = txi * kStemTPW;
    const int oy0 = 2 * py0 - 1, ox0 = 2 * px0 - 1; // conv grid
    const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3; // map

    const int n = mmp_distinct(p.hcount[ped]);
    if (tid < 5) {
        const T* hist = static_cast<const T*>(p.hist) + ped * 10;
        double cx, cy;
        mmp_centre(hist, 5 - n + (tid < n - 1 ? tid : n - 1), p.offx, p.offy, p.scale, p.xr, p.xmax, p.yr, p.ymax, p.rescale, cx, cy);
        cen[tid][0] = cx, cen[tid][1] = cy;
        cen[tid][2] = mmp_gauss(mmp_nearest(cx, p.Wm), mmp_nearest(cy, p.Hm), cx, cy, p.s2, p.k);
    }
    __syncthreads();

    // ---- 2. the input tile, once
    for (int pix = tid; pix < kStemIH * kStemIW; pix += kStemThreads) {
        const int r = pix / kStemIW, j = pix - r * kStemIW;
        const int gy = iy0 + r, gx = ix0 + j;
        float v[6];
        if (gy >= 0 && gy < p.Hm && gx >= 0 && gx < p.Wm) {
#pragma unroll
            for (int c = 0; c < 5; ++c) {
                if (c >= n) { // workgroup-uniform; c >= n >= 1
                    v[c] = v[c > 0 ? c - 1 : 0];
                    continue;
                }
                v[c] = (float)(mmp_gauss((double)gx, (double)gy, cen[c][0], cen[c][1], p.s2, p.k) / cen[c][2]);
            }
            v[5] = p.ref[(long long)gy * p.Wm + gx];
        } else {
#pragma unroll
            for (int c = 0; c < 6; ++c) v[c] = 0.0f;
        }
        float* dst = xs + (r * 2 + (j & 1)) * kStemIW2 + (j >> 1);
#pragma unroll
        for (int c = 0; c < 6; ++c) dst[c * (kStemIH * 2 * kStemIW2)] = v[c];
    }

    // the thread's conv output
    const bool has = tid < kStemNP;
    const int oyl = has ? tid / kStemCW : 0, oxl = has ? tid - oyl * kStemCW : 0;
    const int oy = oy0 + oyl, ox = ox0 + oxl;
    const bool valid = has && oy >= 0 && oy < p.Ho && ox >= 0 && ox < p.Wo;
    float cm[7]; // 1 where the tap's column lies inside the map
#pragma unroll
    for (int kx = 0; kx < 7; ++kx) {
        const int gx = ix0 + 2 * oxl + kx;
        cm[kx] = gx >= 0 && gx < p.Wm ? 1.0f : 0.0f;
    }
    const size_t plane = (size_t)p.Hp * p.Wp;
    const float ninf = -__builtin_huge_valf();
    // binary16 out: the thread's share of step 3c, the same for every pass
    // lane = [offset parity hs][pixel q][half hf]: channels 4 hf .. 4 hf + 3 of the octet at one pixel, offsets hs, hs + 2, ..
    int hs = 0, hn = 0, hpos = 0;      // first offset; offsets the lane stores (0: none); (A, B) index of channel 4 hf, tap 0
    mmp_blkh_h4* hdst = nullptr;       // the lane's 8 bytes of octet 0 at offset hs
    size_t hpass = 0, hoff2 = 0;       // from one pass to the next; two offsets on (units of 8 bytes)
    int hng = 0;                       // the passes, C / 8 (read back pass by pass)
    const float* weight = p.weight;    // (binary16 out: the pointer in vector registers too, two SGPRs fewer live through 3b)
    if constexpr (OH) {
        hs = tid / kStemHQ;
        const int r = tid - hs * kStemHQ, q = r >> 1, hf = r & 1;
        const int pyl = q / kStemTPW, pxl = q - pyl * kStemTPW;
        const int py = py0 + pyl, px = px0 + pxl;
        if (hs < 2 && py < p.Hp && px < p.Wp) hn = (p.n_off - hs + 1) >> 1;
        hpos = 4 * hf * kStemNP + 2 * pyl * kStemCW + 2 * pxl;
        hdst = reinterpret_cast<mmp_blkh_h4*>(p.out)
               + 2 * (((size_t)item * p.n_off + hs) * (size_t)(p.C / kStemCG) * plane + (size_t)py * p.Wp + px) + hf;
        hng = p.C / kStemCG;
        asm("" : "+v"(hng));
        weight = reinterpret_cast<const float*>(mmp_stem_in_vgprs(reinterpret_cast<size_t>(p.weight)));
        hpass = mmp_stem_in_vgprs(2 * plane), hoff2 = mmp_stem_in_vgprs(4 * (size_t)(p.C / kStemCG) * plane);
    }

    for (int g = 0; g < (OH ? __builtin_amdgcn_readfirstlane(hng) : p.C / kStemCG); ++g) {
        __syncthreads(); // the input tile is written; the previous group's (A, B) have been read
        // ---- 3a. weights [8][343] -> [343][8]
        const float* wg = weight + (size_t)g * kStemCG * kStemTaps;
        for (int i = tid; i < kStemCG * kStemTaps; i += kStemThreads) {
            const int j = i / kStemTaps, r = i - j * kStemTaps;
            wab[r * kStemCG + j] = wg[i];
        }
        __syncthreads();
        // ---- 3b. base and E
        float acc[kStemCG], e[kStemCG];
#pragma unroll
        for (int j = 0; j < kStemCG; ++j) acc[j] = 0.0f, e[j] = 0.0f;
        if (has) {
            for (int ck = 0; ck < 6 * 7; ++ck) { // (input channel, ky)
                const int ch = ck / 7, ky = ck - ch * 7;
                const float* xr = xs + ((ch * kStemIH + 2 * oyl + ky) * 2) * kStemIW2 + oxl;
                const float* w = wab + ck * 7 * kStemCG;
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const float x = xr[(kx & 1) * kStemIW2 + (kx >> 1)];
#pragma unroll
                    for (int j = 0; j < kStemCG; ++j) acc[j] = fmaf(w[kx * kStemCG + j], x, acc[j]);
                }
            }
            for (int ky = 0; ky < 7; ++ky) {
                const int gy = iy0 + 2 * oyl + ky;
                const float rm = gy >= 0 && gy < p.Hm ? 1.0f : 0.0f;
                const float* w = wab + (6 * 7 + ky) * 7 * kStemCG;
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const float m = rm * cm[kx];
#pragma unroll
                    for (int j = 0; j < kStemCG; ++j) e[j] = fmaf(w[kx * kStemCG + j], m, e[j]);
                }
            }
        }
        __syncthreads(); // every weight has been read: (A, B) go over them
        bool ok = valid;
        if constexpr (OH) {
            int t = valid;
            asm volatile("" : "+v"(t)); // (as n below: the mask is made here, not carried through the passes)
            ok = t != 0;
        }
        if (has) {
#pragma unroll
            for (int j = 0; j < kStemCG; ++j) {
                const float s = p.bn_scale[g * kStemCG + j], sh = p.bn_shift[g * kStemCG + j];
                wab[j * kStemNP + tid] = ok ? fmaf(s, acc[j], sh) : ninf;
                wab[(kStemCG + j) * kStemNP + tid] = ok ? s * e[j] : 0.0f;
            }
        }
        __syncthreads();
        // ---- 3c. pool and store, n_off times
        if constexpr (OH) {
            int n = hn;
            asm volatile("" : "+v"(n)); // (compared here, pass by pass: hoisted, the lane mask is one more pair of live SGPRs)
            if (n > 0) {
                float a[4][9], b[4][9];
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) {
                            const int pos = hpos + c * kStemNP + dy * kStemCW + dx;
                            a[c][dy * 3 + dx] = wab[pos];
                            b[c][dy * 3 + dx] = wab[kStemCG * kStemNP + pos];
                        }
                mmp_blkh_h4* dst = hdst;
                for (int k = 0; k < n; ++k) {
                    const float t = (float)(hs + 2 * k + 1);
                    mmp_blkh_h4 v;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        float m;
                        if (p.mono) {
                            m = fmaf(t, b[c][0], a[c][0]);
#pragma unroll
                            for (int i = 1; i < 9; ++i) m = fmaxf(m, fmaf(t, b[c][i], a[c][i]));
                            m = m > 0.0f ? m : m * p.slope;
                        } else {
                            m = ninf;
#pragma unroll
                            for (int i = 0; i < 9; ++i) {
                                const float z = fmaf(t, b[c][i], a[c][i]);
                                const float w = z > 0.0f ? z : z * p.slope;
                                m = fmaxf(m, a[c][i] > ninf ? w : ninf);
                            }
                        }
                        v[c] = mmp_blkh_round(m);
                    }
                    *dst = v;
                    dst += hoff2;
                }
            }
            hdst += hpass;
        } else {
            for (int it = tid; it < kStemCG * kStemTPH * kStemTPW; it += kStemThreads) {
                const int j = it / (kStemTPH * kStemTPW), q = it - j * (kStemTPH * kStemTPW);
                const int pyl = q / kStemTPW, pxl = q - pyl * kStemTPW;
                const int py = py0 + pyl, px = px0 + pxl;
                if (py >= p.Hp || px >= p.Wp) continue;
                float a[9], b[9];
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const int pos = (2 * pyl + dy) * kStemCW + 2 * pxl + dx;
                        a[dy * 3 + dx] = wab[j * kStemNP + pos];
                        b[dy * 3 + dx] = wab[(kStemCG + j) * kStemNP + pos];
                    }
                float* dst = p.out + ((size_t)item * p.n_off * p.C + (size_t)(g * kStemCG + j)) * plane + (size_t)py * p.Wp + px;
                if (p.mono) {
                    for (int off = 0; off < p.n_off; ++off) {
                        const float t = (float)(off + 1);
                        float m = fmaf(t, b[0], a[0]);
#pragma unroll
                        for (int i = 1; i < 9; ++i) m = fmaxf(m, fmaf(t, b[i], a[i]));
                        *dst = m > 0.0f ? m : m * p.slope;
                        dst += (size_t)p.C * plane;
                    }
                } else {
                    for (int off = 0; off < p.n_off; ++off) {
                        const float t = (float)(off + 1);
                        float m = ninf;
#pragma unroll
                        for (int i = 0; i < 9; ++i) {
                            const float z = fmaf(t, b[i], a[i]);
                            const float v = z > 0.0f ? z : z * p.slope;
                            m = fmaxf(m, a[i] > ninf ? v : ninf);
                        }
                        *dst = m;
                        dst += (size_t)p.C * plane;
                    }
                }
            }
        }
    }
}

} // namespace nmpc
