// nmpc_snap.h -- predictor output in network pixels -> hypothesis points in world coordinates, on the device (the stage in
// front of row f2, nmpc_hypotheses.h).
//
// Replaces, for a whole batch (reference = /root/reference/src), what the reference does on the host per pedestrian and
// time offset between the network's output tensor and fit_DBSCAN:
//   pkg_motion_prediction/utils/utils_np.py:102-140  get_closest_edge_point: every hypothesis in an occupied map cell moves
//                                                    to the nearest edge pixel, the moved points are put FIRST
//   interfaces/mmp_interface.py:60                   ... / rescale
//   main_base.py:196                                 ScaleOffsetReverseTransform.cvt_coords (basic_map/map_tf.py:124-151)
//
// A segment = the K hypotheses of one pedestrian at one time offset, points (x, y) in pixels; the map is H x W.
//   1. point i is IN when occupied[int(y_i)][int(x_i)], int() truncating toward zero
//   2. m = max over the segment's in-points (xc, yc) and ALL pixels (c, r) of d = (c - xc)^2 + (r - yc)^2 (attained at a
//      corner pixel, per axis at c = 0 or c = W - 1: every operation below is monotone in |c - xc|)
//   3. an in-point moves to the FIRST edge pixel in row-major order with minimal q = d / m among those with q != 0 (the
//      reference overwrites zeros with the maximum); without any candidate it moves to pixel (0, 0) -- the reference's
//      argmin over a constant map
//   4. output order of the segment: moved points in their original relative order, then the untouched ones in theirs
//   5. every point: x / rescale, optionally x_max - x / y_max - y, scale * x + offset
// The selection of 3. is discrete, so the arithmetic is what numpy does: float64 with every subtract, multiply, add and
// divide rounded on its own -- the functions below switch contraction off (the library is built with hipcc's default
// -ffp-contract=fast, which would turn d into one multiply and one fma and move exact ties). The fp32 entry converts its
// input to float64 (exact), computes the same and rounds the result once.
//
// NOT mirrored:
//   * a point whose cell lies outside the map (the reference wraps negative indices or raises): it is left untouched,
//     nothing is read out of bounds, and it is counted in n_outside
//   * the reference's result dtype follows numpy promotion (a segment without in-points stays float32); here the contract
//     is "float64 arithmetic on the given inputs"
//   * a map whose candidates all share ONE value of q for an in-point (a single edge pixel): the reference's
//     "overwrite zeros with the maximum" then makes every pixel equal and its argmin returns (0, 0); rule 3 returns
//     the candidate
//
// Lane mapping: one wavefront per (instance, time offset), four wavefronts per workgroup which share the edge list in
// LDS (int16 (col, row) pairs in row-major order, built on the host once per map: 3576 pixels = 14 KB for the
// reference's warehouse; above kSnapLdsPixels the list is streamed from L2 instead) and take items in a grid-stride
// loop, so that the list is staged once per workgroup, not once per item. Lanes hold the points (lane + 64 w, up to four
// per lane); in / out is one ballot per 64 points, and everything after it -- segment bounds, the in-points' numbers,
// the stable partition -- is popcounts of those masks. The in-points are then taken up to four at a time: the 64 LANES
// STRIDE THE EDGE LIST (lane l looks at pixels l, l + 64, ...; a pixel's two int16 -> float64 conversions are shared by
// the in-points of the pass), each lane keeps its first minimum (strict <, ascending pixel index), and a lexicographic
// (q, pixel index) butterfly over the wavefront picks the first minimum overall. The other mapping, lane = in-point with
// all lanes walking the whole list, needs 3576 steps per wavefront whatever the in-count, against ~56 steps + one
// reduction per in-point here: it only wins above ~60 in-points of 64 lanes, which a batch of predictions does not have
// (a third of 40 points in the test batch, ~9 % in the reference's scenes).
#pragma once

#include <hip/hip_runtime.h>

#include "wave_ops.h"

namespace nmpc {

constexpr int kSnapThreads = 256;     // four wavefronts per workgroup
constexpr int kSnapLdsPixels = 12288; // edge list in LDS up to here (48 KB), streamed from L2 above
constexpr int kSnapBlock = 4;         // in-points per pass over the edge list

struct SnapParams {
    int items;         // B * N (instance, time offset) pairs
    int N, P, K;       // time offsets, points per offset (= n_ped * K), hypotheses per pedestrian
    int H, W;          // map
    int n_edge, n_edge_pad; // edge pixels; the list is zero-padded to a multiple of 64
    int xr, yr;
    double rescale, scale, offx, offy, xmax, ymax;
    const unsigned char* occ; // [H][W]
    const unsigned* edge;     // [n_edge_pad] col | row << 16
    int* n_snapped;           // [items][n_ped] (may be null)
    int* n_outside;           // [B], zeroed before the launch (may be null)
};

// d of rule 2: numpy's (c - xc)**2 + (r - yc)**2, four roundings
__device__ __forceinline__ double snap_d(double c, double r, double xc, double yc)
{
#pragma clang fp contract(off)
    const double dx = c - xc, dy = r - yc;
    const double dx2 = dx * dx, dy2 = dy * dy;
    return dx2 + dy2;
}

// max of d over all pixels for one in-point: per axis the larger of the two border columns / rows
__device__ __forceinline__ double snap_corner_max(double xc, double yc, int W, int H)
{
#pragma clang fp contract(off)
    const double a0 = 0.0 - xc, a1 = (double)(W - 1) - xc, b0 = 0.0 - yc, b1 = (double)(H - 1) - yc;
    const double a02 = a0 * a0, a12 = a1 * a1, b02 = b0 * b0, b12 = b1 * b1;
    const double ax = a02 > a12 ? a02 : a12, by = b02 > b12 ? b02 : b12;
    return ax + by;
}

// rule 5 (mmp_interface.py:60, map_tf.py:124-151): multiply and add rounded separately
__device__ __forceinline__ void snap_world(const SnapParams& a, double x, double y, double& wx, double& wy)
{
#pragma clang fp contract(off)
    x = x / a.rescale;
    y = y / a.rescale;
    if (a.xr) x = a.xmax - x;
    if (a.yr) y = a.ymax - y;
    const double sx = a.scale * x, sy = a.scale * y;
    wx = sx + a.offx;
    wy = sy + a.offy;
}

// bits [lo, hi) of the point range that fall into mask word w (points 64 w .. 64 w + 63)
__device__ __forceinline__ unsigned long long snap_word_range(int lo, int hi, int w)
{
    int l = lo - 64 * w, h = hi - 64 * w;
    l = l < 0 ? 0 : (l > 64 ? 64 : l);
    h = h < 0 ? 0 : (h > 64 ? 64 : h);
    const unsigned long long ml = l >= 64 ? ~0ull : (1ull << l) - 1ull, mh = h >= 64 ? ~0ull : (1ull << h) - 1ull;
    return mh & ~ml;
}

// NB in-points against the edge list: lanes stride the list, then the first minimum over the wavefront. xc / yc / m are
// wave-uniform; on return pix[i] = (col | row << 16) of the chosen pixel, 0 (= pixel (0, 0)) without a candidate.
template <int NB, typename E>
__device__ __forceinline__ void snap_walk(const SnapParams& a, E edge, const int lane, const double* xc, const double* yc,
                                          const double* m, unsigned* pix)
{
    const double inf = __builtin_huge_val();
    double qb[NB];
    int kb[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        qb[i] = inf;
        kb[i] = 0x7fffffff;
    }
#pragma clang loop unroll_count(2)
    for (int k = lane; k < a.n_edge_pad; k += 64) {
        const unsigned w = edge[k];
        const bool valid = k < a.n_edge;
        const double c = (double)(int)(w & 0xffffu), r = (double)(int)(w >> 16);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const double q = __ddiv_rn(snap_d(c, r, xc[i], yc[i]), m[i]);
            if (valid && q != 0.0 && q < qb[i]) { // (a NaN -- 1 x 1 map -- is never smaller: pixel (0, 0) then)
                qb[i] = q;
                kb[i] = k;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        double q = qb[i];
        int k = kb[i];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const double oq = __shfl_xor(q, s, 64);
            const int ok = __shfl_xor(k, s, 64);
            if (oq < q || (oq == q && ok < k)) {
                q = oq;
                k = ok;
            }
        }
        pix[i] = k == 0x7fffffff ? 0u : edge[k];
    }
}

// T: element type of raw / out; PPL: points per lane (P <= 64 PPL); LDS: edge list staged in LDS
template <typename T, int PPL, bool LDS>
__global__ __launch_bounds__(kSnapThreads) void snap_kernel(SnapParams a, const T* raw, T* out)
{
    extern __shared__ unsigned snap_lds[];
    if (LDS) {
        for (int k = threadIdx.x; k < a.n_edge_pad; k += kSnapThreads) snap_lds[k] = a.edge[k];
        __syncthreads(); // the only workgroup barrier: from here on the wavefronts run on their own
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int WPG = kSnapThreads / 64;
    const int n_ped = a.P / a.K;
    for (int item = blockIdx.x * WPG + wave; item < a.items; item += gridDim.x * WPG) {
        const T* src = raw + (size_t)item * a.P * 2;
        T* dst = out + (size_t)item * a.P * 2;
        // every point of the item is read before anything is written (raw and out may be the same array)
        double x[PPL], y[PPL], mi[PPL];
        unsigned long long inmask[PPL];
        int n_out = 0;
#pragma unroll
        for (int w = 0; w < PPL; ++w) {
            const int p = lane + 64 * w;
            const bool on = p < a.P;
            x[w] = on ? (double)src[2 * p] : 0.0;
            y[w] = on ? (double)src[2 * p + 1] : 0.0;
        }
#pragma unroll
        for (int w = 0; w < PPL; ++w) {
            const bool on = lane + 64 * w < a.P;
            // the cell int(x), int(y) lies on the map (a NaN fails every comparison)
            const bool onmap = x[w] > -1.0 && x[w] < (double)a.W && y[w] > -1.0 && y[w] < (double)a.H;
            bool in = false;
            if (on && onmap) in = a.occ[(size_t)(int)y[w] * a.W + (int)x[w]] != 0;
            inmask[w] = __ballot(in);
            n_out += __popcll(__ballot(on && !onmap));
            mi[w] = snap_corner_max(x[w], y[w], a.W, a.H);
        }
        if (a.n_outside && n_out > 0 && lane == 0) atomicAdd(a.n_outside + item / a.N, n_out);
        // in-points before point q (exclusive), from the masks
        auto before = [&](int q) {
            int c = 0;
#pragma unroll
            for (int w = 0; w < PPL; ++w) c += __popcll(inmask[w] & snap_word_range(0, q, w));
            return c;
        };
        // stable partition: destination of every point inside its segment; the untouched ones are written now
        int dest[PPL];
#pragma unroll
        for (int w = 0; w < PPL; ++w) {
            const int p = lane + 64 * w;
            const int p0 = (p / a.K) * a.K;
            const int b0 = before(p0), rank = before(p) - b0, n_in = before(p0 + a.K) - b0;
            const bool in = (inmask[w] >> lane) & 1ull;
            dest[w] = in ? p0 + rank : p0 + n_in + (p - p0 - rank);
            if (p < a.P && !in) {
                double wx, wy;
                snap_world(a, x[w], y[w], wx, wy);
                dst[2 * dest[w]] = (T)wx;
                dst[2 * dest[w] + 1] = (T)wy;
            }
        }
        // the in-points, segment by segment (wave-uniform from here: the masks are), kSnapBlock at a time; the newest
        // sits in slot kSnapBlock - 1
        double bx[kSnapBlock], by[kSnapBlock], bm[kSnapBlock];
        int bd[kSnapBlock];
#pragma unroll
        for (int i = 0; i < kSnapBlock; ++i) {
            bx[i] = by[i] = 0.0;
            bm[i] = 1.0;
            bd[i] = 0;
        }
        int nb = 0;
        auto flush = [&]() {
            static_assert(kSnapBlock == 4, "flush dispatches on nb = 1..4");
            unsigned pix[kSnapBlock];
            if (nb == kSnapBlock)
                snap_walk<4>(a, LDS ? snap_lds : a.edge, lane, bx, by, bm, pix);
            else if (nb == 3)
                snap_walk<3>(a, LDS ? snap_lds : a.edge, lane, bx + 1, by + 1, bm + 1, pix + 1);
            else if (nb == 2)
                snap_walk<2>(a, LDS ? snap_lds : a.edge, lane, bx + 2, by + 2, bm + 2, pix + 2);
            else
                snap_walk<1>(a, LDS ? snap_lds : a.edge, lane, bx + 3, by + 3, bm + 3, pix + 3);
#pragma unroll
            for (int i = 0; i < kSnapBlock; ++i) {
                if (i >= kSnapBlock - nb && lane == i) { // one lane per result
                    double wx, wy;
                    snap_world(a, (double)(int)(pix[i] & 0xffffu), (double)(int)(pix[i] >> 16), wx, wy);
                    dst[2 * bd[i]] = (T)wx;
                    dst[2 * bd[i] + 1] = (T)wy;
                }
            }
            nb = 0;
        };
        for (int s = 0; s < n_ped; ++s) {
            const int p0 = s * a.K;
            unsigned long long seg[PPL];
            int n_in = 0;
#pragma unroll
            for (int w = 0; w < PPL; ++w) {
                seg[w] = inmask[w] & snap_word_range(p0, p0 + a.K, w);
                n_in += __popcll(seg[w]);
            }
            if (a.n_snapped && lane == 0) a.n_snapped[(size_t)item * n_ped + s] = n_in;
            if (n_in == 0) continue;
            double m = 0.0; // rule 2: over the segment's in-points
#pragma unroll
            for (int w = 0; w < PPL; ++w) {
                for (unsigned long long bits = seg[w]; bits; bits &= bits - 1ull) {
                    const double v = read_lane(mi[w], (int)__builtin_ctzll(bits));
                    m = v > m ? v : m;
                }
            }
#pragma unroll
            for (int w = 0; w < PPL; ++w) {
                for (unsigned long long bits = seg[w]; bits; bits &= bits - 1ull) {
                    const int l = (int)__builtin_ctzll(bits);
#pragma unroll
                    for (int i = 0; i + 1 < kSnapBlock; ++i) {
                        bx[i] = bx[i + 1];
                        by[i] = by[i + 1];
                        bm[i] = bm[i + 1];
                        bd[i] = bd[i + 1];
                    }
                    bx[kSnapBlock - 1] = read_lane(x[w], l);
                    by[kSnapBlock - 1] = read_lane(y[w], l);
                    bm[kSnapBlock - 1] = m;
                    bd[kSnapBlock - 1] = __builtin_amdgcn_readlane(dest[w], l);
                    if (++nb == kSnapBlock) flush();
                }
            }
        }
        if (nb) flush();
    }
}

} // namespace nmpc
