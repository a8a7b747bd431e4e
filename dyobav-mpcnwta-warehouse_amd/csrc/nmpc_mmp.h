// nmpc_mmp.h -- the input stack of the multi-hypothesis predictor's network ("next" row f3, predictor `mmp`): one kernel in
// front of the network, which itself stays a PyTorch module (the stage behind it is nmpc_snap.h -> nmpc_hypotheses.h).
//
// Replaces, per pedestrian and time step (lines of the reference project's src/):
//   main_base.py:190,193                    ct2real(x, forward=False): (x - offset) / scale, then the optional reversals
//   interfaces/mmp_interface.py:36          ... * rescale
//   pkg_motion_prediction/pre_load.py:119-136   traj_to_input: the last obsv_len = 5 positions, the newest one repeated AT THE
//                                           END when there are fewer; one Gaussian map per position, then the label image twice
//   pkg_motion_prediction/utils/utils_np.py:76-91   np_gaudist_map(centre, sigmas = [s, s], rho = 0): z / z.max() with
//                                           z = 1 / (2 pi s s) exp(-0.5 ((x - cx)^2 / s^2 + (y - cy)^2 / s^2)), max over the GRID
//   interfaces/mmp_interface.py:45-49       one copy of the stack per time offset 1 .. pred_offset, the offset in channel 6
//   network_manager.inference               input_data.float(): the float64 stack is rounded to float once
// out[item][off][7][Hm][Wm] float: channels 0..4 the Gaussian maps (oldest first), 5 the label image, 6 the constant off + 1.
//
// Arithmetic: float64 in numpy's order -- dx = x - cx, dx * dx / s2, the sum of the two quotients, * -0.5, exp, * k, / zmax
// (no product feeds an addition, so contraction has nothing to fuse) -- and ONE rounding to float. The only operation that is
// not correctly rounded is exp, so a value differs from numpy's by a few fp64 ulps and from its float rounding only where
// that moves the double across a float rounding boundary. zmax is the same expression at the pixel nearest the centre,
// clamped to the map: every operation of the chain is monotone in |x - cx| and |y - cy|, so the grid maximum is there (at a
// half-integer centre the two nearest pixels give equal values). Each thread recomputes it, nothing is shared.
//
// Mapping (store-bound: a pixel is computed once -- five exp for the maps, five for their maxima, fewer while the
// trajectory has fewer than five distinct entries -- and stored 7 n_off times): one thread per V consecutive pixels of the
// plane, 256 threads per workgroup, workgroups [item][plane piece] flattened in x; the thread keeps its 6 V values in
// registers and walks the n_off copies with 7 stores each. No LDS, no atomics, no cross-lane traffic; the centres are
// workgroup-uniform loads. V is the widest vector for which EVERY plane start stays aligned: plane p starts at p Hm Wm
// floats, so 16-byte stores need Hm Wm % 4 == 0, 8-byte stores Hm Wm % 2 == 0 (the warehouse map: 293 x 330 = 96 690,
// even, not a multiple of four -> dwordx2), otherwise one dword per lane (256 contiguous bytes per wave-instruction; that
// form of plain store has been measured at 6.0-6.2 TB/s on an MI355X against 6.29 TB/s for a float4 copy).
// A pedestrian's values depend on its own hist / hcount rows and the pixel only: not on the other items of the launch.
#pragma once

#include <hip/hip_runtime.h>

namespace nmpc {

struct MmpParams {
    int n_item, n_off, H, Hm, Wm, xr, yr, bpi; // bpi: workgroups per item
    long long n_ped;                           // B * H: rows of hist / hcount
    const long long* items;                    // [n_item] ascending or nullptr = 0 .. n_item - 1
    const void* hist;                          // [B][H][5][2]
    const long long* hcount;                   // [B][H]
    double scale, offx, offy, xmax, ymax, rescale, s2, k;
    const float* ref;                          // [Hm][Wm]
    float* out;                                // [n_item][n_off][7][Hm][Wm]
};

constexpr int kMmpThreads = 256;

template <int V>
struct MmpVec;
template <>
struct MmpVec<1> { using type = float; };
template <>
struct MmpVec<2> { using type = float2; };
template <>
struct MmpVec<4> { using type = float4; };

// k exp(-0.5 (dx dx / s2 + dy dy / s2)), every operation rounded on its own
__device__ __forceinline__ double mmp_gauss(double x, double y, double cx, double cy, double s2, double k)
{
    const double dx = x - cx, dy = y - cy;
    const double a = dx * dx / s2, b = dy * dy / s2;
    return k * exp(-0.5 * (a + b));
}

__device__ __forceinline__ double mmp_nearest(double c, int n)
{
    const double r = rint(c);
    return !(r > 0.0) ? 0.0 : r > (double)(n - 1) ? (double)(n - 1) : r; // (a NaN centre: pixel 0, the values are NaN anyway)
}

// distinct entries of a history that has seen cnt positions: channels n - 1 .. 4 all show the newest one
__device__ __forceinline__ int mmp_distinct(long long cnt) { return cnt < 1 ? 1 : cnt > 5 ? 5 : (int)cnt; }

// The centre of history entry e in network pixels, for both kernels (their planes must be the same floats): ct2real backwards,
// the reversals, * rescale. The constants come as values: a reference to or a copy of the kernel's params struct keeps its
// private copy alive past the pass that marks the argument loads (hipcc, gfx950: all marks lost, mmp_stem_kernel + 6 instructions).
template <typename T>
__device__ __forceinline__ void mmp_centre(const T* hist, int e, double offx, double offy, double scale, int xr, double xmax, int yr, double ymax,
                                           double rescale, double& cx, double& cy)
{
    cx = ((double)hist[2 * e] - offx) / scale, cy = ((double)hist[2 * e + 1] - offy) / scale;
    if (xr) cx = xmax - cx;
    if (yr) cy = ymax - cy;
    cx *= rescale, cy *= rescale;
}

template <typename T, int V>
__global__ __launch_bounds__(kMmpThreads) void mmp_input_kernel(MmpParams p)
{
    using Vec = typename MmpVec<V>::type;
    const int item = blockIdx.x / p.bpi, piece = blockIdx.x - item * p.bpi;
    const long long HW = (long long)p.Hm * p.Wm;
    const long long pix0 = ((long long)piece * kMmpThreads + threadIdx.x) * V;
    if (item >= p.n_item || pix0 >= HW) return; // (HW % V == 0: a vector never straddles the end of a plane)
    const long long ped = p.items ? p.items[item] : item;
    if (ped < 0 || ped >= p.n_ped) return; // (a device-side item list is not validated by the host: stay inside the arrays)
    const int n = mmp_distinct(p.hcount[ped]);
    const T* hist = static_cast<const T*>(p.hist) + ped * 10;

    float val[6][V]; // (every index below is a compile-time constant after unrolling: registers)
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        if (c >= n) { // workgroup-uniform; c >= n >= 1
#pragma unroll
            for (int v = 0; v < V; ++v) val[c][v] = val[c > 0 ? c - 1 : 0][v];
            continue;
        }
        double cx, cy;
        mmp_centre(hist, 5 - n + c, p.offx, p.offy, p.scale, p.xr, p.xmax, p.yr, p.ymax, p.rescale, cx, cy);
        const double zmax = mmp_gauss(mmp_nearest(cx, p.Wm), mmp_nearest(cy, p.Hm), cx, cy, p.s2, p.k);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const long long pix = pix0 + v;
            const int y = (int)(pix / p.Wm), x = (int)(pix - (long long)y * p.Wm);
            val[c][v] = (float)(mmp_gauss((double)x, (double)y, cx, cy, p.s2, p.k) / zmax);
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) val[5][v] = p.ref[pix0 + v];

    float* dst = p.out + (size_t)item * p.n_off * 7 * (size_t)HW + (size_t)pix0;
    for (int off = 0; off < p.n_off; ++off) {
        const float tv = (float)(off + 1);
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            Vec w;
            float* wf = reinterpret_cast<float*>(&w);
#pragma unroll
            for (int v = 0; v < V; ++v) wf[v] = c < 6 ? val[c][v] : tv;
            *reinterpret_cast<Vec*>(dst + (size_t)c * HW) = w;
        }
        dst += 7 * (size_t)HW;
    }
}

} // namespace nmpc
