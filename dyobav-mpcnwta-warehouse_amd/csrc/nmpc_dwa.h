// nmpc_dwa.h -- the dynamic-window (DWA) baseline tracker of the closed loop ("next" row f3, tracker `dwa`): one kernel,
// between loop_pre_kernel (or kf_predict_kernel) and loop_post_kernel, in place of nmpc_assemble_params + the solve.
//
// Replaces, for the running scenarios in lock-step (lines of the reference project's src/):
//   pkg_dwa_tracker/trajectory_tracker.py:304-355  run_step: base-speed correction near the goal, dynamic window around the
//                             previous control, the np.arange grid over (v, w), first strict minimum of the cost, the
//                             stuck rule (|v| < stuck_threshold -> w = -ang_vel_max)
//   trajectory_tracker.py:110-125   pred_trajectory: N_hor unicycle RK4 steps with the constant candidate control
//   trajectory_tracker.py:128-203   the five cost terms; pkg_dwa_tracker/utils_geo.py:6-34 lineseg_dists (normalised
//                             tangent, h = max(s, t, 0), hypot(h, c): NO inside test -- a point inside a rectangle has a
//                             positive distance to its edges, kept)
//   main_base.py:303-321, interfaces/dwa_interface.py   how it is driven: predictor None -> current positions (dyn_mode 1),
//                             a predictor -> its mu lists, offset 0 = the current positions (dyn_mode 2)
// Thresholds as written there: static d < 0.05 -> +inf, d > 0.5 -> 0, else q_stc / d; current positions d > 0.5 -> 0 FIRST,
// then d < 0.2 -> +inf, else q_dyn / d; per-step term d_i = sqrt(i + 1) * min_h |p_i - mu[h][i + 1]| for i = 0 .. N-1
// (trajectory point i is paired with offset i + 1, as written), any d_i < 0.2 -> +inf, min_i d_i > 0.5 -> 0, else q_dyn / min.
//
// DELIBERATE DEVIATION: the reference's calc_cost_dynamic_obstacles_steps expands a 1-D point along axis 1, so that
// (2,1) meets (1,H,2): it raises for H >= 3 and mixes x with y for H = 1, 2. The evaluator runs 4 pedestrians. This kernel
// computes the Euclidean distance that the function's name and its sibling (calc_cost_dynamic_obstacles) state.
//
// Window and grid are computed in double with contraction off in both builds: np.arange gives n = ceil((stop - start) /
// step) values start + i * ((start + step) - start), every operation rounded on its own; the candidates are cast to T
// afterwards. Candidate order is v-major, w-minor.
//
// Mapping: ONE WAVEFRONT PER RUNNING SCENARIO, LANE = CANDIDATE (stride 64 when nv * nw > 64); a workgroup is four
// wavefronts that share the rectangle edges, staged once in LDS as (a, b, unit tangent). A lane rolls its candidate out
// point by point and folds every point into the running minima at once, so no trajectory is stored: no scratch. The
// minimum over the edges is taken on h^2 + c^2 and hypot(h, c) is evaluated once, for the closest edge. Selection is a
// lexicographic (cost, index) butterfly like the snap stage's: smallest index among equal costs; NaN and +inf never win.
// No atomics, nothing depends on which other scenarios are in the launch.
//
// Per-offset lists (dwa_step_lists_kernel, entry points nmpc_dwa_step_lists_*): the mmp predictor's cluster means, whose
// number differs from offset to offset. dyn_c is [n_run][R][N+1][6] with dyn_count [n_run][N+1]: row r of offset t exists
// when r < count[t], and nothing else of dyn_c is read (f2 pads with rows that cannot be told from a cluster).
// DELIBERATE DEVIATION: the reference takes its per-step path only when np.array(dynamic_obstacles).ndim == 3
// (trajectory_tracker.py:186-203), i.e. when every offset has the same number of entries, and raises otherwise. Where it is
// defined its meaning is dyn_mode 2's, the Euclidean deviation above included; this variant extends exactly that: offset 0
// is the mode-1 term over the count[0] current positions; trajectory point i is paired with offset i + 1, d_i = sqrt(i + 1)
// * min over the count[i + 1] means of that offset; an offset with no cluster contributes no d_i; if no offset has a
// cluster the per-step term is 0; thresholds and their order are mode 2's. Clusters beyond the R rows are dropped (as on the
// MPC path, where f2's n_obs reports them), counts are clamped to 0 .. R on the device.
// Mode 2 reads its rows from global memory at wave-uniform addresses inside the point loop; with up to 40 rows at 21 offsets
// that would be ten times the loads per candidate, so each wavefront stages its scenario's means once in LDS, next to the
// edge table, compacted [offset][row][2] -- a point's loop is a run of broadcast reads -- with the clamped counts and their
// running sums behind them: 2 R (N + 1) reals + 2 (N + 1) ints per wavefront (R = 40, N = 20: 6.7 KB in fp32, 27 KB per
// workgroup beside the 5.2 KB of 55 rectangles; twice that in fp64). The entry refuses R (N + 1) > kDwaListsMaxMeans = 840
// and a workgroup total above 64 KB. The arithmetic per point is mode 2's. The variant is a compile-time constant of the one
// body (nmpc_dwa_step.inl): the kernels for modes 0 .. 2 keep their instructions, byte for byte.
#pragma once

#include <hip/hip_runtime.h>

namespace nmpc {

constexpr int kDwaThreads = 256;   // four wavefronts = four scenarios per workgroup
constexpr int kDwaEdgeReals = 6;   // ax, ay, bx, by, tx, ty

template <typename T>
struct DwaParams {
    int B, n_run, N, H, M, Pmax, cap, dyn_mode;
    const long long* run;      // [n_run] or nullptr = all B
    const T* state_c;          // [n_run][3]
    const T* last_u_c;         // [n_run][2]
    const T* dyn_c;            // [n_run][H][N+1][6]
    const T* goal;             // [B][2]
    const T* path;             // [B][Pmax][2]
    const long long* path_len; // [B]
    const T* polys;            // [M][4][2]
    double ts, vmin, vmax, acc, wmax, wacc, dv, dw; // window and grid: double in both builds
    T tsT, lin_vel_max, base_speed, stuck, q_speed, q_goal, q_ref, q_stc, q_dyn;
    T* U_c;                    // [n_run][2N]
    T* min_cost;               // [n_run]
    int* choice;               // [n_run]
    int* counts;               // [n_run][2]
    T* cost_all;               // [n_run][cap] or nullptr
    T* cand_all;               // [n_run][cap][2] or nullptr
};

// the lists variant's block: DwaParams as it is (H unused, dyn_mode 2, dyn_c [n_run][R][N+1][6]) and the counts behind it
template <typename T>
struct DwaListsParams : DwaParams<T> {
    int R;                     // rows per scenario
    const int* dyn_count;      // [n_run][N+1], clamped to 0 .. R on the device
};

constexpr int kDwaListsMaxMeans = 840;        // R (N + 1) the lists entry takes: 40 rows x 21 offsets
constexpr size_t kDwaListsMaxLds = 64 * 1024; // edge table + lists of a workgroup

// dynamic LDS of dwa_step_lists_kernel: edges, then per wavefront 2 R (N + 1) reals, then per wavefront 2 (N + 1) ints
template <typename T>
constexpr size_t dwa_lists_lds(int M, int R, int N)
{
    return ((size_t)M * 4 * kDwaEdgeReals + (size_t)(kDwaThreads / 64) * 2 * R * (N + 1)) * sizeof(T) +
           (size_t)(kDwaThreads / 64) * 2 * (N + 1) * sizeof(int);
}

__device__ __forceinline__ float tatan2(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ double tatan2(double y, double x) { return atan2(y, x); }

// np.arange(start, stop, step): the count and the increment, every operation rounded on its own
__device__ __forceinline__ void dwa_arange(double start, double stop, double step, int limit, int& n, double& delta)
{
#pragma clang fp contract(off)
    const double x = ceil((stop - start) / step);
    n = x > 0.0 ? (x < (double)limit ? (int)x : limit) : 0; // (NaN -> 0)
    delta = (start + step) - start;
}

__device__ __forceinline__ double dwa_grid(double start, double delta, int i)
{
#pragma clang fp contract(off)
    return start + (double)i * delta;
}

__device__ __forceinline__ void dwa_window(double last, double acc, double ts, double lo, double hi, double& w0, double& w1)
{
#pragma clang fp contract(off)
    const double a = last - acc * ts, b = last + acc * ts;
    w0 = a > lo ? a : lo; // max(lo, a): lo unless a > lo
    w1 = b < hi ? b : hi; // min(hi, b)
}

// squared lineseg_dists components of p against the edge e = (ax, ay, bx, by, tx, ty)
template <typename T>
__device__ __forceinline__ void dwa_edge(const T* e, T px, T py, T& h, T& c)
{
    const T s = (e[0] - px) * e[4] + (e[1] - py) * e[5];
    const T t = (px - e[2]) * e[4] + (py - e[3]) * e[5];
    h = s > t ? s : t;
    h = h > T(0) ? h : T(0);
    c = (px - e[0]) * e[5] - (py - e[1]) * e[4];
}

// Both kernels are the one body of nmpc_dwa_step.inl; LISTS selects the variant at compile time.
template <typename T>
__global__ __launch_bounds__(kDwaThreads) void dwa_step_kernel(DwaParams<T> p)
{
    constexpr bool LISTS = false;
#include "nmpc_dwa_step.inl"
}

template <typename T>
__global__ __launch_bounds__(kDwaThreads) void dwa_step_lists_kernel(DwaListsParams<T> p)
{
    constexpr bool LISTS = true;
#include "nmpc_dwa_step.inl"
}

} // namespace nmpc
