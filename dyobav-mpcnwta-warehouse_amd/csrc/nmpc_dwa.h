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

template <typename T>
__global__ __launch_bounds__(kDwaThreads) void dwa_step_kernel(DwaParams<T> p)
{
    extern __shared__ __align__(16) unsigned char dwa_smem[];
    T* edges = reinterpret_cast<T*>(dwa_smem);
    const int n_edge = 4 * p.M;
    for (int e = threadIdx.x; e < n_edge; e += kDwaThreads) {
        const T* q = p.polys + (size_t)(e >> 2) * 8;
        const int k = e & 3, k1 = (k + 1) & 3;
        const T ax = q[2 * k], ay = q[2 * k + 1], bx = q[2 * k1], by = q[2 * k1 + 1];
        const T len = thypot(bx - ax, by - ay);
        T* o = edges + (size_t)e * kDwaEdgeReals;
        o[0] = ax, o[1] = ay, o[2] = bx, o[3] = by, o[4] = (bx - ax) / len, o[5] = (by - ay) / len;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int a = blockIdx.x * (kDwaThreads / 64) + (threadIdx.x >> 6);
    if (a >= p.n_run) return;
    const long long bl = p.run ? p.run[a] : a;
    if (bl < 0 || bl >= p.B) return; // (a device-side run list is not validated by the host: stay inside the arrays)
    const size_t b = (size_t)bl;
    const int N = p.N, H = p.H;
    const T inf = T(INFINITY);
    const T x0 = p.state_c[3 * (size_t)a], y0 = p.state_c[3 * (size_t)a + 1], th0 = p.state_c[3 * (size_t)a + 2];
    const T gx = p.goal[2 * b], gy = p.goal[2 * b + 1];
    // base speed: 0.8 lin_vel_max, lowered near the goal (trajectory_tracker.py:312-316)
    T base = p.base_speed;
    {
        const T dg = thypot(x0 - gx, y0 - gy);
        if (dg < base * T(N) * p.tsT) {
            const T sp = T(2) * dg / T(N) / p.tsT;
            base = sp < p.lin_vel_max ? sp : p.lin_vel_max;
        }
    }
    // window and grid in double
    double v0, v1, w0, w1, dvd, dwd;
    int nv, nw;
    dwa_window((double)p.last_u_c[2 * (size_t)a], p.acc, p.ts, p.vmin, p.vmax, v0, v1);
    dwa_window((double)p.last_u_c[2 * (size_t)a + 1], p.wacc, p.ts, -p.wmax, p.wmax, w0, w1);
    dwa_arange(v0, v1, p.dv, p.cap, nv, dvd);
    dwa_arange(w0, w1, p.dw, p.cap, nw, dwd);
    if (nv > 0 && nw > p.cap / nv) nw = p.cap / nv; // (never with the host's bound on cap: keeps the writes inside [cap])
    const int n_cand = nv * nw;
    long long plen = p.path_len[b];
    plen = plen < 2 ? 2 : plen > p.Pmax ? p.Pmax : plen;
    const T* path = p.path + b * (size_t)p.Pmax * 2;
    const T* dyn = p.dyn_c + (size_t)a * H * (size_t)(N + 1) * 6;
    const size_t hstride = (size_t)(N + 1) * 6;

    T best = inf;
    int bidx = 0x7fffffff;
    for (int cnd = lane; cnd < n_cand; cnd += 64) {
        const int iv = cnd / nw, iw = cnd - iv * nw;
        const T v = (T)dwa_grid(v0, dvd, iv), w = (T)dwa_grid(w0, dwd, iw);
        T x = x0, y = y0, th = th0;
        T q_near = inf, h_near = inf, c_near = inf; // closest edge over all points: h^2 + c^2 and its components
        T q_cur = inf;                           // squared distance to the closest current position
        T d_steps = inf;                         // min_i sqrt(i + 1) * min_h |p_i - mu[h][i + 1]|
        const T kth = p.tsT * w;
        for (int i = 0; i <= N; ++i) {
            for (int e = 0; e < n_edge; ++e) {
                T h, c;
                dwa_edge(edges + (size_t)e * kDwaEdgeReals, x, y, h, c);
                const T q = h * h + c * c;
                if (q < q_near) q_near = q, h_near = h, c_near = c;
            }
            if (p.dyn_mode >= 1) {
                T qs = inf;
                for (int hh = 0; hh < H; ++hh) {
                    const T* r = dyn + hh * hstride;
                    const T ex = x - r[0], ey = y - r[1];
                    const T q = ex * ex + ey * ey;
                    q_cur = q < q_cur ? q : q_cur;
                    if (p.dyn_mode == 2 && i < N) {
                        const T fx = x - r[6 * (i + 1)], fy = y - r[6 * (i + 1) + 1];
                        const T q2 = fx * fx + fy * fy;
                        qs = q2 < qs ? q2 : qs;
                    }
                }
                if (p.dyn_mode == 2 && i < N) {
                    const T di = tsqrt(qs) * tsqrt(T(i + 1));
                    d_steps = di < d_steps ? di : d_steps;
                }
            }
            if (i < N) { // unicycle RK4 with a constant control, stage by stage (motion_model.py:141-163)
                T s0, c0, s1, c1, s2, c2;
                tsincos(th, s0, c0);
                tsincos(th + T(0.5) * kth, s1, c1);
                tsincos(th + kth, s2, c2);
                const T k1x = p.tsT * (v * c0), k2x = p.tsT * (v * c1), k4x = p.tsT * (v * c2);
                const T k1y = p.tsT * (v * s0), k2y = p.tsT * (v * s1), k4y = p.tsT * (v * s2);
                x = x + T(1.0 / 6.0) * (k1x + T(2) * k2x + T(2) * k2x + k4x);
                y = y + T(1.0 / 6.0) * (k1y + T(2) * k2y + T(2) * k2y + k4y);
                th = th + T(1.0 / 6.0) * (kth + T(2) * kth + T(2) * kth + kth);
            }
        }
        // cost (trajectory_tracker.py:186-203): speed + goal direction + path deviation + static + dynamic
        const T c_speed = tabs(v - base) * p.q_speed;
        const T ang = tatan2(gy - y, gx - x) - th;
        T sa, ca;
        tsincos(ang, sa, ca);
        const T c_goal = tabs(tatan2(sa, ca)) * p.q_goal;
        T d_ref = inf;
        for (int j = 0; j + 1 < (int)plen; ++j) {
            const T ax = path[2 * j], ay = path[2 * j + 1], bx = path[2 * j + 2], by = path[2 * j + 3];
            const T len = thypot(bx - ax, by - ay);
            const T e[6] = {ax, ay, bx, by, (bx - ax) / len, (by - ay) / len};
            T h, c;
            dwa_edge(e, x, y, h, c);
            const T d = thypot(h, c);
            d_ref = d < d_ref ? d : d_ref; // (a NaN of a zero-length segment is skipped here; np.min would return it)
        }
        const T c_ref = d_ref * p.q_ref;
        T c_stc = T(0);
        if (n_edge > 0) {
            const T d = thypot(h_near, c_near);
            c_stc = d < T(0.05) ? inf : d > T(0.5) ? T(0) : T(1) / d * p.q_stc;
        }
        T c_dyn = T(0);
        if (p.dyn_mode >= 1) {
            const T d = tsqrt(q_cur);
            const T c_cur = d > T(0.5) ? T(0) : d < T(0.2) ? inf : T(1) / d * p.q_dyn;
            T c_st = T(0);
            if (p.dyn_mode == 2) c_st = d_steps < T(0.2) ? inf : d_steps > T(0.5) ? T(0) : T(1) / d_steps * p.q_dyn;
            c_dyn = c_st + c_cur;
        }
        const T cost = c_speed + c_goal + c_ref + c_stc + c_dyn;
        if (p.cost_all) p.cost_all[(size_t)a * p.cap + cnd] = cost;
        if (p.cand_all) {
            p.cand_all[((size_t)a * p.cap + cnd) * 2] = v;
            p.cand_all[((size_t)a * p.cap + cnd) * 2 + 1] = w;
        }
        if (cost < best) best = cost, bidx = cnd; // (a lane's candidates come in ascending order: strict keeps the first)
    }
    for (int s = 32; s > 0; s >>= 1) { // (cost, index) minimum, lowest index among equals
        const T ob = __shfl_xor(best, s, 64);
        const int oj = __shfl_xor(bidx, s, 64);
        if (ob < best || (ob == best && oj < bidx)) best = ob, bidx = oj;
    }
    T uv = T(0), uw = T(0);
    if (bidx != 0x7fffffff) {
        const int iv = bidx / nw, iw = bidx - iv * nw;
        uv = (T)dwa_grid(v0, dvd, iv), uw = (T)dwa_grid(w0, dwd, iw);
        if (tabs(uv) < p.stuck) uw = (T)(-p.wmax);
    }
    for (int e = lane; e < 2 * N; e += 64) p.U_c[(size_t)a * 2 * N + e] = (e & 1) ? uw : uv;
    if (lane == 0) {
        p.min_cost[a] = best;
        p.choice[a] = bidx == 0x7fffffff ? -1 : bidx;
        p.counts[2 * (size_t)a] = nv, p.counts[2 * (size_t)a + 1] = nw;
    }
}

} // namespace nmpc
