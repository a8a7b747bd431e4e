// nmpc_kf.h -- the Kalman-filter pedestrian predictor of the closed loop ("next" row f3, predictor `kfmp`): one kernel, one
// wavefront per running scenario, between loop_pre_kernel (nmpc_step.h) and nmpc_assemble_params.
//
// Replaces, for B scenarios in lock-step (lines of the reference project's src/):
//   main_base.py:210-236      run_kf_prediction: ONE filter object serves the pedestrians h = 0, 1, ... of a scenario in order
//   interfaces/kfmp_interface.py:26-56   get_motion_prediction: initial state from the first two points of past_traj
//                             (velocity = displacement per STEP, as written there), filter over the whole past_traj, then
//                             N_hor predictions without evolving P; uncertainty = (P[0,0], P[1,1]) for EVERY offset, no root
//   zfilter.py:45-78          KalmanFilter.predict / update / inference, input U = 0 (B, D never matter):
//                               X = A X;  P = A (P A') + Q
//                               S = R + C (P C');  K = P (C' S^-1);  X += K (Y - C X);  P = P - K (S K')
//   main_base.py:221-222, 234-235, 293-302   rows [x, y, HUMAN_SIZE, HUMAN_SIZE, 0, 1] at offset 0 (current position) and
//                             [mu_x, mu_y, P00, P11, 0, 1] at offsets 1 .. N_hor
// P IS NEVER RESET by the reference (set_init_state resets X only), so the covariance chain runs on from pedestrian to
// pedestrian and from time step to time step of a run: kf_P[b] is read at the start of the call, carried through the
// pedestrians in order and written back. The filter is re-run over the whole stored trajectory in every call (the
// reference does; an incremental filter gives other bits until the chain is stationary). S^-1 is the closed-form 2 x 2
// inverse (the reference calls LAPACK), P is not symmetrised (the reference does not). A, C, Q, R are general dense
// matrices: nothing assumes the constant-velocity model's zeros.
//
// Per running scenario b = run[a]:
//   1. append: hcount[b,h] > kf_len[b,h] -> humans[b,h] becomes kf_traj[b,h,kf_len], kf_len += 1; at most one point per
//      call, nothing beyond row cap - 1 (the point is dropped and kf_len stays at cap)
//   2. filter over kf_traj[b,h,0:kf_len] for h = 0 .. H-1 (an empty trajectory is filtered as the single point humans[b,h])
//   3. all six columns of the N_hor + 1 rows of dyn_c[a][h]
//
// Lane mapping: EVERY LANE CARRIES THE SAME 4 x 4 RECURSION IN REGISTERS. The recursion is a serial chain of small dense
// products (about 300 multiply-adds per one-step written for general matrices) whose only data are two reals per step,
// read by all lanes from one address (a broadcast load); the matrices are kernel arguments, i.e. scalar registers. That
// needs no LDS, no cross-lane traffic and has no divergence; the lanes differ only when the rows are written (lane
// t mod 64 stores offset t) and lane 0 stores the appended point, kf_len and kf_P. 63 of 64 lanes compute redundantly; the
// wavefront is there because a scenario's chain through its pedestrians is serial and B wavefronts fill the device at the
// batch sizes the evaluator runs at. Splitting the covariance over 16 lanes or the pedestrians over lanes (the chain
// links them: only X could be split) is the alternative if this stage ever shows in a time step's budget -- DESIGN.md
// section 7 has the measured share.
// Stationarity shortcut: once a one-step returns, bit for bit, the covariance it was given, every later one-step of the
// call would compute the same products again and return the same covariance and gain (the recursion of P does not see the
// data), so the gain is kept and only X = A X, X += K (Y - C X) remains: ~50 of ~300 multiply-adds. It cannot change a bit.
// With the default matrices the chain is stationary after about a hundred one-steps of a run, i.e. from the first
// one-step of every call after the first twenty-odd time steps (measured: DESIGN.md section 7).
// The appended point is kept in registers and substituted where the filter reaches its index, so no lane reads what
// another lane stored in this call.
#pragma once

#include <hip/hip_runtime.h>

namespace nmpc {

template <typename T>
struct KfParams {
    int B, n_run, N, H, cap;
    const long long* run;    // [n_run] ascending or nullptr = all B
    const T* humans;         // [B][H][2]
    const long long* hcount; // [B][H]
    T* kf_traj;              // [B][H][cap][2]
    long long* kf_len;       // [B][H]
    T* kf_P;                 // [B][4][4]
    T* dyn_c;                // [n_run][H][N+1][6]
    T A[16], C[8], Q[16], R[4], human_size;
};

template <typename T>
__device__ __forceinline__ bool kf_same_bits(T a, T b)
{
    if constexpr (sizeof(T) == 4)
        return __builtin_bit_cast(unsigned, a) == __builtin_bit_cast(unsigned, b);
    else
        return __builtin_bit_cast(unsigned long long, a) == __builtin_bit_cast(unsigned long long, b);
}

template <typename T>
__global__ __launch_bounds__(64) void kf_predict_kernel(KfParams<T> p)
{
    const int a = blockIdx.x, lane = threadIdx.x;
    const long long bl = p.run ? p.run[a] : a;
    if (bl < 0 || bl >= p.B) return; // (a device-side run list is not validated by the host: stay inside the arrays)
    const size_t b = (size_t)bl;
    const int N = p.N, H = p.H, cap = p.cap;
    T P[16], K[8]; // K: the gain of the last full one-step, reused once the covariance is stationary
    bool stationary = false;
#pragma unroll
    for (int i = 0; i < 16; ++i) P[i] = p.kf_P[b * 16 + i];
#pragma unroll
    for (int i = 0; i < 8; ++i) K[i] = T(0);
    for (int h = 0; h < H; ++h) {
        const size_t hb = b * H + h;
        const T cx = p.humans[2 * hb], cy = p.humans[2 * hb + 1];
        T* tr = p.kf_traj + hb * (size_t)cap * 2;
        long long len = p.kf_len[hb];
        len = len < 0 ? 0 : len > cap ? cap : len;
        int L = (int)len, app = -1; // app: index of the point appended in this call
        if (p.hcount[hb] > len && L < cap) {
            app = L;
            L += 1;
            if (lane == 0) {
                tr[2 * app] = cx, tr[2 * app + 1] = cy;
                p.kf_len[hb] = L;
            }
        }
        // initial state: first point, displacement to the second one (kfmp_interface.py:44-50)
        const T x0 = L == 0 || app == 0 ? cx : tr[0], y0 = L == 0 || app == 0 ? cy : tr[1];
        T X[4] = {x0, y0, T(0), T(0)};
        if (L > 1) {
            const T x1 = app == 1 ? cx : tr[2], y1 = app == 1 ? cy : tr[3];
            X[2] = x1 - x0, X[3] = y1 - y0;
        }
        for (int i = 1; i < L; ++i) {
            const T Yx = i == app ? cx : tr[2 * i], Yy = i == app ? cy : tr[2 * i + 1];
            T M[16], Xn[4], P0[16];
            // predict
#pragma unroll
            for (int r = 0; r < 4; ++r) Xn[r] = p.A[4 * r] * X[0] + p.A[4 * r + 1] * X[1] + p.A[4 * r + 2] * X[2] + p.A[4 * r + 3] * X[3];
            const T ex = Yx - (p.C[0] * Xn[0] + p.C[1] * Xn[1] + p.C[2] * Xn[2] + p.C[3] * Xn[3]);
            const T ey = Yy - (p.C[4] * Xn[0] + p.C[5] * Xn[1] + p.C[6] * Xn[2] + p.C[7] * Xn[3]);
            if (!stationary) { // (uniform: every lane carries the same numbers) covariance and gain
#pragma unroll
                for (int e = 0; e < 16; ++e) P0[e] = P[e];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) // M = P A'
                        M[4 * r + c] = P[4 * r] * p.A[4 * c] + P[4 * r + 1] * p.A[4 * c + 1]
                                       + P[4 * r + 2] * p.A[4 * c + 2] + P[4 * r + 3] * p.A[4 * c + 3];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        P[4 * r + c] = p.A[4 * r] * M[c] + p.A[4 * r + 1] * M[4 + c]
                                       + p.A[4 * r + 2] * M[8 + c] + p.A[4 * r + 3] * M[12 + c] + p.Q[4 * r + c];
                // update
                T G[8], S[4], Si[4], D[8], E[8]; // G = P C' [4][2], D = C' S^-1 [4][2], K [4][2], E = S K' [2][4]
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                        G[2 * r + c] = P[4 * r] * p.C[4 * c] + P[4 * r + 1] * p.C[4 * c + 1]
                                       + P[4 * r + 2] * p.C[4 * c + 2] + P[4 * r + 3] * p.C[4 * c + 3];
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                        S[2 * r + c] = p.R[2 * r + c] + (p.C[4 * r] * G[c] + p.C[4 * r + 1] * G[2 + c] + p.C[4 * r + 2] * G[4 + c] + p.C[4 * r + 3] * G[6 + c]);
                const T det = S[0] * S[3] - S[1] * S[2];
                Si[0] = S[3] / det, Si[1] = -S[1] / det, Si[2] = -S[2] / det, Si[3] = S[0] / det;
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 2; ++c) D[2 * r + c] = p.C[r] * Si[c] + p.C[4 + r] * Si[2 + c];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                        K[2 * r + c] = P[4 * r] * D[c] + P[4 * r + 1] * D[2 + c] + P[4 * r + 2] * D[4 + c] + P[4 * r + 3] * D[6 + c];
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) E[4 * r + c] = S[2 * r] * K[2 * c] + S[2 * r + 1] * K[2 * c + 1];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) P[4 * r + c] = P[4 * r + c] - (K[2 * r] * E[c] + K[2 * r + 1] * E[4 + c]);
                bool same = true;
#pragma unroll
                for (int e = 0; e < 16; ++e) same = same && kf_same_bits(P[e], P0[e]);
                stationary = same;
            }
            // the one place X is updated, with the gain just computed or the kept one
#pragma unroll
            for (int r = 0; r < 4; ++r) X[r] = Xn[r] + (K[2 * r] * ex + K[2 * r + 1] * ey);
        }
        // rows: offset 0 = the current position, offsets 1 .. N = A^t X with the same (P00, P11)
        T* rows = p.dyn_c + ((size_t)a * H + h) * (size_t)(N + 1) * 6;
        for (int t = 0; t <= N; ++t) {
            if (t > 0) {
                T Xn[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) Xn[r] = p.A[4 * r] * X[0] + p.A[4 * r + 1] * X[1] + p.A[4 * r + 2] * X[2] + p.A[4 * r + 3] * X[3];
#pragma unroll
                for (int r = 0; r < 4; ++r) X[r] = Xn[r];
            }
            if (lane == (t & 63)) {
                T* row = rows + (size_t)t * 6;
                row[0] = t == 0 ? cx : X[0];
                row[1] = t == 0 ? cy : X[1];
                row[2] = t == 0 ? p.human_size : P[0];
                row[3] = t == 0 ? p.human_size : P[5];
                row[4] = 0;
                row[5] = 1;
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) p.kf_P[b * 16 + i] = P[i];
    }
}

} // namespace nmpc
