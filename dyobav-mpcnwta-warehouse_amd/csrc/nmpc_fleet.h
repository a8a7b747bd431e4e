// nmpc_fleet.h -- closed-loop fleets: the other-robot blocks of the parameter vector filled from the peers, and the
// robot-robot clearance / collision of a time step; two kernels, one wavefront per running robot.
//
// The solver this project replaces is a fleet solver (reference = /root/reference/src): its parameter vector carries
// c_0 [3 Nother] and c [3 N Nother], "states / predicted states of other robots" (pkg_mpc_tracker/solver_build/
// mpc_builder.py:53-54), and its cost two fleet terms (mpc_builder.py:85-97, mpc_cost.py:65-76). A FLEET here is a group of
// R consecutive scenarios b = g R + i (1 <= R <= 64, B = G R) that share the static map and the pedestrians (replicated per
// member: loop_pre / loop_post are untouched).
//
//   fleet_exchange (between loop_pre and nmpc_assemble_params; writes nmpc_assemble_args.other_robots)
//     what a peer publishes  the reference's pred_states (pkg_mpc_tracker/trajectory_tracker.py:369-378): its CURRENT state
//                            rolled through ALL N controls of its previous solution, unshifted, with the MPC's motion
//                            model (UnicycleModel, RK4, motion_model.py:141-163 -- the closed form of loop_post_kernel):
//                            N states. Rolled from the peer's actual state this equals the reference's pred_states whenever
//                            the no-backward clip did not fire, and is the honest prediction when it did. A peer without a
//                            previous solution (U = nullptr: first step of a run) or with alive == 0 (completed or collided:
//                            a parked robot stays visible as an obstacle) is predicted AT REST at its current state.
//     block layout           per running robot [c_0 | c]: slot s of c_0 at 3 s; slot s of c at 3 Nother + s 3 N + 3 j,
//                            j = 0 .. N-1 (the builder slices c[kt*ns :: ns*N_hor]); c_0 = the peer's current state; theta
//                            is written although the cost ignores it.
//     slot 0 stays zero      in both parts: the builder skips slot 0 of c_0 (c_0[ns::ns]); a peer sits in the same slot of
//                            both parts, so the capacity is Nother - 1 peers. Unused slots are zeros, the reference's default
//                            (trajectory_tracker.py:295-296) -- the phantom robot at the world origin that this implies in
//                            the predictive term is existing behaviour of the cost, not something this stage adds or removes.
//     which peers            with more than Nother - 1 other members the nearest by current centre distance, nearest first,
//                            equal distances to the lower member index; slot s >= 1 holds the s-th nearest; never itself.
//                            Distances are compared through d2 = dx dx + dy dy, every operation rounded on its own
//                            (contraction off below), so that numpy's `dx * dx + dy * dy` in the same type has the same bits
//                            and decides the same.
//     every element of other_c[a] is written, zeros included: no call depends on what the buffer held.
//   fleet_post (after loop_post, on the same run list: every robot that ran this step)
//     clr_fleet[b]           running minimum of the distance to the other members' positions after the step (all moved in
//                            lock-step; parked ones stand where they stopped)
//     collision              distance <= vehicle_width = two radii, Robot(radius = vehicle_width / 2) (main_base.py:144), the
//                            `<=` of check_collision's pedestrian rule: collision = 1, complete = 0, alive = 0 -- a collision
//                            beats a completion reached in the same step (main_base.py:330-334).
//     A block writes only its own robot's flags and metrics and reads only positions, which no block of this launch writes:
//     no race. A parked robot is not in the run list, so its recorded outcome is never changed by a later hit.
//
// Mapping of the exchange, counted. Chosen: one wavefront per running robot, lane = group member. Lane l forms its key,
// ranks itself by counting the smaller (d2, index) keys of the R lanes (R shuffles, as select_static of nmpc_assemble.h does
// for M <= 64 polygons) and, with rank < Nother - 1, rolls its peer: N sequential steps of 3 sincos and ~12 flops. A group
// of R robots therefore rolls R min(R - 1, Nother - 1) peers where R rollouts would do: at R = 64, Nother = 10 that is 576
// against 64 per group, 9 x the arithmetic. But the rollouts of a wavefront run side by side in its lanes, so the wavefront's
// time is ONE rollout's latency (N dependent steps, ~N x 3 sincos) whatever the number of lanes rolling, and the 9 x is paid
// in lanes that would idle otherwise. The alternative -- one workgroup per group, every member rolled once into LDS
// (R x 3 N reals: 15 KB at R = 64, N = 20 in fp32), then R selections reading it -- saves those lanes' work but serialises R
// selections and R row stores (R x 3 (N + 1) Nother reals = 161 KB per group in fp32) behind one workgroup of <= 16
// wavefronts, i.e. 1 024 workgroups instead of 65 536 wavefronts at B = 65 536: the stage is a byte mover (the row it
// writes, 2.5 KB per robot in fp32 at the yaml dimensions, is what the time goes into) and the first mapping spreads those
// stores over the whole device with no cross-wavefront synchronisation. U rows of a group are read by up to R wavefronts,
// 160 B each, from L2. Measured on an MI355X (tools/bench_fleet.py, profiles/fleet_evaluate.json), 65 536
// robots in fp32: the exchange takes 0.15 % of a run at R = 8 and 0.13 % at R = 64, at most 0.27 ms = 0.3 % of its step's solve,
// against the 5 % the project allows a stage beside the solve -- so the second mapping is NOT built.
//
// The row is staged in LDS (3 (N + 1) Nother reals, dynamic): zeroed by all lanes, the rolling lanes scatter their slots,
// then all 64 lanes store it to memory in order -- coalesced, and the zeros cost no second pass over memory.
#pragma once

#include <hip/hip_runtime.h>

#include "nmpc_assemble.h"
#include "nmpc_step.h"
#include "wave_ops.h"

namespace nmpc {

template <typename T>
struct FleetParams {
    int B, R, n_run, N, Nother;
    const long long* run;        // [n_run] or nullptr = all B
    T ts, width;
    const T* robot;              // [B][3]
    const T* U;                  // [B][2N] previous solutions, or nullptr = none
    unsigned char *alive, *collision, *complete, *collision_fleet; // [B]; collision_fleet may be nullptr
    T* other_c;                  // [n_run][3 (N + 1) Nother]
    T* clr_fleet;                // [B]
};

// the key peers are ranked by: numpy's dx * dx + dy * dy, three roundings
template <typename T>
__device__ __forceinline__ T fleet_d2(T ax, T ay, T bx, T by)
{
#pragma clang fp contract(off)
    const T dx = ax - bx, dy = ay - by;
    const T dx2 = dx * dx, dy2 = dy * dy;
    return dx2 + dy2;
}

template <typename T>
__global__ __launch_bounds__(64) void fleet_exchange_kernel(FleetParams<T> p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fleet_smem[];
    T* row = reinterpret_cast<T*>(fleet_smem); // [3 (N + 1) Nother]
    const int a = blockIdx.x, lane = threadIdx.x;
    const long long bl = p.run ? p.run[a] : (long long)a;
    if (bl < 0 || bl >= p.B) return; // (a device-side list the host cannot validate: stay inside the arrays; block-uniform)
    const int b = (int)bl, N = p.N, R = p.R;
    const int g = b / R, me = b - g * R;
    const int len = 3 * (N + 1) * p.Nother, cap = p.Nother - 1;
    for (int e = lane; e < len; e += 64) row[e] = T(0);
    const bool member = lane < R && lane != me;
    const int m = g * R + (lane < R ? lane : me); // (idle lanes read the robot itself: inside the arrays)
    const T ox = p.robot[3 * b], oy = p.robot[3 * b + 1];
    T x = p.robot[3 * m], y = p.robot[3 * m + 1], th = p.robot[3 * m + 2];
    const T d = member ? fleet_d2(x, y, ox, oy) : T(INFINITY);
    int rank = 0;
    for (int j = 0; j < R; ++j) {
        const T dj = __shfl(d, j, 64);
        rank += (j != me && (dj < d || (dj == d && j < lane))) ? 1 : 0;
    }
    __syncthreads();
    if (member && rank < cap) {
        const int s = rank + 1;
        T* c0 = row + 3 * s;
        T* c = row + 3 * p.Nother + (size_t)s * 3 * N;
        c0[0] = x, c0[1] = y, c0[2] = th;
        const bool rest = p.U == nullptr || p.alive[m] == 0;
        const T* u = rest ? nullptr : p.U + (size_t)m * 2 * N;
        for (int j = 0; j < N; ++j) {
            if (!rest) { // UnicycleModel, RK4, in closed form: the expressions of loop_post_kernel
                const T v = u[2 * j], w = u[2 * j + 1];
                const T hh = T(0.5) * p.ts * w;
                T s0, k0, s1, k1, s2, k2;
                tsincos(th, s0, k0);
                tsincos(th + hh, s1, k1);
                tsincos(th + T(2) * hh, s2, k2);
                const T cc = (k0 + T(4) * k1 + k2) / T(6), ss = (s0 + T(4) * s1 + s2) / T(6);
                x = x + p.ts * v * cc;
                y = y + p.ts * v * ss;
                th = th + p.ts * w;
            }
            c[3 * j] = x, c[3 * j + 1] = y, c[3 * j + 2] = th;
        }
    }
    __syncthreads();
    T* out = p.other_c + (size_t)a * len;
    for (int e = lane; e < len; e += 64) out[e] = row[e];
}

template <typename T>
__global__ __launch_bounds__(64) void fleet_post_kernel(FleetParams<T> p)
{
    const int a = blockIdx.x, lane = threadIdx.x;
    const long long bl = p.run ? p.run[a] : (long long)a;
    if (bl < 0 || bl >= p.B) return;
    const int b = (int)bl, R = p.R;
    const int g = b / R, me = b - g * R;
    const T x = p.robot[3 * b], y = p.robot[3 * b + 1];
    T dmin = T(INFINITY);
    for (int l = lane; l < R; l += 64) {
        if (l == me) continue;
        const int m = g * R + l;
        const T d = thypot(x - p.robot[3 * m], y - p.robot[3 * m + 1]);
        dmin = d < dmin ? d : dmin;
    }
    dmin = wave_min(dmin);
    if (lane == 0) {
        p.clr_fleet[b] = dmin < p.clr_fleet[b] ? dmin : p.clr_fleet[b];
        if (dmin <= p.width) { // a collision beats a completion of the same step
            p.collision[b] = 1;
            p.complete[b] = 0;
            p.alive[b] = 0;
            if (p.collision_fleet) p.collision_fleet[b] = 1;
        }
    }
}

} // namespace nmpc
