// nmpc_capi.hip -- C ABI (include/nmpc_hip.h) over the gfx950 kernels in nmpc_device.h.
// Host side of the drop-in boundary for `solver.run(p)` of the reference
// (/root/reference/src/pkg_mpc_tracker/trajectory_tracker.py:54-66, :362). No CPU fallback: every entry point
// either launches the HIP kernels or returns an error code.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/nmpc_hip.h"
#include "nmpc_assemble.h"
#include "nmpc_device.h"
#include "nmpc_plan.h"
#include "nmpc_spec.h"
#include "nmpc_hypotheses.h"
#include "nmpc_step.h"
#include "nmpc_kf.h"
#include "nmpc_fleet.h"
#include "nmpc_dwa.h"
#include "nmpc_snap.h"
#include "nmpc_mmp.h"
#include "nmpc_mmp_stem.h"
#include "nmpc_mmp_block.h"
#include "nmpc_mmp_block2.h"
#include "nmpc_mmp_block1_f16.h"
#include "nmpc_mmp_block2_f16.h"
#include "nmpc_mmp_block3.h"
#include "nmpc_mmp_block3_f16.h"
#include "nmpc_mmp_block4.h"
#include "nmpc_mmp_block4_f16.h"
#include "nmpc_mmp_head.h"

using namespace nmpc_plan;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                        \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return fail(e_ == hipErrorOutOfMemory ? NMPC_ERR_OUT_OF_MEMORY : NMPC_ERR_HIP, "%s: %s", #expr, \
                        hipGetErrorString(e_));                                                              \
    } while (0)

// grow-only device buffer, freed when it goes out of scope (or with the handle that holds it)
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) return fail(NMPC_ERR_OUT_OF_MEMORY, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
        cap = bytes;
        return 0;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

bool is_device_ptr(const void* ptr)
{
    if (!ptr) return false;
    hipPointerAttribute_t a;
    hipError_t e = hipPointerGetAttributes(&a, ptr);
    if (e != hipSuccess) {
        (void)hipGetLastError(); // plain host memory: clear the sticky error
        return false;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

} // namespace

struct nmpc_handle_s {
    nmpc_config cfg;
    Layouts lays;  // the four layouts and lanes per step (nmpc_plan.h)
    int n_simd = 0; // SIMDs of the device (4 per CU): latency_waves = 0 picks the wavefront count from B / n_simd
    bool spec_ok[2] = {true, true}; // [f32, f64]
    bool coop_ok[2] = {true, true};
    int last_mode = 0;              // kernel of the last solve: 0 throughput, 1 latency (speculative), 2 cooperative
    int last_axis = -1;             // axis-aligned variant: -1 not applicable, 0 general only, 1 AXIS only, 2 decided on the device
    int last_staged = 0;            // pilot outer iterations of the last solve (0 = one launch)
    int last_polish_selected = 0, last_polish_converged = -1;
    template <typename T>
    const Layout& lay() const
    {
        return lays.main(sizeof(T));
    }
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int last_tail = 0;              // tail hand-off of the last solve: the parking threshold it ran with (0 = none)
    int last_order = 0;             // dispatch order of the last solve: 0 index order, 1 the caller's, 2 one evaluation, 3 a pilot launch
    bool timed = false;
    int ptr_mode = NMPC_PTR_DETECT;
    DevBuf dP, dU, dcost, dstatus, diters, du0, dy, dc0, dinfo, dY2, dC2, dpsi, dgrad, df2, dws;
    DevBuf dorder;   // dispatch order of the next solves (nmpc_set_dispatch_order), order_B entries; 0 = none
    int order_B = 0;
    DevBuf dflag;    // [0]: epoch of the last call whose batch had an ellipse with angle != 0 (KParams::axis_flag)
    int axis_epoch = 0;
    DevBuf dresume, dorder2, dhist; // resumable solve: parked states, ranked order of the second launch, bucket counters
    DevBuf ddeep;                   // tail hand-off: solver states parked inside an inner solve (KParams::deep)
    DevBuf dproxy;                  // dispatch order from one evaluation (run_solve): nominal controls, zeros, penalties, psi, ||F2||^2
    // polish: compact fp64 copies of the selected instances and their results
    DevBuf psel, pP, pU0, pY, pC, pU, pcost, pstatus, piters, pinfo;
    std::vector<int32_t> host_status, host_sel;
    // nmpc_set_map: occupancy mask [map_h][map_w] and the row-major list of edge pixels (col | row << 16), zero-padded
    DevBuf dmap_occ, dmap_edge;
    int map_h = 0, map_w = 0, map_n_edge = 0, map_n_edge_pad = 0;
};

namespace {

// waves per SIMD a kernel variant is compiled for: the large register table needs the 256-register budget
template <typename T, int RS>
constexpr int wpe(int f32_default)
{
    return sizeof(T) == 8 ? (RS > 0 ? 1 : NMPC_WPE_F64) : RS >= kRegSlotsLarge ? 2 : RS > 0 ? 3 : f32_default;
}
// (register-table kernels exist per code path -- general / axis-aligned -- see KParams::axis_mode)
template <typename T, int LPS, int RS>
constexpr bool kHasAxisVariant = LPS == 3 && RS > 0;

// ONLY: 1 / 2 = the axis-aligned / the general path alone, returning at once when the launch takes the other one -- how every
// register-table kernel is built and launched since round 4 (solve_kernel_of below). (0 = both paths inlined into one kernel,
// chosen per workgroup: round 3's fp32 form, no longer instantiated. In fp64 that form never worked: the 512-register
// kernel computed garbage on the general path, nondeterministically, while each path compiled alone is right -- it was
// 142 KB of code, beyond the +-128 KB reach of s_cbranch, its far branches relaxed into s_getpc / s_setpc sequences;
// tests/test_kernel_resources_cpu.py keeps every kernel below that size.)
template <typename T, int LPS, bool GLB, int RS = 0, int ONLY = 0>
__global__ __launch_bounds__(64, (wpe<T, RS>(NMPC_WPE_F32))) void solve_kernel(nmpc::KParams<T> kp)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if constexpr (kHasAxisVariant<T, LPS, RS> && !GLB) {
        const bool axis = nmpc::axis_path(kp);
        if (ONLY != 0 && axis != (ONLY == 1)) return; // (a pair: the twin of the path this launch takes returns at once)
        const int inst = nmpc::dispatch_index(kp);
        if (nmpc::finished_in_pilot<T>(inst)) return;
        if (ONLY != 2 && axis) {
            nmpc::solve_instance<T, LPS, GLB, RS, false, false, true>(kp, inst, reinterpret_cast<T*>(smem));
            return;
        }
        if constexpr (ONLY != 1) nmpc::solve_instance<T, LPS, GLB, RS>(kp, inst, reinterpret_cast<T*>(smem));
    } else {
        const int inst = nmpc::dispatch_index(kp);
        if (nmpc::finished_in_pilot<T>(inst)) return;
        nmpc::solve_instance<T, LPS, GLB, RS>(kp, inst, reinterpret_cast<T*>(smem));
    }
}

// diagnostic: the one-wavefront fp64 solver (LDS / global table) writing one record per inner iteration (KParams::trace)
template <int LPS, bool GLB>
__global__ __launch_bounds__(64, NMPC_WPE_F64) void trace_kernel(nmpc::KParams<double> kp)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    nmpc::solve_instance<double, LPS, GLB, 0, false, false, false, true>(kp, (int)blockIdx.x, reinterpret_cast<double*>(smem));
}

// cooperative mode: up to kSpecWaves wavefronts per instance share every evaluation (nmpc_device.h, COOP)
// GLB: a PAIR like the register-table kernels -- ONLY = 1: the compressed table of axis-aligned ellipses (5 instead of 9
// values streamed per entry, nmpc_device.h Instance::CMP), ONLY = 2: the general table; the member the launch does not take
// returns at once (KParams::axis_mode). ONLY = 0: no variants (table in LDS).
template <typename T, int LPS, bool GLB, int ONLY = 0>
__global__ __launch_bounds__(64 * kSpecWaves, (sizeof(T) == 4 ? NMPC_SPEC_WPE_F32 : NMPC_WPE_F64)) void solve_coop_kernel(nmpc::KParams<T> kp)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if constexpr (ONLY != 0) {
        static_assert(GLB, "the compressed table is a variant of the global one");
        if (nmpc::axis_path(kp) != (ONLY == 1)) return;
    }
    const int inst = nmpc::dispatch_index(kp);
    if (nmpc::finished_in_pilot<T>(inst)) return;
    nmpc::solve_instance<T, LPS, GLB, 0, true, false, ONLY == 1>(kp, inst, reinterpret_cast<T*>(smem));
}
// ... with the obstacle table on chip instead of in global memory, for one lane per horizon step (N > 32), where it does
// not fit LDS: EIGHT wavefronts (two per SIMD) keep 12 rows each in registers, the remaining rows live in LDS
template <bool HLP>
__global__ __launch_bounds__(64 * kCoopRegWaves, 2) void solve_coop_reg_kernel(nmpc::KParams<float> kp)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int inst = nmpc::dispatch_index(kp);
    if (nmpc::finished_in_pilot<float>(inst)) return;
    nmpc::solve_instance<float, 1, false, kRegSlotsCoop, true, HLP>(kp, inst, reinterpret_cast<float*>(smem));
}

// latency mode: kSpecWaves wavefronts per instance, speculative line search (nmpc_spec.h)
// FLAT = false: the TAIL member (nmpc_spec.h) -- this kernel with the throughput kernels' evaluation, bit-identical to them
template <typename T, int LPS, bool GLB, int RS = 0, int ONLY = 0, bool FLAT = true>
__global__ __launch_bounds__(64 * kSpecWavesMax, (wpe<T, RS>(NMPC_SPEC_WPE_F32))) void solve_spec_kernel(nmpc::KParams<T> kp)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if constexpr (kHasAxisVariant<T, LPS, RS> && !GLB) {
        const bool axis = nmpc::axis_path(kp);
        if (ONLY != 0 && axis != (ONLY == 1)) return; // (a pair: the twin of the path this launch takes returns at once)
        const int inst = nmpc::dispatch_index(kp);
        if (nmpc::finished_in_pilot<T>(inst)) return;
        if (ONLY != 2 && axis) {
            nmpc::solve_instance_spec<T, LPS, GLB, RS, true, FLAT>(kp, inst, reinterpret_cast<T*>(smem));
            return;
        }
        if constexpr (ONLY != 1) nmpc::solve_instance_spec<T, LPS, GLB, RS, false, FLAT>(kp, inst, reinterpret_cast<T*>(smem));
    } else {
        const int inst = nmpc::dispatch_index(kp);
        if (nmpc::finished_in_pilot<T>(inst)) return;
        nmpc::solve_instance_spec<T, LPS, GLB, RS, false, FLAT>(kp, inst, reinterpret_cast<T*>(smem));
    }
}

template <typename T, int LPS, bool GLB, int RS, bool AXIS>
__device__ __forceinline__ void eval_instance(const nmpc::KParams<T>& kp, const nmpc::EvalParams<T>& ep, T* lds)
{
    const int inst = blockIdx.x, N = kp.N;
    nmpc::Instance<T, LPS, GLB, RS, false, false, AXIS> I(kp, kp.P + (size_t)inst * kp.np, lds,
                                                        GLB ? kp.ws + (long long)inst * kp.ws_stride : nullptr);
    if (I.load()) { // (not evaluated: every output of the instance is NaN)
        if (I.lane == 0) {
            ep.psi[inst] = __builtin_nanf("");
            if (ep.f2sq) ep.f2sq[inst] = __builtin_nanf("");
        }
        if (ep.grad)
            for (int j = threadIdx.x; j < 2 * N; j += blockDim.x) ep.grad[(size_t)inst * 2 * N + j] = __builtin_nanf("");
        return;
    }
    const int kk = I.act ? I.k : 0;
    T v = ep.U[(size_t)inst * 2 * N + 2 * kk], w = ep.U[(size_t)inst * 2 * N + 2 * kk + 1];
    T yv = ep.Y[(size_t)inst * 2 * N + kk], yw = ep.Y[(size_t)inst * 2 * N + N + kk];
    if (!I.act) v = w = yv = yw = 0;
    const T c = ep.C[inst];
    const T icd = T(1) / (c > T(1) ? c : T(1));
    T psi, f2, gv, gw;
    if (ep.grad)
        I.template eval<true>(v, w, c, icd, yv, yw, psi, f2, gv, gw);
    else
        I.template eval<false>(v, w, c, icd, yv, yw, psi, f2, gv, gw);
    if (I.lead && ep.grad) {
        ep.grad[(size_t)inst * 2 * N + 2 * I.k] = gv;
        ep.grad[(size_t)inst * 2 * N + 2 * I.k + 1] = gw;
    }
    if (I.lane == 0) {
        ep.psi[inst] = psi;
        if (ep.f2sq) ep.f2sq[inst] = f2;
    }
}
template <typename T, int LPS, bool GLB, int RS = 0, int ONLY = 0>
__global__ __launch_bounds__(64, 1) void eval_kernel(nmpc::KParams<T> kp, nmpc::EvalParams<T> ep)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if constexpr (kHasAxisVariant<T, LPS, RS> && !GLB) {
        const bool axis = nmpc::axis_path(kp);
        if (ONLY != 0 && axis != (ONLY == 1)) return;
        if (ONLY != 2 && axis) {
            eval_instance<T, LPS, GLB, RS, true>(kp, ep, reinterpret_cast<T*>(smem));
            return;
        }
    }
    if constexpr (ONLY != 1) eval_instance<T, LPS, GLB, RS, false>(kp, ep, reinterpret_cast<T*>(smem));
}

// ---- small data kernels around the solves ------------------------------------------------------------------------
// Is some ellipse of the batch not axis-aligned (angle != 0)? One workgroup per instance over o_d[j][t][4]; any
// workgroup that finds a non-zero angle stores the call's epoch in *flag (plain store: all writers agree).
template <typename T>
__global__ __launch_bounds__(256) void axis_scan_kernel(const T* P, int np, int off_od, int n_entries, int* flag, int epoch)
{
    const T* s = P + (size_t)blockIdx.x * np + off_od;
    bool skew = false;
    for (int e = threadIdx.x; e < n_entries; e += 256) skew = skew || s[6 * e + 4] != T(0);
    if (skew) *flag = epoch; // (this call's epoch: the flag needs no reset between calls)
}

// Resumable solve, ranking of the next launch: counting sort, descending, of a key the parked state holds -- key 0: the
// hard-constraint violation ||F2|| (bucket = the top 10 bits of the float: monotonic for values >= 0), key 1: the psi
// evaluations used so far (64 per bucket). Finished instances -- and only they -- go to bucket 0.
constexpr int kRankBuckets = 1024;
template <typename T>
__device__ __forceinline__ int rank_bucket(const T* resume, const int* status, int b, int key)
{
    if (status[b] != -1) return 0;
    const T* sc = resume + (size_t)b * nmpc::kResumeStride + 6 * 64;
    unsigned bits;
    if (key == 0) {
        const float f = (float)sc[3];
        bits = __float_as_uint(f >= 0.0f ? f : 0.0f) >> 21;
    } else {
        bits = (unsigned)((int)sc[7]) >> 6;
    }
    // (an unfinished instance never shares bucket 0 with the finished ones -- ||F2|| = 0 is common: no obstacle in reach --:
    //  the launch that follows counts on the unfinished instances standing FIRST in its order, and on their number, offs[0])
    return (int)(bits < 1u ? 1u : bits < (unsigned)kRankBuckets ? bits : (unsigned)kRankBuckets - 1u);
}
template <typename T>
__global__ __launch_bounds__(256) void rank_hist_kernel(const T* resume, const int* status, int B, int* hist, int key)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    const int q = b < B ? rank_bucket(resume, status, b, key) : -1;
    // Bucket 0 -- the instances that finished in the pilot, half of a `passing`-type batch -- is counted once per wavefront:
    // 34 k atomics on one address took 0.41 ms here and again in the scatter (profiles/r05_cfg2_passing_kernel_timeline.txt).
    const unsigned long long m0 = __ballot(q == 0);
    if (q > 0) atomicAdd(&hist[q], 1);
    else if (q == 0 && (int)(threadIdx.x & 63) == __ffsll((long long)m0) - 1) atomicAdd(&hist[0], __popcll(m0));
}
// (tail hand-off under a caller's dispatch order, no ranking before the launch: all B instances are to be solved)
__global__ void dyn_init_kernel(int* dyn_ctr, int total) { dyn_ctr[0] = 0, dyn_ctr[1] = 0, dyn_ctr[2] = total, dyn_ctr[3] = 0; }
// offs[q] = number of instances in buckets above q (one workgroup of kRankBuckets threads; reversed inclusive scan)
// (the counters are left zeroed for the next ranking: no memset between launches)
__global__ __launch_bounds__(kRankBuckets) void rank_scan_kernel(int* hist, int* offs, int* dyn_ctr)
{
    __shared__ int sh[kRankBuckets];
    const int t = threadIdx.x;                 // t = 0 is the top bucket
    const int mine = hist[kRankBuckets - 1 - t];
    hist[kRankBuckets - 1 - t] = 0;
    sh[t] = mine;
    __syncthreads();
    for (int d = 1; d < kRankBuckets; d <<= 1) {
        const int add = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    offs[kRankBuckets - 1 - t] = sh[t] - mine;
    // (tail hand-off, KParams::dyn_ctr: the launch that follows has offs[0] unfinished instances to solve -- everything above bucket 0)
    if (dyn_ctr && t == kRankBuckets - 1) dyn_ctr[0] = 0, dyn_ctr[1] = 0, dyn_ctr[2] = sh[t] - mine, dyn_ctr[3] = 0;
}
template <typename T>
__global__ __launch_bounds__(256) void rank_scatter_kernel(const T* resume, const int* status, int B, int* offs, int* order, int key)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    const int q = b < B ? rank_bucket(resume, status, b, key) : -1;
    const unsigned long long m0 = __ballot(q == 0);
    if (q > 0) {
        order[atomicAdd(&offs[q], 1)] = b;
    } else if (q == 0) { // one atomic per wavefront for the finished instances (see rank_hist_kernel)
        const int lane = (int)(threadIdx.x & 63), leader = __ffsll((long long)m0) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(&offs[0], __popcll(m0));
        base = __shfl(base, leader);
        order[base + __popcll(m0 & ((1ull << lane) - 1ull))] = b;
    }
}

// Dispatch order of a latency-plan batch from ONE evaluation instead of a pilot launch (run_solve): the nominal controls
// (v_nom, 0) at every step, zero multipliers, the initial penalty; and the key -- ||F2||^2 there -- written where rank_bucket
// reads it (every instance counts as unfinished: nothing has been solved yet).
template <typename T>
__global__ __launch_bounds__(256) void proxy_fill_kernel(T* U, T* Y, T* C, int B, int n, T v_nom, T c_init)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)B * n) {
        U[i] = (i & 1) ? T(0) : v_nom;
        Y[i] = T(0);
    }
    if (i < (size_t)B) C[i] = c_init;
}
template <typename T>
__global__ __launch_bounds__(256) void proxy_key_kernel(const T* f2sq, T* resume, int* status, int B)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) {
        status[b] = -1;
        resume[(size_t)b * nmpc::kResumeStride + 6 * 64 + 3] = f2sq[b];
    }
}

// Polish: fp64 copies of the selected instances' parameters and of the main solve's (u, y, c) / results back into the
// caller's arrays where the continuation converged (nmpc_config.polish)
template <typename T>
__global__ __launch_bounds__(256) void polish_gather_kernel(const T* P, const T* U, const T* y, const T* info, const int* sel,
                                                            int np, int n2, double* P64, double* U64, double* Y64, double* C64)
{
    const int i = blockIdx.x, b = sel[i];
    const T* src = P + (size_t)b * np;
    double* dst = P64 + (size_t)i * np;
    for (int j = threadIdx.x; j < np; j += 256) dst[j] = (double)src[j];
    if ((int)threadIdx.x < n2) {
        U64[(size_t)i * n2 + threadIdx.x] = (double)U[(size_t)b * n2 + threadIdx.x];
        Y64[(size_t)i * n2 + threadIdx.x] = (double)y[(size_t)b * n2 + threadIdx.x];
    }
    if (threadIdx.x == 0) C64[i] = (double)info[(size_t)b * 8 + 3];
}
// (info[:, 6] is the polish outcome when the polish is on: 0 for the instances it does not touch)
template <typename T>
__global__ __launch_bounds__(256) void polish_clear_flag_kernel(T* info, int B)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) info[(size_t)b * 8 + 6] = T(0);
}
template <typename T>
__global__ __launch_bounds__(128) void polish_scatter_kernel(const int* sel, const double* U64, const double* Y64, const double* cost64,
                                                            const int* status64, const int* iters64, const double* info64, int n2,
                                                            T* U, T* y, bool y_user, T* cost, int* iters, T* info, bool info_user)
{
    const int i = blockIdx.x, b = sel[i], t = threadIdx.x;
    const bool ok = status64[i] == 0;
    if (ok && t < n2) {
        U[(size_t)b * n2 + t] = (T)U64[(size_t)i * n2 + t];
        if (y_user) y[(size_t)b * n2 + t] = (T)Y64[(size_t)i * n2 + t];
    }
    if (t == 0) {
        if (ok && cost) cost[b] = (T)cost64[i];
        if (iters) {
            iters[2 * b] += iters64[2 * i];
            iters[2 * b + 1] += iters64[2 * i + 1];
        }
        if (info_user) {
            T* o = info + (size_t)b * 8;
            const double* q = info64 + (size_t)i * 8;
            if (ok) o[0] = (T)q[0], o[1] = (T)q[1], o[2] = (T)q[2], o[3] = (T)q[3];
            o[4] += (T)q[4];
            o[5] += (T)q[5];
            o[6] = ok ? T(1) : T(2);
        }
    }
}

// wave-primitive self test: integer-valued data so that every summation order gives the same float
template <typename T>
__global__ __launch_bounds__(64) void selftest_kernel(int* fails)
{
    const int lane = threadIdx.x & 63;
    int bad = 0;
    for (int round = 0; round < 8; ++round) {
        const T x = T(((lane * 37 + round * 11) % 23) - 9);
        if (nmpc::wave_sum(x) != nmpc::ref_wave_sum(x)) bad |= 1;
        if (nmpc::wave_scan_incl(x) != nmpc::ref_wave_scan_incl(x)) bad |= 2;
        if (nmpc::wave_scan_suffix_incl(x) != nmpc::ref_wave_scan_suffix_incl(x)) bad |= 4;
        const T up3 = nmpc::wave_shift_up<3>(x), up3r = __shfl_up(x, 3, 64);
        if (up3 != (lane >= 3 ? up3r : T(0))) bad |= 8;
        const T dn2 = nmpc::wave_shift_down<2>(x), dn2r = __shfl_down(x, 2, 64);
        if (dn2 != (lane < 62 ? dn2r : T(0))) bad |= 16;
        if (nmpc::wave_reverse(x) != __shfl(x, 63 - lane, 64)) bad |= 32;
        {
            T a = x, b = T(3) - x;
            nmpc::wave_scan_incl2(a, b);
            if (a != nmpc::ref_wave_scan_incl(x) || b != nmpc::ref_wave_scan_incl(T(3) - x)) bad |= 128;
            T c = x, d = T(2) * x;
            nmpc::wave_scan_suffix_incl2(c, d);
            if (c != nmpc::ref_wave_scan_suffix_incl(x) || d != nmpc::ref_wave_scan_suffix_incl(T(2) * x)) bad |= 256;
            T s1, s2, s3;
            nmpc::wave_sum2(x, T(1) + x, s1, s2);
            if (s1 != nmpc::ref_wave_sum(x) || s2 != nmpc::ref_wave_sum(T(1) + x)) bad |= 512;
            nmpc::wave_sum3(x, T(2) - x, T(5) * x, s1, s2, s3);
            if (s1 != nmpc::ref_wave_sum(x) || s2 != nmpc::ref_wave_sum(T(2) - x) || s3 != nmpc::ref_wave_sum(T(5) * x)) bad |= 1024;
        }
        if (nmpc::read_lane(x, 17) != __shfl(x, 17, 64)) bad |= 64;
        {
            int a[4];
            nmpc::class3_addresses(lane % 3, a);
            T c1 = x, c2 = T(4) - x;
            nmpc::class3_sum2(c1, c2, a);
            if (c1 != nmpc::ref_class3_sum(x) || c2 != nmpc::ref_class3_sum(T(4) - x)) bad |= 2048;
        }
    }
    if (sizeof(T) == 4) { // sincos_medium against the library on its whole range, sign and quadrant boundaries included
        for (int round = 0; round < 64; ++round) {
            const int i = round * 64 + lane;
            float x = (float)((i * 2654435761u) >> 8) * (1.0f / 16777216.0f);            // [0, 1)
            x = (i & 3) == 0 ? x * 8.0f - 4.0f : (i & 3) == 1 ? (x - 0.5f) * 200.0f : (i & 3) == 2 ? (x - 0.5f) * 2.6e5f
                                                                                                : 0.78539816f * (float)((i >> 2) % 17 - 8) + (x - 0.5f) * 1e-4f;
            float s1, c1, s2, c2;
            sincosf(x, &s1, &c1);
            nmpc::sincos_medium(x, s2, c2);
            if (__builtin_bit_cast(unsigned, s1) != __builtin_bit_cast(unsigned, s2) ||
                __builtin_bit_cast(unsigned, c1) != __builtin_bit_cast(unsigned, c2)) bad |= 4096;
        }
    }
    if (bad) atomicOr(fails, bad);
}

// nmpc_probe_*: ONE product function per kernel, every lane's result stored (include/nmpc_hip.h, nmpc_probe_op). One kernel
// per (op, T), so that no primitive's schedule depends on another's; the wave-uniform guard on the wave index is the only
// control flow. Wave w reads in[w][4][64] and writes out[w][6][64] (rows an op does not produce: 0).
constexpr int kProbeLps = 3; // lanes per horizon step of the shipped configurations: the shift counts and classes of the compositions
template <int OP, typename T>
__global__ __launch_bounds__(256) void probe_kernel(const T* __restrict__ in, T* __restrict__ out, int n_waves)
{
    const int wave = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); // (<= n_waves + 3: no overflow)
    if (wave >= n_waves) return;
    const int lane = (int)(threadIdx.x & 63);
    const T* src = in + (size_t)wave * (4 * 64) + lane;
    const T x0 = src[0], x1 = src[64], x2 = src[128], x3 = src[192];
    T o0 = 0, o1 = 0, o2 = 0, o3 = 0, o4 = 0, o5 = 0;
    if constexpr (OP == NMPC_PROBE_WAVE_SUM) {
        o0 = nmpc::wave_sum(x0);
    } else if constexpr (OP == NMPC_PROBE_WAVE_SUM2) {
        nmpc::wave_sum2(x0, x1, o0, o1);
    } else if constexpr (OP == NMPC_PROBE_WAVE_SUM3) {
        nmpc::wave_sum3(x0, x1, x2, o0, o1, o2);
    } else if constexpr (OP == NMPC_PROBE_WAVE_SCAN_INCL) {
        o0 = nmpc::wave_scan_incl(x0);
    } else if constexpr (OP == NMPC_PROBE_WAVE_SCAN_INCL2) {
        o0 = x0, o1 = x1;
        nmpc::wave_scan_incl2(o0, o1);
    } else if constexpr (OP == NMPC_PROBE_WAVE_SCAN_SUFFIX_INCL) {
        o0 = nmpc::wave_scan_suffix_incl(x0);
    } else if constexpr (OP == NMPC_PROBE_WAVE_SCAN_SUFFIX_INCL2) {
        o0 = x0, o1 = x1;
        nmpc::wave_scan_suffix_incl2(o0, o1);
    } else if constexpr (OP == NMPC_PROBE_WAVE_SUFFIX_FIX_ROWS) {
        o0 = nmpc::wave_suffix_fix_rows(x0);
    } else if constexpr (OP == NMPC_PROBE_CLASS3_SUM2) {
        int a[4];
        nmpc::class3_addresses(lane % 3, a);
        o0 = x0, o1 = x1;
        nmpc::class3_sum2(o0, o1, a);
    } else if constexpr (OP == NMPC_PROBE_CLASS3_SUM1) {
        int a[4];
        nmpc::class3_addresses(lane % 3, a);
        o0 = x0;
        nmpc::class3_sum1(o0, a);
    } else if constexpr (OP == NMPC_PROBE_CLASS3_ISSUE1_FINISH1) {
        int a[4];
        nmpc::class3_addresses(lane % 3, a);
        nmpc::Class3Pending1<T> pend;
        nmpc::class3_issue1(x0, a, pend);
        o0 = nmpc::class3_finish1(pend);
    } else if constexpr (OP == NMPC_PROBE_CLASS3_ADDRESSES) {
        int a[4];
        nmpc::class3_addresses(lane % 3, a);
        o0 = T(a[0]), o1 = T(a[1]), o2 = T(a[2]), o3 = T(a[3]);
    } else if constexpr (OP == NMPC_PROBE_WAVE_REVERSE) {
        o0 = nmpc::wave_reverse(x0);
    } else if constexpr (OP == NMPC_PROBE_READ_LANE) { // (the lanes the kernels read: the row starts of the suffix scan, the last tail lane, 63)
        o0 = nmpc::read_lane(x0, 0), o1 = nmpc::read_lane(x0, 16), o2 = nmpc::read_lane(x0, 32);
        o3 = nmpc::read_lane(x0, 48), o4 = nmpc::read_lane(x0, 57), o5 = nmpc::read_lane(x0, 63);
    } else if constexpr (OP == NMPC_PROBE_BPERM) {
        o0 = nmpc::bperm(x0, (int)x1);
    } else if constexpr (OP == NMPC_PROBE_WAVE_SHIFT_UP_1) {
        o0 = nmpc::wave_shift_up<1>(x0);
    } else if constexpr (OP == NMPC_PROBE_WAVE_SHIFT_UP_3) {
        o0 = nmpc::wave_shift_up<3>(x0);
    } else if constexpr (OP == NMPC_PROBE_WAVE_SHIFT_DOWN_1) {
        o0 = nmpc::wave_shift_down<1>(x0);
    } else if constexpr (OP == NMPC_PROBE_WAVE_SHIFT_DOWN_2) {
        o0 = nmpc::wave_shift_down<2>(x0);
    } else if constexpr (OP == NMPC_PROBE_WAVE_SHIFT_DOWN_3) {
        o0 = nmpc::wave_shift_down<3>(x0);
    } else if constexpr (OP == NMPC_PROBE_ROLLOUT_PREFIX) { // nmpc_device.h, rollout: the heading prefix and its shift by one step
        o1 = nmpc::wave_scan_incl(x0);
        o0 = nmpc::wave_shift_up<kProbeLps>(o1);
    } else if constexpr (OP == NMPC_PROBE_ADJOINT_SUFFIX) { // nmpc_device.h, adjoint: step totals at the tail lane, two suffix sums, the shift back
        const bool tail = lane % kProbeLps == kProbeLps - 1;
        T Gx = x0, Gy = x1;
        T a = x0, b = x1;
#pragma unroll
        for (int i = 1; i < kProbeLps; ++i) {
            a = nmpc::wave_shift_up<1>(a);
            b = nmpc::wave_shift_up<1>(b);
            Gx += a;
            Gy += b;
        }
        T Lx = tail ? Gx : T(0), Ly = tail ? Gy : T(0);
        nmpc::wave_scan_suffix_incl2(Lx, Ly);
        const T Mx = nmpc::wave_scan_suffix_incl(tail ? Lx : T(0));
        o2 = nmpc::wave_shift_down<kProbeLps>(Mx);
        const T My = nmpc::wave_scan_suffix_incl(tail ? Ly : T(0));
        o3 = nmpc::wave_shift_down<kProbeLps>(My);
        o0 = Lx, o1 = Ly;
    } else if constexpr (OP == NMPC_PROBE_CLASS_SUMS_BY_WAVE_SUM3) { // nmpc_device.h, obstacle passes on the LDS / global table
        const int r = lane % 3;
        nmpc::wave_sum3(r == 0 ? x0 : T(0), r == 1 ? x0 : T(0), r == 2 ? x0 : T(0), o0, o1, o2);
    } else if constexpr (OP == NMPC_PROBE_SINCOS_MEDIUM) {
        if constexpr (sizeof(T) == 4) {
            nmpc::sincos_medium(x0, o0, o1);
            sincosf(x0, &o2, &o3);
        }
    } else if constexpr (OP == NMPC_PROBE_SINCOS_SMALL) {
        if constexpr (sizeof(T) == 4) {
            nmpc::sincos_small(x0, o0, o1);
            sincosf(x0, &o2, &o3);
        }
    } else if constexpr (OP == NMPC_PROBE_FAST_RCP) {
        o0 = nmpc::fast_rcp(x0);
        o1 = T(1) / x0;
    } else if constexpr (OP == NMPC_PROBE_LS_POINT) {
        o0 = nmpc::ls_point(x0, x1, x2, x3);
    } else if constexpr (OP == NMPC_PROBE_WAVE_SCAN_SUFFIX_INCL_MASKED) {
        if constexpr (sizeof(T) == 4) o0 = nmpc::wave_scan_suffix_incl_masked(x0);
    } else if constexpr (OP == NMPC_PROBE_WAVE_SCAN_SUFFIX_INCL2_MASKED) {
        if constexpr (sizeof(T) == 4) {
            o0 = x0, o1 = x1;
            nmpc::wave_scan_suffix_incl2_masked(o0, o1);
        }
    } else if constexpr (OP == NMPC_PROBE_WAVE_SUFFIX_FIX_ROWS_MASKED) {
        if constexpr (sizeof(T) == 4) o0 = nmpc::wave_suffix_fix_rows_masked(x0);
    }
    T* dst = out + (size_t)wave * (6 * 64) + lane;
    dst[0] = o0, dst[64] = o1, dst[128] = o2, dst[192] = o3, dst[256] = o4, dst[320] = o5;
}
template <typename T>
using ProbeFn = void (*)(const T*, T*, int);
template <typename T, int... OP>
ProbeFn<T> probe_kernel_of(int op, std::integer_sequence<int, OP...>)
{
    static constexpr ProbeFn<T> table[] = {probe_kernel<OP, T>...};
    return table[op];
}

// The layout-dependent fields only (parameter offsets, LDS map): what a kernel choice that brings its own layout re-fills,
// leaving the batch buffers and -- ADVICE r3 -- the solver options of the caller (the polish's tolerances and caps) alone.
template <typename T>
void fill_layout(nmpc::KParams<T>& k, const Layout& L)
{
    k.np = L.np;
    k.dyn_cap = L.dyn_cap;
    k.off_rs = L.off_rs;
    k.off_rv = L.off_rv;
    k.off_c0 = L.off_c0;
    k.off_c = L.off_c;
    k.off_os = L.off_os;
    k.off_od = L.off_od;
    k.off_qstc = L.off_qstc;
    k.off_qdyn = L.off_qdyn;
    k.lds_alpha = L.lds_alpha;
    k.lds_poly = L.lds_poly;
    k.lds_seg = L.lds_seg;
    k.lds_seginv = L.lds_seginv;
    k.lds_fl0 = L.lds_fl0;
    k.lds_fl = L.lds_fl;
    k.lds_iflag = L.lds_iflag;
    k.lds_hist = L.lds_hist;
    k.lds_rho = L.lds_rho;
    k.lds_total = L.lds_total;
    k.lds_xch = L.lds_xch;
    k.lds_park = L.lds_park;
    k.lds_deepsc = L.lds_deepsc;
    k.coop_lanes = L.coop_lanes;
    k.lds_t0c = L.lds_t0c;
    k.lds_left = L.lds_left;
    k.lds_left_alpha = L.lds_left_alpha;
}

template <typename T>
void fill_kparams(const nmpc_handle_s* h, nmpc::KParams<T>& k, const Layout* layout = nullptr)
{
    const nmpc_config& c = h->cfg;
    std::memset(&k, 0, sizeof k);
    fill_layout(k, layout ? *layout : h->lay<T>());
    k.N = c.N_hor;
    k.Nother = c.Nother;
    k.Nstc = c.Nstcobs;
    k.Ndyn = c.Ndynobs;
    k.ts = (T)c.ts;
    k.inv_ts = (T)(1.0 / c.ts);
    k.vmin = (T)c.lin_vel_min;
    k.vmax = (T)c.lin_vel_max;
    k.wmax = (T)c.ang_vel_max;
    k.amin = (T)c.lin_acc_min;
    k.amax = (T)c.lin_acc_max;
    k.wamax = (T)c.ang_acc_max;
    k.safe2 = (T)(c.vehicle_width * c.vehicle_width);
    k.vm = (T)c.vehicle_margin;
    k.sm = (T)c.social_margin;
    k.tol = (T)c.tolerance;
    k.init_tol = (T)c.initial_tolerance;
    k.delta_tol = (T)c.delta_tolerance;
    k.c_init = (T)c.initial_penalty;
    k.pen_update = (T)c.penalty_update_factor;
    k.tol_update = (T)c.inner_tolerance_update_factor;
    k.suff_dec = (T)c.sufficient_decrease_coeff;
    const bool f32 = sizeof(T) == 4;
    k.lip_eps = (T)(f32 ? c.lip_eps_f32 : c.lip_eps_f64);
    k.lip_delta = (T)(f32 ? c.lip_delta_f32 : c.lip_delta_f64);
    k.cbfgs_alpha = (T)c.cbfgs_alpha;
    k.cbfgs_eps = (T)c.cbfgs_epsilon;
    k.sy_eps = (T)c.sy_epsilon;
    k.max_outer = c.max_outer_iterations;
    k.max_inner = c.max_inner_iterations;
    k.mem = c.lbfgs_memory;
    k.akkt_form = c.akkt_form;
    k.time_budget = c.max_solver_time_us > 0 ? (long long)(c.max_solver_time_us * 100.0 + 0.5) : 0; // 100 MHz ticks
    k.max_evals = c.max_evaluations > 0 ? c.max_evaluations : 0;
}

// The same evaluation through the cooperative kernels' code path (W wavefronts share it; wavefront 0 writes): what
// nmpc_eval_batch_* launches when the handle's coop_waves asks for the cooperative mode, so that psi / grad psi of the
// row split, the partial-sum exchange and the helper lanes can be compared with the oracle directly.
template <typename T, int LPS, bool GLB, int RS, bool HLP, int WAVES, int ONLY = 0>
__global__ __launch_bounds__(64 * WAVES, (RS > 0 ? 2 : (sizeof(T) == 4 ? NMPC_SPEC_WPE_F32 : NMPC_WPE_F64)))
void eval_coop_kernel(nmpc::KParams<T> kp, nmpc::EvalParams<T> ep)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if constexpr (ONLY != 0)
        if (nmpc::axis_path(kp) != (ONLY == 1)) return; // (global table: compressed / general member of the pair)
    const int inst = blockIdx.x, N = kp.N;
    T* lds = reinterpret_cast<T*>(smem);
    nmpc::Instance<T, LPS, GLB, RS, true, HLP, ONLY == 1> I(kp, kp.P + (size_t)inst * kp.np, lds,
                                                 GLB ? kp.ws + (long long)inst * kp.ws_stride : nullptr);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    I.cw_ = wave;
    I.CW_ = (int)(blockDim.x >> 6);
    I.coop_x = lds + kp.lds_xch;
    if (I.load()) { // (not evaluated: every output of the instance is NaN)
        if (threadIdx.x == 0) {
            ep.psi[inst] = __builtin_nanf("");
            if (ep.f2sq) ep.f2sq[inst] = __builtin_nanf("");
        }
        if (ep.grad)
            for (int j = threadIdx.x; j < 2 * N; j += blockDim.x) ep.grad[(size_t)inst * 2 * N + j] = __builtin_nanf("");
        return;
    }
    const int kk = I.act ? I.k : 0;
    T v = ep.U[(size_t)inst * 2 * N + 2 * kk], w = ep.U[(size_t)inst * 2 * N + 2 * kk + 1];
    T yv = ep.Y[(size_t)inst * 2 * N + kk], yw = ep.Y[(size_t)inst * 2 * N + N + kk];
    if (!I.act) v = w = yv = yw = 0;
    const T c = ep.C[inst];
    const T icd = T(1) / (c > T(1) ? c : T(1));
    T psi, f2, gv, gw;
    if (ep.grad)
        I.template eval<true>(v, w, c, icd, yv, yw, psi, f2, gv, gw);
    else
        I.template eval<false>(v, w, c, icd, yv, yw, psi, f2, gv, gw);
    if (wave != 0) return;
    if (I.lead && ep.grad) {
        ep.grad[(size_t)inst * 2 * N + 2 * I.k] = gv;
        ep.grad[(size_t)inst * 2 * N + 2 * I.k + 1] = gw;
    }
    if (I.lane == 0) {
        ep.psi[inst] = psi;
        if (ep.f2sq) ep.f2sq[inst] = f2;
    }
}

template <typename T>
using SolveFn = void (*)(nmpc::KParams<T>);
template <typename T>
using EvalFn = void (*)(nmpc::KParams<T>, nmpc::EvalParams<T>);

// ---- variant -> kernel: the one place that names the instantiations -------------------------------------------------------
// f(lanes per step) / f(register-table slots) with the run-time value as a compile-time constant
template <int I>
using IC = std::integral_constant<int, I>;
template <typename F>
auto with_lps(int lps, F f)
{
    return lps == 3 ? f(IC<3>{}) : lps == 2 ? f(IC<2>{}) : f(IC<1>{});
}
template <typename T, typename F>
auto with_reg_slots(int rs, F f) // (fp64 has the 14-slot table only)
{
    if constexpr (sizeof(T) == 4) {
        if (rs == kRegSlotsSmall) return f(IC<kRegSlotsSmall>{});
        if (rs == kRegSlotsMid) return f(IC<kRegSlotsMid>{});
    }
    return f(IC<kRegSlotsLarge>{});
}

// The kernel of a variant (nmpc_plan.h); member = 1 / 2 of a pair -- nullptr for the second member of a variant that is
// not one, and for a family of the other signature.
template <typename T>
SolveFn<T> solve_kernel_of(const Variant& v, int member = 1)
{
    using Fn = SolveFn<T>;
    const bool second = member == 2, tail = v.family == kLatencyTail;
    if (second && !v.pair) return nullptr;
    switch (v.family) {
    case kThroughput:
        if (v.pair) return with_reg_slots<T>(v.rs, [&](auto r) -> Fn { return second ? solve_kernel<T, 3, false, r(), 2> : solve_kernel<T, 3, false, r(), 1>; });
        return with_lps(v.lps, [&](auto l) -> Fn { return v.glb ? solve_kernel<T, l(), true> : solve_kernel<T, l(), false>; });
    case kLatencyFlat:
    case kLatencyTail: // (the register-table members, and with them the tail members, exist in fp32 only)
        if constexpr (sizeof(T) == 4)
            if (v.pair)
                return with_reg_slots<T>(v.rs, [&](auto r) -> Fn {
                    if (tail) return second ? solve_spec_kernel<T, 3, false, r(), 2, false> : solve_spec_kernel<T, 3, false, r(), 1, false>;
                    return second ? solve_spec_kernel<T, 3, false, r(), 2> : solve_spec_kernel<T, 3, false, r(), 1>;
                });
        if (tail) return nullptr;
        return with_lps(v.lps, [&](auto l) -> Fn { return v.glb ? solve_spec_kernel<T, l(), true> : solve_spec_kernel<T, l(), false>; });
    case kCoop:
        return with_lps(v.lps, [&](auto l) -> Fn {
            return !v.glb ? solve_coop_kernel<T, l(), false> : second ? solve_coop_kernel<T, l(), true, 2> : solve_coop_kernel<T, l(), true, 1>;
        });
    case kCoopOnChip:
        if constexpr (sizeof(T) == 4) return v.hlp ? solve_coop_reg_kernel<true> : solve_coop_reg_kernel<false>;
        return nullptr;
    default:
        return nullptr;
    }
}
template <typename T>
EvalFn<T> eval_kernel_of(const Variant& v, int member = 1)
{
    using Fn = EvalFn<T>;
    constexpr int W = kSpecWaves;
    const bool second = member == 2;
    if (second && !v.pair) return nullptr;
    switch (v.family) {
    case kEval:
        if (v.pair) return with_reg_slots<T>(v.rs, [&](auto r) -> Fn { return second ? eval_kernel<T, 3, false, r(), 2> : eval_kernel<T, 3, false, r(), 1>; });
        return with_lps(v.lps, [&](auto l) -> Fn { return v.glb ? eval_kernel<T, l(), true> : eval_kernel<T, l(), false>; });
    case kEvalCoop:
        return with_lps(v.lps, [&](auto l) -> Fn {
            return !v.glb ? eval_coop_kernel<T, l(), false, 0, false, W> : second ? eval_coop_kernel<T, l(), true, 0, false, W, 2> : eval_coop_kernel<T, l(), true, 0, false, W, 1>;
        });
    case kEvalCoopOnChip:
        if constexpr (sizeof(T) == 4)
            return v.hlp ? eval_coop_kernel<float, 1, false, kRegSlotsCoop, true, kCoopRegWaves> : eval_coop_kernel<float, 1, false, kRegSlotsCoop, false, kCoopRegWaves>;
        return nullptr;
    default:
        return nullptr;
    }
}
// diagnostic kernel of nmpc_solve_trace_f64
SolveFn<double> trace_kernel_of(int lps, bool glb)
{
    return with_lps(lps, [&](auto l) -> SolveFn<double> { return glb ? trace_kernel<l(), true> : trace_kernel<l(), false>; });
}

// stage `count` elements: returns the device pointer to use (src itself if already on the device)
template <typename T>
int stage_in(nmpc_handle_s* h, DevBuf& buf, const T* src, size_t count, const T** out)
{
    if (!src) {
        *out = nullptr;
        return 0;
    }
    if (h->ptr_mode == NMPC_PTR_DEVICE || (h->ptr_mode == NMPC_PTR_DETECT && is_device_ptr(src))) {
        *out = src;
        return 0;
    }
    if (int rc = buf.reserve(count * sizeof(T))) return rc;
    HIP_TRY(hipMemcpyAsync(buf.p, src, count * sizeof(T), hipMemcpyHostToDevice, h->stream));
    *out = static_cast<const T*>(buf.p);
    return 0;
}
template <typename T>
int stage_out(nmpc_handle_s* h, DevBuf& buf, T* dst, size_t count, T** dev, bool* is_host)
{
    *is_host = false;
    if (!dst) {
        *dev = nullptr;
        return 0;
    }
    if (h->ptr_mode == NMPC_PTR_DEVICE || (h->ptr_mode == NMPC_PTR_DETECT && is_device_ptr(dst))) {
        *dev = dst;
        return 0;
    }
    if (int rc = buf.reserve(count * sizeof(T))) return rc;
    *dev = static_cast<T*>(buf.p);
    *is_host = true;
    return 0;
}

// ---- the solve plan (nmpc_plan.h) and its execution ---------------------------------------------------------------------
// (development builds, -DNMPC_DEV_ENV: the thresholds of PlanTuning from the environment -- tools/exp_mid_batches.py,
//  tools/exp_cfg1_proxy_order.py; the shipped library has the constants)
#ifdef NMPC_DEV_ENV
static double dev_env(const char* name, double dflt) { const char* v = getenv(name); return v ? atof(v) : dflt; }
static PlanTuning plan_tuning()
{
    const PlanTuning d;
    return {dev_env("NMPC_PROXY_ORDER", d.proxy_order), dev_env("NMPC_PROXY_FILLS", d.proxy_fills), dev_env("NMPC_PROXY_VNOM", d.proxy_vnom),
            dev_env("NMPC_STAGE_FILLS", d.stage_fills), dev_env("NMPC_TAIL_FILLS", d.tail_fills), dev_env("NMPC_TAIL_WAVES", d.tail_waves),
            dev_env("NMPC_TAIL_MINB", d.tail_min_parks)};
}
#else
static PlanTuning plan_tuning() { return PlanTuning(); }
#endif

template <typename T>
PlanStatic plan_static(const nmpc_handle_s* h)
{
    const int i = sizeof(T) == 4 ? 0 : 1;
    return {&h->cfg, &h->lays, sizeof(T), h->n_simd, h->spec_ok[i], h->coop_ok[i]};
}

// point `k` at the layout and the global workspace of a kernel choice (the batch buffers and solver options are kept)
template <typename T>
int bind_choice(nmpc_handle_s* h, const KernelChoice& kc, nmpc::KParams<T>& k, int B)
{
    if (kc.use != kLayMain) fill_layout(k, *kc.L);
    if (kc.coop) k.lds_xch = kc.L->lds_xch_coop;
    k.ws = nullptr;
    k.ws_stride = 0;
    if (kc.uses_ws) { // (only the variants that stream the obstacle table reserve the global workspace)
        if (int rc = h->dws.reserve((size_t)B * kc.L->ws_stride * sizeof(T))) return rc;
        k.ws = static_cast<T*>(h->dws.p);
        k.ws_stride = kc.L->ws_stride;
    }
    return 0;
}

// one launch of a kernel choice over `grid` workgroups (solve kernels: no `ep`; evaluation kernels: one). Of a pair, the
// member whose path KParams::axis_mode rules out -- 0: the general path only, 1: the axis-aligned only -- is not launched.
template <typename T, typename... Ep>
int launch_choice(nmpc_handle_s* h, const KernelChoice& kc, int grid, const nmpc::KParams<T>& k, const Ep&... ep)
{
    if (grid <= 0) return 0;
    for (int member = 1; member <= (kc.variant.pair ? 2 : 1); ++member) {
        if (kc.variant.pair && k.axis_mode == member - 1) continue;
        if constexpr (sizeof...(Ep) == 0)
            hipLaunchKernelGGL(solve_kernel_of<T>(kc.variant, member), dim3(grid), dim3(kc.threads), kc.lds_bytes, h->stream, k);
        else
            hipLaunchKernelGGL(eval_kernel_of<T>(kc.variant, member), dim3(grid), dim3(kc.threads), kc.lds_bytes, h->stream, k, ep...);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// How the axis-aligned variant takes part in a call over B instances at P (device): sets k.axis_mode to 0 (general only),
// 1 (the caller's promise) or 2 (decided on the device: the scan of the batch's angle entries is enqueued here).
template <typename T>
int prepare_axis(nmpc_handle_s* h, bool has_axis, nmpc::KParams<T>& k, int B)
{
    k.axis_mode = 0;
    if (!has_axis || h->cfg.axis_aligned < 0) return 0;
    if (h->cfg.axis_aligned > 0) {
        k.axis_mode = 1;
        return 0;
    }
    const Layout& L = h->lay<T>();
    const int n_entries = h->cfg.Ndynobs * (h->cfg.N_hor + 1);
    h->axis_epoch = h->axis_epoch == 0x7ffffff0 ? 1 : h->axis_epoch + 1;
    k.axis_mode = 2;
    k.axis_epoch = h->axis_epoch;
    k.axis_flag = static_cast<const int*>(h->dflag.p);
    if (n_entries > 0) {
        hipLaunchKernelGGL(axis_scan_kernel<T>, dim3(B), dim3(256), 0, h->stream, k.P, L.np, L.off_od, n_entries,
                           static_cast<int*>(h->dflag.p), h->axis_epoch);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// Solve B instances whose buffers (all on the device) are in `k`: asks nmpc_plan.h for the plan and carries it out -- the
// axis scan, the dispatch order from one evaluation, the stages of the resumable solve with the ranking behind each, the
// tail hand-off. `allow_staging`: the caller's status array may be used for the in-progress marker.
template <typename T>
int run_solve(nmpc_handle_s* h, nmpc::KParams<T>& k, int B, bool allow_staging)
{
    const PlanStatic s = plan_static<T>(h);
    const PlanTuning tune = plan_tuning();
    const SolvePlan pl = plan_solve(s, {B, k.order != nullptr, allow_staging, k.status != nullptr}, tune);
    if (int rc = bind_choice<T>(h, pl.main, k, B)) return rc;
    if (int rc = prepare_axis<T>(h, pl.main.has_axis, k, B)) return rc;
    h->last_mode = pl.last_mode;
    h->last_axis = pl.main.has_axis ? k.axis_mode : -1;
    h->last_staged = pl.last_staged;
    h->last_order = pl.last_order;
    h->last_tail = 0;
    // (the evaluation order below goes into k.order for the rest of this function only: the caller's k gets its own back)
    struct OrderGuard {
        nmpc::KParams<T>& kk;
        decltype(nmpc::KParams<T>::order) saved;
        ~OrderGuard() { kk.order = saved; }
    } order_guard{k, k.order};
    int* const hist = static_cast<int*>(h->dhist.p);
    int* const offs = hist + kRankBuckets;
    int* const dctr = offs + kRankBuckets;       // (KParams::dyn_ctr: four counters behind the bucket tables)
    const int nb = (B + 255) / 256;
    // counting sort of the instances by `key` of their parked state (rank_bucket) into dorder2; publish: the number of
    // unfinished ones goes to the hand-off's counters
    const auto rank = [&](const T* resume, int key, bool publish) {
        int* const order2 = static_cast<int*>(h->dorder2.p);
        hipLaunchKernelGGL(rank_hist_kernel<T>, dim3(nb), dim3(256), 0, h->stream, resume, k.status, B, hist, key);
        hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(kRankBuckets), 0, h->stream, hist, offs, publish ? dctr : nullptr);
        hipLaunchKernelGGL(rank_scatter_kernel<T>, dim3(nb), dim3(256), 0, h->stream, resume, k.status, B, offs, order2, key);
        return hipGetLastError();
    };
    if (pl.eval_order) {
        // one evaluation at the nominal controls (v_nom, 0), zero multipliers, the initial penalty; its ||F2||^2 is the key
        const size_t n = 2 * (size_t)h->cfg.N_hor;
        if (int rc = h->dresume.reserve((size_t)B * nmpc::kResumeStride * sizeof(T))) return rc;
        if (int rc = h->dorder2.reserve((size_t)B * sizeof(int))) return rc;
        if (int rc = h->dproxy.reserve((2 * (size_t)B * n + 3 * (size_t)B) * sizeof(T))) return rc;
        T* const Un = static_cast<T*>(h->dproxy.p);
        nmpc::EvalParams<T> ep;
        ep.U = Un, ep.Y = Un + (size_t)B * n, ep.C = Un + 2 * (size_t)B * n;
        ep.psi = Un + 2 * (size_t)B * n + B, ep.grad = nullptr, ep.f2sq = Un + 2 * (size_t)B * n + 2 * (size_t)B;
        const int nbf = (int)(((size_t)B * n + 255) / 256);
        hipLaunchKernelGGL(proxy_fill_kernel<T>, dim3(nbf), dim3(256), 0, h->stream, Un, Un + (size_t)B * n, Un + 2 * (size_t)B * n, B, (int)n,
                           T(tune.proxy_vnom) * k.vmax, k.c_init);
        if (int rc = launch_choice<T>(h, choose_single(s, kEval), B, k, ep)) return rc;
        T* const resume = static_cast<T*>(h->dresume.p);
        hipLaunchKernelGGL(proxy_key_kernel<T>, dim3(nb), dim3(256), 0, h->stream, ep.f2sq, resume, k.status, B);
        HIP_TRY(rank(resume, 0, false));
        k.order = static_cast<const int*>(h->dorder2.p); // (from here on as under a caller's order)
    }
    if (pl.n_stage == 0 && !pl.tail) return launch_choice<T>(h, pl.main, B, k);
    if (pl.tail) {
        if (int rc = h->ddeep.reserve((size_t)pl.park * nmpc::deep_park_stride(h->cfg.N_hor) * sizeof(T))) return rc;
        k.deep = static_cast<T*>(h->ddeep.p);   // (read by the tail launch; handed to the LAST throughput launch only)
    }
    if (int rc = h->dresume.reserve((size_t)B * nmpc::kResumeStride * sizeof(T))) return rc;
    if (int rc = h->dorder2.reserve((size_t)B * sizeof(int))) return rc;
    k.resume = static_cast<T*>(h->dresume.p);
    const int* const order2 = static_cast<const int*>(h->dorder2.p);
    for (int i = 0; i <= pl.n_stage; ++i) {
        nmpc::KParams<T> ki = k;
        ki.deep = nullptr;
        ki.stage_in = i > 0;
        ki.stage_outer_cap = i < pl.n_stage ? pl.stage_cap[i] : 0;
        if (i > 0) ki.order = order2;
        if (i == pl.n_stage && pl.tail) { // the last throughput launch parks its drain phase (the counters: set by the ranking before it)
            if (pl.n_stage == 0) {        // (one launch under the caller's order: all B instances are to be solved)
                hipLaunchKernelGGL(dyn_init_kernel, dim3(1), dim3(1), 0, h->stream, dctr, B);
                HIP_TRY(hipGetLastError());
            }
            ki.dyn_ctr = dctr;
            ki.dyn_park = pl.park;
            ki.deep = k.deep;       // (parking inside an inner solve: the slots reserved above)
            ki.deep_slots = pl.park;
        }
        if (int rc = launch_choice<T>(h, pl.main, B, ki)) return rc;
        if (i == pl.n_stage) break;
        HIP_TRY(rank(k.resume, pl.stage_key[i], i + 1 == pl.n_stage && pl.tail));
    }
    if (pl.tail) {
        // the parked instances (status -1) first in order2 -- at most `park` of them by construction -- and the tail member over them
        HIP_TRY(rank(k.resume, 0, false));
        nmpc::KParams<T> kt = k;
        kt.stage_in = 1;
        kt.stage_outer_cap = 0;
        kt.order = order2;
        if (int rc = launch_choice<T>(h, pl.tail_kernel, std::min(B, pl.park), kt)) return rc;
        h->last_tail = pl.park;
    }
    return 0;
}

template <typename T>
int polish_batch(nmpc_handle_s* h, const nmpc::KParams<T>& k, int B, bool y_user, bool info_user);

template <typename T>
int solve_batch(nmpc_handle_s* h, const T* P, int32_t B, T* U, T* cost, int32_t* status, int32_t* iters,
                const T* u0, T* y, int32_t y_is_input, const T* c0, T* info, int32_t sync)
{
    if (!h) return fail(NMPC_ERR_INVALID_ARGUMENT, "null handle");
    if (!P || !U) return fail(NMPC_ERR_INVALID_ARGUMENT, "P and U must not be NULL");
    if (B < 0) return fail(NMPC_ERR_INVALID_ARGUMENT, "B = %d < 0", B);
    if (B == 0) return 0;
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    const Layout& L = h->lay<T>();
    const size_t n = 2 * (size_t)h->cfg.N_hor, np = L.np;
    nmpc::KParams<T> k;
    fill_kparams(h, k);
    k.B = B;
    k.y_is_input = y_is_input;
    bool hU, hcost, hstatus, hiters, hy, hinfo;
    int rc;
    if ((rc = stage_in(h, h->dP, P, (size_t)B * np, &k.P))) return rc;
    if ((rc = stage_in(h, h->du0, u0, (size_t)B * n, &k.u0))) return rc;
    if ((rc = stage_in(h, h->dc0, c0, (size_t)B, &k.c0v))) return rc;
    if ((rc = stage_out(h, h->dU, U, (size_t)B * n, &k.U, &hU))) return rc;
    if ((rc = stage_out(h, h->dcost, cost, (size_t)B, &k.cost, &hcost))) return rc;
    if ((rc = stage_out(h, h->dstatus, status, (size_t)B, &k.status, &hstatus))) return rc;
    if ((rc = stage_out(h, h->diters, iters, (size_t)B * 2, &k.iters, &hiters))) return rc;
    if ((rc = stage_out(h, h->dy, y, (size_t)B * n, &k.y, &hy))) return rc;
    const size_t info_row = 8 + nmpc::kProfSlots; // 8 in the shipped library (kProfSlots = 0)
    if ((rc = stage_out(h, h->dinfo, info, (size_t)B * info_row, &k.info, &hinfo))) return rc;
    if (hy && y_is_input) HIP_TRY(hipMemcpyAsync(k.y, y, (size_t)B * n * sizeof(T), hipMemcpyHostToDevice, h->stream));
    // arrays the caller did not ask for but the resumable solve (status) / the polish (status, y, info) need: the
    // handle's own buffers stand in
    const bool polish = h->cfg.polish > 0 && nmpc::kProfSlots == 0;
    const bool y_user = y != nullptr, info_user = info != nullptr;
    if (!k.status) {
        if ((rc = h->dstatus.reserve((size_t)B * sizeof(int32_t)))) return rc;
        k.status = static_cast<int*>(h->dstatus.p);
    }
    if (polish && !k.y) {
        if ((rc = h->dy.reserve((size_t)B * n * sizeof(T)))) return rc;
        k.y = static_cast<T*>(h->dy.p);
    }
    if (polish && !k.info) {
        if ((rc = h->dinfo.reserve((size_t)B * info_row * sizeof(T)))) return rc;
        k.info = static_cast<T*>(h->dinfo.p);
    }
    k.order = h->order_B == B ? static_cast<const int*>(h->dorder.p) : nullptr;

    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    if ((rc = run_solve<T>(h, k, B, true))) return rc;
    h->last_polish_selected = 0;
    h->last_polish_converged = -1;
    if (polish && (rc = polish_batch<T>(h, k, B, y_user, info_user))) return rc;
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    h->timed = true;

    const bool any_host = hU || hcost || hstatus || hiters || hy || hinfo;
    if (hU) HIP_TRY(hipMemcpyAsync(U, k.U, (size_t)B * n * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    if (hcost) HIP_TRY(hipMemcpyAsync(cost, k.cost, (size_t)B * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    if (hstatus)
        HIP_TRY(hipMemcpyAsync(status, k.status, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (hiters)
        HIP_TRY(hipMemcpyAsync(iters, k.iters, (size_t)B * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (hy) HIP_TRY(hipMemcpyAsync(y, k.y, (size_t)B * n * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    if (hinfo)
        HIP_TRY(hipMemcpyAsync(info, k.info, (size_t)B * info_row * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    if (any_host || sync) HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

// nmpc_config.polish: fp64 continuation of the instances the main solve flagged Converged (results of the main solve
// in k.U / k.y / k.info / k.status on the device). One stream synchronisation: the selection is made on the host.
template <typename T>
int polish_batch(nmpc_handle_s* h, const nmpc::KParams<T>& k, int B, bool y_user, bool info_user)
{
    const int n2 = 2 * h->cfg.N_hor;
    h->host_status.resize((size_t)B);
    HIP_TRY(hipMemcpyAsync(h->host_status.data(), k.status, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->host_sel.clear();
    for (int b = 0; b < B; ++b)
        if (h->host_status[(size_t)b] == NMPC_CONVERGED) h->host_sel.push_back(b);
    const int ns = (int)h->host_sel.size();
    h->last_polish_selected = ns;
    h->last_polish_converged = 0;
    if (info_user) {
        hipLaunchKernelGGL(polish_clear_flag_kernel<T>, dim3((B + 255) / 256), dim3(256), 0, h->stream, k.info, B);
        HIP_TRY(hipGetLastError());
    }
    if (ns == 0) return 0;
    const Layout& L64 = h->lays.lay64;
    const size_t np = (size_t)L64.np;
    int rc;
    if ((rc = h->psel.reserve((size_t)ns * sizeof(int)))) return rc;
    if ((rc = h->pP.reserve((size_t)ns * np * sizeof(double)))) return rc;
    if ((rc = h->pU0.reserve((size_t)ns * n2 * sizeof(double)))) return rc;
    if ((rc = h->pY.reserve((size_t)ns * n2 * sizeof(double)))) return rc;
    if ((rc = h->pC.reserve((size_t)ns * sizeof(double)))) return rc;
    if ((rc = h->pU.reserve((size_t)ns * n2 * sizeof(double)))) return rc;
    if ((rc = h->pcost.reserve((size_t)ns * sizeof(double)))) return rc;
    if ((rc = h->pstatus.reserve((size_t)ns * sizeof(int)))) return rc;
    if ((rc = h->piters.reserve((size_t)ns * 2 * sizeof(int)))) return rc;
    if ((rc = h->pinfo.reserve((size_t)ns * 8 * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpyAsync(h->psel.p, h->host_sel.data(), (size_t)ns * sizeof(int), hipMemcpyHostToDevice, h->stream));
    const int* sel = static_cast<const int*>(h->psel.p);
    hipLaunchKernelGGL(polish_gather_kernel<T>, dim3(ns), dim3(256), 0, h->stream, k.P, (const T*)k.U, (const T*)k.y,
                       (const T*)k.info, sel, (int)np, n2, static_cast<double*>(h->pP.p), static_cast<double*>(h->pU0.p),
                       static_cast<double*>(h->pY.p), static_cast<double*>(h->pC.p));
    HIP_TRY(hipGetLastError());
    nmpc::KParams<double> q;
    fill_kparams(h, q);
    const nmpc_config& c = h->cfg;
    // The exit test bounds ||gamma fpr||, which pins u only to ~tol / gamma, and the curvature of the path term grows with
    // the lever arm of the horizon: at N = 40 a tolerance of 1e-6 leaves the controls 2-3e-4 from the fixed point where
    // N = 20 gets 2e-5. Beyond the reference's horizon the continuation's tolerance therefore shrinks with (20 / N)^3
    // (N = 40: 1.25e-7) and its iteration cap grows with (N / 20)^2.
    const double hscale = c.N_hor > 20 ? 20.0 / c.N_hor : 1.0;
    q.tol = q.init_tol = c.polish_tolerance * hscale * hscale * hscale;
    q.max_inner = (int)(c.polish_max_inner_iterations / (hscale * hscale) + 0.5);
    if (c.polish == 1) {
        // ONE inner solve at the penalty and multipliers the main solve ended with (KParams::single_inner): what the
        // continuation needs is stationarity to polish_tolerance; the hard-constraint criterion stays at the main solve's delta.
        // Measured (tools/exp_polish_stats.py, configs[2] `passing`): the first inner solve of the ALM continuation takes
        // 123 evaluations and leaves the controls 1.8e-5 (median) from the 1e-8 fixed point, 86.6 % below 1e-4; the outer
        // iterations behind it -- the second one is mandatory in OpEn's loop -- add 131 evaluations for 1.1e-5 / 86.9 %.
        q.single_inner = 1;
        q.max_outer = 1;
        q.delta_tol = c.delta_tolerance;
    } else {
        q.delta_tol = c.polish_delta_tolerance;
        q.max_outer = c.polish_max_outer_iterations;
    }
    q.time_budget = 0;
    q.max_evals = 0; // (the continuation of a converged instance is not budgeted)
    q.B = ns;
    q.P = static_cast<const double*>(h->pP.p);
    q.u0 = static_cast<const double*>(h->pU0.p);
    q.y = static_cast<double*>(h->pY.p);
    q.y_is_input = 1;
    q.c0v = static_cast<const double*>(h->pC.p);
    q.U = static_cast<double*>(h->pU.p);
    q.cost = static_cast<double*>(h->pcost.p);
    q.status = static_cast<int*>(h->pstatus.p);
    q.iters = static_cast<int*>(h->piters.p);
    q.info = static_cast<double*>(h->pinfo.p);
    const int keep_mode = h->last_mode, keep_axis = h->last_axis, keep_staged = h->last_staged, keep_tail = h->last_tail,
              keep_order = h->last_order;
    rc = run_solve<double>(h, q, ns, false);
    h->last_mode = keep_mode, h->last_axis = keep_axis, h->last_staged = keep_staged, h->last_tail = keep_tail,
    h->last_order = keep_order;
    if (rc) return rc;
    hipLaunchKernelGGL(polish_scatter_kernel<T>, dim3(ns), dim3(128), 0, h->stream, sel, (const double*)q.U, (const double*)q.y,
                       (const double*)q.cost, (const int*)q.status, (const int*)q.iters, (const double*)q.info, n2, k.U, k.y,
                       y_user, k.cost, k.iters, k.info, info_user);
    HIP_TRY(hipGetLastError());
    return 0;
}

// nmpc_solve_trace_f64: ONE instance (host pointers) through trace_kernel; see include/nmpc_hip.h
int solve_trace(nmpc_handle_s* h, const double* p, const double* u0, const double* y0, double c0, double* U, double* y,
                int32_t* status, int32_t* iters, double* info, double* trace, int32_t max_records, int32_t* n_records)
{
    if (!h) return fail(NMPC_ERR_INVALID_ARGUMENT, "null handle");
    if (!p || !U || !trace || !n_records || max_records < 1)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "p, U, trace, n_records must not be NULL and max_records >= 1");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    const Layout& L = h->lays.lay64;
    const size_t n = 2 * (size_t)h->cfg.N_hor, np = L.np;
    const size_t rec = (size_t)nmpc::kTraceHead + n, tlen = (size_t)nmpc::kTraceHead + (size_t)max_records * rec;
    nmpc::KParams<double> k;
    fill_kparams(h, k);
    k.B = 1;
    int rc;
    DevBuf dtrace, dc0; // (local buffers: freed on every path out of this function)
    if ((rc = dtrace.reserve(tlen * sizeof(double)))) return rc;
    if ((rc = h->dP.reserve(np * sizeof(double)))) return rc;
    if ((rc = h->dU.reserve(n * sizeof(double)))) return rc;
    if ((rc = h->dy.reserve(n * sizeof(double)))) return rc;
    if ((rc = h->du0.reserve(n * sizeof(double)))) return rc;
    if ((rc = h->dcost.reserve(sizeof(double)))) return rc;
    if ((rc = h->dstatus.reserve(sizeof(int32_t)))) return rc;
    if ((rc = h->diters.reserve(2 * sizeof(int32_t)))) return rc;
    if ((rc = h->dinfo.reserve((8 + nmpc::kProfSlots) * sizeof(double)))) return rc; // (a -DNMPC_PROFILE build writes its slots behind the 8)
    if ((rc = dc0.reserve(sizeof(double)))) return rc;
    // the handle's staging buffers are shared with nmpc_solve_batch_*: a solve enqueued with sync = 0 must have finished
    // with them (its results copied out) before this call overwrites them
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpyAsync(h->dP.p, p, np * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (u0) HIP_TRY(hipMemcpyAsync(h->du0.p, u0, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (y0) HIP_TRY(hipMemcpyAsync(h->dy.p, y0, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (c0 > 0) HIP_TRY(hipMemcpyAsync(dc0.p, &c0, sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(dtrace.p, 0, nmpc::kTraceHead * sizeof(double), h->stream));
    k.P = static_cast<const double*>(h->dP.p);
    k.u0 = u0 ? static_cast<const double*>(h->du0.p) : nullptr;
    k.y = static_cast<double*>(h->dy.p);
    k.y_is_input = y0 != nullptr;
    k.c0v = c0 > 0 ? static_cast<const double*>(dc0.p) : nullptr;
    k.U = static_cast<double*>(h->dU.p);
    k.cost = static_cast<double*>(h->dcost.p);
    k.status = static_cast<int*>(h->dstatus.p);
    k.iters = static_cast<int*>(h->diters.p);
    k.info = static_cast<double*>(h->dinfo.p);
    k.trace = static_cast<double*>(dtrace.p);
    k.trace_cap = max_records;
    k.time_budget = 0;
    if (L.glb) {
        if ((rc = h->dws.reserve((size_t)L.ws_stride * sizeof(double)))) return rc;
        k.ws = static_cast<double*>(h->dws.p);
        k.ws_stride = L.ws_stride;
    }
    const SolveFn<double> fn = trace_kernel_of(h->lays.lps, L.glb);
    const size_t lds_bytes = (size_t)L.lds_total * sizeof(double);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    hipLaunchKernelGGL(fn, dim3(1), dim3(64), lds_bytes, h->stream, k);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(U, k.U, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (y) HIP_TRY(hipMemcpyAsync(y, k.y, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (status) HIP_TRY(hipMemcpyAsync(status, k.status, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (iters) HIP_TRY(hipMemcpyAsync(iters, k.iters, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (info) HIP_TRY(hipMemcpyAsync(info, k.info, 8 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    std::vector<double> host(tlen);
    HIP_TRY(hipMemcpyAsync(host.data(), dtrace.p, tlen * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const int nr = (int)host[0];
    *n_records = nr;
    std::memcpy(trace, host.data() + nmpc::kTraceHead, (size_t)nr * rec * sizeof(double));
    return 0;
}

template <typename T>
int eval_batch(nmpc_handle_s* h, const T* P, const T* U, const T* Y, const T* C, int32_t B, T* psi, T* grad,
               T* f2sq)
{
    if (!h) return fail(NMPC_ERR_INVALID_ARGUMENT, "null handle");
    if (!P || !U || !Y || !C || !psi) return fail(NMPC_ERR_INVALID_ARGUMENT, "P, U, Y, C, psi must not be NULL");
    if (B <= 0) return B == 0 ? 0 : fail(NMPC_ERR_INVALID_ARGUMENT, "B = %d < 0", B);
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    const Layout& L = h->lay<T>();
    const size_t n = 2 * (size_t)h->cfg.N_hor, np = L.np;
    nmpc::KParams<T> k;
    fill_kparams(h, k);
    k.B = B;
    nmpc::EvalParams<T> ep;
    bool hpsi, hgrad, hf2;
    int rc;
    if ((rc = stage_in(h, h->dP, P, (size_t)B * np, &k.P))) return rc;
    if ((rc = stage_in(h, h->du0, U, (size_t)B * n, &ep.U))) return rc;
    if ((rc = stage_in(h, h->dY2, Y, (size_t)B * n, &ep.Y))) return rc;
    if ((rc = stage_in(h, h->dC2, C, (size_t)B, &ep.C))) return rc;
    if ((rc = stage_out(h, h->dpsi, psi, (size_t)B, &ep.psi, &hpsi))) return rc;
    if ((rc = stage_out(h, h->dgrad, grad, (size_t)B * n, &ep.grad, &hgrad))) return rc;
    if ((rc = stage_out(h, h->df2, f2sq, (size_t)B, &ep.f2sq, &hf2))) return rc;
    const KernelChoice kc = plan_eval(plan_static<T>(h));
    if ((rc = bind_choice<T>(h, kc, k, B))) return rc;
    if ((rc = prepare_axis<T>(h, kc.has_axis, k, B))) return rc;
    h->last_mode = kc.coop ? 2 : 0;
    h->last_axis = kc.has_axis ? k.axis_mode : -1;
    h->last_staged = 0;
    h->last_polish_selected = 0;
    h->last_tail = 0;
    h->last_order = 0;
    if ((rc = launch_choice<T>(h, kc, B, k, ep))) return rc;
    if (hpsi) HIP_TRY(hipMemcpyAsync(psi, ep.psi, (size_t)B * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    if (hgrad) HIP_TRY(hipMemcpyAsync(grad, ep.grad, (size_t)B * n * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    if (hf2) HIP_TRY(hipMemcpyAsync(f2sq, ep.f2sq, (size_t)B * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

template <typename T>
int assemble_params(nmpc_handle_s* h, const nmpc_assemble_args* g, int32_t B, T* P)
{
    if (!h || !g || !P) return fail(NMPC_ERR_INVALID_ARGUMENT, "null argument");
    if (B <= 0) return B == 0 ? 0 : fail(NMPC_ERR_INVALID_ARGUMENT, "B = %d < 0", B);
    const nmpc_config& c = h->cfg;
    if (g->n_dyn < 0 || g->n_dyn > c.Ndynobs)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "n_dyn = %d outside [0, Ndynobs = %d]", g->n_dyn, c.Ndynobs);
    if (g->n_map_polygons < 0) return fail(NMPC_ERR_INVALID_ARGUMENT, "n_map_polygons < 0");
    const void* required[] = {g->last_u, g->state, g->ref_states, g->speed_ref, g->tuning, g->stc_weights,
                              g->dyn_weights, P};
    for (const void* q : required)
        if (!is_device_ptr(q))
            return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_assemble_params: every array must be a device pointer");
    if ((g->n_map_polygons > 0 && !is_device_ptr(g->map_polygons)) || (g->n_dyn > 0 && !is_device_ptr(g->dyn_obstacles)) ||
        (g->other_robots && !is_device_ptr(g->other_robots)))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_assemble_params: every array must be a device pointer");
    HIP_TRY(hipSetDevice(c.device_id));
    const Layout& L = h->lay<T>();
    nmpc::AsmParams<T> a;
    std::memset(&a, 0, sizeof a);
    a.N = c.N_hor;
    a.Nother = c.Nother;
    a.Nstc = c.Nstcobs;
    a.Ndyn = c.Ndynobs;
    a.np = L.np;
    a.off_rs = L.off_rs;
    a.off_rv = L.off_rv;
    a.off_c0 = L.off_c0;
    a.off_os = L.off_os;
    a.off_od = L.off_od;
    a.off_qstc = L.off_qstc;
    a.off_qdyn = L.off_qdyn;
    a.B = B;
    a.M = g->n_map_polygons;
    a.n_dyn = g->n_dyn;
    a.last_u = static_cast<const T*>(g->last_u);
    a.state = static_cast<const T*>(g->state);
    a.ref_states = static_cast<const T*>(g->ref_states);
    a.speed_ref = static_cast<const T*>(g->speed_ref);
    a.tuning = static_cast<const T*>(g->tuning);
    a.other_robots = static_cast<const T*>(g->other_robots);
    a.map_polygons = static_cast<const T*>(g->map_polygons);
    a.dyn = g->n_dyn > 0 ? static_cast<const T*>(g->dyn_obstacles) : nullptr;
    a.stc_weights = static_cast<const T*>(g->stc_weights);
    a.dyn_weights = static_cast<const T*>(g->dyn_weights);
    a.P = P;
    a.selected = g->selected;
    if (g->selected && !is_device_ptr(g->selected))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_assemble_params: every array must be a device pointer");
    const size_t lds = (size_t)a.M * sizeof(T) + (size_t)a.Nstc * sizeof(int) + 16;
    if (lds > kLdsLimit) return fail(NMPC_ERR_UNSUPPORTED, "%d map polygons do not fit the selection kernel's LDS", a.M);
    // (every argument is validated before the first launch)
    // element pairs (8 / 16 B per lane) need every block boundary and every source row pair-aligned
    const unsigned per = 6u * (a.N + 1);
    const bool even = (a.np % 2 == 0) && (a.off_od % 2 == 0) && (a.off_qstc % 2 == 0) && (a.off_c0 % 2 == 0) &&
                      (a.off_os % 2 == 0) && ((a.n_dyn * per) % 2 == 0);
    const auto aligned = [](const void* q, size_t al) { return q == nullptr || reinterpret_cast<uintptr_t>(q) % al == 0; };
    const unsigned vec_ok = even && aligned(a.P, 2 * sizeof(T)) && aligned(a.dyn, 2 * sizeof(T)) &&
                            aligned(a.other_robots, 2 * sizeof(T));
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(nmpc::assemble_kernel<T>, dim3((unsigned)B), dim3(nmpc::kAsmThreads), lds, h->stream, a, vec_ok);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    h->timed = true;
    return 0;
}

template <typename T>
int hypotheses_to_ellipses(nmpc_handle_s* h, const T* hypos, int32_t P, const T* cur, int32_t H, double human_size,
                           double eps, double enlarge, double extra_margin, int32_t B, T* dyn, int32_t* n_obs, int32_t* counts = nullptr)
{
    if (!h || !hypos || !cur || !dyn) return fail(NMPC_ERR_INVALID_ARGUMENT, "null argument");
    if (B <= 0) return B == 0 ? 0 : fail(NMPC_ERR_INVALID_ARGUMENT, "B = %d < 0", B);
    if (P < 1 || P > 256) return fail(NMPC_ERR_UNSUPPORTED, "P = %d hypothesis points per time offset outside [1, 256]", P);
    if (h->cfg.N_hor > 64) return fail(NMPC_ERR_UNSUPPORTED, "nmpc_hypotheses_to_ellipses: N_hor = %d > 64", h->cfg.N_hor);
    if (H < 0 || H > h->cfg.Ndynobs) return fail(NMPC_ERR_INVALID_ARGUMENT, "H = %d outside [0, Ndynobs]", H);
    if (!is_device_ptr(hypos) || !is_device_ptr(cur) || !is_device_ptr(dyn) || (n_obs && !is_device_ptr(n_obs)) ||
        (counts && !is_device_ptr(counts)))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_hypotheses_to_ellipses: every array must be a device pointer");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    nmpc::HypParams<T> a;
    a.B = B;
    a.N = h->cfg.N_hor;
    a.P = P;
    a.H = H;
    a.Ndyn = h->cfg.Ndynobs;
    a.eps = (T)eps;
    a.human_size = (T)human_size;
    a.enlarge = (T)enlarge;
    a.extra_margin = (T)extra_margin;
    a.hypos = hypos;
    a.cur = cur;
    a.dyn = dyn;
    a.n_obs = n_obs;
    a.counts = counts;
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    if (P <= 32)
        hipLaunchKernelGGL((nmpc::hypotheses_kernel<T, unsigned>), dim3(B), dim3(64), 0, h->stream, a);
    else if (P <= 64)
        hipLaunchKernelGGL((nmpc::hypotheses_kernel<T, unsigned long long>), dim3(B), dim3(64), 0, h->stream, a);
    else if (P <= 128)
        hipLaunchKernelGGL((nmpc::hypotheses_wide_kernel<T, 2>), dim3(B), dim3(64), 0, h->stream, a);
    else if (P <= 192)
        hipLaunchKernelGGL((nmpc::hypotheses_wide_kernel<T, 3>), dim3(B), dim3(64), 0, h->stream, a);
    else
        hipLaunchKernelGGL((nmpc::hypotheses_wide_kernel<T, 4>), dim3(B), dim3(64), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    h->timed = true;
    return 0;
}

int set_map(nmpc_handle_s* h, const uint8_t* occupied, const uint8_t* edge, int32_t height, int32_t width)
{
    if (!h) return fail(NMPC_ERR_INVALID_ARGUMENT, "null handle");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    HIP_TRY(hipStreamSynchronize(h->stream)); // a snap that is still running reads the previous map
    if (!occupied) {
        h->dmap_occ.release();
        h->dmap_edge.release();
        h->map_h = h->map_w = h->map_n_edge = h->map_n_edge_pad = 0;
        return 0;
    }
    if (!edge) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_set_map: edge mask is NULL");
    if (height < 1 || width < 1 || height > 32767 || width > 32767)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_set_map: map %d x %d outside [1, 32767]", height, width);
    std::vector<uint32_t> list;
    for (int r = 0; r < height; ++r)
        for (int c = 0; c < width; ++c)
            if (edge[(size_t)r * width + c]) list.push_back((uint32_t)c | ((uint32_t)r << 16));
    const int n_edge = (int)list.size();
    list.resize(((size_t)n_edge + 63) / 64 * 64 + 64, 0u); // (never empty: a map without edge pixels is legal)
    const size_t occ_bytes = (size_t)height * width;
    if (int rc = h->dmap_occ.reserve(occ_bytes)) return rc;
    if (int rc = h->dmap_edge.reserve(list.size() * sizeof(uint32_t))) return rc;
    h->map_h = 0; // (no map while the copies can still fail)
    HIP_TRY(hipMemcpy(h->dmap_occ.p, occupied, occ_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->dmap_edge.p, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    h->map_h = height;
    h->map_w = width;
    h->map_n_edge = n_edge;
    h->map_n_edge_pad = (n_edge + 63) / 64 * 64;
    return 0;
}

template <typename T, int PPL>
void launch_snap(nmpc_handle_s* h, const nmpc::SnapParams& a, const T* raw, T* hypos, unsigned grid)
{
    if (a.n_edge_pad <= nmpc::kSnapLdsPixels)
        hipLaunchKernelGGL((nmpc::snap_kernel<T, PPL, true>), dim3(grid), dim3(nmpc::kSnapThreads),
                           (size_t)a.n_edge_pad * sizeof(unsigned), h->stream, a, raw, hypos);
    else
        hipLaunchKernelGGL((nmpc::snap_kernel<T, PPL, false>), dim3(grid), dim3(nmpc::kSnapThreads), 0, h->stream, a, raw, hypos);
}

template <typename T>
int snap_hypotheses(nmpc_handle_s* h, const T* raw, const nmpc_snap_args* g, int32_t B, T* hypos)
{
    if (!h || !raw || !g || !hypos) return fail(NMPC_ERR_INVALID_ARGUMENT, "null argument");
    if (B <= 0) return B == 0 ? 0 : fail(NMPC_ERR_INVALID_ARGUMENT, "B = %d < 0", B);
    if (h->map_h == 0) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_snap_hypotheses: no map set (nmpc_set_map)");
    if (g->n_ped < 1 || g->n_hyp < 1) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_snap_hypotheses: n_ped = %d, n_hyp = %d", g->n_ped, g->n_hyp);
    if ((long long)g->n_ped * g->n_hyp > 256)
        return fail(NMPC_ERR_UNSUPPORTED, "nmpc_snap_hypotheses: n_ped * n_hyp = %lld points per time offset > 256", (long long)g->n_ped * g->n_hyp);
    if (!(g->rescale != 0.0)) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_snap_hypotheses: rescale = %g", g->rescale);
    if ((long long)B * h->cfg.N_hor > 0x7fffffffLL / 256) return fail(NMPC_ERR_UNSUPPORTED, "nmpc_snap_hypotheses: B = %d too large", B);
    if (!is_device_ptr(raw) || !is_device_ptr(hypos) || (g->n_snapped && !is_device_ptr(g->n_snapped)) ||
        (g->n_outside && !is_device_ptr(g->n_outside)))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_snap_hypotheses: every array must be a device pointer");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    nmpc::SnapParams a;
    a.items = B * h->cfg.N_hor;
    a.N = h->cfg.N_hor;
    a.K = g->n_hyp;
    a.P = g->n_ped * g->n_hyp;
    a.H = h->map_h;
    a.W = h->map_w;
    a.n_edge = h->map_n_edge;
    a.n_edge_pad = h->map_n_edge_pad;
    a.xr = g->x_reverse != 0;
    a.yr = g->y_reverse != 0;
    a.rescale = g->rescale;
    a.scale = g->scale;
    a.offx = g->offset_x;
    a.offy = g->offset_y;
    a.xmax = g->x_max;
    a.ymax = g->y_max;
    a.occ = static_cast<const unsigned char*>(h->dmap_occ.p);
    a.edge = static_cast<const unsigned*>(h->dmap_edge.p);
    a.n_snapped = g->n_snapped;
    a.n_outside = g->n_outside;
    if (a.n_outside) HIP_TRY(hipMemsetAsync(a.n_outside, 0, (size_t)B * sizeof(int32_t), h->stream));
    // four items per workgroup pass; at most 8 workgroups per CU, so that the edge list is staged a few times per CU only
    const int wpg = nmpc::kSnapThreads / 64;
    const long long want = ((long long)a.items + wpg - 1) / wpg, cap = 8LL * std::max(1, h->n_simd / 4);
    const unsigned grid = (unsigned)std::min(want, cap);
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    if (a.P <= 64)
        launch_snap<T, 1>(h, a, raw, hypos, grid);
    else if (a.P <= 128)
        launch_snap<T, 2>(h, a, raw, hypos, grid);
    else if (a.P <= 192)
        launch_snap<T, 3>(h, a, raw, hypos, grid);
    else
        launch_snap<T, 4>(h, a, raw, hypos, grid);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    h->timed = true;
    return 0;
}

template <typename T>
int loop_step(nmpc_handle_s* h, const nmpc_loop_args* g, bool post)
{
    if (!h || !g) return fail(NMPC_ERR_INVALID_ARGUMENT, "null argument");
    if (g->n_run <= 0) return g->n_run == 0 ? 0 : fail(NMPC_ERR_INVALID_ARGUMENT, "n_run < 0");
    if (g->B < g->n_run || g->H < 1 || g->H > 64 || g->W < 1 || g->Lmax < 1 || g->M < 0 || g->step < 0 || g->step >= g->max_steps)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_loop_*: bad dimensions (B %d, n_run %d, H %d, W %d, Lmax %d, M %d, step %d of %d)",
                    g->B, g->n_run, g->H, g->W, g->Lmax, g->M, g->step, g->max_steps);
    if (!g->run && g->n_run != g->B) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_loop_*: run = NULL needs n_run = B");
    if (g->n_hyp < 0 || (g->n_hyp > 1 && (long long)g->H * g->n_hyp > h->cfg.Ndynobs))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_loop_*: H * n_hyp = %d x %d rows exceed Ndynobs = %d", g->H, g->n_hyp, h->cfg.Ndynobs);
    const void* need[] = {g->robot, g->last_u, g->humans, g->hist, g->hcount, g->hidx, g->hpath, g->ref_traj, g->ref_len,
                          g->idx_ref, g->goal, g->alive, g->collision, g->complete, g->steps, g->clr_dyn, g->clr_stc,
                          g->dev_sum, g->dev_max, g->n_traj, g->traj, g->acts, g->state_c, g->last_u_c, g->refs_c,
                          g->speed_c, g->dyn_c, g->U_c, g->y_c, g->U, g->y};
    for (const void* q : need)
        if (!q) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_loop_*: a required array is NULL");
    if (g->M > 0 && !g->polys) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_loop_*: polys is NULL");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    // (a host pointer here would fault inside the kernel: three samples of the argument block are looked up)
    if (h->ptr_mode != NMPC_PTR_DEVICE && (!is_device_ptr(g->robot) || !is_device_ptr(g->U_c) || !is_device_ptr(g->dyn_c)))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_loop_*: every array must be a device pointer");
    nmpc::LoopParams<T> p;
    std::memset(&p, 0, sizeof p);
    p.B = g->B, p.n_run = g->n_run, p.N = h->cfg.N_hor, p.H = g->H, p.W = g->W, p.Lmax = g->Lmax, p.M = g->M;
    p.step = g->step, p.max_steps = g->max_steps;
    p.run = reinterpret_cast<const long long*>(g->run);
    p.ts = (T)h->cfg.ts, p.base_speed = (T)g->base_speed, p.lin_vel_max = (T)g->lin_vel_max;
    p.human_size = (T)g->human_size, p.human_vmax = (T)g->human_vmax;
    p.robot = static_cast<T*>(g->robot), p.last_u = static_cast<T*>(g->last_u), p.humans = static_cast<T*>(g->humans);
    p.hist = static_cast<T*>(g->hist);
    p.hcount = reinterpret_cast<long long*>(g->hcount), p.hidx = reinterpret_cast<long long*>(g->hidx);
    p.hpath = static_cast<const T*>(g->hpath), p.ref_traj = static_cast<const T*>(g->ref_traj);
    p.ref_len = reinterpret_cast<const long long*>(g->ref_len), p.idx_ref = reinterpret_cast<long long*>(g->idx_ref);
    p.goal = static_cast<const T*>(g->goal), p.polys = static_cast<const T*>(g->polys);
    p.stagger = static_cast<const T*>(g->stagger);
    p.alive = g->alive, p.collision = g->collision, p.complete = g->complete;
    p.steps = reinterpret_cast<long long*>(g->steps);
    p.clr_dyn = static_cast<T*>(g->clr_dyn), p.clr_stc = static_cast<T*>(g->clr_stc), p.dev_sum = static_cast<T*>(g->dev_sum);
    p.dev_max = static_cast<T*>(g->dev_max), p.n_traj = static_cast<T*>(g->n_traj);
    p.traj = static_cast<T*>(g->traj), p.acts = static_cast<T*>(g->acts);
    p.state_c = static_cast<T*>(g->state_c), p.last_u_c = static_cast<T*>(g->last_u_c), p.refs_c = static_cast<T*>(g->refs_c);
    p.speed_c = static_cast<T*>(g->speed_c), p.dyn_c = static_cast<T*>(g->dyn_c);
    p.U_c = static_cast<T*>(g->U_c), p.y_c = static_cast<T*>(g->y_c), p.U = static_cast<T*>(g->U), p.y = static_cast<T*>(g->y);
    p.gather_y = g->gather_y;
    p.n_hyp = g->n_hyp, p.hyp_fan = (T)g->hyp_fan_rad, p.hyp_r0 = (T)g->hyp_radius0, p.hyp_grow = (T)g->hyp_radius_growth;
    if (post)
        hipLaunchKernelGGL(nmpc::loop_post_kernel<T>, dim3(g->n_run), dim3(64), 0, h->stream, p);
    else
        hipLaunchKernelGGL(nmpc::loop_pre_kernel<T>, dim3(g->n_run), dim3(64), 0, h->stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T>
int kf_predict(nmpc_handle_s* h, const nmpc_kf_args* g)
{
    if (!h || !g) return fail(NMPC_ERR_INVALID_ARGUMENT, "null argument");
    if (g->n_run <= 0) return g->n_run == 0 ? 0 : fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_kf_predict: n_run < 0");
    if (g->B < g->n_run || g->H < 1 || g->cap < 1)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_kf_predict: bad dimensions (B %d, n_run %d, H %d, cap %d)", g->B, g->n_run, g->H, g->cap);
    if (g->H > h->cfg.Ndynobs) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_kf_predict: H = %d rows exceed Ndynobs = %d", g->H, h->cfg.Ndynobs);
    if (!g->run && g->n_run != g->B) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_kf_predict: run = NULL needs n_run = B");
    if (!g->humans || !g->hcount || !g->kf_traj || !g->kf_len || !g->kf_P || !g->dyn_c)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_kf_predict: a required array is NULL");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    // (a host pointer here would fault inside the kernel: three samples of the argument block are looked up)
    if (h->ptr_mode != NMPC_PTR_DEVICE && (!is_device_ptr(g->humans) || !is_device_ptr(g->kf_traj) || !is_device_ptr(g->dyn_c)))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_kf_predict: every array must be a device pointer");
    nmpc::KfParams<T> p;
    std::memset(&p, 0, sizeof p);
    p.B = g->B, p.n_run = g->n_run, p.N = h->cfg.N_hor, p.H = g->H, p.cap = g->cap;
    p.run = reinterpret_cast<const long long*>(g->run);
    p.humans = static_cast<const T*>(g->humans), p.hcount = reinterpret_cast<const long long*>(g->hcount);
    p.kf_traj = static_cast<T*>(g->kf_traj), p.kf_len = reinterpret_cast<long long*>(g->kf_len);
    p.kf_P = static_cast<T*>(g->kf_P), p.dyn_c = static_cast<T*>(g->dyn_c);
    for (int i = 0; i < 16; ++i) p.A[i] = (T)g->A[i], p.Q[i] = (T)g->Q[i];
    for (int i = 0; i < 8; ++i) p.C[i] = (T)g->C[i];
    for (int i = 0; i < 4; ++i) p.R[i] = (T)g->R[i];
    p.human_size = (T)g->human_size;
    hipLaunchKernelGGL(nmpc::kf_predict_kernel<T>, dim3(g->n_run), dim3(64), 0, h->stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// nmpc_fleet_exchange_* (post = false) and nmpc_fleet_post_* (post = true): csrc/nmpc_fleet.h
template <typename T>
int fleet_step(nmpc_handle_s* h, const nmpc_fleet_args* g, bool post)
{
    const char* fn = post ? "nmpc_fleet_post" : "nmpc_fleet_exchange";
    if (!h || !g) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: the handle or the argument block is NULL", fn);
    if (g->R < 1) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: R = %d, a fleet has at least one member", fn, g->R);
    if (g->R > 64) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: R = %d exceeds the 64 members one wavefront holds", fn, g->R);
    if (g->B < 1 || g->B % g->R != 0) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: B = %d is not a positive multiple of R = %d", fn, g->B, g->R);
    if (g->n_run <= 0) return g->n_run == 0 ? 0 : fail(NMPC_ERR_INVALID_ARGUMENT, "%s: n_run = %d < 0", fn, g->n_run);
    if (g->n_run > g->B) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: n_run = %d exceeds B = %d", fn, g->n_run, g->B);
    if (!g->run && g->n_run != g->B) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: run = NULL needs n_run = B", fn);
    if (!g->robot) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: robot is NULL", fn);
    if (post) {
        if (!g->alive || !g->clr_fleet || !g->collision || !g->complete)
            return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: alive, clr_fleet, collision or complete is NULL", fn);
    } else {
        if (!g->other_c) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: other_c is NULL", fn);
        if (g->U_prev && !g->alive) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: alive is NULL beside a U_prev", fn);
    }
    const size_t row_bytes = (size_t)3 * (h->cfg.N_hor + 1) * h->cfg.Nother * sizeof(T);
    if (!post && row_bytes > kLdsOptIn)
        return fail(NMPC_ERR_UNSUPPORTED, "%s: the staged row of 3 (N_hor + 1) Nother reals = %zu bytes exceeds 48 KB", fn, row_bytes);
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    // (a host pointer here would fault inside the kernel: samples of the argument block are looked up)
    if (h->ptr_mode != NMPC_PTR_DEVICE && (!is_device_ptr(g->robot) || !is_device_ptr(post ? g->clr_fleet : g->other_c) ||
                                           (g->run && !is_device_ptr(g->run))))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: every array must be a device pointer", fn);
    nmpc::FleetParams<T> p;
    std::memset(&p, 0, sizeof p);
    p.B = g->B, p.R = g->R, p.n_run = g->n_run, p.N = h->cfg.N_hor, p.Nother = h->cfg.Nother;
    p.run = reinterpret_cast<const long long*>(g->run);
    p.ts = (T)(g->ts > 0.0 ? g->ts : h->cfg.ts), p.width = (T)(g->width > 0.0 ? g->width : h->cfg.vehicle_width);
    p.robot = static_cast<const T*>(g->robot), p.U = static_cast<const T*>(g->U_prev);
    p.alive = g->alive, p.collision = g->collision, p.complete = g->complete, p.collision_fleet = g->collision_fleet;
    p.other_c = static_cast<T*>(g->other_c), p.clr_fleet = static_cast<T*>(g->clr_fleet);
    if (post)
        hipLaunchKernelGGL(nmpc::fleet_post_kernel<T>, dim3(g->n_run), dim3(64), 0, h->stream, p);
    else
        hipLaunchKernelGGL(nmpc::fleet_exchange_kernel<T>, dim3(g->n_run), dim3(64), row_bytes, h->stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// What nmpc_mmp_input and nmpc_mmp_stem share (their args and params structs agree in these names): the refusals both open
// with, under the name fn, and the item list, history and plane constants -- both kernels must compute the same planes.
template <typename Args>
int mmp_check(const char* fn, const Args* g)
{
    if (g->B < 1 || g->H < 1) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: B = %d, H = %d", fn, g->B, g->H);
    if (g->n_item < 0 || g->n_item > (long long)g->B * g->H)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: n_item = %d outside 0 .. B * H = %lld", fn, g->n_item, (long long)g->B * g->H);
    if (g->n_off < 1) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: n_off = %d < 1", fn, g->n_off);
    if (g->Hm < 1 || g->Wm < 1) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: map %d x %d", fn, g->Hm, g->Wm);
    if (!(g->sigma > 0.0)) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: sigma = %g", fn, g->sigma);
    if (!(g->scale != 0.0)) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: scale = %g", fn, g->scale);
    return 0;
}

template <typename Params, typename Args>
void mmp_fill(Params& p, const Args* g)
{
    p.n_item = g->n_item, p.n_off = g->n_off, p.Hm = g->Hm, p.Wm = g->Wm;
    p.xr = g->x_reverse != 0, p.yr = g->y_reverse != 0;
    p.n_ped = (long long)g->B * g->H;
    p.items = reinterpret_cast<const long long*>(g->items);
    p.hist = g->hist, p.hcount = reinterpret_cast<const long long*>(g->hcount);
    p.scale = g->scale, p.offx = g->offset_x, p.offy = g->offset_y, p.xmax = g->x_max, p.ymax = g->y_max, p.rescale = g->rescale;
    p.s2 = g->sigma * g->sigma;
    p.k = 1.0 / (2.0 * 3.141592653589793 * g->sigma * g->sigma); // numpy's order: ((2 pi) sigma_x) sigma_y
    p.ref = g->ref_image;
}

template <typename T, int V>
void launch_mmp(nmpc_handle_s* h, nmpc::MmpParams& p, long long groups)
{
    p.bpi = (int)((groups / V + nmpc::kMmpThreads - 1) / nmpc::kMmpThreads);
    hipLaunchKernelGGL((nmpc::mmp_input_kernel<T, V>), dim3((unsigned)((long long)p.n_item * p.bpi)), dim3(nmpc::kMmpThreads), 0, h->stream, p);
}

template <typename T>
int mmp_input(nmpc_handle_s* h, const nmpc_mmp_args* g)
{
    if (!h || !g) return fail(NMPC_ERR_INVALID_ARGUMENT, "null argument");
    if (const int rc = mmp_check("nmpc_mmp_input", g)) return rc;
    if (!g->hist || !g->hcount || !g->ref_image || !g->out) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_input: a required array is NULL");
    if (g->n_item == 0) return 0;
    const long long HW = (long long)g->Hm * g->Wm;
    // the widest store for which every plane start (a multiple of HW floats behind out) stays aligned
    const uintptr_t addr = reinterpret_cast<uintptr_t>(g->out);
    if (addr % 4) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_input: out is not aligned to float");
    const int V = (HW % 4 == 0 && addr % 16 == 0) ? 4 : (HW % 2 == 0 && addr % 8 == 0) ? 2 : 1;
    const long long bpi = (HW / V + nmpc::kMmpThreads - 1) / nmpc::kMmpThreads;
    if (bpi * g->n_item > 0x7fffffffLL) return fail(NMPC_ERR_UNSUPPORTED, "nmpc_mmp_input: %lld workgroups", bpi * g->n_item);
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    // (a host pointer here would fault inside the kernel: three samples of the argument block are looked up)
    if (h->ptr_mode != NMPC_PTR_DEVICE && (!is_device_ptr(g->hist) || !is_device_ptr(g->ref_image) || !is_device_ptr(g->out)))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_input: every array must be a device pointer");
    nmpc::MmpParams p;
    std::memset(&p, 0, sizeof p);
    mmp_fill(p, g);
    p.H = g->H, p.out = g->out;
    if (V == 4)
        launch_mmp<T, 4>(h, p, HW);
    else if (V == 2)
        launch_mmp<T, 2>(h, p, HW);
    else
        launch_mmp<T, 1>(h, p, HW);
    HIP_TRY(hipGetLastError());
    return 0;
}

// IO: the entry nmpc_mmp_stem_io_*, whose out (out_f16 = 1) is binary16 in the octet form (mmp_stem_kernel<MmpStemH<T>>); every other
// refusal keeps the words of nmpc_mmp_stem_*
template <typename T, bool IO = false>
int mmp_stem(nmpc_handle_s* h, const nmpc_mmp_stem_args* g, int32_t out_f16 = 0)
{
    if (!h || !g) return fail(NMPC_ERR_INVALID_ARGUMENT, "null argument");
    if constexpr (IO) {
        if (out_f16 != 0 && out_f16 != 1) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_stem_io: out_f16 = %d (0 or 1)", out_f16);
    }
    if (const int rc = mmp_check("nmpc_mmp_stem", g)) return rc;
    if (g->C < nmpc::kStemCG || g->C % nmpc::kStemCG) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_stem: C = %d is no positive multiple of 8", g->C);
    if (!std::isfinite(g->slope)) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_stem: slope = %g", (double)g->slope);
    if (!g->hist || !g->hcount || !g->ref_image || !g->weight || !g->bn_scale || !g->bn_shift || !g->out)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_stem: a required array is NULL");
    if (g->n_item == 0) return 0;
    if (reinterpret_cast<uintptr_t>(g->out) % 4) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_stem: out is not aligned to float");
    if (out_f16 && reinterpret_cast<uintptr_t>(g->out) % 16) // (half an octet is one 8-byte store, and the blocks load whole octets)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_stem_io: a binary16 out is not aligned to 16 bytes");
    nmpc::MmpStemParams p;
    std::memset(&p, 0, sizeof p);
    p.Ho = (g->Hm - 1) / 2 + 1, p.Wo = (g->Wm - 1) / 2 + 1;
    p.Hp = nmpc::mmp_stem_out(g->Hm), p.Wp = nmpc::mmp_stem_out(g->Wm);
    p.ty = (p.Hp + nmpc::kStemTPH - 1) / nmpc::kStemTPH, p.tx = (p.Wp + nmpc::kStemTPW - 1) / nmpc::kStemTPW;
    const long long groups = (long long)p.ty * p.tx * g->n_item;
    if ((long long)p.ty * p.tx > 0x7fffffffLL || groups > 0x7fffffffLL) return fail(NMPC_ERR_UNSUPPORTED, "nmpc_mmp_stem: %lld workgroups", groups);
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    // (a host pointer here would fault inside the kernel: samples of the argument block are looked up)
    if (h->ptr_mode != NMPC_PTR_DEVICE && (!is_device_ptr(g->hist) || !is_device_ptr(g->ref_image) || !is_device_ptr(g->weight) || !is_device_ptr(g->out)))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_stem: every array must be a device pointer");
    mmp_fill(p, g);
    p.C = g->C, p.mono = g->slope >= 0.0f;
    p.weight = g->weight, p.bn_scale = g->bn_scale, p.bn_shift = g->bn_shift, p.slope = g->slope, p.out = g->out;
    auto kernel = nmpc::mmp_stem_kernel<T>;
    if (out_f16) kernel = nmpc::mmp_stem_kernel<nmpc::MmpStemH<T>>; // (p.out points at binary16: the kernel casts it)
    hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(nmpc::kStemThreads), 0, h->stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// (layer1's entry, on its own: no stride, and -- on record, unlike mmp_strided below -- neither |slope| <= 1 nor planes up to 2^30 are demanded)
int mmp_block(nmpc_handle_s* h, const nmpc_mmp_block_args* g)
{
    if (!h || !g) return fail(NMPC_ERR_INVALID_ARGUMENT, "null argument");
    if (g->M < 0) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_block: M = %d < 0", g->M);
    if (g->H < 1 || g->W < 1) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_block: plane %d x %d", g->H, g->W);
    if (g->Cin < 8 || g->Cin > 256 || g->Cin % nmpc::kBlkCC)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_block: Cin = %d is no multiple of 8 from 8 to 256", g->Cin);
    if (!g->wd && g->Cin != nmpc::kBlkC)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_block: Cin = %d without a projection (the identity needs Cin = 16)", g->Cin);
    if (!std::isfinite(g->slope_mid) || !std::isfinite(g->slope_out))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_block: slope_mid = %g, slope_out = %g", (double)g->slope_mid, (double)g->slope_out);
    if (!g->x || !g->w1 || !g->s1 || !g->b1 || !g->w2 || !g->s2 || !g->b2 || (g->wd && (!g->sd || !g->bd)) || !g->out)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_block: a required array is NULL");
    if (reinterpret_cast<uintptr_t>(g->out) % 4 || reinterpret_cast<uintptr_t>(g->x) % 4)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_block: x or out is not aligned to float");
    if (g->M == 0) return 0;
    nmpc::MmpBlockParams p;
    std::memset(&p, 0, sizeof p);
    const long long ty = ((long long)g->H + nmpc::kBlkTH - 1) / nmpc::kBlkTH, tx = ((long long)g->W + nmpc::kBlkTW - 1) / nmpc::kBlkTW;
    const long long tiles = ty * tx; // < 2^56
    if (tiles > 0x7fffffffLL || tiles * g->M > 0x7fffffffLL) return fail(NMPC_ERR_UNSUPPORTED, "nmpc_mmp_block: %lld x %d workgroups", tiles, g->M);
    const long long groups = tiles * g->M;
    p.ty = (int)ty, p.tx = (int)tx;
    // out must not overlap x: a tile's halo is read after the neighbouring tiles have been written
    const unsigned long long hw = (unsigned long long)g->H * g->W * g->M * 4; // < 2^31 * 420 * 4 after the test above
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(g->x), o0 = reinterpret_cast<uintptr_t>(g->out);
    if (x0 < o0 + hw * nmpc::kBlkC && o0 < x0 + hw * g->Cin) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_block: out overlaps x");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    // (a host pointer here would fault inside the kernel)
    if (h->ptr_mode != NMPC_PTR_DEVICE) {
        const void* ptrs[] = {g->x, g->w1, g->s1, g->b1, g->w2, g->s2, g->b2, g->out, g->wd, g->sd, g->bd};
        for (int i = 0; i < (g->wd ? 11 : 8); ++i)
            if (!is_device_ptr(ptrs[i])) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_block: every array must be a device pointer");
    }
    p.M = g->M, p.Cin = g->Cin, p.H = g->H, p.W = g->W;
    p.x = g->x, p.w1 = g->w1, p.s1 = g->s1, p.b1 = g->b1, p.w2 = g->w2, p.s2 = g->s2, p.b2 = g->b2;
    p.wd = g->wd, p.sd = g->sd, p.bd = g->bd, p.slope_mid = g->slope_mid, p.slope_out = g->slope_out, p.out = g->out;
    if (g->wd)
        hipLaunchKernelGGL(nmpc::mmp_block_kernel<true>, dim3((unsigned)groups), dim3(nmpc::kBlkThreads), 0, h->stream, p);
    else
        hipLaunchKernelGGL(nmpc::mmp_block_kernel<false>, dim3((unsigned)groups), dim3(nmpc::kBlkThreads), 0, h->stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The three strided stages (layer2 .. layer4) behind one entry, mmp_strided<Stage>. A Stage says what differs: the name in the
// messages, the structs, the output channels C, the threads of a workgroup, how the plane of outputs H2 x W2 is cut into ty x tx
// tiles, the alignment of packed weights (0: plain float arrays), and the kernels <stride 2, projection>, <stride 1, projection>,
// <stride 1, identity>; a stage on binary16 operands has an Io beside them: the same three kernels for each other form of x and
// out in memory (MmpBlkhIoKernels below; nmpc_mmp_blockN_f16_io). Two numbers of the entry follow from
// a stage's tile: the kernels' pixel coordinates are ints and reach 2 (tile origin + reach) + 1, which must not wrap -- hence no
// plane over 2^30 --, and once the workgroup count has passed H2 W2 M <= (outputs of a tile) x 2^31, with H W <= 4 H2 W2: the byte
// counts of the overlap test do not overflow.
// The kernels of a geometry G of the float32 block (csrc/nmpc_mmp_block_f32.h), in a stage's order
template <typename G>
struct MmpBlkfKernels {
    static constexpr void (*table[3])(typename G::Params) = {nmpc::mmp_blkf_kernel<G, 2, true>, nmpc::mmp_blkf_kernel<G, 1, true>, nmpc::mmp_blkf_kernel<G, 1, false>};
};

// The kernels of a geometry G on the octet form of binary16 activations (csrc/nmpc_mmp_block_f16.h): table[2 x_f16 + out_f16 - 1]
// holds <stride 2, projection>, <stride 1, projection>, <stride 1, identity>, as a stage's kernels[] does for float32 memory
template <typename G>
struct MmpBlkhIoKernels {
    template <bool XH, bool OH>
    using Io = nmpc::MmpBlkhIo<G, XH, OH>;
    static constexpr void (*table[3][3])(typename G::Params) = {
        {nmpc::mmp_blkh_kernel<Io<false, true>, 2, true>, nmpc::mmp_blkh_kernel<Io<false, true>, 1, true>, nmpc::mmp_blkh_kernel<Io<false, true>, 1, false>},
        {nmpc::mmp_blkh_kernel<Io<true, false>, 2, true>, nmpc::mmp_blkh_kernel<Io<true, false>, 1, true>, nmpc::mmp_blkh_kernel<Io<true, false>, 1, false>},
        {nmpc::mmp_blkh_kernel<Io<true, true>, 2, true>, nmpc::mmp_blkh_kernel<Io<true, true>, 1, true>, nmpc::mmp_blkh_kernel<Io<true, true>, 1, false>}};
};

struct MmpLayer2 {
    using Args = nmpc_mmp_block2_args;
    using Params = nmpc::MmpBlock2Params;
    static constexpr const char* name = "nmpc_mmp_block2";
    static constexpr int C = nmpc::kB2C, threads = nmpc::kB2Threads, packed_align = 0;
    static constexpr auto& kernels = MmpBlkfKernels<nmpc::MmpBlock2Geom>::table;
    // tiles of 8 x 44 = 352 outputs; reach 11
    template <typename P>
    static void tile(P& p, long long& ty, long long& tx)
    {
        ty = ((long long)p.H2 + nmpc::kB2TH - 1) / nmpc::kB2TH, tx = ((long long)p.W2 + nmpc::kB2TW - 1) / nmpc::kB2TW;
    }
};

// layer2 with binary16 MFMA operands (csrc/nmpc_mmp_block2_f16.h): layer2's channels, threads and tiles; w1, w2 and wd are the
// packed fragments, 16 bytes per lane, which is what packed_align adds to the checks
struct MmpLayer2F16 : MmpLayer2 {
    using Args = nmpc_mmp_block2_f16_args;
    using Params = nmpc::MmpBlock2HParams;
    using Io = MmpBlkhIoKernels<nmpc::MmpBlock2HGeom>;
    static constexpr const char* name = "nmpc_mmp_block2_f16";
    static constexpr const char* io_name = "nmpc_mmp_block2_f16_io";
    static constexpr int packed_align = 16;
    static constexpr void (*kernels[3])(Params) = {nmpc::mmp_blkh_kernel<nmpc::MmpBlock2HGeom, 2, true>, nmpc::mmp_blkh_kernel<nmpc::MmpBlock2HGeom, 1, true>, nmpc::mmp_blkh_kernel<nmpc::MmpBlock2HGeom, 1, false>};
};

struct MmpLayer3 {
    using Args = nmpc_mmp_block3_args;
    using Params = nmpc::MmpBlock3Params;
    static constexpr const char* name = "nmpc_mmp_block3";
    static constexpr int C = nmpc::kB3C, threads = nmpc::kB3Threads, packed_align = 0;
    static constexpr auto& kernels = MmpBlkfKernels<nmpc::MmpBlock3Geom>::table;
    // tiles of 7 x 21 = 147 outputs; reach 10
    template <typename P>
    static void tile(P& p, long long& ty, long long& tx)
    {
        ty = ((long long)p.H2 + nmpc::kB3TH - 1) / nmpc::kB3TH, tx = ((long long)p.W2 + nmpc::kB3TW - 1) / nmpc::kB3TW;
    }
};

// layer3 with binary16 MFMA operands (csrc/nmpc_mmp_block3_f16.h): layer3's channels, threads and tiles; w1, w2 and wd are the
// packed fragments, 16 bytes per lane, which is what packed_align adds to the checks
struct MmpLayer3F16 : MmpLayer3 {
    using Args = nmpc_mmp_block3_f16_args;
    using Params = nmpc::MmpBlock3HParams;
    using Io = MmpBlkhIoKernels<nmpc::MmpBlock3HGeom>;
    static constexpr const char* name = "nmpc_mmp_block3_f16";
    static constexpr const char* io_name = "nmpc_mmp_block3_f16_io";
    static constexpr int packed_align = 16;
    static constexpr void (*kernels[3])(Params) = {nmpc::mmp_blkh_kernel<nmpc::MmpBlock3HGeom, 2, true>, nmpc::mmp_blkh_kernel<nmpc::MmpBlock3HGeom, 1, true>, nmpc::mmp_blkh_kernel<nmpc::MmpBlock3HGeom, 1, false>};
};

struct MmpLayer4 {
    using Args = nmpc_mmp_block4_args;
    using Params = nmpc::MmpBlock4Params;
    static constexpr const char* name = "nmpc_mmp_block4";
    static constexpr int C = nmpc::kB4C, threads = nmpc::kB4Threads, packed_align = 0;
    static constexpr auto& kernels = MmpBlkfKernels<nmpc::MmpBlock4Geom>::table;
    // tiles of at most 10 x 11 = 110 outputs; reach 11. A side that fits the tile's plane of m is one tile without a halo; a longer
    // one is cut with a halo of one
    template <typename P>
    static void tile(P& p, long long& ty, long long& tx)
    {
        ty = nmpc::mmp_b4_tiles(p.H2, nmpc::kB4MH), tx = nmpc::mmp_b4_tiles(p.W2, nmpc::kB4MW);
        p.oy = p.H2 <= nmpc::kB4MH ? 1 : 2, p.ox = p.W2 <= nmpc::kB4MW ? 1 : 2;
    }
};

// layer4 with binary16 MFMA operands (csrc/nmpc_mmp_block4_f16.h): layer4's channels and tiles on workgroups of 256 threads; w1,
// w2 and wd are the packed fragments, 16 bytes per lane, which is what packed_align adds to the checks
struct MmpLayer4F16 : MmpLayer4 {
    using Args = nmpc_mmp_block4_f16_args;
    using Params = nmpc::MmpBlock4HParams;
    using Io = MmpBlkhIoKernels<nmpc::MmpBlock4HGeom>;
    static constexpr const char* name = "nmpc_mmp_block4_f16";
    static constexpr const char* io_name = "nmpc_mmp_block4_f16_io";
    static constexpr int threads = nmpc::kB4HThreads, packed_align = 16;
    static constexpr void (*kernels[3])(Params) = {nmpc::mmp_blkh_kernel<nmpc::MmpBlock4HGeom, 2, true>, nmpc::mmp_blkh_kernel<nmpc::MmpBlock4HGeom, 1, true>, nmpc::mmp_blkh_kernel<nmpc::MmpBlock4HGeom, 1, false>};
};

// layer1 with binary16 MFMA operands (csrc/nmpc_mmp_block1_f16.h): 16 channels, tiles of 15 x 28 outputs (reach 3), no stride --
// the entry hands its struct on with stride = 1 -- and so no kernel <stride 2, .>; the geometry follows the projection
struct MmpLayer1F16 {
    struct Args : nmpc_mmp_block_f16_args {
        int32_t stride;
    };
    using Params = nmpc::MmpBlock1HParams;
    template <bool PROJ, bool XH, bool OH>
    using G = nmpc::MmpBlkhIo<nmpc::MmpBlock1HGeom<PROJ>, XH, OH>;
    struct Io {
        static constexpr void (*table[3][3])(Params) = {
            {nullptr, nmpc::mmp_blkh_kernel<G<true, false, true>, 1, true>, nmpc::mmp_blkh_kernel<G<false, false, true>, 1, false>},
            {nullptr, nmpc::mmp_blkh_kernel<G<true, true, false>, 1, true>, nmpc::mmp_blkh_kernel<G<false, true, false>, 1, false>},
            {nullptr, nmpc::mmp_blkh_kernel<G<true, true, true>, 1, true>, nmpc::mmp_blkh_kernel<G<false, true, true>, 1, false>}};
    };
    static constexpr const char* name = "nmpc_mmp_block_f16";
    static constexpr const char* io_name = "nmpc_mmp_block_f16_io";
    static constexpr int C = nmpc::kBlkC, threads = nmpc::kBlkThreads, packed_align = 16;
    static constexpr void (*kernels[3])(Params) = {nullptr, nmpc::mmp_blkh_kernel<nmpc::MmpBlock1HGeom<true>, 1, true>,
                                                   nmpc::mmp_blkh_kernel<nmpc::MmpBlock1HGeom<false>, 1, false>};
    template <typename P>
    static void tile(P& p, long long& ty, long long& tx)
    {
        ty = ((long long)p.H2 + nmpc::kBlkTH - 1) / nmpc::kBlkTH, tx = ((long long)p.W2 + nmpc::kBlkTW - 1) / nmpc::kBlkTW;
    }
};

// IO: the entry nmpc_mmp_blockN_f16_io, whose x (x_f16 = 1) and out (out_f16 = 1) are binary16 in the octet form
template <typename Stage, bool IO = false>
int mmp_strided(nmpc_handle_s* h, const typename Stage::Args* g, int32_t x_f16 = 0, int32_t out_f16 = 0)
{
    const char* fn = Stage::name;
    if constexpr (IO) fn = Stage::io_name;
    if (!h || !g) return fail(NMPC_ERR_INVALID_ARGUMENT, "null argument");
    if ((x_f16 != 0 && x_f16 != 1) || (out_f16 != 0 && out_f16 != 1))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: x_f16 = %d, out_f16 = %d (each is 0 or 1)", fn, x_f16, out_f16);
    if (g->M < 0) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: M = %d < 0", fn, g->M);
    if (g->H < 1 || g->W < 1) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: plane %d x %d", fn, g->H, g->W);
    if (g->stride != 1 && g->stride != 2) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: stride = %d is neither 1 nor 2", fn, g->stride);
    if (g->Cin < 8 || g->Cin > 256 || g->Cin % 8) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: Cin = %d is no multiple of 8 from 8 to 256", fn, g->Cin);
    if (!g->wd && (g->Cin != Stage::C || g->stride != 1))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: Cin = %d, stride = %d without a projection (the identity needs Cin = %d and stride 1)", fn, g->Cin,
                    g->stride, Stage::C);
    if (!std::isfinite(g->slope_mid) || !std::isfinite(g->slope_out) || std::fabs(g->slope_mid) > 1.0f || std::fabs(g->slope_out) > 1.0f)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: slope_mid = %g, slope_out = %g (finite, |slope| <= 1)", fn, (double)g->slope_mid,
                    (double)g->slope_out);
    if (!g->x || !g->w1 || !g->s1 || !g->b1 || !g->w2 || !g->s2 || !g->b2 || (g->wd && (!g->sd || !g->bd)) || !g->out)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: a required array is NULL", fn);
    if (reinterpret_cast<uintptr_t>(g->out) % 4 || reinterpret_cast<uintptr_t>(g->x) % 4)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: x or out is not aligned to float", fn);
    if ((x_f16 && reinterpret_cast<uintptr_t>(g->x) % 16) || (out_f16 && reinterpret_cast<uintptr_t>(g->out) % 16)) // (an octet is one 16-byte access)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: a binary16 x or out is not aligned to 16 bytes", fn);
    if constexpr (Stage::packed_align != 0) { // (the stages with packed weights: each lane loads a whole fragment)
        const void* packed[] = {g->w1, g->w2, g->wd};
        for (const void* q : packed)
            if (reinterpret_cast<uintptr_t>(q) % Stage::packed_align)
                return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: w1, w2 or wd is not aligned to %d bytes", fn, Stage::packed_align);
    }
    if (g->M == 0) return 0;
    if (g->H > (1 << 30) || g->W > (1 << 30)) return fail(NMPC_ERR_UNSUPPORTED, "%s: plane %d x %d over 2^30", fn, g->H, g->W);
    typename Stage::Params p;
    std::memset(&p, 0, sizeof p);
    p.H2 = (g->H - 1) / g->stride + 1, p.W2 = (g->W - 1) / g->stride + 1;
    long long ty, tx;
    Stage::tile(p, ty, tx);
    const long long tiles = ty * tx; // < 2^56
    if (tiles > 0x7fffffffLL || tiles * g->M > 0x7fffffffLL) return fail(NMPC_ERR_UNSUPPORTED, "%s: %lld x %d workgroups", fn, tiles, g->M);
    const long long groups = tiles * g->M;
    p.ty = (int)ty, p.tx = (int)tx;
    // out must not overlap x: a tile's halo is read after the neighbouring tiles have been written
    // (2 bytes per element on a binary16 side)
    const unsigned long long xb = (unsigned long long)g->H * g->W * g->M * (x_f16 ? 2 : 4) * g->Cin;
    const unsigned long long ob = (unsigned long long)p.H2 * p.W2 * g->M * (out_f16 ? 2 : 4) * Stage::C;
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(g->x), o0 = reinterpret_cast<uintptr_t>(g->out);
    if (x0 < o0 + ob && o0 < x0 + xb) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: out overlaps x", fn);
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    // (a host pointer here would fault inside the kernel)
    if (h->ptr_mode != NMPC_PTR_DEVICE) {
        const void* ptrs[] = {g->x, g->w1, g->s1, g->b1, g->w2, g->s2, g->b2, g->out, g->wd, g->sd, g->bd};
        for (int i = 0; i < (g->wd ? 11 : 8); ++i)
            if (!is_device_ptr(ptrs[i])) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: every array must be a device pointer", fn);
    }
    p.M = g->M, p.Cin = g->Cin, p.H = g->H, p.W = g->W;
    p.x = g->x, p.w1 = g->w1, p.s1 = g->s1, p.b1 = g->b1, p.w2 = g->w2, p.s2 = g->s2, p.b2 = g->b2;
    p.wd = g->wd, p.sd = g->sd, p.bd = g->bd, p.slope_mid = g->slope_mid, p.slope_out = g->slope_out, p.out = g->out;
    const int variant = g->stride == 2 ? 0 : g->wd ? 1 : 2;
    auto kernel = Stage::kernels[variant];
    if constexpr (IO) {
        if (x_f16 || out_f16) kernel = Stage::Io::table[2 * x_f16 + out_f16 - 1][variant]; // (p.x / p.out point at binary16: the kernel casts them)
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(Stage::threads), 0, h->stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mmp_head(nmpc_handle_s* h, const nmpc_mmp_head_args* g)
{
    if (!h || !g) return fail(NMPC_ERR_INVALID_ARGUMENT, "null argument");
    if (g->M < 0) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_head: M = %d < 0", g->M);
    if (g->H < 2 || g->W < 2) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_head: plane %d x %d has no 2 x 2 window", g->H, g->W);
    if (g->C < 1) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_head: C = %d < 1", g->C);
    if (g->O < 2 || g->O > 512 || g->O % 2) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_head: O = %d is no even number from 2 to 512", g->O);
    if (!std::isfinite(g->slope) || std::fabs(g->slope) > 1.0f)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_head: slope = %g (finite, |slope| <= 1)", (double)g->slope);
    if (!g->x || !g->w1 || !g->c1 || !g->w2 || !g->c2 || !g->out) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_head: a required array is NULL");
    {
        const void* ptrs[] = {g->x, g->w1, g->c1, g->w2, g->c2, g->out};
        for (const void* q : ptrs)
            if (reinterpret_cast<uintptr_t>(q) % 4) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_head: an array is not aligned to float");
    }
    if (g->M == 0) return 0;
    // (the kernel's feature index is an int)
    const long long F = (long long)g->C * (g->H / 2) * (long long)(g->W / 2);
    if (g->H > (1 << 30) || g->W > (1 << 30) || F > (1 << 24)) return fail(NMPC_ERR_UNSUPPORTED, "nmpc_mmp_head: %lld features over 2^24", F);
    // out must not overlap x: a group's rows of out are written while other groups read theirs of x
    // (C H W <= 9 F <= 9 x 2^24 after the test above: no overflow)
    const unsigned long long xb = (unsigned long long)g->C * g->H * g->W * 4 * g->M, ob = (unsigned long long)g->O * 4 * g->M;
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(g->x), o0 = reinterpret_cast<uintptr_t>(g->out);
    if (x0 < o0 + ob && o0 < x0 + xb) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_head: out overlaps x");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    // (a host pointer here would fault inside the kernel)
    if (h->ptr_mode != NMPC_PTR_DEVICE) {
        const void* ptrs[] = {g->x, g->w1, g->c1, g->w2, g->c2, g->out};
        for (const void* q : ptrs)
            if (!is_device_ptr(q)) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_head: every array must be a device pointer");
    }
    nmpc::MmpHeadParams p;
    std::memset(&p, 0, sizeof p);
    p.M = g->M, p.C = g->C, p.H = g->H, p.W = g->W, p.O = g->O, p.F = (int)F;
    p.x = g->x, p.w1 = g->w1, p.c1 = g->c1, p.w2 = g->w2, p.c2 = g->c2, p.slope = g->slope, p.out = g->out;
    const dim3 grid((unsigned)(((long long)g->M + nmpc::kHeadRows - 1) / nmpc::kHeadRows)), block(nmpc::kHeadThreads);
    hipLaunchKernelGGL(nmpc::mmp_head_kernel, grid, block, 0, h->stream, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// largest nv * nw a scenario's window can give: per axis the window is at most min(range, 2 acc ts) wide and np.arange's
// count is ceil of a quotient that rounding can lift past an integer, so floor(...) + 1 (host only)
static long long dwa_axis_bound(double range, double acc, double ts, double res)
{
    const double w = std::min(range, 2.0 * acc * ts);
    if (!(w > 0.0)) return 1;
    const double q = w / res * (1.0 + 1e-9);
    return q < 1e9 ? (long long)q + 1 : 1000000000LL;
}

// LISTS: nmpc_dwa_step_lists_* on nmpc_dwa_lists_args (R rows per scenario with dyn_count; H and dyn_mode are not read)
template <typename T, bool LISTS = false, typename A = nmpc_dwa_args>
int dwa_step(nmpc_handle_s* h, const A* g)
{
    const char* const fn = LISTS ? "nmpc_dwa_step_lists" : "nmpc_dwa_step";
    if (!h || !g) return fail(NMPC_ERR_INVALID_ARGUMENT, "null argument");
    if constexpr (LISTS) {
        if (g->n_run < 0 || g->B < g->n_run || g->M < 0 || g->Pmax < 2 || g->cap < 1 || g->R < 1)
            return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: bad dimensions (B %d, n_run %d, R %d, M %d, Pmax %d, cap %d)", fn, g->B, g->n_run,
                        g->R, g->M, g->Pmax, g->cap);
    } else if (g->n_run < 0 || g->B < g->n_run || g->M < 0 || g->Pmax < 2 || g->cap < 1 || g->dyn_mode < 0 || g->dyn_mode > 2 ||
               (g->dyn_mode > 0 && g->H < 1) || g->H < 0)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: bad dimensions (B %d, n_run %d, H %d, M %d, Pmax %d, cap %d, dyn_mode %d)", fn,
                    g->B, g->n_run, g->H, g->M, g->Pmax, g->cap, g->dyn_mode);
    if (!g->run && g->n_run != g->B) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: run = NULL needs n_run = B", fn);
    if (!(g->vel_resolution > 0.0) || !(g->ang_resolution > 0.0) || !(g->lin_vel_max >= g->lin_vel_min) || !(g->ang_vel_max >= 0.0) ||
        !(g->lin_acc_max >= 0.0) || !(g->ang_acc_max >= 0.0))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: resolutions must be positive, limits ordered, accelerations non-negative", fn);
    if (!g->state_c || !g->last_u_c || !g->goal || !g->path || !g->path_len || !g->U_c || !g->min_cost || !g->choice || !g->counts ||
        ((LISTS || g->dyn_mode > 0) && !g->dyn_c) || (g->M > 0 && !g->polys))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: a required array is NULL", fn);
    if constexpr (LISTS)
        if (!g->dyn_count) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: a required array is NULL (dyn_count)", fn);
    const auto aligned = [](const void* q, size_t al) { return q == nullptr || reinterpret_cast<uintptr_t>(q) % al == 0; };
    for (const void* q : {g->state_c, g->last_u_c, g->dyn_c, g->goal, g->path, g->polys, (const void*)g->U_c, (const void*)g->min_cost,
                          (const void*)g->cost_all, (const void*)g->cand_all})
        if (!aligned(q, sizeof(T))) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: a real array is not aligned to its element type", fn);
    if (!aligned(g->run, 8) || !aligned(g->path_len, 8) || !aligned(g->choice, 4) || !aligned(g->counts, 4))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: an integer array is not aligned to its element type", fn);
    if constexpr (LISTS)
        if (!aligned(g->dyn_count, 4)) return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: an integer array is not aligned to its element type", fn);
    const long long need = dwa_axis_bound(g->lin_vel_max - g->lin_vel_min, g->lin_acc_max, h->cfg.ts, g->vel_resolution) *
                           dwa_axis_bound(2.0 * g->ang_vel_max, g->ang_acc_max, h->cfg.ts, g->ang_resolution);
    if (need > g->cap)
        return fail(NMPC_ERR_UNSUPPORTED, "%s: cap = %d candidates, these limits and resolutions can give %lld", fn, g->cap, need);
    size_t lds = (size_t)g->M * 4 * nmpc::kDwaEdgeReals * sizeof(T);
    if (g->M > 256) return fail(NMPC_ERR_UNSUPPORTED, "%s: M = %d rectangles > 256", fn, g->M);
    if constexpr (LISTS) {
        const long long means = (long long)g->R * (h->cfg.N_hor + 1);
        if (means > nmpc::kDwaListsMaxMeans)
            return fail(NMPC_ERR_UNSUPPORTED, "%s: R (N_hor + 1) = %lld means per scenario > %d", fn, means, nmpc::kDwaListsMaxMeans);
        lds = nmpc::dwa_lists_lds<T>(g->M, g->R, h->cfg.N_hor);
        if (lds > nmpc::kDwaListsMaxLds)
            return fail(NMPC_ERR_UNSUPPORTED, "%s: %zu B of LDS for M = %d rectangles and R = %d rows > %zu", fn, lds, g->M, g->R,
                        nmpc::kDwaListsMaxLds);
    }
    if (g->n_run == 0) return 0;
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    // (a host pointer here would fault inside the kernel: three samples of the argument block are looked up)
    if (h->ptr_mode != NMPC_PTR_DEVICE && (!is_device_ptr(g->state_c) || !is_device_ptr(g->U_c) || !is_device_ptr(g->path)))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: every array must be a device pointer", fn);
    std::conditional_t<LISTS, nmpc::DwaListsParams<T>, nmpc::DwaParams<T>> p;
    std::memset(static_cast<void*>(&p), 0, sizeof p);
    p.B = g->B, p.n_run = g->n_run, p.N = h->cfg.N_hor, p.M = g->M, p.Pmax = g->Pmax, p.cap = g->cap;
    if constexpr (LISTS) {
        if (h->ptr_mode != NMPC_PTR_DEVICE && (!is_device_ptr(g->dyn_c) || !is_device_ptr(g->dyn_count)))
            return fail(NMPC_ERR_INVALID_ARGUMENT, "%s: every array must be a device pointer", fn);
        p.H = 0, p.dyn_mode = 2, p.R = g->R, p.dyn_count = g->dyn_count;
    } else {
        p.H = g->dyn_mode > 0 ? g->H : 0, p.dyn_mode = g->dyn_mode;
    }
    p.run = reinterpret_cast<const long long*>(g->run);
    p.state_c = static_cast<const T*>(g->state_c), p.last_u_c = static_cast<const T*>(g->last_u_c);
    p.dyn_c = static_cast<const T*>(g->dyn_c), p.goal = static_cast<const T*>(g->goal), p.path = static_cast<const T*>(g->path);
    p.path_len = reinterpret_cast<const long long*>(g->path_len), p.polys = static_cast<const T*>(g->polys);
    p.ts = h->cfg.ts, p.vmin = g->lin_vel_min, p.vmax = g->lin_vel_max, p.acc = g->lin_acc_max;
    p.wmax = g->ang_vel_max, p.wacc = g->ang_acc_max, p.dv = g->vel_resolution, p.dw = g->ang_resolution;
    p.tsT = (T)h->cfg.ts, p.lin_vel_max = (T)g->lin_vel_max, p.base_speed = (T)g->lin_vel_max * (T)g->base_speed_factor;
    p.stuck = (T)g->stuck_threshold, p.q_speed = (T)g->q_speed, p.q_goal = (T)g->q_goal_dir, p.q_ref = (T)g->q_ref_deviation;
    p.q_stc = (T)g->q_stc_obstacle, p.q_dyn = (T)g->q_dyn_obstacle;
    p.U_c = static_cast<T*>(g->U_c), p.min_cost = static_cast<T*>(g->min_cost), p.choice = g->choice, p.counts = g->counts;
    p.cost_all = static_cast<T*>(g->cost_all), p.cand_all = static_cast<T*>(g->cand_all);
    const int wpg = nmpc::kDwaThreads / 64;
    if constexpr (LISTS) {
        if (lds > kLdsOptIn)
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(nmpc::dwa_step_lists_kernel<T>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(nmpc::dwa_step_lists_kernel<T>, dim3((g->n_run + wpg - 1) / wpg), dim3(nmpc::kDwaThreads), lds, h->stream, p);
    } else {
        hipLaunchKernelGGL(nmpc::dwa_step_kernel<T>, dim3((g->n_run + wpg - 1) / wpg), dim3(nmpc::kDwaThreads), lds, h->stream, p);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// the kernel(s) of a variant may use `bytes` of dynamic LDS (beyond 48 KB a kernel has to be told)
template <typename T>
int allow_lds(const Variant& v, size_t bytes)
{
    if (bytes <= kLdsOptIn) return 0;
    for (int member = 1; member <= (v.pair ? 2 : 1); ++member) {
        const void* fn = v.family >= kEval ? reinterpret_cast<const void*>(eval_kernel_of<T>(v, member))
                                           : reinterpret_cast<const void*>(solve_kernel_of<T>(v, member));
        if (fn) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    }
    return 0;
}

// every variant the plans of this handle can name, by family; families whose LDS does not fit are switched off
template <typename T>
int set_lds_limit(nmpc_handle_s* h)
{
    const Layout& L = h->lay<T>();
    const int lps = h->lays.lps, prec = sizeof(T) == 4 ? 0 : 1;
    int rc = 0;
    for (Family f : {kThroughput, kEval})
        if ((rc = allow_lds<T>(single_variant(f, L, lps), (size_t)L.lds_total * sizeof(T)))) return rc;
    if (sizeof(T) == 4 && h->lays.lay32c.rs > 0)
        for (bool eval : {false, true})
            if ((rc = allow_lds<T>(coop_onchip_variant(eval, h->cfg.N_hor), (size_t)h->lays.lay32c.lds_total_coop * sizeof(T)))) return rc;
    h->coop_ok[prec] = coop_fits(L, sizeof(T));
    if (h->coop_ok[prec])
        for (bool eval : {false, true})
            if ((rc = allow_lds<T>(coop_variant(eval, L, lps), (size_t)L.lds_total_coop * sizeof(T)))) return rc;
    h->spec_ok[prec] = latency_fits(L, sizeof(T)); // (no room for the exchange area: latency mode unavailable)
    if (h->spec_ok[prec])
        for (Family f : {kLatencyFlat, kLatencyTail}) // (allow_lds skips the tail member where there is none)
            if ((rc = allow_lds<T>(single_variant(f, L, lps), (size_t)L.lds_total_spec * sizeof(T)))) return rc;
    return 0;
}

} // namespace

// nmpc_probe_*: see include/nmpc_hip.h
template <typename T>
int probe(nmpc_handle_s* h, int op, int block_threads, int n_waves, const T* in, T* out)
{
    // (the arguments before the handle: every refusal below needs no device)
    if (op < 0 || op >= NMPC_PROBE_N_OPS) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_probe: unknown op %d (0 .. %d)", op, NMPC_PROBE_N_OPS - 1);
    if (sizeof(T) == 8 && (op == NMPC_PROBE_SINCOS_MEDIUM || op == NMPC_PROBE_SINCOS_SMALL || op >= NMPC_PROBE_WAVE_SCAN_SUFFIX_INCL_MASKED))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_probe: unknown op %d for f64 (sincos_medium / sincos_small and the masked-row scans are float only)", op);
    if (block_threads != 64 && block_threads != 128 && block_threads != 256)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_probe: block_threads %d is not 64, 128 or 256", block_threads);
    if (n_waves < 0) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_probe: negative n_waves %d", n_waves);
    if (!in || !out) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_probe: NULL in / out");
    if (!h) return fail(NMPC_ERR_INVALID_ARGUMENT, "null handle");
    if (n_waves == 0) return 0;
    const size_t waves_per_block = (size_t)block_threads / 64, blocks = ((size_t)n_waves + waves_per_block - 1) / waves_per_block;
    if (blocks > 0x7fffffffull) return fail(NMPC_ERR_UNSUPPORTED, "nmpc_probe: %d waves need more than 2^31 - 1 workgroups", n_waves);
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    DevBuf bin, bout; // freed on every path below
    const T* din = nullptr;
    T* dout = nullptr;
    bool out_host = false;
    const size_t n_in = (size_t)n_waves * 4 * 64, n_out = (size_t)n_waves * 6 * 64;
    if (int rc = stage_in(h, bin, in, n_in, &din)) return rc;
    if (int rc = stage_out(h, bout, out, n_out, &dout, &out_host)) return rc;
    hipLaunchKernelGGL(probe_kernel_of<T>(op, std::make_integer_sequence<int, NMPC_PROBE_N_OPS>{}), dim3((unsigned)blocks), dim3(block_threads),
                       0, h->stream, din, dout, n_waves);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && out_host) e = hipMemcpyAsync(out, dout, n_out * sizeof(T), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream); // (synchronous: the staging buffers go out of scope)
    if (e != hipSuccess) return fail(NMPC_ERR_HIP, "nmpc_probe: %s", hipGetErrorString(e));
    return 0;
}

extern "C" {

const char* nmpc_last_error(void) { return g_err.c_str(); }

int nmpc_default_config(nmpc_config* c)
{
    if (!c) return fail(NMPC_ERR_INVALID_ARGUMENT, "null config");
    std::memset(c, 0, sizeof *c);
    c->abi_version = NMPC_ABI_VERSION;
    c->device_id = 0;
    // config/mpc_fast.yaml == config/mpc_default.yaml for everything the solver consumes
    c->N_hor = 20;
    c->Nother = 10;
    c->Nstcobs = 10;
    c->Ndynobs = 15;
    c->ts = 0.2;
    c->lin_vel_min = -0.5;
    c->lin_vel_max = 1.5;
    c->ang_vel_max = 0.5;
    c->lin_acc_min = -1.0;
    c->lin_acc_max = 1.0;
    c->ang_acc_max = 3.0;
    c->vehicle_width = 0.5;
    c->vehicle_margin = 0.2;
    c->social_margin = 0.2;
    c->tolerance = 1e-4;
    c->initial_tolerance = 1e-4;
    c->delta_tolerance = 1e-4;
    c->max_outer_iterations = 10;
    c->max_inner_iterations = 500;
    c->lbfgs_memory = 10;
    c->max_active_dynobs = 0;
    c->initial_penalty = 10.0;
    c->penalty_update_factor = 5.0;
    c->inner_tolerance_update_factor = 0.1;
    c->sufficient_decrease_coeff = 0.1;
    c->lip_eps_f64 = 1e-6;
    c->lip_delta_f64 = 1e-12;
    c->lip_eps_f32 = 1e-4;
    c->lip_delta_f32 = 1e-4;
    c->cbfgs_alpha = 1.0;
    c->cbfgs_epsilon = 1e-8;
    c->sy_epsilon = 1e-10;
    c->latency_waves = 0;
    c->akkt_form = 0;
    c->max_solver_time_us = 0.0;
    c->coop_waves = 0;
    c->axis_aligned = 0;
    c->reg_table = 0;
    c->staged = 0;
    c->polish = 0;
    c->polish_max_outer_iterations = 4;
    c->polish_max_inner_iterations = 150; // (round 4: 300 -> 150, see nmpc_hip.h)
    c->staged_evals = 0;
    c->polish_tolerance = 1e-6;
    c->polish_delta_tolerance = 1e-5;
    c->max_evaluations = 0;
    c->tail_latency = 0;
    c->batch_invariant = 0;
    return 0;
}

int nmpc_layout(const nmpc_config* cfg, nmpc_layout_info* out)
{
    if (!cfg || !out) return fail(NMPC_ERR_INVALID_ARGUMENT, "null argument");
    if (cfg->abi_version != NMPC_ABI_VERSION)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "abi_version %d != %d", cfg->abi_version, NMPC_ABI_VERSION);
    if (cfg->N_hor < 1 || cfg->N_hor > NMPC_MAX_HORIZON || cfg->Nother < 1 || cfg->Nstcobs < 0 || cfg->Ndynobs < 0 ||
        cfg->max_active_dynobs < 0)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "bad dimensions");
    const Layout a = make_layout(*cfg, sizeof(float)), b = make_layout(*cfg, sizeof(double));
    std::memset(out, 0, sizeof *out);
    out->np = a.np;
    out->lds_bytes_f32 = (int32_t)((size_t)a.lds_total * sizeof(float));
    out->lds_bytes_f64 = (int32_t)((size_t)b.lds_total * sizeof(double));
    out->reg_slots_f32 = a.rs;
    out->global_table_f32 = a.glb ? 1 : 0;
    out->global_table_f64 = b.glb ? 1 : 0;
    out->ws_elems_f32 = a.ws_stride;
    out->ws_elems_f64 = b.ws_stride;
    out->table_entries_f32 = a.table_entries;
    out->table_entries_f64 = b.table_entries;
    out->dyn_cap = a.dyn_cap;
    return 0;
}

int nmpc_create(const nmpc_config* cfg, nmpc_handle* out)
{
    if (!cfg || !out) return fail(NMPC_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (cfg->abi_version != NMPC_ABI_VERSION)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "abi_version %d != %d", cfg->abi_version, NMPC_ABI_VERSION);
    if (cfg->N_hor < 1 || cfg->N_hor > NMPC_MAX_HORIZON)
        return fail(NMPC_ERR_UNSUPPORTED, "N_hor = %d outside [1, %d] (one horizon step per lane group)", cfg->N_hor,
                    NMPC_MAX_HORIZON);
    if (cfg->Nother < 1 || cfg->Nstcobs < 0 || cfg->Ndynobs < 0)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "bad dimensions Nother=%d Nstcobs=%d Ndynobs=%d", cfg->Nother,
                    cfg->Nstcobs, cfg->Ndynobs);
    if (cfg->max_active_dynobs < 0)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "max_active_dynobs = %d < 0", cfg->max_active_dynobs);
    if (cfg->lbfgs_memory < 1 || cfg->lbfgs_memory > NMPC_LBFGS_MAX_MEMORY)
        return fail(NMPC_ERR_UNSUPPORTED, "lbfgs_memory = %d outside [1, %d]", cfg->lbfgs_memory,
                    NMPC_LBFGS_MAX_MEMORY);
    if (cfg->latency_waves < -1)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "latency_waves = %d < -1", cfg->latency_waves);
    if (cfg->coop_waves < 0 || cfg->coop_waves > kSpecWaves)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "coop_waves = %d outside [0, %d]", cfg->coop_waves, kSpecWaves);
    if (cfg->akkt_form != 0 && cfg->akkt_form != 1)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "akkt_form = %d (0 = OpEn source form, 1 = documented form)", cfg->akkt_form);
    if (!(cfg->max_solver_time_us >= 0))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "max_solver_time_us < 0");
    if (cfg->max_evaluations < 0) return fail(NMPC_ERR_INVALID_ARGUMENT, "max_evaluations = %d < 0", cfg->max_evaluations);
    if (cfg->tail_latency < -1) return fail(NMPC_ERR_INVALID_ARGUMENT, "tail_latency = %d < -1", cfg->tail_latency);
    if (cfg->batch_invariant < -1 || cfg->batch_invariant > 1)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "batch_invariant = %d (0 automatic, 1 always, -1 never)", cfg->batch_invariant);
    if (cfg->staged_evals < -1) return fail(NMPC_ERR_INVALID_ARGUMENT, "staged_evals = %d < -1", cfg->staged_evals);
    if (cfg->axis_aligned < -1 || cfg->axis_aligned > 1)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "axis_aligned = %d (0 automatic, 1 promised, -1 never)", cfg->axis_aligned);
    if (cfg->staged < -1) return fail(NMPC_ERR_INVALID_ARGUMENT, "staged = %d < -1", cfg->staged);
    if (cfg->polish < 0 || cfg->polish > 2) return fail(NMPC_ERR_INVALID_ARGUMENT, "polish = %d (0, 1 or 2)", cfg->polish);
    if (cfg->polish && (!(cfg->polish_tolerance > 0) || !(cfg->polish_delta_tolerance > 0) ||
                        cfg->polish_max_outer_iterations < 1 || cfg->polish_max_inner_iterations < 1))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "bad polish tolerances / iteration caps");
    if (!(cfg->ts > 0) || cfg->max_outer_iterations < 1 || cfg->max_inner_iterations < 1 ||
        !(cfg->initial_penalty > 0))
        return fail(NMPC_ERR_INVALID_ARGUMENT, "bad ts / iteration caps / initial penalty");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(NMPC_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    }
    if (cfg->device_id < 0 || cfg->device_id >= ndev)
        return fail(NMPC_ERR_INVALID_ARGUMENT, "device_id %d not in [0, %d)", cfg->device_id, ndev);
    nmpc_handle_s* h = new (std::nothrow) nmpc_handle_s();
    if (!h) return fail(NMPC_ERR_OUT_OF_MEMORY, "host allocation failed");
    h->cfg = *cfg;
    h->lays = make_layouts(*cfg);
    if ((size_t)h->lays.lay64.lds_total * sizeof(double) > kLdsLimit || (size_t)h->lays.lay32.lds_total * sizeof(float) > kLdsLimit) {
        const size_t need = (size_t)h->lays.lay64.lds_total * sizeof(double);
        delete h;
        return fail(NMPC_ERR_UNSUPPORTED,
                    "polygon / robot / path tables alone need %zu B of LDS per instance (> 160 KiB)", need);
    }
    hipError_t e = hipSetDevice(cfg->device_id);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&h->ev0);
    if (e == hipSuccess) e = hipEventCreate(&h->ev1);
    if (e != hipSuccess) {
        nmpc_destroy(h);
        return fail(NMPC_ERR_HIP, "handle setup: %s", hipGetErrorString(e));
    }
    h->stream = h->own_stream;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cfg->device_id) == hipSuccess)
            h->n_simd = prop.multiProcessorCount * 4; // 4 SIMDs per CU
    }
    int rc = h->dflag.reserve(4 * sizeof(int));
    if (rc == 0 && hipMemset(h->dflag.p, 0, 4 * sizeof(int)) != hipSuccess) rc = fail(NMPC_ERR_HIP, "hipMemset failed");
    if (rc == 0) rc = h->dhist.reserve((2 * kRankBuckets + 4) * sizeof(int)); // (bucket counters of the resumable solve, kept zeroed; + the tail hand-off's three)
    if (rc == 0 && hipMemset(h->dhist.p, 0, (2 * kRankBuckets + 4) * sizeof(int)) != hipSuccess) rc = fail(NMPC_ERR_HIP, "hipMemset failed");
    if (rc == 0) rc = set_lds_limit<float>(h);
    if (rc == 0) rc = set_lds_limit<double>(h);
    if (rc) {
        nmpc_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

int nmpc_destroy(nmpc_handle h)
{
    if (!h) return 0;
    (void)hipSetDevice(h->cfg.device_id);
    if (h->own_stream) (void)hipStreamSynchronize(h->own_stream);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h; // (the device buffers: DevBuf's destructor)
    return 0;
}

int nmpc_param_len(nmpc_handle h)
{
    if (!h) return fail(NMPC_ERR_INVALID_ARGUMENT, "null handle");
    return h->lays.lay32.np;
}

int nmpc_set_stream(nmpc_handle h, void* s)
{
    if (!h) return fail(NMPC_ERR_INVALID_ARGUMENT, "null handle");
    h->stream = static_cast<hipStream_t>(s); // NULL is a stream too: the HIP null stream (torch's default stream)
    return 0;
}

int nmpc_set_pointer_mode(nmpc_handle h, int32_t mode)
{
    if (!h) return fail(NMPC_ERR_INVALID_ARGUMENT, "null handle");
    if (mode < NMPC_PTR_DETECT || mode > NMPC_PTR_DEVICE) return fail(NMPC_ERR_INVALID_ARGUMENT, "pointer mode %d", mode);
    h->ptr_mode = mode;
    return 0;
}

int nmpc_set_dispatch_order(nmpc_handle h, const int32_t* order, int32_t B)
{
    if (!h) return fail(NMPC_ERR_INVALID_ARGUMENT, "null handle");
    if (!order || B <= 0) {
        h->order_B = 0;
        return 0;
    }
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (int rc = h->dorder.reserve((size_t)B * sizeof(int32_t))) return rc;
    if (is_device_ptr(order)) {
        // (a device-resident order is taken as it is: it must be a permutation of 0..B-1)
        HIP_TRY(hipMemcpyAsync(h->dorder.p, order, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
    } else {
        std::vector<unsigned char> seen((size_t)B, 0);
        for (int32_t i = 0; i < B; ++i) {
            const int32_t v = order[i];
            if (v < 0 || v >= B || seen[(size_t)v])
                return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_set_dispatch_order: order[%d] = %d: not a permutation of 0..%d", i, v, B - 1);
            seen[(size_t)v] = 1;
        }
        HIP_TRY(hipMemcpyAsync(h->dorder.p, order, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream)); // (the host array may be released by the caller on return)
    }
    h->order_B = B;
    return 0;
}

int nmpc_use_own_stream(nmpc_handle h)
{
    if (!h) return fail(NMPC_ERR_INVALID_ARGUMENT, "null handle");
    h->stream = h->own_stream;
    return 0;
}

int nmpc_solve_batch_f32(nmpc_handle h, const float* P, int32_t B, float* U, float* cost, int32_t* status,
                         int32_t* iters, const float* u0, float* y, int32_t y_is_input, const float* c0, float* info,
                         int32_t sync)
{
    return solve_batch<float>(h, P, B, U, cost, status, iters, u0, y, y_is_input, c0, info, sync);
}

int nmpc_solve_batch_f64(nmpc_handle h, const double* P, int32_t B, double* U, double* cost, int32_t* status,
                         int32_t* iters, const double* u0, double* y, int32_t y_is_input, const double* c0,
                         double* info, int32_t sync)
{
    return solve_batch<double>(h, P, B, U, cost, status, iters, u0, y, y_is_input, c0, info, sync);
}

int nmpc_solve_trace_f64(nmpc_handle h, const double* p, const double* u0, const double* y0, double c0, double* U, double* y,
                         int32_t* status, int32_t* iters, double* info, double* trace, int32_t max_records,
                         int32_t* n_records)
{
    return solve_trace(h, p, u0, y0, c0, U, y, status, iters, info, trace, max_records, n_records);
}

int nmpc_eval_batch_f32(nmpc_handle h, const float* P, const float* U, const float* Y, const float* C, int32_t B,
                        float* psi, float* grad, float* f2sq)
{
    return eval_batch<float>(h, P, U, Y, C, B, psi, grad, f2sq);
}

int nmpc_eval_batch_f64(nmpc_handle h, const double* P, const double* U, const double* Y, const double* C, int32_t B,
                        double* psi, double* grad, double* f2sq)
{
    return eval_batch<double>(h, P, U, Y, C, B, psi, grad, f2sq);
}

int nmpc_assemble_params_f32(nmpc_handle h, const nmpc_assemble_args* args, int32_t B, float* P)
{
    return assemble_params<float>(h, args, B, P);
}

int nmpc_assemble_params_f64(nmpc_handle h, const nmpc_assemble_args* args, int32_t B, double* P)
{
    return assemble_params<double>(h, args, B, P);
}

int nmpc_hypotheses_to_ellipses_f32(nmpc_handle h, const float* hypos, int32_t P, const float* cur, int32_t H,
                                    double human_size, double eps, double enlarge, double extra_margin, int32_t B,
                                    float* dyn, int32_t* n_obs)
{
    return hypotheses_to_ellipses<float>(h, hypos, P, cur, H, human_size, eps, enlarge, extra_margin, B, dyn, n_obs);
}

int nmpc_hypotheses_to_ellipses_f64(nmpc_handle h, const double* hypos, int32_t P, const double* cur, int32_t H,
                                    double human_size, double eps, double enlarge, double extra_margin, int32_t B,
                                    double* dyn, int32_t* n_obs)
{
    return hypotheses_to_ellipses<double>(h, hypos, P, cur, H, human_size, eps, enlarge, extra_margin, B, dyn, n_obs);
}

int nmpc_hypotheses_to_ellipses_counts_f32(nmpc_handle h, const float* hypos, int32_t P, const float* cur, int32_t H,
                                           double human_size, double eps, double enlarge, double extra_margin, int32_t B,
                                           float* dyn, int32_t* n_obs, int32_t* counts)
{
    return hypotheses_to_ellipses<float>(h, hypos, P, cur, H, human_size, eps, enlarge, extra_margin, B, dyn, n_obs, counts);
}

int nmpc_hypotheses_to_ellipses_counts_f64(nmpc_handle h, const double* hypos, int32_t P, const double* cur, int32_t H,
                                           double human_size, double eps, double enlarge, double extra_margin, int32_t B,
                                           double* dyn, int32_t* n_obs, int32_t* counts)
{
    return hypotheses_to_ellipses<double>(h, hypos, P, cur, H, human_size, eps, enlarge, extra_margin, B, dyn, n_obs, counts);
}

int nmpc_set_map(nmpc_handle h, const uint8_t* occupied, const uint8_t* edge, int32_t height, int32_t width)
{
    return set_map(h, occupied, edge, height, width);
}

int nmpc_snap_hypotheses_f32(nmpc_handle h, const float* raw, const nmpc_snap_args* a, int32_t B, float* hypos)
{
    return snap_hypotheses<float>(h, raw, a, B, hypos);
}

int nmpc_snap_hypotheses_f64(nmpc_handle h, const double* raw, const nmpc_snap_args* a, int32_t B, double* hypos)
{
    return snap_hypotheses<double>(h, raw, a, B, hypos);
}

int nmpc_loop_pre_f32(nmpc_handle h, const nmpc_loop_args* a) { return loop_step<float>(h, a, false); }
int nmpc_loop_pre_f64(nmpc_handle h, const nmpc_loop_args* a) { return loop_step<double>(h, a, false); }
int nmpc_loop_post_f32(nmpc_handle h, const nmpc_loop_args* a) { return loop_step<float>(h, a, true); }
int nmpc_loop_post_f64(nmpc_handle h, const nmpc_loop_args* a) { return loop_step<double>(h, a, true); }

int nmpc_kf_predict_f32(nmpc_handle h, const nmpc_kf_args* a) { return kf_predict<float>(h, a); }
int nmpc_kf_predict_f64(nmpc_handle h, const nmpc_kf_args* a) { return kf_predict<double>(h, a); }

int nmpc_fleet_exchange_f32(nmpc_handle h, const nmpc_fleet_args* a) { return fleet_step<float>(h, a, false); }
int nmpc_fleet_exchange_f64(nmpc_handle h, const nmpc_fleet_args* a) { return fleet_step<double>(h, a, false); }
int nmpc_fleet_post_f32(nmpc_handle h, const nmpc_fleet_args* a) { return fleet_step<float>(h, a, true); }
int nmpc_fleet_post_f64(nmpc_handle h, const nmpc_fleet_args* a) { return fleet_step<double>(h, a, true); }
int nmpc_dwa_step_f32(nmpc_handle h, const nmpc_dwa_args* a) { return dwa_step<float>(h, a); }
int nmpc_dwa_step_f64(nmpc_handle h, const nmpc_dwa_args* a) { return dwa_step<double>(h, a); }
int nmpc_dwa_step_lists_f32(nmpc_handle h, const nmpc_dwa_lists_args* a) { return dwa_step<float, true, nmpc_dwa_lists_args>(h, a); }
int nmpc_dwa_step_lists_f64(nmpc_handle h, const nmpc_dwa_lists_args* a) { return dwa_step<double, true, nmpc_dwa_lists_args>(h, a); }
int nmpc_mmp_input_f32(nmpc_handle h, const nmpc_mmp_args* a) { return mmp_input<float>(h, a); }
int nmpc_mmp_input_f64(nmpc_handle h, const nmpc_mmp_args* a) { return mmp_input<double>(h, a); }
int nmpc_mmp_stem_f32(nmpc_handle h, const nmpc_mmp_stem_args* a) { return mmp_stem<float>(h, a); }
int nmpc_mmp_stem_f64(nmpc_handle h, const nmpc_mmp_stem_args* a) { return mmp_stem<double>(h, a); }
int nmpc_mmp_stem_io_f32(nmpc_handle h, const nmpc_mmp_stem_args* a, int32_t out_f16) { return mmp_stem<float, true>(h, a, out_f16); }
int nmpc_mmp_stem_io_f64(nmpc_handle h, const nmpc_mmp_stem_args* a, int32_t out_f16) { return mmp_stem<double, true>(h, a, out_f16); }
int nmpc_mmp_block_f32(nmpc_handle h, const nmpc_mmp_block_args* a) { return mmp_block(h, a); }
int nmpc_mmp_block2_f32(nmpc_handle h, const nmpc_mmp_block2_args* a) { return mmp_strided<MmpLayer2>(h, a); }
static int mmp_block_f16(nmpc_handle_s* h, const nmpc_mmp_block_f16_args* a, int32_t x_f16, int32_t out_f16, bool io)
{
    MmpLayer1F16::Args g;
    if (a) static_cast<nmpc_mmp_block_f16_args&>(g) = *a, g.stride = 1;
    return io ? mmp_strided<MmpLayer1F16, true>(h, a ? &g : nullptr, x_f16, out_f16) : mmp_strided<MmpLayer1F16>(h, a ? &g : nullptr);
}
int nmpc_mmp_block_f16(nmpc_handle h, const nmpc_mmp_block_f16_args* a) { return mmp_block_f16(h, a, 0, 0, false); }
int nmpc_mmp_block_f16_io(nmpc_handle h, const nmpc_mmp_block_f16_args* a, int32_t x_f16, int32_t out_f16) { return mmp_block_f16(h, a, x_f16, out_f16, true); }
int nmpc_mmp_block2_f16(nmpc_handle h, const nmpc_mmp_block2_f16_args* a) { return mmp_strided<MmpLayer2F16>(h, a); }
int nmpc_mmp_block2_f16_io(nmpc_handle h, const nmpc_mmp_block2_f16_args* a, int32_t x_f16, int32_t out_f16) { return mmp_strided<MmpLayer2F16, true>(h, a, x_f16, out_f16); }
int nmpc_mmp_block3_f32(nmpc_handle h, const nmpc_mmp_block3_args* a) { return mmp_strided<MmpLayer3>(h, a); }
int nmpc_mmp_block3_f16(nmpc_handle h, const nmpc_mmp_block3_f16_args* a) { return mmp_strided<MmpLayer3F16>(h, a); }
int nmpc_mmp_block3_f16_io(nmpc_handle h, const nmpc_mmp_block3_f16_args* a, int32_t x_f16, int32_t out_f16) { return mmp_strided<MmpLayer3F16, true>(h, a, x_f16, out_f16); }
int nmpc_mmp_block4_f32(nmpc_handle h, const nmpc_mmp_block4_args* a) { return mmp_strided<MmpLayer4>(h, a); }
int nmpc_mmp_block4_f16(nmpc_handle h, const nmpc_mmp_block4_f16_args* a) { return mmp_strided<MmpLayer4F16>(h, a); }
int nmpc_mmp_block4_f16_io(nmpc_handle h, const nmpc_mmp_block4_f16_args* a, int32_t x_f16, int32_t out_f16) { return mmp_strided<MmpLayer4F16, true>(h, a, x_f16, out_f16); }
int nmpc_mmp_head_f32(nmpc_handle h, const nmpc_mmp_head_args* a) { return mmp_head(h, a); }
int nmpc_mmp_stem_shape(int32_t Hm, int32_t Wm, int32_t* Hp, int32_t* Wp)
{
    if (Hm < 1 || Wm < 1 || !Hp || !Wp) return fail(NMPC_ERR_INVALID_ARGUMENT, "nmpc_mmp_stem_shape: map %d x %d or a NULL output", Hm, Wm);
    *Hp = nmpc::mmp_stem_out(Hm), *Wp = nmpc::mmp_stem_out(Wm);
    return 0;
}

int nmpc_last_kernel_ms(nmpc_handle h, float* ms)
{
    if (!h || !ms) return fail(NMPC_ERR_INVALID_ARGUMENT, "null argument");
    if (!h->timed) return fail(NMPC_ERR_INVALID_ARGUMENT, "no solve has been launched on this handle yet");
    HIP_TRY(hipEventSynchronize(h->ev1));
    HIP_TRY(hipEventElapsedTime(ms, h->ev0, h->ev1));
    return 0;
}

int nmpc_last_launch_info(nmpc_handle h, int32_t out[8])
{
    if (!h || !out) return fail(NMPC_ERR_INVALID_ARGUMENT, "null argument");
    std::memset(out, 0, 8 * sizeof(int32_t));
    out[0] = h->last_mode;
    out[1] = h->last_axis;
    out[2] = h->last_staged;
    out[3] = h->last_polish_selected;
    out[4] = h->last_tail;
    if (h->last_tail > 0) { // instances the tail launch took over inside an inner solve: KParams::dyn_ctr[3], capped at the slots
        int parked = 0;
        HIP_TRY(hipSetDevice(h->cfg.device_id));
        HIP_TRY(hipMemcpyAsync(&parked, static_cast<const int*>(h->dhist.p) + 2 * kRankBuckets + 3, sizeof(int),
                               hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        out[5] = std::min(parked, h->last_tail);
    }
    out[6] = h->last_order;
    return 0;
}

int nmpc_kernel_info(nmpc_handle h, int32_t* lds_bytes_f32, int32_t* lds_bytes_f64, int32_t* lanes_per_step,
                     int32_t* waves_per_cu_f32, int32_t* waves_per_cu_f64)
{
    if (!h) return fail(NMPC_ERR_INVALID_ARGUMENT, "null handle");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    const size_t l32 = (size_t)h->lays.lay32.lds_total * 4, l64 = (size_t)h->lays.lay64.lds_total * 8;
    if (lds_bytes_f32) *lds_bytes_f32 = (int32_t)l32;
    if (lds_bytes_f64) *lds_bytes_f64 = (int32_t)l64;
    if (lanes_per_step) *lanes_per_step = h->lays.lps;
    if (waves_per_cu_f32) {
        int nb = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &nb, reinterpret_cast<const void*>(solve_kernel_of<float>(single_variant(kThroughput, h->lays.lay32, h->lays.lps))), 64, l32));
        *waves_per_cu_f32 = nb;
    }
    if (waves_per_cu_f64) {
        int nb = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &nb, reinterpret_cast<const void*>(solve_kernel_of<double>(single_variant(kThroughput, h->lays.lay64, h->lays.lps))), 64, l64));
        *waves_per_cu_f64 = nb;
    }
    return 0;
}

int nmpc_probe_f32(nmpc_handle h, int32_t op, int32_t block_threads, int32_t n_waves, const float* in, float* out)
{
    return probe<float>(h, op, block_threads, n_waves, in, out);
}
int nmpc_probe_f64(nmpc_handle h, int32_t op, int32_t block_threads, int32_t n_waves, const double* in, double* out)
{
    return probe<double>(h, op, block_threads, n_waves, in, out);
}

int nmpc_selftest(nmpc_handle h)
{
    if (!h) return fail(NMPC_ERR_INVALID_ARGUMENT, "null handle");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    DevBuf buf; // freed on every path below
    if (int rc = buf.reserve(2 * sizeof(int))) return rc;
    int* d = static_cast<int*>(buf.p);
    int res[2] = {-1, -1};
    hipError_t e = hipMemsetAsync(d, 0, 2 * sizeof(int), h->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(selftest_kernel<float>, dim3(1), dim3(64), 0, h->stream, d);
        hipLaunchKernelGGL(selftest_kernel<double>, dim3(1), dim3(64), 0, h->stream, d + 1);
        e = hipMemcpyAsync(res, d, sizeof res, hipMemcpyDeviceToHost, h->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    buf.release();
    if (e != hipSuccess) return fail(NMPC_ERR_HIP, "selftest: %s", hipGetErrorString(e));
    if (res[0] || res[1]) {
        g_err = "wave primitive self-test failed: f32 mask " + std::to_string(res[0]) + ", f64 mask " +
                std::to_string(res[1]);
        return __builtin_popcount(res[0]) + __builtin_popcount(res[1]);
    }
    return 0;
}

} // extern "C"
