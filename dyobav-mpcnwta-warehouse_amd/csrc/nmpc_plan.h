// nmpc_plan.h -- which kernel runs a batch and how its launches are scheduled: the whole host-side decision as pure
// functions of plain data. No HIP header (compiles with g++ -std=c++17; tests/test_plan_cpu.py runs it without a device);
// nmpc_capi.hip maps the variant descriptions to kernels and executes the plans. The measurements behind the thresholds
// are told in HISTORY.md ("The solve plan's thresholds"); each constant below names its record.
#pragma once

#include <algorithm>
#include <cstddef>

#include "../../include/nmpc_hip.h"
#include "nmpc_sizes.h"

namespace nmpc_plan {

struct Layout {
    int np, off_rs, off_rv, off_c0, off_c, off_os, off_od, off_qstc, off_qdyn;
    int lds_alpha, lds_poly, lds_seg, lds_seginv, lds_fl0, lds_fl, lds_iflag, lds_hist, lds_rho, lds_total;
    int lds_xch, lds_total_spec; // latency mode: exchange area + the other wavefronts' parking areas behind lds_total
    int lds_park, lds_deepsc;
    int coop_lanes, lds_t0c; // cooperative kernels: lanes per plane of the exchange area; t = 0 rows of the compressed global table
    int lds_xch_coop, lds_total_coop; // cooperative mode: two shared parking areas, then the partial-sum exchange area
    int lds_left, lds_left_alpha;     // LDS table of the rows beyond the register-resident ones (cooperative register kernel)
    int dyn_cap;          // obstacle rows provisioned per instance
    int table_entries;    // entries of the obstacle table the kernels index in LDS / the workspace
    int rs;               // > 0: register-resident obstacle table with this many slots per lane (LDS keeps t = 0 only)
    bool glb;             // obstacle table streamed from a global workspace instead of LDS
    long long ws_stride;  // workspace elements per instance (glb only)
};

#ifndef NMPC_MID_SLOTS
#define NMPC_MID_SLOTS 1 // offer the 6-slot register-table kernels (13..18 provisioned rows)
#endif
// second launch-bound argument of the kernels = minimum waves per SIMD; it caps the register allocation (512 / waves)
#ifndef NMPC_SPEC_WPE_F32
#define NMPC_SPEC_WPE_F32 3 // wavefronts per SIMD the fp32 latency kernel is compiled for (caps VGPRs at 168)
#endif
#ifndef NMPC_WPE_F32
#define NMPC_WPE_F32 3 // throughput kernel, table in LDS / global memory (133 VGPRs; one spill short of fitting 128)
#endif
#ifndef NMPC_WPE_F64
#define NMPC_WPE_F64 2
#endif
constexpr int kWpeReg = 3, kWpeRegLarge = 2; // fp32 register-table kernels: 4- / 6-slot (168 registers), 14-slot (256)
constexpr int kSimdsPerCu = 4;
constexpr int kSpecWaves = 4; // wavefronts per instance in latency mode (nmpc_spec.h): automatic choice for batches up to one
                              // workgroup per SIMD; wavefronts of the cooperative kernels
constexpr int kSpecWavesWide = 6; // ... for batches of at most one workgroup per CU (the master + five workers: LIP + 5 candidates a round)
constexpr int kSpecWavesMax = 8;  // most that nmpc_config.latency_waves may ask for
constexpr size_t kLdsLimit = 160 * 1024; // bytes of LDS one workgroup may use on gfx950
constexpr size_t kLdsOptIn = 48 * 1024;  // above this a kernel needs hipFuncAttributeMaxDynamicSharedMemorySize

inline int round4(int x) { return (x + 3) & ~3; }
// exchange area of a latency-kernel workgroup of W wavefronts (nmpc_spec.h: xch + command area)
inline int spec_xch_elems(int W) { return round4(W * (2 * 64 + 4) + 2 * 64 * W + 8); } // (+ 8 command scalars: c, 1/max(c,1), flags, exit, gamma, 1/gamma)

constexpr int kRegSlotsSmall = 4, kRegSlotsMid = 6, kRegSlotsLarge = 14; // compiled register-table sizes (rows = 3 x slots)
// (Mid, round 5: 13..18 provisioned rows -- the reference's shipped yaml provisions 15 -- at the 168-register budget of the 4-slot
//  kernels, three wavefronts per SIMD / four per instance in latency mode, instead of the 256-register 14-slot kernels)
constexpr int kRegSlotsCoop = 12; // one lane per step: 8 cooperating wavefronts (2 per SIMD, 256 registers each) x 12 slots in
                                  // registers (96 rows; 144 with helper lanes, below); the rows beyond those in LDS
constexpr int kCoopRegWaves = 8;
// Horizons of 33..42 steps leave 22..31 lanes of every wavefront without a step: there the kernel is compiled with helper
// lanes (nmpc_device.h, HLP) that take a third row in each pass of two slots -- 8 x 18 = 144 rows in registers.
inline bool coop_helper_lanes(int N) { return N >= 33 && N <= 42; }
inline int coop_reg_rows(int N) { return kCoopRegWaves * (coop_helper_lanes(N) ? 3 * (kRegSlotsCoop / 2) : kRegSlotsCoop); }

// coop_rs: layout of the cooperative register-table kernel (fp32, one lane per step): 4 x kRegSlotsCoop rows in the
// registers of the four wavefronts, the t = 0 snapshot of all rows and the full table of the remaining rows in LDS --
// nothing is streamed from global memory. L.rs = 0 on return if the configuration does not qualify.
// reg64: layout of the fp64 register-table kernel (one wavefront per SIMD, 512 registers: 14 slots of 9 doubles = 252 of
// them) -- offered for 13..42 provisioned rows and N <= 21; used for large batches where the 72-byte entries of the fp64
// LDS table leave room for fewer than four instances per CU (use64r_auto below).
inline Layout make_layout(const nmpc_config& c, size_t elem_size, bool coop_rs = false, bool reg64 = false)
{
    Layout L;
    const int N = c.N_hor;
    L.off_rs = 18;
    L.off_rv = L.off_rs + 3 * N;
    L.off_c0 = L.off_rv + N;
    L.off_c = L.off_c0 + 3 * c.Nother;
    L.off_os = L.off_c + 3 * N * c.Nother;
    L.off_od = L.off_os + 12 * c.Nstcobs;
    L.off_qstc = L.off_od + 6 * (N + 1) * c.Ndynobs;
    L.off_qdyn = L.off_qstc + N;
    L.np = L.off_qdyn + N;
    const int cap = c.max_active_dynobs > 0 && c.max_active_dynobs < c.Ndynobs ? c.max_active_dynobs : c.Ndynobs;
    // fp32, three lanes per horizon step: the table entries of t >= 1 live in the registers of the one lane that reads
    // them (nmpc_device.h, RS > 0) when the provisioned rows fit 3 x 4 or 3 x 14
    L.rs = 0;
    if (elem_size == 4 && c.reg_table >= 0 && N <= 21 && 64 / N >= 3 && cap > 0) {
        if (cap <= 3 * kRegSlotsSmall) L.rs = kRegSlotsSmall;
        else if (cap <= 3 * kRegSlotsMid && NMPC_MID_SLOTS) L.rs = kRegSlotsMid;
        else if (cap <= 3 * kRegSlotsLarge) L.rs = kRegSlotsLarge;
    }
    if (elem_size == 8 && reg64 && c.reg_table >= 0 && N <= 21 && 64 / N >= 3 && cap > 3 * kRegSlotsSmall && cap <= 3 * kRegSlotsLarge)
        L.rs = kRegSlotsLarge;
    int left_ne = 0; // entries of the LDS table of the rows beyond the register-resident ones (cooperative register kernel)
    if (coop_rs) {
        L.rs = 0;
        if (elem_size == 4 && c.reg_table >= 0 && 64 / N == 1 && cap > 0) {
            L.rs = kRegSlotsCoop;
            left_ne = std::max(0, cap - coop_reg_rows(N)) * (N + 1);
        }
    }
    // table entries provisioned in LDS / the workspace. Register table: the t = 0 rows + the dummy row(s) -- three lanes per
    // step: every row a pass can address (3 x slots), so that the passes read at fixed offsets without a clamp
    int ne = L.rs ? std::max(cap + 1, coop_rs ? 0 : 3 * L.rs) : cap * (N + 1);
    // three lanes per step, register table: the table of groups of rows with identical t = 0 snapshots (nmpc_device.h,
    // load()) takes the place of the cooperative kernel's left-over table
    if (L.rs && !coop_rs) left_ne = 3 * L.rs;
    L.dyn_cap = cap;
    L.glb = false;
    L.ws_stride = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
    L.lds_alpha = L.glb ? 0 : nmpc::kEllStride * ne;
    L.lds_left = L.lds_alpha + (L.glb ? 0 : round4(ne));
    L.lds_left_alpha = L.lds_left + nmpc::kEllStride * left_ne;
    L.lds_poly = L.lds_left_alpha + round4(left_ne);
    L.lds_seg = L.lds_poly + 12 * (c.Nstcobs + 3); // (+3: dummy polygons behind the stored ones, nmpc_device.h load())
    // path segments: N real ones + far-away dummies up to 2 N + 4, so that every lane can run the same number of loop trips
    // over `first segment + 3 j` without a bound (nmpc_device.h, eval(): the segment loop)
    const int nseg = nmpc::seg_table_len(N);
    L.lds_seginv = L.lds_seg + 4 * nseg;
    L.lds_fl0 = L.lds_seginv + round4(nseg);
    L.lds_fl = L.lds_fl0 + round4(c.Nother);          // int list: robots with a non-zero t=0 position
    L.lds_iflag = L.lds_fl + round4(c.Nother);         // int list: robots with a non-zero predicted position
    L.lds_hist = L.lds_iflag + round4(c.Ndynobs);  // int flags / compaction map (an int fits in a T)
    L.lds_rho = L.lds_hist + 4 * nmpc::kMem * nmpc::lbfgs_slot_stride(N); // L-BFGS ring: kMem slots x (N | 1) x (s_v, s_w, y_v, y_w)
    L.lds_park = L.lds_rho + round4(2 * nmpc::kMem);   // rho[kMem], alpha[kMem]; then the parking area(s) (16-B aligned)
    const int park_one = nmpc::kParkQuads * 4 * 64;    // elements per wavefront
    L.lds_deepsc = L.lds_park + park_one;              // scalar block of a deep park (tail hand-off), throughput kernels only
    L.lds_total = L.lds_deepsc + nmpc::kDeepScalars;
    // latency kernel: the exchange area of W wavefronts (nmpc_spec.h) in place of the parking area (its solver vectors stay
    // in registers): W result rows of 64 x 2 gradient entries + psi (padded to 132), the master's command area of
    // 2 x 64 x W + 4 scalars
    L.lds_xch = L.lds_park;
    L.lds_total_spec = L.lds_xch + spec_xch_elems(kSpecWavesMax);
    const int cw = coop_rs ? kCoopRegWaves : kSpecWaves;
    L.lds_xch_coop = L.lds_park + 2 * park_one; // cooperative kernels: two shared parking areas, used alternately
    // exchange area: 2 buffers x cw wavefronts x 2 planes x coop_lanes Quads. Global-table kernels with one lane per step keep
    // only the lanes that carry a step (nmpc_device.h) and put the t = 0 rows of the compressed table behind it
    L.coop_lanes = (L.glb && 64 / N == 1) ? std::min(64, round4(N)) : 64;
    L.lds_t0c = L.lds_xch_coop + 2 * cw * 2 * 4 * L.coop_lanes;
    L.lds_total_coop = L.lds_t0c + (L.glb ? round4((nmpc::kEllStride + 1) * cap) : 0);
    if (coop_rs) { // no global fallback for this variant: it either fits LDS or is not offered
        if ((size_t)L.lds_total_coop * elem_size > kLdsLimit) L.rs = 0;
        break;
    }
    if (L.glb || (size_t)L.lds_total * elem_size <= kLdsLimit) break;
    L.glb = true; // second attempt: everything but the ellipse table in LDS
    L.rs = 0;     // (the GLB kernels index the full [row][t] table: the register-table layout does not apply)
    left_ne = 0;
    ne = cap * (N + 1);
    // (room for the general table, 9 values per entry, and for the compressed one: 5 per entry + the expanded t = 0 rows)
    L.ws_stride = (long long)(nmpc::kEllStride + 1) * ne; // (the compressed table -- 5 values per entry -- uses a prefix of it)
    }
    L.table_entries = ne;
    return L;
}

// ---- what a handle fixes at creation ---------------------------------------------------------------------------------
struct Layouts {
    Layout lay32, lay64;
    Layout lay32c; // cooperative register-table kernel (fp32, one lane per step); rs = 0 if not available
    Layout lay64r; // fp64 register-table kernel (three lanes per step, one wavefront per SIMD); rs = 0 if not available
    bool use64r_auto; // ... chosen automatically for large batches (the LDS table allows < 4 instances per CU)
    int lps;          // lanes per horizon step: 64 / N, capped at 3
    const Layout& main(size_t elem) const { return elem == 4 ? lay32 : lay64; }
};
inline Layouts make_layouts(const nmpc_config& c)
{
    Layouts s = {make_layout(c, sizeof(float)), make_layout(c, sizeof(double)), make_layout(c, sizeof(float), true),
                 make_layout(c, sizeof(double), false, true), false, std::max(1, std::min(3, 64 / c.N_hor))};
    s.use64r_auto = s.lay64r.rs > 0 && !s.lay64.glb &&
                    std::min<size_t>(4 * NMPC_WPE_F64, kLdsLimit / ((size_t)s.lay64.lds_total * sizeof(double))) < 4;
    return s;
}

// ---- kernel variants -----------------------------------------------------------------------------------------------
enum Family : int { kThroughput, kLatencyFlat, kLatencyTail, kCoop, kCoopOnChip, kEval, kEvalCoop, kEvalCoopOnChip };
// One compiled kernel, or a PAIR of them (since round 4 every register-table kernel, and the cooperative kernels of the
// global table): member 1 = the axis-aligned path (global table: the compressed table) alone, member 2 = the general path
// alone, launched one behind the other; every workgroup of the member that the launch does not take returns at once
// (KParams::axis_mode). One kernel with both paths inlined reported the resources of the worse path and had grown to
// 125 KB of code, against the 128 KB reach of s_cbranch.
struct Variant {
    Family family;
    int lps;   // lanes per horizon step the kernel is compiled for
    bool glb;  // obstacle table streamed from the global workspace
    int rs;    // register-table slots per lane (0: table in LDS / global memory)
    bool hlp;  // on-chip cooperative kernels: helper lanes
    bool pair;
};
// Register tables exist for float with three lanes per step and the table not global (Layout::rs > 0 says exactly that), for
// double in the layout of the fp64 register-table kernel; those kernels are pairs.
inline Variant single_variant(Family f, const Layout& L, int lps) { return {f, lps, L.glb, L.rs, false, L.rs > 0 && lps == 3 && !L.glb}; }
// cooperative kernels. Global table: the pair (compressed table of axis-aligned ellipses / general table); LDS table: one kernel
inline Variant coop_variant(bool eval, const Layout& L, int lps) { return {eval ? kEvalCoop : kCoop, lps, L.glb, 0, false, L.glb}; }
// ... with the table on chip (fp32, one lane per step): eight wavefronts hold it in registers, nothing is streamed
inline Variant coop_onchip_variant(bool eval, int N) { return {eval ? kEvalCoopOnChip : kCoopOnChip, 1, false, kRegSlotsCoop, coop_helper_lanes(N), false}; }

enum LayoutUse : int { kLayMain, kLay32c, kLay64r };
// a variant with the layout and the launch shape it runs with
struct KernelChoice {
    Variant variant;
    LayoutUse use = kLayMain;
    const Layout* L = nullptr;
    int threads = 64;
    size_t lds_bytes = 0;
    bool uses_ws = false;  // the variant reads the global obstacle workspace
    bool has_axis = false; // a pair: the launches go by KParams::axis_mode
    bool coop = false;     // cooperative kernels: KParams::lds_xch = L->lds_xch_coop
};

// room in LDS for the exchange areas of the latency / the cooperative kernels? (else the family is not offered)
inline bool latency_fits(const Layout& L, size_t elem) { return (size_t)L.lds_total_spec * elem <= kLdsLimit; }
inline bool coop_fits(const Layout& L, size_t elem) { return (size_t)L.lds_total_coop * elem <= kLdsLimit; }

struct PlanStatic {        // of a handle and one element size
    const nmpc_config* cfg;
    const Layouts* lay;
    size_t elem;           // 4 / 8
    int n_simd;            // SIMDs of the device (4 per CU)
    bool spec_ok, coop_ok; // the latency / cooperative kernels' LDS fits
    const Layout& L() const { return lay->main(elem); }
};

inline KernelChoice choose_single(const PlanStatic& s, Family f)
{
    const Variant v = single_variant(f, s.L(), s.lay->lps);
    return {v, kLayMain, &s.L(), 64, (size_t)s.L().lds_total * s.elem, s.L().glb, v.pair, false};
}
// latency kernels over `waves` wavefronts: the exchange area by the W actually launched (about half of the 8-wavefront maximum at W = 4)
inline KernelChoice choose_latency(const PlanStatic& s, Family f, int waves)
{
    KernelChoice k = choose_single(s, f);
    k.threads = 64 * waves;
    k.lds_bytes = (size_t)(s.L().lds_xch + spec_xch_elems(waves)) * s.elem;
    return k;
}
// fp64 register-table kernel (its own layout; callers check lay64r.rs > 0)
inline KernelChoice choose_reg64(const PlanStatic& s, Family f)
{
    const Layout& R = s.lay->lay64r;
    return {single_variant(f, R, s.lay->lps), kLay64r, &R, 64, (size_t)R.lds_total * s.elem, false, true, false};
}
// cooperative kernels over `waves` wavefronts; the on-chip variant where four are asked for and its layout is available
inline KernelChoice choose_coop(const PlanStatic& s, bool eval, int waves)
{
    const Layout &L = s.L(), &C = s.lay->lay32c;
    if (s.elem == 4 && waves == kSpecWaves && C.rs > 0 && s.lay->lps == 1)
        return {coop_onchip_variant(eval, s.cfg->N_hor), kLay32c, &C, 64 * kCoopRegWaves, (size_t)C.lds_total_coop * s.elem, false, false, true};
    return {coop_variant(eval, L, s.lay->lps), kLayMain, &L, 64 * waves, (size_t)L.lds_total_coop * s.elem, L.glb, L.glb, true};
}

// ---- thresholds (batch sizes in units of S = n_simd, or in device fills of the planned kernel) --------------------------------
// wavefronts per instance, automatic (latency_waves = 0); cap = S in fp32, S / 2 in fp64 (2 wavefronts per SIMD against 3)
constexpr int kTwoWavesCaps = 4;                   // two wavefronts up to B = 4 cap, four up to cap, one beyond -- profiles/r04_exp_cfg1_waves.txt
constexpr int kLarge4Num = 3, kLarge4Den = 4;      // 14-slot kernels: four wavefronts up to 3/4 S, two up to S -- profiles/r06_exp_mid_batches.txt
constexpr double kFillsLarge = 0.7;                // 14-slot kernels: throughput plan, pilot and hand-off from 0.7 fills on -- profiles/r06_exp_mid_batches.txt
// six wavefronts up to one workgroup per CU (kSimdsPerCu B <= S) -- profiles/r04_exp_cfg1_batch_size_and_up_to_8_wavefronts.txt
constexpr int kSharedNum = 3, kSharedDen = 2;      // LDS-bound tables: W wavefronts share them if 1.5x more stay resident -- profiles/r02_cfg2_bench.json
constexpr int kReg64Caps = 2;                      // fp64 register table, automatic: from B = 2 cap (1 024) on -- round 3, HISTORY.md (no record under profiles/)
// resumable solve (pilot launch + ranking) and tail hand-off, in device fills -- profiles/r06_exp_mid_batches.txt
constexpr double kStageFills = 4, kTailFills = 4;        // fp64, LDS- and global-table kernels (rounds 3-4: profiles/r03_variants.txt)
constexpr double kStageFillsReg = 1, kTailFillsReg = 1;  // 4- / 6-slot fp32 register-table kernels
constexpr int kCoopStageFills = 4;                 // cooperative kernels with the table on chip -- round 4, HISTORY.md (no record under profiles/)
constexpr int kRankMinDiv = 2;                     // latency plan: some dispatch order from B > cap / 2 -- profiles/r03_variants.txt
// dispatch order from one evaluation instead of a pilot launch -- profiles/r06_exp_proxy_order.txt
constexpr int kProxyFullNum = 7, kProxyFullDen = 8; // 4- / 6-slot latency plan: up to 7/8 cap (beyond: the pilot)
constexpr int kProxyTwoWavesCaps = 4;              // ... and their two-wavefront plans, cap < B <= 4 cap
constexpr double kProxyFills = 8;                  // throughput plans below this many fills
constexpr double kProxyVnom = 2.0 / 3.0;           // the evaluation point: (v_nom, 0) with v_nom = 2/3 v_max
// tail hand-off -- profiles/r06_exp_mid_batches.txt, profiles/r06_ab_tail_handoff.jsonl
constexpr int kTailParkMin = 32;                   // automatic parking threshold: one tail workgroup per CU, at least 32
constexpr double kTailMinParks = 5;                // the hand-off needs a batch of at least this many parking thresholds
constexpr int kTailWideWpe = 2;                    // six wavefronts per parked instance while all are resident at two per SIMD, else four

// (development builds, -DNMPC_DEV_ENV: thresholds from the environment -- tools/exp_mid_batches.py,
//  tools/exp_cfg1_proxy_order.py; nmpc_capi.hip reads them. < 0: the constant.)
struct PlanTuning {
    double proxy_order = 1;              // NMPC_PROXY_ORDER: <= 0 switches the evaluation order off
    double proxy_fills = kProxyFills;    // NMPC_PROXY_FILLS
    double proxy_vnom = kProxyVnom;      // NMPC_PROXY_VNOM
    double stage_fills = -1;             // NMPC_STAGE_FILLS
    double tail_fills = -1;              // NMPC_TAIL_FILLS
    double tail_waves = -1;              // NMPC_TAIL_WAVES
    double tail_min_parks = kTailMinParks; // NMPC_TAIL_MINB
};

struct SolveRequest {
    int B;
    bool caller_order;  // nmpc_set_dispatch_order holds for this batch
    bool allow_staging; // the caller's status array may carry the in-progress marker
    bool has_status;
};

struct SolvePlan {
    KernelChoice main;
    int mode = 0;          // 0 throughput, 1 latency (speculative), 2 cooperative
    int resident = 0;      // workgroups of the one-wavefront / cooperative kernel resident on the device: one fill
    bool eval_order = false; // dispatch order from one evaluation at the nominal controls (then one launch, or launch + hand-off)
    int n_stage = 0, stage_cap[2] = {0, 0}, stage_key[2] = {0, 0}; // resumable solve: outer-iteration caps, ranking key behind each
    bool tail = false;     // the last throughput launch parks its drain phase, the tail member finishes it
    int park = 0;          // ... at most this many instances
    KernelChoice tail_kernel;
    int last_mode = 0, last_staged = 0, last_order = 0; // nmpc_last_launch_info
};

// wavefronts per instance of the latency kernel (1: the throughput kernel) where nmpc_config.latency_waves = 0
inline int auto_latency_waves(const PlanStatic& s, int B, int cap, int wpe_tp, int lds_per_cu)
{
    const Layout& L = s.L();
    const bool f32 = s.elem == 4, reg32 = f32 && L.rs > 0 && !L.glb, large = f32 && L.rs >= kRegSlotsLarge;
    int lw = B <= cap ? kSpecWaves : B <= kTwoWavesCaps * cap ? 2 : 1;
    if (large && B <= cap && kLarge4Den * B > kLarge4Num * s.n_simd) lw = 2;
    if (large && !L.glb && B >= kFillsLarge * kWpeRegLarge * cap) lw = 1;
    if (reg32 && kSimdsPerCu * B <= s.n_simd) lw = kSpecWavesWide;
    // table streamed from the global workspace: the wavefronts of a workgroup read the same rows at about the same time
    if (L.glb) lw = kSpecWaves;
    // LDS-bound tables: the wavefronts of a latency workgroup SHARE them -- the smallest W that keeps the most wavefronts
    // resident, if that is at least 1.5x what the throughput kernel gets
    const int wpe_sp = !f32 ? NMPC_WPE_F64 : L.rs >= kRegSlotsLarge ? kWpeRegLarge : NMPC_SPEC_WPE_F32;
    const int tp = std::min(kSimdsPerCu * wpe_tp, lds_per_cu);
    const int wg_spec = (int)(kLdsLimit / ((size_t)(L.lds_xch + spec_xch_elems(kSpecWaves)) * s.elem));
    int best = tp;
    for (int w = std::max(lw, 2); w <= kSpecWaves; ++w) {
        const int res = std::min(kSimdsPerCu * wpe_sp / w, wg_spec) * w;
        if (kSharedDen * res >= kSharedNum * tp && res > best) {
            best = res;
            lw = w;
        }
    }
    return lw;
}

inline SolvePlan plan_solve(const PlanStatic& s, const SolveRequest& q, const PlanTuning& tune = PlanTuning())
{
    const nmpc_config& c = *s.cfg;
    const Layout& L = s.L();
    const int B = q.B;
    const bool f32 = s.elem == 4;
    const bool reg32 = f32 && L.rs > 0 && !L.glb; // fp32 register-table kernels: the ones with a tail member
    const bool large = L.rs >= kRegSlotsLarge;
    // fp64 runs 2 wavefronts per SIMD (256 VGPRs) against 3 in fp32, so fewer 4-wavefront workgroups are resident
    const int cap = f32 ? s.n_simd : s.n_simd / 2;
    // resident wavefronts per SIMD of the one-wavefront kernel (its register budget), workgroups per CU that fit LDS
    const int wpe_tp = !f32 ? NMPC_WPE_F64 : large ? kWpeRegLarge : L.rs > 0 ? kWpeReg : NMPC_WPE_F32;
    const int lds_per_cu = (int)(kLdsLimit / ((size_t)L.lds_total * s.elem));

    // ---- family, variant, wavefronts ----
    // wavefronts per instance: 1 = throughput kernel; more = latency kernel (pays off while the batch leaves SIMDs idle)
    const int lw = c.latency_waves == 0 ? auto_latency_waves(s, B, cap, wpe_tp, lds_per_cu) : c.latency_waves;
    int waves = lw == 1 ? 0 : lw < 0 ? 1 : std::min(lw, kSpecWavesMax);
    if (!s.spec_ok) waves = 0;
    // cooperative evaluation (nmpc_config.coop_waves): explicit request, or automatic where the obstacle table is streamed
    // from global memory. Needs the LDS / global table (not the register table), room for the exchange area and no
    // wall-clock budget (each wavefront would read its own clock).
    int coop = std::min(c.coop_waves, kSpecWaves);
    if (coop == 0) coop = (L.glb && c.latency_waves == 0) ? kSpecWaves : 1;
    if (L.rs > 0 || c.max_solver_time_us > 0 || !s.coop_ok) coop = 1;
    // fp64, three lanes per step, 13..42 rows: the register-table kernel where the LDS table leaves room for fewer than
    // four instances per CU, from B = 2 cap on. reg_table = 1 forces it (tests), -1 switches it off (no layout then).
    const bool reg64 = !f32 && s.lay->lay64r.rs > 0 && coop <= 1 && c.latency_waves <= 1 &&
                       (c.reg_table > 0 || (s.lay->use64r_auto && B >= kReg64Caps * cap));
    // nmpc_config.batch_invariant: the latency plan on the TAIL members -- the throughput kernels' evaluation, hence their
    // bits. Automatic (0): the 14-slot kernels.
    const bool gated = reg32 && (c.batch_invariant > 0 || (c.batch_invariant == 0 && large));
    SolvePlan p;
    p.mode = reg64 ? 0 : coop > 1 ? 2 : waves ? 1 : 0;
    p.main = reg64 ? choose_reg64(s, kThroughput) : p.mode == 2 ? choose_coop(s, false, coop)
             : p.mode == 1 ? choose_latency(s, gated ? kLatencyTail : kLatencyFlat, waves) : choose_single(s, kThroughput);
    // one device fill. Cooperative kernels: LDS-bound, one workgroup per CU for the on-chip variant
    p.resident = reg64 ? s.n_simd
                 : p.mode == 2 ? std::min(std::max<int>(1, (int)(kLdsLimit / std::max<size_t>(p.main.lds_bytes, 1))), std::max(1, 8 / (p.main.threads / 64))) * (s.n_simd / kSimdsPerCu)
                               : std::max(1, std::min(wpe_tp * s.n_simd, lds_per_cu * (s.n_simd / kSimdsPerCu)));

    // ---- dispatch order and stages ----
    // (every kernel family parks / resumes; a wall-clock budget does not survive it)
    const bool stageable = q.allow_staging && c.max_solver_time_us <= 0 && q.has_status;
    const auto fills = [&](double plain, double reg) { return !reg32 ? plain : large ? kFillsLarge : reg; };
    const double stage_fills = fills(kStageFills, kStageFillsReg);
    int caps[2] = {c.staged, c.staged_evals};
    p.eval_order = reg32 && caps[0] == 0 && stageable && !q.caller_order && tune.proxy_order > 0 &&
                   (p.mode == 1 ? (B > cap / kRankMinDiv && (B <= cap ? (large || kProxyFullDen * B <= kProxyFullNum * cap)
                                                                     : (!large && B <= kProxyTwoWavesCaps * cap)))
                                : (p.mode == 0 && B >= stage_fills * p.resident && B < tune.proxy_fills * p.resident));
    if (p.eval_order) caps[0] = -1;
    // first boundary (nmpc_config.staged, ranked by ||F2||): automatic = one outer iteration for throughput plans of enough
    // fills, the latency plan at about one workgroup per SIMD, the on-chip cooperative kernels from four fills on;
    // second (nmpc_config.staged_evals, ranked by the evaluations used so far): explicit only
    if (caps[0] == 0)
        caps[0] = ((p.mode == 0 && B >= (tune.stage_fills >= 0 ? tune.stage_fills : stage_fills) * p.resident) ||
                   (p.mode == 1 && B > cap / kRankMinDiv && B <= cap) ||
                   (p.mode == 2 && !p.main.uses_ws && B >= kCoopStageFills * p.resident)) ? 1 : -1;
    if (caps[1] == 0) caps[1] = -1;
    for (int i = 0; i < 2; ++i)
        if (stageable && !q.caller_order && caps[i] > 0 && caps[i] < c.max_outer_iterations && (p.n_stage == 0 || caps[i] > p.stage_cap[p.n_stage - 1])) {
            p.stage_cap[p.n_stage] = caps[i];
            p.stage_key[p.n_stage] = i;
            ++p.n_stage;
        }
    p.last_mode = p.mode;
    p.last_staged = p.n_stage == 0 ? 0 : p.n_stage == 1 ? p.stage_cap[0] : 100 * p.stage_cap[0] + p.stage_cap[1];
    p.last_order = p.eval_order ? 2 : p.n_stage > 0 ? 3 : q.caller_order ? 1 : 0;
    // (the latency plan in the evaluation order is one launch: an explicit staged_evals is reported above but not run)
    if (p.eval_order && p.mode == 1) p.n_stage = 0;

    // ---- tail hand-off (nmpc_config.tail_latency): throughput plans of the fp32 register-table kernels ----
    p.park = c.tail_latency != 0 ? c.tail_latency : std::max(kTailParkMin, s.n_simd / kSimdsPerCu);
    const bool ordered = q.caller_order || p.eval_order;
    const double tail_fills = tune.tail_fills >= 0 ? tune.tail_fills : fills(kTailFills, kTailFillsReg);
    p.tail = p.mode == 0 && reg32 && s.spec_ok && p.park > 0 && stageable &&
             (p.n_stage > 0 || (ordered && B >= tail_fills * p.resident)) && B >= tune.tail_min_parks * p.park;
    if (p.tail)
        p.tail_kernel = choose_latency(s, kLatencyTail, tune.tail_waves >= 0 ? (int)tune.tail_waves
                                       : p.park * kSpecWavesWide <= kTailWideWpe * s.n_simd ? kSpecWavesWide : kSpecWaves);
    return p;
}

// What nmpc_eval_batch_* launches: the one-wavefront evaluation of the main layout; the fp64 register-table kernel wherever
// large fp64 solves would run it; with coop_waves > 1 the cooperative kernels' code path, so that the row split, the
// partial-sum exchange and the helper lanes can be compared with the oracle directly.
inline KernelChoice plan_eval(const PlanStatic& s)
{
    const nmpc_config& c = *s.cfg;
    if (c.coop_waves > 1 && s.L().rs == 0 && s.coop_ok) return choose_coop(s, true, std::min(c.coop_waves, kSpecWaves));
    if (s.elem == 8 && s.lay->lay64r.rs > 0 && c.coop_waves <= 1 && c.latency_waves <= 1 && (c.reg_table > 0 || s.lay->use64r_auto))
        return choose_reg64(s, kEval);
    return choose_single(s, kEval);
}

} // namespace nmpc_plan
