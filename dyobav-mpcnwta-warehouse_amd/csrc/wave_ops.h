// wave_ops.h -- 64-lane wavefront primitives for gfx950 (CDNA4): DPP reductions / scans / shifts.
//
// One MPC instance lives in one wavefront; every inner product, prefix sum of the rollout and suffix sum of
// the adjoint is a cross-lane operation done in registers with DPP (no LDS round trip).
// All functions must be called with EXEC = all 64 lanes (wave-uniform control flow).
#pragma once

#include <hip/hip_runtime.h>

namespace nmpc {

// DPP control encodings (GFX9 family)
enum : int {
    DPP_QUAD_1032 = 0xB1,    // quad_perm:[1,0,3,2]
    DPP_QUAD_2301 = 0x4E,    // quad_perm:[2,3,0,1]
    DPP_ROW_SHR0 = 0x110,    // row_shr:n = 0x110 + n
    DPP_WAVE_SHL1 = 0x130,   // lane i <- lane i+1
    DPP_WAVE_SHR1 = 0x138,   // lane i <- lane i-1
    DPP_ROW_MIRROR = 0x140,
    DPP_ROW_HALF_MIRROR = 0x141,
    DPP_ROW_BCAST15 = 0x142,
    DPP_ROW_BCAST31 = 0x143,
};

template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf, bool BOUND_CTRL = false>
__device__ __forceinline__ float dpp_mov(float old, float x)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old),
                                                                  __builtin_bit_cast(int, x), CTRL, ROW_MASK,
                                                                  BANK_MASK, BOUND_CTRL));
}
template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf, bool BOUND_CTRL = false>
__device__ __forceinline__ double dpp_mov(double old, double x)
{
    const unsigned long long o = __builtin_bit_cast(unsigned long long, old);
    const unsigned long long v = __builtin_bit_cast(unsigned long long, x);
    const int lo = __builtin_amdgcn_update_dpp((int)(unsigned)o, (int)(unsigned)v, CTRL, ROW_MASK, BANK_MASK,
                                               BOUND_CTRL);
    const int hi = __builtin_amdgcn_update_dpp((int)(unsigned)(o >> 32), (int)(unsigned)(v >> 32), CTRL,
                                               ROW_MASK, BANK_MASK, BOUND_CTRL);
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// value of x in lane addr4 / 4 (ds_bpermute_b32: any lane pattern, through the LDS crossbar, no memory touched)
__device__ __forceinline__ float bperm(float x, int addr4)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr4, __builtin_bit_cast(int, x)));
}
__device__ __forceinline__ double bperm(double x, int addr4)
{
    const unsigned long long v = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_ds_bpermute(addr4, (int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_ds_bpermute(addr4, (int)(unsigned)(v >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ float read_lane(float x, int lane)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), lane));
}
__device__ __forceinline__ double read_lane(double x, int lane)
{
    const unsigned long long v = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// ---- f32 reductions / scans: each step is x += dpp(x) as ONE VALU instruction (v_add_f32_dpp). Steps with full row and
//      bank masks go through update_dpp builtins: the compiler folds mov + add into v_add_f32_dpp (with
//      -fno-slp-vectorize) and fills the two wait states a DPP read needs after a VALU write of the same register with
//      the caller's independent instructions, inserting s_nop only where none is at hand. Steps with partial row masks
//      (row_bcast) would come out as v_mov (old) + v_mov_dpp + v_add: those are asm blocks with their own s_nop.

// Sum over the 64 lanes; the result is wave-uniform (read back from lane 63 into scalar registers).
// Association (every wave_sum / wave_sum2 / wave_sum3, float and double): in each 16-lane row a butterfly -- every lane
// adds its quad neighbour (lane ^ 1), then the other pair of its quad (lane ^ 2), then the mirrored lane of its half row
// (lane ^ 7), then the mirrored lane of its row (lane ^ 15) -- which leaves the row sum r0..r3 in every lane of the row;
// then r1 += r0 and r3 += r2 (row_bcast:15 into rows 1, 3), then rows 2 and 3 += (r0 + r1) (row_bcast:31), and lane 63
// holds (r3 + r2) + (r0 + r1).
__device__ __forceinline__ float wave_sum(float x)
{
    // The four in-row steps (full row / bank masks) through builtins: the compiler folds each into one v_add_f32_dpp and
    // fills the two wait states a dependent DPP read needs with whatever independent instructions the caller has (the
    // two-loop recursion: the next pair's LDS read, slot arithmetic, the alpha bookkeeping) instead of s_nop. The two
    // cross-row steps have partial row masks -- there it would emit v_mov + v_mov_dpp + v_add -- and stay an asm block.
    x += dpp_mov<DPP_QUAD_1032, 0xf, 0xf, true>(0.0f, x);
    x += dpp_mov<DPP_QUAD_2301, 0xf, 0xf, true>(0.0f, x);
    x += dpp_mov<DPP_ROW_HALF_MIRROR, 0xf, 0xf, true>(0.0f, x);
    x += dpp_mov<DPP_ROW_MIRROR, 0xf, 0xf, true>(0.0f, x);                                   // row sums everywhere
    asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"    // rows 1,3 += rows 0,2
        "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf"        // rows 2,3 += rows 0+1
        : "+v"(x));
    return read_lane(x, 63);
}
__device__ __forceinline__ double wave_sum(double x)
{
    x += dpp_mov<DPP_QUAD_1032>(x, x);
    x += dpp_mov<DPP_QUAD_2301>(x, x);
    x += dpp_mov<DPP_ROW_HALF_MIRROR>(x, x);
    x += dpp_mov<DPP_ROW_MIRROR>(x, x);
    x += dpp_mov<DPP_ROW_BCAST15, 0xa>(0.0, x);
    x += dpp_mov<DPP_ROW_BCAST31, 0xc>(0.0, x);
    return read_lane(x, 63);
}

// Two / three independent sums at once with interleaved chains.
#define NMPC_P2(ctrl) "s_nop 0\n\tv_add_f32_dpp %0, %0, %0 " ctrl "\n\tv_add_f32_dpp %1, %1, %1 " ctrl "\n\t"
#define NMPC_P3(ctrl) \
    "v_add_f32_dpp %0, %0, %0 " ctrl "\n\tv_add_f32_dpp %1, %1, %1 " ctrl "\n\tv_add_f32_dpp %2, %2, %2 " ctrl "\n\t"
__device__ __forceinline__ void wave_sum2(float x, float y, float& sx, float& sy)
{
    // (in-row steps through builtins, cross-row steps in one asm block: see wave_sum)
    x += dpp_mov<DPP_QUAD_1032, 0xf, 0xf, true>(0.0f, x);
    y += dpp_mov<DPP_QUAD_1032, 0xf, 0xf, true>(0.0f, y);
    x += dpp_mov<DPP_QUAD_2301, 0xf, 0xf, true>(0.0f, x);
    y += dpp_mov<DPP_QUAD_2301, 0xf, 0xf, true>(0.0f, y);
    x += dpp_mov<DPP_ROW_HALF_MIRROR, 0xf, 0xf, true>(0.0f, x);
    y += dpp_mov<DPP_ROW_HALF_MIRROR, 0xf, 0xf, true>(0.0f, y);
    x += dpp_mov<DPP_ROW_MIRROR, 0xf, 0xf, true>(0.0f, x);
    y += dpp_mov<DPP_ROW_MIRROR, 0xf, 0xf, true>(0.0f, y);
    asm("s_nop 0\n\t" NMPC_P2("row_bcast:15 row_mask:0xa bank_mask:0xf") NMPC_P2("row_bcast:31 row_mask:0xc bank_mask:0xf")
        : "+v"(x), "+v"(y));
    sx = read_lane(x, 63);
    sy = read_lane(y, 63);
}
__device__ __forceinline__ void wave_sum3(float x, float y, float z, float& sx, float& sy, float& sz)
{
    asm("s_nop 1\n\t" NMPC_P3("quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf")
            NMPC_P3("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf")
                NMPC_P3("row_half_mirror row_mask:0xf bank_mask:0xf") NMPC_P3("row_mirror row_mask:0xf bank_mask:0xf")
                    NMPC_P3("row_bcast:15 row_mask:0xa bank_mask:0xf")
                        NMPC_P3("row_bcast:31 row_mask:0xc bank_mask:0xf")
        : "+v"(x), "+v"(y), "+v"(z));
    sx = read_lane(x, 63);
    sy = read_lane(y, 63);
    sz = read_lane(z, 63);
}
__device__ __forceinline__ void wave_sum2(double x, double y, double& sx, double& sy)
{
    sx = wave_sum(x);
    sy = wave_sum(y);
}
__device__ __forceinline__ void wave_sum3(double x, double y, double z, double& sx, double& sy, double& sz)
{
    sx = wave_sum(x);
    sy = wave_sum(y);
    sz = wave_sum(z);
}

// Inclusive prefix sum over lanes 0..63 (lane i gets x_0 + ... + x_i).
// Association (float and double, one value or two): in each 16-lane row Hillis-Steele, x_i += x_{i-s} for s = 1, 2, 4, 8
// (a lane with fewer than s lanes below it in its row adds 0.0); then rows 1 and 3 += lane 15 / lane 47 (the totals of
// rows 0 and 2), then rows 2 and 3 += lane 31 (by then r0 + r1): a lane of row 3 ends up as (p + r2) + (r0 + r1).
__device__ __forceinline__ float wave_scan_incl(float x)
{
    x += dpp_mov<DPP_ROW_SHR0 + 1, 0xf, 0xf, true>(0.0f, x);
    x += dpp_mov<DPP_ROW_SHR0 + 2, 0xf, 0xf, true>(0.0f, x);
    x += dpp_mov<DPP_ROW_SHR0 + 4, 0xf, 0xf, true>(0.0f, x);
    x += dpp_mov<DPP_ROW_SHR0 + 8, 0xf, 0xf, true>(0.0f, x);
    asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf"
        : "+v"(x));
    return x;
}
// two prefix sums with interleaved chains
__device__ __forceinline__ void wave_scan_incl2(float& x, float& y)
{
    x += dpp_mov<DPP_ROW_SHR0 + 1, 0xf, 0xf, true>(0.0f, x);
    y += dpp_mov<DPP_ROW_SHR0 + 1, 0xf, 0xf, true>(0.0f, y);
    x += dpp_mov<DPP_ROW_SHR0 + 2, 0xf, 0xf, true>(0.0f, x);
    y += dpp_mov<DPP_ROW_SHR0 + 2, 0xf, 0xf, true>(0.0f, y);
    x += dpp_mov<DPP_ROW_SHR0 + 4, 0xf, 0xf, true>(0.0f, x);
    y += dpp_mov<DPP_ROW_SHR0 + 4, 0xf, 0xf, true>(0.0f, y);
    x += dpp_mov<DPP_ROW_SHR0 + 8, 0xf, 0xf, true>(0.0f, x);
    y += dpp_mov<DPP_ROW_SHR0 + 8, 0xf, 0xf, true>(0.0f, y);
    asm("s_nop 0\n\t" NMPC_P2("row_bcast:15 row_mask:0xa bank_mask:0xf") NMPC_P2("row_bcast:31 row_mask:0xc bank_mask:0xf")
        : "+v"(x), "+v"(y));
}
__device__ __forceinline__ double wave_scan_incl(double x)
{
    x += dpp_mov<DPP_ROW_SHR0 + 1>(0.0, x);
    x += dpp_mov<DPP_ROW_SHR0 + 2>(0.0, x);
    x += dpp_mov<DPP_ROW_SHR0 + 4>(0.0, x);
    x += dpp_mov<DPP_ROW_SHR0 + 8>(0.0, x);
    x += dpp_mov<DPP_ROW_BCAST15, 0xa>(0.0, x);
    x += dpp_mov<DPP_ROW_BCAST31, 0xc>(0.0, x);
    return x;
}
__device__ __forceinline__ void wave_scan_incl2(double& x, double& y)
{
    x = wave_scan_incl(x);
    y = wave_scan_incl(y);
}

// Inclusive suffix sum (lane i gets x_i + ... + x_63): in-row suffix with row_shl, then the totals of the rows
// above (they sit in the first lane of each row) are added from scalar registers. No LDS crossbar involved.
// Association: in each row x_i += x_{i+s} for s = 1, 2, 4, 8 (0.0 past the end of the row); with t1, t2, t3 the totals of
// rows 1..3 (lanes 16, 32, 48) wave_suffix_fix_rows returns x + (t1 + (t2 + t3)) in row 0, x + (t2 + t3) in row 1,
// x + t3 in row 2 and x + 0.0 in row 3.
template <typename T>
__device__ __forceinline__ T wave_suffix_fix_rows(T x)
{
    const T t1 = read_lane(x, 16), t2 = read_lane(x, 32), t3 = read_lane(x, 48);
    int l = (int)(threadIdx.x & 63);
    asm volatile("" : "+v"(l)); // (opaque: keeps the three row masks from being hoisted into long-lived SGPR pairs)
    const int row = l >> 4;
    // The three candidates as finished per-lane values before the selection: left to itself the compiler turns the
    // chain of conditions into divergent branches (exec masking, ~20 instructions) to avoid computing sums a row does
    // not need; as plain selects it is three compares and three v_cndmask.
    T c3 = t3, c23 = t2 + t3, c123 = t1 + c23;
    asm volatile("" : "+v"(c3), "+v"(c23), "+v"(c123));
    T add = row == 2 ? c3 : T(0);
    add = row == 1 ? c23 : add;
    add = row == 0 ? c123 : add;
    return x + add;
}
__device__ __forceinline__ float wave_scan_suffix_incl(float x)
{
    x += dpp_mov<0x100 + 1, 0xf, 0xf, true>(0.0f, x); // row_shl:n = 0x100 + n
    x += dpp_mov<0x100 + 2, 0xf, 0xf, true>(0.0f, x);
    x += dpp_mov<0x100 + 4, 0xf, 0xf, true>(0.0f, x);
    x += dpp_mov<0x100 + 8, 0xf, 0xf, true>(0.0f, x);
    return wave_suffix_fix_rows(x);
}
__device__ __forceinline__ void wave_scan_suffix_incl2(float& x, float& y)
{
    x += dpp_mov<0x100 + 1, 0xf, 0xf, true>(0.0f, x);
    y += dpp_mov<0x100 + 1, 0xf, 0xf, true>(0.0f, y);
    x += dpp_mov<0x100 + 2, 0xf, 0xf, true>(0.0f, x);
    y += dpp_mov<0x100 + 2, 0xf, 0xf, true>(0.0f, y);
    x += dpp_mov<0x100 + 4, 0xf, 0xf, true>(0.0f, x);
    y += dpp_mov<0x100 + 4, 0xf, 0xf, true>(0.0f, y);
    x += dpp_mov<0x100 + 8, 0xf, 0xf, true>(0.0f, x);
    y += dpp_mov<0x100 + 8, 0xf, 0xf, true>(0.0f, y);
    x = wave_suffix_fix_rows(x);
    y = wave_suffix_fix_rows(y);
}
// The cross-row step as three masked-row adds (float): the row totals t1, t2, t3 (lanes 16, 32, 48) into scalars, the three
// addends t3, t2 + t3, t1 + (t2 + t3) formed once in wave-uniform vector registers -- the select tree's own candidates --
// and each added to ITS row by a v_add_f32_dpp with the identity permutation and one row enabled: 10 instructions for the
// select tree's 15, no lane id, no compare, no select.
// Wait states (the compiler does not look into an asm block; gfx90a and later): a VALU write of a VGPR -> v_readlane of it:
// 1 (the s_nop 0 in front: x comes from the last in-row step); v_readlane's SGPR -> a VALU read of it: 2; a VALU write of a
// VGPR -> a DPP read of it: 2. The DPP operand is the addend, never x, and every scalar and addend is used three
// instructions after it is written, so nothing else is padded.
// Same operands, same association in rows 0..2. Row 3 is left alone where wave_suffix_fix_rows adds 0.0: that differs
// in one case only, an in-row suffix of -0.0 (x + 0.0 = +0.0). Every lane of the row but its first has added a 0.0 from
// past the end of the row on the way, so that is lane 48 with -0.0 in ALL of lanes 48..63: it keeps -0.0 here. A caller
// with +0.0 in any lane of row 3 never sees it. (Which NaN's payload survives NaN + NaN follows the operand order, which
// neither form promises.)
#define NMPC_ROW_ADD(x, c, mask) "v_add_f32_dpp " x ", " c ", " x " quad_perm:[0,1,2,3] row_mask:" mask " bank_mask:0xf\n\t"
__device__ __forceinline__ float wave_suffix_fix_rows_masked(float x)
{
    int s1, s2, s3;
    float c3, c23, c123;
    asm("s_nop 0\n\t"
        "v_readlane_b32 %3, %0, 48\n\tv_readlane_b32 %2, %0, 32\n\tv_readlane_b32 %1, %0, 16\n\t"
        "v_mov_b32 %4, %3\n\tv_add_f32 %5, %2, %4\n\tv_add_f32 %6, %1, %5\n\t"
        NMPC_ROW_ADD("%0", "%4", "0x4") NMPC_ROW_ADD("%0", "%5", "0x2") NMPC_ROW_ADD("%0", "%6", "0x1")
        : "+v"(x), "=&s"(s1), "=&s"(s2), "=&s"(s3), "=&v"(c3), "=&v"(c23), "=&v"(c123));
    return x;
}
__device__ __forceinline__ float wave_scan_suffix_incl_masked(float x)
{
    x += dpp_mov<0x100 + 1, 0xf, 0xf, true>(0.0f, x);
    x += dpp_mov<0x100 + 2, 0xf, 0xf, true>(0.0f, x);
    x += dpp_mov<0x100 + 4, 0xf, 0xf, true>(0.0f, x);
    x += dpp_mov<0x100 + 8, 0xf, 0xf, true>(0.0f, x);
    return wave_suffix_fix_rows_masked(x);
}
// two suffix sums with interleaved chains (every distance above only grows)
__device__ __forceinline__ void wave_scan_suffix_incl2_masked(float& x, float& y)
{
    x += dpp_mov<0x100 + 1, 0xf, 0xf, true>(0.0f, x);
    y += dpp_mov<0x100 + 1, 0xf, 0xf, true>(0.0f, y);
    x += dpp_mov<0x100 + 2, 0xf, 0xf, true>(0.0f, x);
    y += dpp_mov<0x100 + 2, 0xf, 0xf, true>(0.0f, y);
    x += dpp_mov<0x100 + 4, 0xf, 0xf, true>(0.0f, x);
    y += dpp_mov<0x100 + 4, 0xf, 0xf, true>(0.0f, y);
    x += dpp_mov<0x100 + 8, 0xf, 0xf, true>(0.0f, x);
    y += dpp_mov<0x100 + 8, 0xf, 0xf, true>(0.0f, y);
    int sx1, sx2, sx3, sy1, sy2, sy3;
    float cx3, cx23, cx123, cy3, cy23, cy123;
    asm("s_nop 0\n\t"
        "v_readlane_b32 %4, %0, 48\n\tv_readlane_b32 %7, %1, 48\n\tv_readlane_b32 %3, %0, 32\n\tv_readlane_b32 %6, %1, 32\n\t"
        "v_readlane_b32 %2, %0, 16\n\tv_readlane_b32 %5, %1, 16\n\t"
        "v_mov_b32 %8, %4\n\tv_mov_b32 %11, %7\n\tv_add_f32 %9, %3, %8\n\tv_add_f32 %12, %6, %11\n\t"
        "v_add_f32 %10, %2, %9\n\tv_add_f32 %13, %5, %12\n\t"
        NMPC_ROW_ADD("%0", "%8", "0x4") NMPC_ROW_ADD("%1", "%11", "0x4") NMPC_ROW_ADD("%0", "%9", "0x2")
        NMPC_ROW_ADD("%1", "%12", "0x2") NMPC_ROW_ADD("%0", "%10", "0x1") NMPC_ROW_ADD("%1", "%13", "0x1")
        : "+v"(x), "+v"(y), "=&s"(sx1), "=&s"(sx2), "=&s"(sx3), "=&s"(sy1), "=&s"(sy2), "=&s"(sy3), "=&v"(cx3), "=&v"(cx23),
          "=&v"(cx123), "=&v"(cy3), "=&v"(cy23), "=&v"(cy123));
}
#undef NMPC_ROW_ADD
__device__ __forceinline__ double wave_scan_suffix_incl(double x)
{
    x += dpp_mov<0x100 + 1, 0xf, 0xf, true>(0.0, x); // row_shl:n = 0x100 + n
    x += dpp_mov<0x100 + 2, 0xf, 0xf, true>(0.0, x);
    x += dpp_mov<0x100 + 4, 0xf, 0xf, true>(0.0, x);
    x += dpp_mov<0x100 + 8, 0xf, 0xf, true>(0.0, x);
    return wave_suffix_fix_rows(x);
}
__device__ __forceinline__ void wave_scan_suffix_incl2(double& x, double& y)
{
    x = wave_scan_suffix_incl(x);
    y = wave_scan_suffix_incl(y);
}
// Stride-3 all-reduce of two values at once: every lane gets the sums of x and of y over the lanes of its own residue
// class lane % 3 (three lanes per horizon step: the class = the obstacle row a lane owns in a slot of the register
// table, the sum runs over the horizon steps). In-row partial sums with three DPP steps (row_shr 3 / 6 / 12: the last
// lane of each class in a 16-lane row ends up with the class's sum over that row), then each lane fetches the four row
// partials of its class through the LDS crossbar (ds_bpermute, no memory touched) -- 10 instructions per value for all
// three classes, against three masked full-wave reductions. `a[q]` = 4 * (last lane of this lane's class in row q),
// see class3_addresses().
// Association (class3_sum2, class3_sum1, class3_issue1 + class3_finish1, float and double): in each row x_i += x_{i-s} for
// s = 3, 6, 12 (0.0 below the start of the row), then (x0 + x1) + (x2 + x3) of the four row partials, row 0 first.
__device__ __forceinline__ void class3_sum2(float& x, float& y, const int (&a)[4])
{
    asm("s_nop 0\n\t" NMPC_P2("row_shr:3 row_mask:0xf bank_mask:0xf bound_ctrl:0")
            NMPC_P2("row_shr:6 row_mask:0xf bank_mask:0xf bound_ctrl:0")
                NMPC_P2("row_shr:12 row_mask:0xf bank_mask:0xf bound_ctrl:0")
        : "+v"(x), "+v"(y));
    const float x0 = bperm(x, a[0]), x1 = bperm(x, a[1]), x2 = bperm(x, a[2]), x3 = bperm(x, a[3]);
    const float y0 = bperm(y, a[0]), y1 = bperm(y, a[1]), y2 = bperm(y, a[2]), y3 = bperm(y, a[3]);
    x = (x0 + x1) + (x2 + x3);
    y = (y0 + y1) + (y2 + y3);
}
// One value (the register-table passes gate their two slots separately since round 4): the same DPP steps and the same
// association of the four row partials as class3_sum2 -- a slot's E_j comes out bit-identical either way.
template <typename T>
__device__ __forceinline__ void class3_sum1(T& x, const int (&a)[4])
{
    x += dpp_mov<DPP_ROW_SHR0 + 3, 0xf, 0xf, true>(T(0), x);
    x += dpp_mov<DPP_ROW_SHR0 + 6, 0xf, 0xf, true>(T(0), x);
    x += dpp_mov<DPP_ROW_SHR0 + 12, 0xf, 0xf, true>(T(0), x);
    const T x0 = bperm(x, a[0]), x1 = bperm(x, a[1]), x2 = bperm(x, a[2]), x3 = bperm(x, a[3]);
    x = (x0 + x1) + (x2 + x3);
}
// The same in two halves, so that independent work can sit between the crossbar requests and their results:
// class3_issue1() leaves the four row partials in flight, class3_finish1() adds them up.
template <typename T>
struct Class3Pending1 {
    T x[4];
};
template <typename T>
__device__ __forceinline__ void class3_issue1(T x, const int (&a)[4], Class3Pending1<T>& p)
{
    x += dpp_mov<DPP_ROW_SHR0 + 3, 0xf, 0xf, true>(T(0), x);
    x += dpp_mov<DPP_ROW_SHR0 + 6, 0xf, 0xf, true>(T(0), x);
    x += dpp_mov<DPP_ROW_SHR0 + 12, 0xf, 0xf, true>(T(0), x);
#pragma unroll
    for (int q = 0; q < 4; ++q) p.x[q] = bperm(x, a[q]);
}
template <typename T>
__device__ __forceinline__ T class3_finish1(const Class3Pending1<T>& p)
{
    return (p.x[0] + p.x[1]) + (p.x[2] + p.x[3]);
}
__device__ __forceinline__ void class3_sum2(double& x, double& y, const int (&a)[4])
{
    auto rows = [](double v) {
        v += dpp_mov<DPP_ROW_SHR0 + 3, 0xf, 0xf, true>(0.0, v);
        v += dpp_mov<DPP_ROW_SHR0 + 6, 0xf, 0xf, true>(0.0, v);
        v += dpp_mov<DPP_ROW_SHR0 + 12, 0xf, 0xf, true>(0.0, v);
        return v;
    };
    x = rows(x);
    y = rows(y);
    x = (bperm(x, a[0]) + bperm(x, a[1])) + (bperm(x, a[2]) + bperm(x, a[3]));
    y = (bperm(y, a[0]) + bperm(y, a[1])) + (bperm(y, a[2]) + bperm(y, a[3]));
}
// byte addresses (ds_bpermute) of the last lane of residue class r = lane % 3 in each of the four 16-lane rows:
// rows start at lanes 0, 16, 32, 48 = classes 0, 1, 2, 0, so the last lanes are 15/13/14, 30/31/29, 45/46/47, 63/61/62.
// Three byte lookups in packed constants (a shift and three bit-field extracts) + one OR: cheap enough to be redone
// where the addresses are needed instead of occupying four registers for a whole evaluation.
__device__ __forceinline__ void class3_addresses(int r, int (&a)[4])
{
    const unsigned sh = (unsigned)r << 3;
    a[0] = (int)((0x38343Cu >> sh) & 0xffu); // 4 * {15, 13, 14}
    a[1] = (int)((0x747C78u >> sh) & 0xffu); // 4 * {30, 31, 29}
    a[2] = (int)((0xBCB8B4u >> sh) & 0xffu); // 4 * {45, 46, 47}
    a[3] = a[0] | 0xC0;                      // 4 * {63, 61, 62} = a[0] + 4 * 48
}
#undef NMPC_P2
#undef NMPC_P3

// lane i <- lane 63-i
template <typename T>
__device__ __forceinline__ T wave_reverse(T x)
{
    return __shfl(x, 63 - (int)(threadIdx.x & 63), 64);
}

// lane i <- lane i-S (zeros shifted in at the bottom)
template <int S, typename T>
__device__ __forceinline__ T wave_shift_up(T x)
{
#pragma unroll
    for (int s = 0; s < S; ++s) x = dpp_mov<DPP_WAVE_SHR1, 0xf, 0xf, true>(T(0), x);
    return x;
}
// lane i <- lane i+S (zeros shifted in at the top)
template <int S, typename T>
__device__ __forceinline__ T wave_shift_down(T x)
{
#pragma unroll
    for (int s = 0; s < S; ++s) x = dpp_mov<DPP_WAVE_SHL1, 0xf, 0xf, true>(T(0), x);
    return x;
}

// (A shift by S lanes as one ds_bpermute_b32 -- address 4 * lane -+ 4 * S in the offset field, the zero fill put back by a
//  select -- was built and measured in the evaluation and is not kept, HISTORY.md "Lane moves". Two things it needs: full
//  EXEC, a lane that is masked off being read as 0 by the others, while the compiler moves the read under the select's mask
//  unless its result is consumed in every lane first (an empty asm volatile on it); and a wait for every LDS read in flight.)

// ---- shuffle-based reference versions (used only by the device self-test) ---------------------------------
template <typename T>
__device__ inline T ref_wave_sum(T x)
{
    T s = 0;
    for (int i = 0; i < 64; ++i) s += __shfl(x, i, 64);
    return s;
}
template <typename T>
__device__ inline T ref_class3_sum(T x)
{
    const int lane = threadIdx.x & 63;
    T s = 0;
    for (int i = 0; i < 64; ++i) {
        T v = __shfl(x, i, 64);
        if (i % 3 == lane % 3) s += v;
    }
    return s;
}
template <typename T>
__device__ inline T ref_wave_scan_incl(T x)
{
    const int lane = threadIdx.x & 63;
    T s = 0;
    for (int i = 0; i < 64; ++i) {
        T v = __shfl(x, i, 64);
        if (i <= lane) s += v;
    }
    return s;
}
template <typename T>
__device__ inline T ref_wave_scan_suffix_incl(T x)
{
    const int lane = threadIdx.x & 63;
    T s = 0;
    for (int i = 63; i >= 0; --i) {
        T v = __shfl(x, i, 64);
        if (i >= lane) s += v;
    }
    return s;
}

} // namespace nmpc
