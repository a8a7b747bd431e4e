// nmpc_sizes.h -- the size constants that the kernels (nmpc_device.h) and the host-side layout / solve plan (nmpc_plan.h)
// must agree on. No HIP header: nmpc_plan.h compiles with a plain C++17 compiler.
#pragma once

#ifdef __HIPCC__
#define NMPC_HD __host__ __device__
#else
#define NMPC_HD
#endif

namespace nmpc {

constexpr int kMem = 10;        // max L-BFGS memory (NMPC_LBFGS_MAX_MEMORY)
// L-BFGS storage in LDS. Ring of (s, y) pairs: kMem slots of lbfgs_slot_stride(N) Quads (an odd stride: slots spread over
// the LDS banks).
NMPC_HD constexpr int lbfgs_slot_stride(int N) { return N | 1; }
constexpr int kParkQuads = 5;   // solver vectors parked in LDS across an evaluation: 5 quads of 4 values per lane
constexpr int kEllStride = 8;   // LDS words per pre-processed ellipse

// entries of the path-segment table in LDS: the N segments of the reference + dummies (see Instance::load / eval)
NMPC_HD constexpr int seg_table_len(int N) { return 2 * N + 4; }
constexpr int kResumeScalars = 16;
constexpr int kResumeStride = 6 * 64 + kResumeScalars; // elements of T per instance

// one slot of a deep park (tail hand-off, KParams::deep; the slot's map is in nmpc_device.h)
constexpr int kDeepScalars = 32;
NMPC_HD constexpr int deep_ring_elems(int N) { return 4 * kMem * lbfgs_slot_stride(N); }
NMPC_HD constexpr int deep_park_stride(int N) { return kParkQuads * 64 * 4 + deep_ring_elems(N) + 3 * 64 + kDeepScalars; }

} // namespace nmpc
