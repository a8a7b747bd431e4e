// nmpc_mmp_block_f16.h -- the residual block of the multi-hypothesis predictor's network (resnet34.layer2 .. layer4: two 3 x 3
// convolutions with folded affines and LeakyReLUs, stride 1 or 2 on the first, projection or identity) with binary16 MFMA
// OPERANDS and float32 everything else, stated ONCE for every stage (predictor `mmp`, opt-in per stage on top of the opt-in fused
// float32 stages: MmpFrontEnd(half=...) / MmpFrontEnd(operands=...) / MmpFrontEnd(precision=...)). A stage is a GEOMETRY G:
// nmpc_mmp_block1_f16.h (16 output channels: layer1, stride 1 only, after nmpc_mmp_block.h), nmpc_mmp_block2_f16.h (32 output
// channels), nmpc_mmp_block3_f16.h (64) and nmpc_mmp_block4_f16.h (128) hold one each, with the stage's Params, its decisions, its
// model and its measured figures; the block itself, its strides, its padding and the zero ring of m are defined by the float32
// sibling nmpc_mmp_block_f32.h (mmp_blkf_kernel) and its geometries in nmpc_mmp_block{2,3,4}.h, whose flat domains, pixel groups and,
// for layer2 and layer3, waves these geometries take over. x [M][Cin][H][W] and out [M][C][H2][W2] stay float32 in memory, unless
// the launch says otherwise (binary16 activations in memory, below).
//
// The rounding rule -- whatever an MFMA reads is f16, nothing else is:
//   - the weights w1, w2, wd are rounded ONCE on the host (mmp_stem.pack_block_f16) and arrive packed in fragment order (below);
//   - x is rounded when it is staged into LDS (the first convolution's operand); the projection reads it again from memory and
//     rounds it the same way;
//   - m = leaky(fma(s1, acc, b1), slope_mid) is rounded when it is written to LDS;
//   - rounding is to nearest even; a value beyond +-65504 saturates to +-65504 (mmp_blkh_round clips, then converts: the
//     infinities saturate with the finite values), NaN stays NaN, subnormals are kept (the kernel runs with f16 denormals on, and
//     the gfx950 MFMA does not flush them: tests/test_gpu_mmp_block{2,3,4}_f16.py pin that on the device);
//   - float32, as in the siblings: the accumulation (the MFMA's), the two affines and both LeakyReLUs, the addition z + id, x as
//     the identity when there is no projection (read again UNROUNDED), x and out in memory.
//   - the tensor between two blocks is binary16 where both blocks say so (XH / OH below): the identity of a block without
//     projection is then that binary16 value, and out is rounded once, after the last LeakyReLU.
// tests/mmp_block_f16_reference.py states the same rule in float64 with a derived bound.
//
// Instruction: v_mfma_f32_16x16x32_f16, K = 32 per instruction against the float32 kernels' 4 at half its cycles (16 against 32
// per SIMD):
//   A: lane l holds w[co = 16 g + (l & 15)][ci = 32 kb + 8 (l >> 4) + j], j = 0 .. 7, of one tap         (4 VGPRs, one 16-byte load)
//   B: lane l holds tile[ci = 32 kb + 8 (l >> 4) + j][q + off(tap)], q = q0 + (l & 15)                   (4 VGPRs, one ds_read_b128)
//   D: 4 VGPRs: channel 16 g + 4 (l >> 4) + r in register r, pixel q0 + (l & 15)                         (as the f32 form)
// C output channels are C / 16 A groups g, of which a wave holds G::NH from G::first_a(wave) on; C channels of m are C / 32 K
// blocks kb per tap -- C = 16 is half of ONE K block: the lane groups l >> 4 in {2, 3} of the second convolution feed zeros
// against the packed zeros of w2. A Cin that is no multiple of 32 has zeros in the last K block (staged zeros in B, packed zeros in A). A
// chunk of fewer than 32 channels (G::ck(STRIDE) = 16: layer2's strided block) is one HALF of a K block: the chunk c0 is half
// (c0 >> 4) & 1 of K block c0 >> 5, the lane groups l >> 4 of that half read its two octets and the other two feed zeros.
//
// LDS layout: channels innermost, in OCTETS: [plane = sub-plane x octet][slot = position q + G::SH][8 halves], 16 bytes per slot,
// planes of G::PL slots, PL x 16 B a multiple of 256 B (each stage's static_assert). A B fragment is one aligned ds_read_b128.
// Banks (b128: bank = (byte / 4) mod 64, four groups of 16 lanes, each two runs of lanes: l & 15 in {0 .. 3, 12 .. 15} of one
// l >> 4 and {4 .. 11} of the next): a group reads slots s0 + {0 .. 3, 12 .. 15} of one plane and s0 + {4 .. 11} of the plane
// behind it; because the plane stride is a multiple of 256 B the sixteen 16-byte slots are s0 + 0 .. 15 mod 16: all distinct,
// conflict-free for every group, every tap offset and every slot shift. The alternative [position][C channels] (128 B or 144 B
// per position at C = 64) was counted and is 2-way conflicted for every stride of 16 a bytes, a odd, 128 .. 240: the two runs of
// a lane group land on the same slots. The m store is one ds_write_b64 per pixel group and A group (the 4 consecutive channels of
// a D fragment are half an octet). m is C / 8 planes and goes over the dead input: a chunk has at least as many.
//
// The packed weights (uint16 = binary16 bits, 16-byte aligned, mmp_stem.pack_block_f16; include/nmpc_hip.h):
//   w1p[tap t = 3 ky + kx][K block kb < ceil(Cin / 32)][group g < C / 16][lane l < 64][j < 8] = f16(w1[16 g + (l & 15)][32 kb + 8 (l >> 4) + j][ky][kx])
//   w2p the same with Cin = C;   wdp[kb][g][l][j] = f16(wd[16 g + (l & 15)][32 kb + 8 (l >> 4) + j]);   0 where the channel is >= Cin.
//
// Steps: workgroup = [row of the batch][tile row][tile column] flattened in x. 1. per chunk: x global -> f16 -> LDS (8 channels
// of a position per 16-byte store, zero outside the plane and for channels >= Cin; a strided block's input is split by parity
// into four sub-planes on the same domain: tap ky reads row parity ky != 1 at offset -S for ky = 0, likewise kx), barrier, per K
// block 9 taps x G::NI pixel groups x G::NH A groups of MFMA; 2. barrier; m -> LDS, exactly zero outside the plane; barrier; 3.
// C / 32 K blocks x 9 taps x G::NO x G::NH on m (the wave's groups of out are its first NO groups of m); 4. per pixel group of
// out: the projection (x read again and rounded, one MFMA per K block and A group), the affines, the identity, the activation,
// one dword store per value. No atomics, no scratch.
//
// Summation order (fixed): per convolution chunks and K blocks ascending, per K block the taps ky-major, per tap the
// instruction's own order over its 32 channels; then one fma per affine and one addition. A row's bits depend on that row of x
// and the weights only: not on M, the row's position, the launch or the alignment of out.
//
// Binary16 activations in memory (opt-in per tensor: MmpFrontEnd(activations="f16"), nmpc_mmp_block{2,3,4}_f16_io): a tensor of
// C channels (C % 8 == 0) on an H x W plane in the OCTET FORM a[n][o = c / 8][y][x][j = c % 8], uint16_t bit patterns, row n
// n C H W halves in, the base aligned to 16 bytes; the values are mmp_blkh_round's. It is the LDS layout's own slot, and half of
// it is a D fragment, so with XH (x is in that form) a staging item is ONE 16-byte load without conversion (zeros outside the
// plane or for octets >= Cin / 8), the projection's B fragment one 16-byte load of octet 4 kb + k4 at the pixel, the identity one
// 8-byte load of channels 16 (hb + h) + 4 k4 .. + 3, converted to float; with OH (out is in that form) the epilogue packs the
// four values of a D fragment with mmp_blkh_round into one 8-byte store at octet 2 (hb + h) + (k4 >> 1), half k4 & 1. The sixteen
// lanes l & 15 of a fragment touch 256 consecutive bytes either way. Fragments, LDS layout, chunking, barriers, m, the ring and
// the summation order do not depend on the two flags: on x that holds binary16 values the bits of a float32 out are those of the
// float32 form, and a binary16 out is mmp_blkh_round of them (tests/test_gpu_mmp_block_f16_io.py, bit for bit).
// The flags travel in the geometry's TYPE, MmpBlkhIo<G, XH, OH> below, not as two further template parameters: the kernels of
// float32 memory keep their names mmp_blkh_kernel<G, STRIDE, PROJ> and their bytes, and tests/test_mmp_block{2,3,4}_f16_cpu.py,
// which count exactly three kernels of that name per stage, keep holding. Everything that follows from the flags is derived in
// the body, as for HALF and ROWS; the geometries gained no switch.
// Modelled before the device run, from the code only. Global memory instructions per thread and tile, float32 form -> octet
// form: staging loads of x in front of the first barrier / loads of x in the epilogue / stores of out:
//   layer2  32 -> 32 identity    72 dwords -> 9 of 16 B   /  48 dwords -> 12 of 8 B              /  48 dwords -> 12 of 8 B
//   layer2  16 -> 32 strided    144 -> 18                 /  6 groups x 8 = 48 -> 6 of 16 B      /  48 -> 12
//   layer3  64 -> 64 identity    72 -> 9                  /  48 -> 12                            /  48 -> 12
//   layer3  32 -> 64 strided    144 -> 18                 /  6 x 8 = 48 -> 6                     /  48 -> 12
//   layer4 128 -> 128 identity   80 -> 10                 /  64 -> 16                            /  64 -> 16
//   layer4  64 -> 128 strided   160 -> 20 (two chunks)    /  4 groups x 2 K blocks x 8 = 64 -> 8 /  64 -> 16
// Bytes per element 4 -> 2 on each binary16 side. 7 / 8 of the staging and projection loads, 3 / 4 of the identity loads and
// 3 / 4 of the stores go, and with them the 8 conversions per staged item. Expected from this: every launch faster, the strided
// layer2 block (144 loads under two workgroups per CU) most; by how much is for the run to say (DESIGN.md section 7,
// profiles/mmp_f16_activations_evaluate.json).
// Measured (both arms on f16 operands in one process, three runs each, 440 rows): the 13 launches of layer2 .. layer4 0.936-0.946 ms
// against 1.291-1.296 on float32 memory, 0.72-0.73 x; the stage 180.5 ms per lock-step against 197.0. The eleven blocks with both
// sides binary16 run at 0.62-0.71 x; the strided layer2 block, expected to gain most, gained least (0.193 -> 0.175 ms): its x is
// layer1's float32 output, so only its stores changed. No counter run was made.
// Compiler (hipcc -O3 --offload-arch=gfx950; tools/kernel_resources.py on the shipped code object), VGPRs of <2, true> / <1, true> /
// <1, false> on float32 x and binary16 out, binary16 x and float32 out, both binary16:
//   layer2 126 / 126 / 128,  126 / 118 / 128,  122 / 118 / 118   (siblings 126 / 126 / 122; bound 256 at stride 2, else 128)
//   layer3 163 / 122 / 124,  171 / 128 / 122,  169 / 128 / 122   (siblings 165 / 124 / 124; bound 256 at stride 2, else 128)
//   layer4 140 / 126 / 146,  138 / 128 / 144,  138 / 122 / 144   (siblings 162 / 142 / 146; bound 168)
// each with its sibling's LDS, no spills, scratch 0 (tests/test_mmp_activations_cpu.py). The one thing a register count forced is in
// the epilogue, where it is said; the nine kernels of float32 memory are byte for byte the parent's
// (profiles/mmp_f16_activations_code_object_identity.txt).
//
// A geometry G holds (nmpc_mmp_block3_f16.h is the plainest to read):
//   Params                   the kernel's argument, a true __global__ argument: handed on by value or by reference it costs
//                            registers (layer3 <1, false>: 124 VGPRs -> 128 and 6 spilled), so helpers take the ints they need
//   C, Threads               output channels; threads per workgroup (4 waves)
//   S, Q, TH, TW             the flat domain: row stride, positions, outputs per tile
//   PL, SH                   slots per LDS plane; the slot of position 0
//   NI, NO, NH               pixel groups of m and of out per wave; A groups per wave
//   ck(STRIDE), min_wg(STRIDE)   input channels per chunk; workgroups per CU of __launch_bounds__
//   Unroll                   the staging loop's unroll factor
//   pixel_wave(wave)         pg: which share of the pixel groups the wave takes;   first_a(wave)   its first A group
//   group(pg, i)             first position of the wave's pixel group i
//   live(pg, i)              whether slot i is a group of its own (false: a recomputed copy, not stored)
//   Fitted                   the domain is fitted to the plane of m (layer4): Params carry the origin oy, ox of out in the domain
//                            (otherwise 2, 2), and the Ring positions ring(j) of a plane that no group covers get zeros
//   RegTight                 the accumulators leave few registers (layer4): the plane test of m is kept as a bit mask, the
//                            affines and the epilogue's loads go one group at a time behind a scheduling barrier, and the
//                            epilogue works its pixel out again
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nmpc {

typedef float mmp_blkh_f4 __attribute__((ext_vector_type(4)));
typedef _Float16 mmp_blkh_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 mmp_blkh_h4 __attribute__((ext_vector_type(4)));

// float32 -> binary16 of the rule: clipped to +-65504 (NaN passes both comparisons), then rounded to nearest even
__device__ __forceinline__ _Float16 mmp_blkh_round(float v)
{
    v = v > 65504.0f ? 65504.0f : v;
    v = v < -65504.0f ? -65504.0f : v;
    return (_Float16)v;
}

// A geometry with the form of x and out in memory: G itself is float32 both ways; MmpBlkhIo<G, XH, OH> is G on the octet form
// of x (XH) and / or of out (OH), p.x / p.out then pointing at binary16 (the Params are G's, the pointers are cast)
template <typename G, bool XH_, bool OH_>
struct MmpBlkhIo : G {
    static constexpr bool XH = XH_, OH = OH_;
};
template <typename G>
struct mmp_blkh_io {
    static constexpr bool XH = false, OH = false;
};
template <typename G, bool XH_, bool OH_>
struct mmp_blkh_io<MmpBlkhIo<G, XH_, OH_>> {
    static constexpr bool XH = XH_, OH = OH_;
};

template <typename G, int STRIDE, bool PROJ>
__global__ __launch_bounds__(G::Threads, G::min_wg(STRIDE)) void mmp_blkh_kernel(typename G::Params p)
{
    static_assert(STRIDE == 1 || STRIDE == 2, "stride");
    constexpr bool XH = mmp_blkh_io<G>::XH, OH = mmp_blkh_io<G>::OH; // x / out in memory in the octet form of binary16
    constexpr int CK = G::ck(STRIDE);                  // input channels per chunk
    constexpr bool HALF = CK < 32;                     // a chunk is half a K block
    constexpr int NOC = CK / 8;                        // octets of channels per chunk
    constexpr int NPL = NOC * STRIDE * STRIDE;         // planes per chunk: [sub-plane][octet]
    constexpr int NIT = NPL * G::Q;                    // 16-byte items per chunk
    constexpr int PRE = (NIT + G::Threads - 1) / G::Threads; // items a thread stages per chunk
    constexpr int NA = G::C / 16, MP = G::C / 8;       // A groups; planes of m
    constexpr int KB2 = (G::C + 31) / 32;              // K blocks of the second convolution
    constexpr bool MHALF = G::C % 32 != 0;             // m is half a K block (C = 16): the lane groups l >> 4 in {2, 3} feed zeros
    constexpr int S = G::S, PL = G::PL, SH = G::SH, NH = G::NH;
    // a pixel group lies in ONE row of the domain and the waves' NO slots are exactly the tile's groups: a group of out has no row
    // outside the tile (layer1's 30 groups leave two of 32 slots to groups of m alone, which the row test then drops)
    constexpr bool ROWS = S % 16 == 0 && G::TH * (S / 16) == G::NO * (G::Threads / 64) * NH / NA;
    static_assert(CK % 32 == 0 || CK == 16, "a chunk is K blocks, or half of one");
    static_assert(NPL >= MP, "m does not fit over the chunk");
    __shared__ __attribute__((aligned(16))) _Float16 lds[NPL * PL * 8]; // [plane][slot][8]; m over the last chunk

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pg = G::pixel_wave(wave), hb = G::first_a(wave); // the wave's share of the pixel groups; its first A group
    const int lane = tid & 63, col = tid & 15, k4 = (tid >> 4) & 3;
    const int tiles = p.tx * p.ty;
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    if (n >= p.M) return; // (workgroup-uniform, in front of every barrier)
    const int tyi = tile / p.tx, txi = tile - tyi * p.tx;
    int oy = 2, ox = 2; // the first row / column of out in the domain
    if constexpr (G::Fitted) oy = p.oy, ox = p.ox;
    const int gy0 = tyi * G::TH - oy, gx0 = txi * G::TW - ox; // the output pixel of position 0
    const size_t plane = (size_t)p.H * p.W, plane2 = (size_t)p.H2 * p.W2;
    const float* xn = p.x + (size_t)n * p.Cin * plane;
    const _Float16* xh = reinterpret_cast<const _Float16*>(p.x) + (size_t)n * p.Cin * plane; // (XH: the row in the octet form)
    const int KB1 = (p.Cin + 31) >> 5;               // K blocks of the first convolution and the projection

    const mmp_blkh_f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    const mmp_blkh_h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    mmp_blkh_f4 acc[G::NI][NH];
    int gq[G::NI]; // the wave's pixel groups: first position + col
#pragma unroll
    for (int i = 0; i < G::NI; ++i) {
        gq[i] = G::group(pg, i) + col;
#pragma unroll
        for (int h = 0; h < NH; ++h) acc[i][h] = zero;
    }

    // ---- 1. the first convolution, the input staged in chunks of CK channels, rounded on the way
    for (int c0 = 0; c0 < p.Cin; c0 += CK) {
        if (c0) __syncthreads(); // the previous chunk has been read
#pragma unroll G::Unroll
        for (int e = 0; e < PRE; ++e) {
            const int i = tid + e * G::Threads;
            if (NIT % G::Threads == 0 || i < NIT) {
                const int pl = i / G::Q, q = i - pl * G::Q;
                const int sub = pl / NOC, o = pl - sub * NOC;
                const int y = STRIDE * (gy0 + q / S) + sub / 2, xx = STRIDE * (gx0 + q % S) + sub % 2;
                const int ch = c0 + 8 * o;               // (Cin is a multiple of 8: an octet is inside or outside)
                const bool in = ch < p.Cin && y >= 0 && y < p.H && xx >= 0 && xx < p.W;
                const size_t at = in ? (size_t)ch * plane + (size_t)y * p.W + xx : (size_t)0;
                mmp_blkh_h8 v;
                if constexpr (XH) { // octet ch / 8 of the pixel: one 16-byte load, already rounded
                    v = in ? *reinterpret_cast<const mmp_blkh_h8*>(xh + 8 * ((size_t)(ch >> 3) * plane + (size_t)y * p.W + xx)) : zero8;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = mmp_blkh_round(in ? xn[at + (size_t)j * plane] : 0.0f);
                }
                *reinterpret_cast<mmp_blkh_h8*>(lds + 8 * (pl * PL + q + SH)) = v;
            }
        }
        __syncthreads();
        // whole K blocks: lane group k4 reads octet 4 kb + k4. Half a K block: the lane groups of that half read octets 0, 1
        const bool feeds = !HALF || (k4 >> 1) == ((c0 >> 4) & 1);
        const int oct = HALF ? (k4 & 1) : k4;
        for (int kb = 0; kb < (HALF ? 1 : CK / 32); ++kb) {
            if (c0 + 32 * kb >= p.Cin) break; // (uniform)
            const uint16_t* wk = p.w1 + ((size_t)((c0 >> 5) + kb) * NA + hb) * 512 + lane * 8;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ky = t / 3, kx = t % 3;
                const int sub = STRIDE == 2 ? 2 * (ky != 1) + (kx != 1) : 0;
                const int off = STRIDE == 2 ? (ky == 0 ? -S : 0) + (kx == 0 ? -1 : 0) : (ky - 1) * S + (kx - 1);
                mmp_blkh_h8 a[NH];
#pragma unroll
                for (int h = 0; h < NH; ++h) a[h] = *reinterpret_cast<const mmp_blkh_h8*>(wk + ((size_t)t * KB1 * NA + h) * 512);
                const _Float16* xb = lds + 8 * ((sub * NOC + 4 * kb + oct) * PL + off + SH);
#pragma unroll
                for (int i = 0; i < G::NI; ++i) {
                    const mmp_blkh_h8 b = feeds ? *reinterpret_cast<const mmp_blkh_h8*>(xb + 8 * gq[i]) : zero8;
#pragma unroll
                    for (int h = 0; h < NH; ++h) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[h], b, acc[i][h], 0, 0, 0);
                }
            }
        }
    }

    // ---- 2. m -> LDS over the last chunk, rounded, zero outside the plane; zeros to what no group covers
    __syncthreads(); // the last chunk has been read
    unsigned inm = 0; // bit i: the wave's pixel group i has a pixel of the plane in this lane
    if constexpr (G::RegTight) {
#pragma unroll
        for (int i = 0; i < G::NI; ++i) {
            const int y = gy0 + gq[i] / S, xx = gx0 + gq[i] % S;
            inm |= (unsigned)(y >= 0 && y < p.H2 && xx >= 0 && xx < p.W2) << i;
        }
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        if constexpr (G::RegTight) __builtin_amdgcn_sched_barrier(0); // (one A group's affine at a time)
        float s[4], sh[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] = p.s1[16 * (hb + h) + 4 * k4 + r], sh[r] = p.b1[16 * (hb + h) + 4 * k4 + r];
        // channels 16 (hb + h) + 4 k4 + r, r = 0 .. 3: half of octet 2 (hb + h) + (k4 >> 1)
        _Float16* mo = lds + 8 * ((2 * (hb + h) + (k4 >> 1)) * PL + SH) + 4 * (k4 & 1);
#pragma unroll
        for (int i = 0; i < G::NI; ++i) {
            if (!G::live(pg, i)) continue;
            const int q = gq[i];
            bool in;
            if constexpr (G::RegTight) {
                in = (inm >> i) & 1;
            } else {
                const int y = gy0 + q / S, xx = gx0 + q % S;
                in = y >= 0 && y < p.H2 && xx >= 0 && xx < p.W2;
            }
            mmp_blkh_h4 mv;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = fmaf(s[r], acc[i][h][r], sh[r]);
                mv[r] = mmp_blkh_round(in ? (v > 0.0f ? v : v * p.slope_mid) : 0.0f);
            }
            *reinterpret_cast<mmp_blkh_h4*>(mo + 8 * q) = mv;
        }
    }
    if constexpr (G::Fitted) {
        for (int i = tid; i < MP * G::Ring; i += G::Threads) {
            const int pl = i / G::Ring, j = i - pl * G::Ring;
            *reinterpret_cast<mmp_blkh_h8*>(lds + 8 * (pl * PL + G::ring(j) + SH)) = zero8;
        }
    }
    __syncthreads();

    // ---- 3. the second convolution on the m tile (the wave's groups of out are its first G::NO groups of m)
#pragma unroll
    for (int i = 0; i < G::NO; ++i)
#pragma unroll
        for (int h = 0; h < NH; ++h) acc[i][h] = zero;
    const bool feeds2 = !MHALF || k4 < 2;
    for (int kb = 0; kb < KB2; ++kb) {
        const uint16_t* wk = p.w2 + ((size_t)kb * NA + hb) * 512 + lane * 8;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int off = (t / 3 - 1) * S + (t % 3 - 1);
            mmp_blkh_h8 a[NH];
#pragma unroll
            for (int h = 0; h < NH; ++h) a[h] = *reinterpret_cast<const mmp_blkh_h8*>(wk + ((size_t)t * KB2 * NA + h) * 512);
            const _Float16* mb = lds + 8 * ((4 * kb + k4) * PL + off + SH);
#pragma unroll
            for (int i = 0; i < G::NO; ++i) {
                const mmp_blkh_h8 b = feeds2 ? *reinterpret_cast<const mmp_blkh_h8*>(mb + 8 * gq[i]) : zero8;
#pragma unroll
                for (int h = 0; h < NH; ++h) acc[i][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[h], b, acc[i][h], 0, 0, 0);
            }
        }
    }

    // ---- 4. the projection, the affine, the identity, the activation and the store
    float* on = p.out + (size_t)n * G::C * plane2;
    _Float16* oh = reinterpret_cast<_Float16*>(p.out) + (size_t)n * G::C * plane2; // (OH: the row in the octet form)
#pragma unroll
    for (int i = 0; i < G::NO; ++i) {
        if constexpr (G::RegTight) __builtin_amdgcn_sched_barrier(0); // (the loads of one pixel group at a time)
        int q = gq[i];
        if constexpr (G::RegTight) asm volatile("" : "+v"(q)); // (worked out again, not kept across the second convolution)
        // (one number in two forms: without a row test the compiler keeps the remainder, with one it reuses the quotient; the
        // other form costs layer2 <1, false> 6 registers, on its bound of 128, and layer3 <2, true> 6 the other way round)
        const int r0 = q / S, c = ROWS ? q % S : q - r0 * S;
        const int y = gy0 + r0, xx = gx0 + c;
        const bool valid = (ROWS || (r0 >= oy && r0 < G::Q / S - oy)) && c >= ox && c < S - ox && y < p.H2 && xx < p.W2; // (then y, xx >= 0)
        mmp_blkh_f4 idacc[NH] = {};
        if (PROJ) { // (every lane takes part in the MFMAs; a lane without a pixel, or with channels >= Cin, feeds zeros)
            const float* xc = xn + (valid ? (size_t)(STRIDE * y) * p.W + STRIDE * xx : (size_t)0);
            for (int kb = 0; kb < KB1; ++kb) {
                const int ch = 32 * kb + 8 * k4;
                const bool ld = valid && ch < p.Cin;
                mmp_blkh_h8 b;
                if constexpr (XH) { // octet 4 kb + k4 at the pixel
                    b = ld ? *reinterpret_cast<const mmp_blkh_h8*>(xh + 8 * ((size_t)(4 * kb + k4) * plane + (size_t)(STRIDE * y) * p.W + STRIDE * xx)) : zero8;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) b[j] = mmp_blkh_round(ld ? xc[(size_t)(ch + j) * plane] : 0.0f);
                }
#pragma unroll
                for (int h = 0; h < NH; ++h)
                    idacc[h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                        *reinterpret_cast<const mmp_blkh_h8*>(p.wd + ((size_t)kb * NA + hb + h) * 512 + lane * 8), b, idacc[h], 0, 0, 0);
            }
        }
        if (!valid) continue;
        const size_t pix = (size_t)y * p.W2 + xx;
        // (with OH the fragment's offset is worked out here, not kept across the second convolution: kept, layer2 <1, false> on
        // float32 x spilled 1 register at its bound of 128 and layer3 <1, true> on binary16 x spilled 3; worked out here with XH
        // alone, layer2 <1, false> spilled 2)
        int k4o = k4;
        if constexpr (OH) asm volatile("" : "+v"(k4o));
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            // the D fragment's four channels in the octet form: half k4 & 1 of octet 2 (hb + h) + (k4 >> 1) at the pixel
            const size_t ho = 8 * ((size_t)(2 * (hb + h) + (k4o >> 1)) * plane2 + pix) + 4 * (k4o & 1);
            mmp_blkh_h4 idh = {0, 0, 0, 0}, ov;
            if constexpr (XH && !PROJ) idh = *reinterpret_cast<const mmp_blkh_h4*>(xh + ho); // (no projection: plane2 == plane)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = 16 * (hb + h) + 4 * k4 + r;
                const size_t o = (size_t)co * plane2 + pix;
                const float z = fmaf(p.s2[co], acc[i][h][r], p.b2[co]);
                const float id = PROJ ? fmaf(p.sd[co], idacc[h][r], p.bd[co]) : XH ? (float)idh[r] : xn[o]; // (no projection: plane2 == plane)
                const float v = z + id;
                const float w = v > 0.0f ? v : v * p.slope_out;
                if constexpr (OH) ov[r] = mmp_blkh_round(w);
                else on[o] = w;
            }
            if constexpr (OH) *reinterpret_cast<mmp_blkh_h4*>(oh + ho) = ov;
        }
    }
}

} // namespace nmpc
