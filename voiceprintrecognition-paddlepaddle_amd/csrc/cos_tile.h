// The cosine tile walk of gallery.hip (gallery_score_kernel), trial_ranks.hip (trial_pass_kernel<MODE, NORM>) and cohort_stats.hip
// (cohort_stats_kernel): device code, included by all three.
//
// A workgroup of 256 threads holds a tile of 32 unit rows ("columns": queries, trials) in LDS as [k][column], the B operand of
// v_mfma_f32_32x32x2_f32, and walks `slabs_per_wg` slabs of SLAB = 128 rows of a unit row matrix.  Each of its four waves owns 32 rows of
// a slab, reads them straight from global memory as 16-byte loads, eight in flight per lane (lane (c, half) takes floats
// 8g + 4 half .. + 3 of row c; a v_permlane32_swap pair per eight k puts k, k + 1 on the two lane halves) and keeps the 32 x 32 scores in
// one accumulator over ALL of D.
//
// THE CONTRACT.  A score is one k-ordered fma chain: ascending groups of eight k, inside a group the pairs (k0, k0 + 1), (k0 + 2, k0 + 3),
// (k0 + 4, k0 + 5), (k0 + 6, k0 + 7) in that order (inside a pair the matrix core's own order), then, for a D that is no multiple of 8,
// the last four k as two pairs.  Nothing else enters it: not the row count, the slab, the wave, the grid, the row's position or which
// kernel walks.  Bit-identical rows therefore give bit-identical scores, in both units and in every pass of the scorer
// (tests/test_gpu_cos_tile.py).  Whoever changes the unroll, the tail or the order inside a group changes it here, for every caller.
// The unit rows take their lengths in float64 (inv_length), so an element is rounded once.
#pragma once
#include "common.h"

#include <math.h>

namespace cos_tile {

constexpr int SLAB = 128;               // 4 waves x 32 rows
constexpr int COLS = 32;                // columns of a tile = the matrix core's N
constexpr int MAX_D = 1024;

typedef __attribute__((ext_vector_type(16))) float f32x16;

static_assert(SLAB == VP_GALLERY_SLAB, "vpmi.h states the slab of the walk");

// "Length in float64, one rounding per element": a row's sum of squares ss (each caller adds sum_sq in its own order) -> 1 / length,
// a zero row stays zero -> the unit row's elements.
__device__ __forceinline__ double sum_sq(float4 v) { return (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w; }
__device__ __forceinline__ double inv_length(double ss) { return ss > 0.0 ? 1.0 / sqrt(ss) : 0.0; }
__device__ __forceinline__ float4 scale4(float4 v, double inv) {
    return make_float4((float)(v.x * inv), (float)(v.y * inv), (float)(v.z * inv), (float)(v.w * inv));
}

// One row -> its unit row, by one wave (lane = 0 .. 63): 16-byte loads, the sum of squares added across the wave's lanes.  The
// unit_rows_kernel of trial_ranks.hip and of cohort_stats.hip are a wave per row around it.
__device__ __forceinline__ void unit_row(const float* __restrict__ src, float* __restrict__ dst, int D, int lane) {
    double ss = 0.0;
    for (int k = lane * 4; k < D; k += 256) ss += sum_sq(*reinterpret_cast<const float4*>(src + k));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const double inv = inv_length(ss);
    for (int k = lane * 4; k < D; k += 256) *reinterpret_cast<float4*>(dst + k) = scale4(*reinterpret_cast<const float4*>(src + k), inv);
}

// Rows first .. first + 31 of x (n rows of D floats) -> qs [Dp][32], Dp = D rounded up to 8: eight threads per column, 16-byte loads;
// the columns past n and the k past D are zero.  NORMALISE: the rows are raw and leave as unit rows (the eight threads' partial sums
// of squares in float64, added across the threads by xor 1, 2, 4).  All 256 threads call it; the caller's barrier follows.
template <bool NORMALISE>
__device__ __forceinline__ void load_tile(float* qs, const float* __restrict__ x, int first, int n, int D) {
    const int j = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const bool qv = first + j < n;
    const float* src = x + (size_t)(qv ? first + j : 0) * D;
    double inv = 0.0;
    if (NORMALISE) {
        double ss = 0.0;
        for (int kk = sub * 4; kk < D; kk += 32) ss += sum_sq(*reinterpret_cast<const float4*>(src + kk));
        ss += __shfl_xor(ss, 1);
        ss += __shfl_xor(ss, 2);
        ss += __shfl_xor(ss, 4);
        inv = inv_length(ss);
    }
    for (int kk = sub * 4; kk < D; kk += 32) {
        float4 v = *reinterpret_cast<const float4*>(src + kk);
        if (NORMALISE) v = scale4(v, inv);
        qs[(kk + 0) * COLS + j] = qv ? v.x : 0.f;
        qs[(kk + 1) * COLS + j] = qv ? v.y : 0.f;
        qs[(kk + 2) * COLS + j] = qv ? v.z : 0.f;
        qs[(kk + 3) * COLS + j] = qv ? v.w : 0.f;
    }
    if (sub == 0)
        for (int kk = D; kk < ((D + 7) & ~7); ++kk) qs[kk * COLS + j] = 0.f;
}

// Eight consecutive k of the wave's 32 rows x the tile's 32 columns.  In: lane (c, half) holds k0 + 4 half + {0, 1, 2, 3} of its row in
// v; the two swaps leave (k0, k0 + 1), (k0 + 2, k0 + 3), (k0 + 4, k0 + 5), (k0 + 6, k0 + 7) on (lower half, upper half) of x, z, y, w.
// FULL = false: the last four k of a D that is no multiple of 8 -- the upper half's v is zero and only x, z are used.
template <bool FULL>
__device__ __forceinline__ void mma_group(float4 v, const float* __restrict__ qb, int c, int half, f32x16& acc) {
    const auto xy = __builtin_amdgcn_permlane32_swap(__float_as_uint(v.x), __float_as_uint(v.y), false, false);
    const auto zw = __builtin_amdgcn_permlane32_swap(__float_as_uint(v.z), __float_as_uint(v.w), false, false);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(xy[0]), qb[(0 + half) * COLS + c], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(zw[0]), qb[(2 + half) * COLS + c], acc, 0, 0, 0);
    if (FULL) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(xy[1]), qb[(4 + half) * COLS + c], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(zw[1]), qb[(6 + half) * COLS + c], acc, 0, 0, 0);
    }
}

// The walk of workgroup `range` of the grid's y: its slabs range slabs_per_wg .. + slabs_per_wg - 1 of the n unit rows `rows`, against
// the tile qs.  Row: the caller's row index type.  Per slab, every wave that has rows calls use(r0, acc): r0 is the wave's first row
// (wave-uniform) and, in lane (c, half), acc[v] is the score of row r0 + 8 (v / 4) + 4 half + v % 4 against column c.  The wave's rows
// past n are computed from row n - 1: `use` must leave them out.
template <typename Row, typename Use>
__device__ __forceinline__ void walk(const float* qs, const float* __restrict__ rows, Row n, int D, int range, int slabs_per_wg, Use&& use) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 31, half = lane >> 5;
    const int ngroups = D >> 3;
    for (int sl = 0; sl < slabs_per_wg; ++sl) {
        const Row r0 = ((Row)range * slabs_per_wg + sl) * SLAB + w * 32;
        if (r0 >= n) break;                     // wave-uniform
        const Row row = r0 + c < n ? r0 + c : n - 1;
        const float* a = rows + (size_t)row * D + 4 * half;
        f32x16 acc;
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] = 0.f;
        int g = 0;
        for (; g + 8 <= ngroups; g += 8) {      // 8 loads (64 k of 32 rows) in flight per wave before the first product
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(a + (size_t)(g + u) * 8);
            __builtin_amdgcn_sched_barrier(0);  // keep the eight loads ahead of the products (the scheduler otherwise sinks them in pairs)
#pragma unroll
            for (int u = 0; u < 8; ++u) mma_group<true>(v[u], qs + (size_t)(g + u) * 8 * COLS, c, half, acc);
        }
        for (; g < ngroups; ++g) {
            const float4 v = *reinterpret_cast<const float4*>(a + (size_t)g * 8);
            mma_group<true>(v, qs + (size_t)g * 8 * COLS, c, half, acc);
        }
        if (D & 4) {                            // the upper half's four k lie past the row: not read
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (half == 0) v = *reinterpret_cast<const float4*>(a + (size_t)ngroups * 8);
            mma_group<false>(v, qs + (size_t)ngroups * 8 * COLS, c, half, acc);
        }
        use(r0, acc);
    }
}

}  // namespace cos_tile
