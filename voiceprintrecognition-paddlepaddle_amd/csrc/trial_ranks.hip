// EER / minDCF without the (Nt, Ne) score matrix (PPVectorTrainer.evaluate, trainer.py:416-431, and metric/metrics.py:4-37): the sorted
// target scores and, for every gap between two of them, HOW MANY non-target scores fall into it.  docs/trial_ranks.md has the method.
//
// vp_trial_ranks_targets_f32  unit_rows_kernel writes both sides as unit rows into the workspace (a wave per row, the length in float64:
//                             one rounding per element, the arithmetic of gallery.hip); then the targets pass.
// trial_pass_kernel<MODE>     gallery_score_kernel's tile walk: a workgroup holds 32 unit trial rows in LDS ([k][trial], the B operand of
//                             v_mfma_f32_32x32x2_f32) and walks `slabs_per_wg` slabs of 128 enrol rows, a wave per 32 rows, the 32 x 32
//                             scores in one accumulator over ALL of D.  A score is one k-ordered fma chain whatever the tile, the wave,
//                             the grid or the row's position: bit-identical rows give bit-identical scores, in every pass.
//                             The passes differ in what a lane does with its 16 scores:
//   TARGETS  a pair with equal labels writes its score to targets[trial_offset[i] + enroll_rank[j]]: a place the labels alone fix.
//   COUNTS   a pair with different labels finds its bin #{j : t[j] < s} in the sorted targets -- all of them in LDS when they fit,
//            else `P` pivots (every stride-th target) in LDS and the `stride` targets between two pivots from global memory -- and
//            adds one to the workgroup's LDS count of that bin (bins past the LDS window: one global integer atomic each).  The
//            workgroup adds its non-zero counts to the 64-bit global histogram when its walk ends.
//   SELECT   a pair with different labels and lo < s <= hi whose order-preserving key agrees with `prefix` above the digit in hand
//            counts that digit (11, 11 and 10 bits: an LDS histogram of 2048 counters; 65 536 would not fit beside the tile).
// Integer counts only: no float atomics, no grid barrier, no spinning; the result does not depend on arrival order.
#include "common.h"

#include <math.h>

namespace {

constexpr int SLAB = 128;               // 4 waves x 32 rows
constexpr int QT = 32;                  // trials of a tile = the matrix core's N
constexpr int MAX_D = 1024;
constexpr long long MAX_NT = 1LL << 24;
constexpr int MAX_LDS = 160 * 1024;
constexpr int PIVOTS = 2048;            // two-level search: at most this many pivots in LDS
constexpr int DIGIT_BINS = 2048;
constexpr int MAX_SLABS_PER_WG = 1 << 16;       // 32 x 128 x 2^16 = 2^28 pairs per workgroup: a 32-bit LDS count cannot wrap

enum { TARGETS = 0, COUNTS = 1, SELECT = 2 };

typedef __attribute__((ext_vector_type(16))) float f32x16;

bool supported(int Nt, int Ne, int D, long long NT) {
    return Nt >= 1 && Ne >= 1 && D >= 4 && D % 4 == 0 && D <= MAX_D && NT >= 1 && NT <= MAX_NT;
}

struct Plan {
    int qtiles, slabs_per_wg, ranges;
    int P, stride, H;                   // COUNTS: pivots in LDS, targets per pivot, bins of the LDS window
    size_t tile_lds, count_lds, unit_t, bytes;      // unit trial rows at ws + 0, unit enrol rows at ws + unit_t
};

Plan plan(int Nt, int Ne, int D, long long NT) {
    Plan p{};
    p.qtiles = (Nt + QT - 1) / QT;
    const int slabs = (Ne + SLAB - 1) / SLAB;
    // about a thousand workgroups where the shape has them; a workgroup walks at least two slabs (its tile is loaded once)
    const int want = (1024 + p.qtiles - 1) / p.qtiles;
    int spw = (slabs + want - 1) / want;
    const int least = slabs < 2 ? slabs : 2, by_grid = (slabs + 65534) / 65535;
    spw = spw > least ? spw : least;
    spw = spw > by_grid ? spw : by_grid;
    spw = spw < MAX_SLABS_PER_WG ? spw : MAX_SLABS_PER_WG;
    p.slabs_per_wg = spw;
    p.ranges = (slabs + spw - 1) / spw;
    const int Dp = (D + 7) / 8 * 8;
    p.tile_lds = (size_t)Dp * QT * 4;
    const size_t room = (MAX_LDS - p.tile_lds) / 4;         // words beside the tile: >= 8192
    if ((size_t)(2 * NT + 1) <= room) {
        p.stride = 1;
        p.P = (int)NT;
        p.H = (int)NT + 1;
    } else {
        p.stride = (int)((NT + PIVOTS - 1) / PIVOTS);
        p.P = (int)((NT + p.stride - 1) / p.stride);
        const size_t h = room - p.P;
        p.H = (size_t)(NT + 1) < h ? (int)(NT + 1) : (int)h;
    }
    p.count_lds = p.tile_lds + ((size_t)p.P + p.H) * 4;
    p.unit_t = vp_align_up((size_t)Nt * D * 4, 256);
    p.bytes = p.unit_t + vp_align_up((size_t)Ne * D * 4, 256);
    return p;
}

// ------------------------------------------------------------------------------------------------ unit rows
// A wave per row, 16-byte loads.  The length in float64, 1 / sqrt exactly rounded: a unit row is rounded once per element; a zero row
// stays zero.
__global__ __launch_bounds__(256) void unit_rows_kernel(const float* __restrict__ x, long long rows, int D, float* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;              // wave-uniform
    const float* src = x + (size_t)r * D;
    float* dst = y + (size_t)r * D;
    double ss = 0.0;
    for (int k = lane * 4; k < D; k += 256) {
        const float4 v = *reinterpret_cast<const float4*>(src + k);
        ss += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const double inv = ss > 0.0 ? 1.0 / sqrt(ss) : 0.0;
    for (int k = lane * 4; k < D; k += 256) {
        const float4 v = *reinterpret_cast<const float4*>(src + k);
        *reinterpret_cast<float4*>(dst + k) = make_float4((float)(v.x * inv), (float)(v.y * inv), (float)(v.z * inv), (float)(v.w * inv));
    }
}

// ------------------------------------------------------------------------------------------------ the tile walk
struct PassArgs {
    const float* tu;                    // (Nt, D) unit trial rows
    const float* eu;                    // (Ne, D) unit enrol rows
    const int* tl;                      // (Nt) labels
    const int* el;                      // (Ne)
    int Nt, Ne, D, slabs_per_wg;
    int NT;
    // TARGETS
    const long long* toff;              // (Nt) the first place of trial i's targets
    const int* erank;                   // (Ne) the rank of enrol row j among the rows of its label
    float* targets;                     // (NT)
    // COUNTS
    const float* st;                    // (NT) the targets, ascending
    int P, stride, H;
    // SELECT
    float lo, hi;                       // lo < s <= hi
    unsigned prefix, prefix_mask;       // (key & prefix_mask) == prefix
    int shift;
    unsigned digit_mask;
    // COUNTS: (NT + 1) bins; SELECT: DIGIT_BINS
    unsigned long long* hist;
};

// Eight consecutive k of the wave's 32 rows x the tile's 32 trials (gallery.hip's mma_group: lane (c, half) holds k0 + 4 half + {0..3}
// of its row in v; the swaps leave (k0, k0 + 1), (k0 + 2, k0 + 3), (k0 + 4, k0 + 5), (k0 + 6, k0 + 7) on the two halves of x, z, y, w).
template <bool FULL>
__device__ __forceinline__ void mma_group(float4 v, const float* __restrict__ qb, int c, int half, f32x16& acc) {
    const auto xy = __builtin_amdgcn_permlane32_swap(__float_as_uint(v.x), __float_as_uint(v.y), false, false);
    const auto zw = __builtin_amdgcn_permlane32_swap(__float_as_uint(v.z), __float_as_uint(v.w), false, false);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(xy[0]), qb[(0 + half) * QT + c], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(zw[0]), qb[(2 + half) * QT + c], acc, 0, 0, 0);
    if (FULL) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(xy[1]), qb[(4 + half) * QT + c], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(zw[1]), qb[(6 + half) * QT + c], acc, 0, 0, 0);
    }
}

// #{i < n : a[i] < s}, a ascending
__device__ __forceinline__ int count_below(const float* a, int n, float s) {
    int lo = 0;
    while (n > 0) {
        const int h = n >> 1;
        if (a[lo + h] < s) { lo += h + 1; n -= h + 1; } else n = h;
    }
    return lo;
}

// a float's bits as an unsigned that orders as the float does
__device__ __forceinline__ unsigned order_key(float s) {
    const unsigned u = __float_as_uint(s);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

// grid (trial tiles, row ranges), 256 threads, dynamic LDS: qs [Dp][32] | COUNTS: pivots [P], counts [H] | SELECT: counts [DIGIT_BINS]
template <int MODE>
__global__ __launch_bounds__(256) void trial_pass_kernel(const PassArgs a) {
    extern __shared__ __align__(16) float smem[];
    const int D = a.D, Dp = (D + 7) & ~7;
    float* qs = smem;
    float* piv = smem + (size_t)Dp * QT;
    unsigned* cnt = reinterpret_cast<unsigned*>(piv + (MODE == COUNTS ? a.P : 0));
    const int nbins = MODE == COUNTS ? a.H : (MODE == SELECT ? DIGIT_BINS : 0);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, half = lane >> 5;
    const int qt = blockIdx.x, range = blockIdx.y;

    {   // the trial tile: eight threads per trial, 16-byte loads; trials past Nt and the k past D are zero
        const int j = tid >> 3, sub = tid & 7;
        const int q = qt * QT + j;
        const bool qv = q < a.Nt;
        const float* src = a.tu + (size_t)(qv ? q : 0) * D;
        for (int kk = sub * 4; kk < D; kk += 32) {
            const float4 v = *reinterpret_cast<const float4*>(src + kk);
            qs[(kk + 0) * QT + j] = qv ? v.x : 0.f;
            qs[(kk + 1) * QT + j] = qv ? v.y : 0.f;
            qs[(kk + 2) * QT + j] = qv ? v.z : 0.f;
            qs[(kk + 3) * QT + j] = qv ? v.w : 0.f;
        }
        if (sub == 0)
            for (int kk = D; kk < Dp; ++kk) qs[kk * QT + j] = 0.f;
        if (MODE == COUNTS)
            for (int i = tid; i < a.P; i += 256) piv[i] = a.st[(size_t)i * a.stride];       // i stride < NT: P = ceil(NT / stride)
        for (int i = tid; i < nbins; i += 256) cnt[i] = 0u;
    }
    __syncthreads();

    const int q = qt * QT + c;
    const bool my_q = q < a.Nt;         // the tile's columns past Nt are zero trials: nothing is kept for them
    const int lq = my_q ? a.tl[q] : 0;
    long long off = 0;
    if (MODE == TARGETS && my_q) off = a.toff[q];
    const int ngroups = D >> 3;
    for (int sl = 0; sl < a.slabs_per_wg; ++sl) {
        const long long r0 = ((long long)range * a.slabs_per_wg + sl) * SLAB + w * 32;
        if (r0 >= a.Ne) break;          // wave-uniform
        const long long row = r0 + c < a.Ne ? r0 + c : a.Ne - 1;    // rows past Ne are computed from row Ne - 1 and never used
        const float* e = a.eu + (size_t)row * D + 4 * half;
        f32x16 acc;
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] = 0.f;
        int g = 0;
        for (; g + 8 <= ngroups; g += 8) {      // 8 loads (64 k of 32 rows) in flight per wave before the first product
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(e + (size_t)(g + u) * 8);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 8; ++u) mma_group<true>(v[u], qs + (size_t)(g + u) * 8 * QT, c, half, acc);
        }
        for (; g < ngroups; ++g) {
            const float4 v = *reinterpret_cast<const float4*>(e + (size_t)g * 8);
            mma_group<true>(v, qs + (size_t)g * 8 * QT, c, half, acc);
        }
        if (D & 4) {                            // the upper half's four k lie past the row: not read
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (half == 0) v = *reinterpret_cast<const float4*>(e + (size_t)ngroups * 8);
            mma_group<false>(v, qs + (size_t)ngroups * 8 * QT, c, half, acc);
        }
        // acc[v] = score of enrol row r0 + 8 (v / 4) + 4 half + v % 4 against trial c
        const long long rb = r0 + 4 * half;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const long long r = rb + 8 * (v >> 2) + (v & 3);
            if (!my_q || r >= a.Ne) continue;
            const bool same = a.el[r] == lq;
            const float s = acc[v];
            if (MODE == TARGETS) {
                if (!same) continue;
                const long long at = off + a.erank[r];
                if (at >= 0 && at < a.NT) a.targets[at] = s;        // labels that disagree with the offsets write nowhere
            } else if (MODE == COUNTS) {
                if (same) continue;
                const int m = count_below(piv, a.P, s);
                int bin = m;
                if (a.stride > 1 && m > 0) {    // st[(m - 1) stride] < s, and s <= st[m stride] where that exists
                    const int base = (m - 1) * a.stride + 1;
                    const long long end = (long long)m * a.stride < a.NT ? m * a.stride : a.NT;
                    bin = base + count_below(a.st + base, (int)(end - base), s);
                }
                if (bin < a.H) atomicAdd(&cnt[bin], 1u);
                else atomicAdd(&a.hist[bin], 1ull);
            } else {
                if (same || !(s > a.lo && s <= a.hi)) continue;
                const unsigned key = order_key(s);
                if ((key & a.prefix_mask) == a.prefix) atomicAdd(&cnt[(key >> a.shift) & a.digit_mask], 1u);
            }
        }
    }
    if (MODE != TARGETS) {
        __syncthreads();
        for (int b = tid; b < nbins; b += 256) {
            const unsigned n = cnt[b];
            if (n) atomicAdd(&a.hist[b], (unsigned long long)n);
        }
    }
}

template <int MODE>
int launch(vp_ctx* ctx, const PassArgs& a, const Plan& p, size_t lds, hipStream_t st, const char* name) {
    static bool attr_dev[64] = {};              // the attribute is per device (and per instantiation)
    bool& attr_set = attr_dev[ctx->device & 63];
    if (!attr_set) {
        VP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(trial_pass_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        MAX_LDS));
        attr_set = true;
    }
    hipLaunchKernelGGL(trial_pass_kernel<MODE>, dim3(p.qtiles, p.ranges), dim3(256), lds, st, a);
    VP_LAUNCH_CHECK(ctx, name);
    return VP_OK;
}

PassArgs common_args(const Plan& p, const void* ws, const int* tl, int Nt, const int* el, int Ne, int D, long long NT) {
    PassArgs a{};
    a.tu = (const float*)ws;
    a.eu = (const float*)((const char*)ws + p.unit_t);
    a.tl = tl;
    a.el = el;
    a.Nt = Nt;
    a.Ne = Ne;
    a.D = D;
    a.slabs_per_wg = p.slabs_per_wg;
    a.NT = (int)NT;
    return a;
}

#define TRIAL_UNSUP(ctx, what) \
    VP_FAIL(ctx, VP_EUNSUP, what ": Nt, Ne >= 1, D %% 4 == 0, D <= %d, 1 <= NT <= %lld", MAX_D, MAX_NT)

}  // namespace

extern "C" {

size_t vp_trial_ranks_workspace_bytes(int Nt, int Ne, int D, long long NT) {
    return supported(Nt, Ne, D, NT) ? plan(Nt, Ne, D, NT).bytes : 0;
}

int vp_trial_ranks_targets_f32(vp_ctx* ctx, const float* trials, const int* trial_labels, const long long* trial_offsets, int Nt,
                               const float* enroll, const int* enroll_labels, const int* enroll_ranks, int Ne, int D, long long NT,
                               float* targets, void* ws, size_t ws_bytes, vp_stream stream) {
    if (!supported(Nt, Ne, D, NT)) TRIAL_UNSUP(ctx, "trial_ranks_targets");       // first, and without a context: needs no device
    if (!ctx || !trials || !trial_labels || !trial_offsets || !enroll || !enroll_labels || !enroll_ranks || !targets || !ws)
        VP_FAIL(ctx, VP_EINVAL, "trial_ranks_targets: null pointer");
    const Plan p = plan(Nt, Ne, D, NT);
    if (ws_bytes < p.bytes) VP_FAIL(ctx, VP_EWORKSPACE, "trial_ranks_targets: workspace %zu < %zu bytes", ws_bytes, p.bytes);
    hipStream_t st = (hipStream_t)stream;
    PassArgs a = common_args(p, ws, trial_labels, Nt, enroll_labels, Ne, D, NT);
    hipLaunchKernelGGL(unit_rows_kernel, dim3((Nt + 3) / 4), dim3(256), 0, st, trials, (long long)Nt, D, (float*)ws);
    VP_LAUNCH_CHECK(ctx, "unit_rows_kernel");
    hipLaunchKernelGGL(unit_rows_kernel, dim3((Ne + 3) / 4), dim3(256), 0, st, enroll, (long long)Ne, D, (float*)((char*)ws + p.unit_t));
    VP_LAUNCH_CHECK(ctx, "unit_rows_kernel");
    a.toff = trial_offsets;
    a.erank = enroll_ranks;
    a.targets = targets;
    return launch<TARGETS>(ctx, a, p, p.tile_lds, st, "trial_pass_kernel<targets>");
}

int vp_trial_ranks_counts_f32(vp_ctx* ctx, const int* trial_labels, int Nt, const int* enroll_labels, int Ne, int D,
                              const float* sorted_targets, long long NT, long long* hist, const void* ws, size_t ws_bytes,
                              vp_stream stream) {
    if (!supported(Nt, Ne, D, NT)) TRIAL_UNSUP(ctx, "trial_ranks_counts");
    if (!ctx || !trial_labels || !enroll_labels || !sorted_targets || !hist || !ws)
        VP_FAIL(ctx, VP_EINVAL, "trial_ranks_counts: null pointer");
    const Plan p = plan(Nt, Ne, D, NT);
    if (ws_bytes < p.bytes) VP_FAIL(ctx, VP_EWORKSPACE, "trial_ranks_counts: workspace %zu < %zu bytes", ws_bytes, p.bytes);
    hipStream_t st = (hipStream_t)stream;
    PassArgs a = common_args(p, ws, trial_labels, Nt, enroll_labels, Ne, D, NT);
    a.st = sorted_targets;
    a.P = p.P;
    a.stride = p.stride;
    a.H = p.H;
    a.hist = reinterpret_cast<unsigned long long*>(hist);
    VP_HIP(ctx, hipMemsetAsync(hist, 0, (size_t)(NT + 1) * 8, st));
    return launch<COUNTS>(ctx, a, p, p.count_lds, st, "trial_pass_kernel<counts>");
}

int vp_trial_ranks_select_f32(vp_ctx* ctx, const int* trial_labels, int Nt, const int* enroll_labels, int Ne, int D, long long NT,
                              float lo, float hi, int level, long long prefix, long long* digits, const void* ws, size_t ws_bytes,
                              vp_stream stream) {
    if (!supported(Nt, Ne, D, NT)) TRIAL_UNSUP(ctx, "trial_ranks_select");
    if (!ctx || !trial_labels || !enroll_labels || !digits || !ws) VP_FAIL(ctx, VP_EINVAL, "trial_ranks_select: null pointer");
    if (level < 0 || level > 2 || prefix < 0 || prefix > 0xffffffffLL) VP_FAIL(ctx, VP_EINVAL, "trial_ranks_select: level, prefix");
    const Plan p = plan(Nt, Ne, D, NT);
    if (ws_bytes < p.bytes) VP_FAIL(ctx, VP_EWORKSPACE, "trial_ranks_select: workspace %zu < %zu bytes", ws_bytes, p.bytes);
    hipStream_t st = (hipStream_t)stream;
    PassArgs a = common_args(p, ws, trial_labels, Nt, enroll_labels, Ne, D, NT);
    static const int shifts[3] = {21, 10, 0};
    static const unsigned masks[3] = {0u, 0xffe00000u, 0xfffffc00u}, digit_masks[3] = {2047u, 2047u, 1023u};
    a.lo = lo;
    a.hi = hi;
    a.shift = shifts[level];
    a.prefix_mask = masks[level];
    a.prefix = (unsigned)prefix & masks[level];
    a.digit_mask = digit_masks[level];
    a.hist = reinterpret_cast<unsigned long long*>(digits);
    VP_HIP(ctx, hipMemsetAsync(digits, 0, (size_t)DIGIT_BINS * 8, st));
    return launch<SELECT>(ctx, a, p, p.tile_lds + DIGIT_BINS * 4, st, "trial_pass_kernel<select>");
}

}  // extern "C"
