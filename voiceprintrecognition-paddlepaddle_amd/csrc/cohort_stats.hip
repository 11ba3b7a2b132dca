// Adaptive score normalisation (AS-norm): for every embedding the mean and the standard deviation of its N largest cosines against
// a cohort, without the (Q, C) score matrix.  No reference call site: an extension (docs/score_norm.md has the method and the contract).
//
// vp_cohort_stats_f32      unit_rows_kernel writes the cohort as unit rows into the workspace (a wave per row); then
// cohort_stats_kernel      one workgroup per tile of 32 embeddings, which it holds as unit rows in LDS.  It walks the WHOLE unit cohort
//                          with cos_tile.h's walk once per digit of a radix selection on vp_order_key(score), per column: the walk gives
//                          a pair the same bits every time, so the workgroup counts a digit into its own LDS histograms
//                          [digit][column], picks the digit that holds the N-th largest score of each column, and walks again for the
//                          next one -- no host round trip, no global histogram, nothing of size Q C anywhere.  Digits are 8 bits wide
//                          (four selection walks) where 32 x 256 counters fit beside the tile, else 7 bits (five walks; D >= 1020).
//                          A last walk adds (double)s and (double)s s of the scores above the N-th largest; the N-th largest itself
//                          enters N - #above times, so ties at the N-th place need no rule.
// Integer counts in LDS, float64 sums per lane in walk order, then lane halves, then the four waves in order: no float atomics, no
// dependence on arrival order, no grid barrier, no spinning; two runs give the same bits.
// vp_cohort_stats_split_f32  the same statistics for few rows, the cohort split over workgroups (below, in front of its kernels);
// vp_unit_rows_f32         unit_rows_kernel on its own, for the caller that keeps the unit cohort.
// vp_score_norm_recip_f32  r = 1 / max(std, floor);  vp_score_norm_apply_f32: z over an (Nt, Ne) cosine matrix in place -- the
//                          arithmetic of score_norm.h, which the normalised passes of trial_ranks.hip share.
#include "cos_tile.h"
#include "score_norm.h"

namespace {

using cos_tile::SLAB;
using cos_tile::MAX_D;
constexpr int QT = cos_tile::COLS;      // embeddings of a tile
constexpr int MAX_LDS = 160 * 1024;
constexpr int STATE_LDS = 2 * QT * 4;   // per column: the key's digits so far, and the rank that is left inside them

bool supported(int Q, int C, int D) { return Q >= 1 && C >= 1 && D >= 4 && D % 4 == 0 && D <= MAX_D; }

struct Plan {
    int qtiles, slabs, digit_bits;
    size_t lds, bytes;                  // the unit cohort at ws + 0
};

Plan plan(int Q, int C, int D) {
    Plan p{};
    p.qtiles = (Q + QT - 1) / QT;
    p.slabs = (C + SLAB - 1) / SLAB;
    const size_t tile = (size_t)((D + 7) / 8 * 8) * QT * 4;
    p.digit_bits = tile + STATE_LDS + (size_t)QT * 256 * 4 <= MAX_LDS ? 8 : 7;
    p.lds = tile + STATE_LDS + ((size_t)QT << p.digit_bits) * 4;
    p.bytes = vp_align_up((size_t)C * D * 4, 256);
    return p;
}

__global__ __launch_bounds__(256) void unit_rows_kernel(const float* __restrict__ x, long long rows, int D, float* __restrict__ y) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;              // wave-uniform
    cos_tile::unit_row(x + (size_t)r * D, y + (size_t)r * D, D, threadIdx.x & 63);
}

struct StatsArgs {
    const float* x;                     // (Q, D) raw rows
    const float* cu;                    // (C, D) unit cohort rows
    int Q, C, D, N;                     // N = min(top_n, C)
    int slabs, digit_bits;
    float* mean;                        // (Q)
    float* std;                         // (Q)
};

__device__ __forceinline__ float key_score(unsigned key) {      // vp_order_key's inverse
    return __uint_as_float(key >> 31 ? key ^ 0x80000000u : ~key);
}

// grid (tiles of 32 embeddings), 256 threads, dynamic LDS: qs [Dp][32] | prefix [32] | left [32] | counts [1 << digit_bits][32]
__global__ __launch_bounds__(256) void cohort_stats_kernel(const StatsArgs a) {
    extern __shared__ __align__(16) float smem[];
    const int D = a.D, Dp = (D + 7) & ~7, W = a.digit_bits;
    float* qs = smem;
    unsigned* prefix = reinterpret_cast<unsigned*>(smem + (size_t)Dp * QT);
    unsigned* left = prefix + QT;
    unsigned* cnt = left + QT;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, half = lane >> 5;
    const long long C = a.C;

    cos_tile::load_tile<true>(qs, a.x, blockIdx.x * QT, a.Q, D);
    if (tid < QT) {
        prefix[tid] = 0u;
        left[tid] = (unsigned)a.N;
    }
    // the N-th largest key of every column, digit by digit from the top: the candidates of a digit are the scores whose key agrees
    // with the column's prefix above it, and left[] is the rank wanted among them, counted from the largest
    for (int top = 32; top > 0;) {
        const int bits = W < top ? W : top, sh = top - bits, nb = 1 << bits;
        const unsigned above_mask = top == 32 ? 0u : ~0u << top;
        for (int i = tid; i < nb * QT; i += 256) cnt[i] = 0u;
        __syncthreads();                // and, the first time, the tile and the state
        const unsigned mine = prefix[c];
        cos_tile::walk<long long>(qs, a.cu, C, D, 0, a.slabs, [&](long long r0, const cos_tile::f32x16& acc) {
            const long long rb = r0 + 4 * half;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                if (rb + 8 * (v >> 2) + (v & 3) >= C) continue;
                const unsigned key = vp_order_key(acc[v]);
                if ((key & above_mask) == mine) atomicAdd(&cnt[((key >> sh) & (nb - 1)) * QT + c], 1u);
            }
        });
        __syncthreads();
        if (tid < QT) {                 // the first digit, from the largest down, at which the count reaches the rank
            const unsigned k = left[tid];
            unsigned seen = 0u, before = 0u, digit = 0u;
            bool found = false;
            for (int b = nb - 1; b >= 0; --b) {
                const unsigned n = cnt[b * QT + tid];
                if (!found && seen + n >= k) {
                    found = true;
                    digit = (unsigned)b;
                    before = seen;
                }
                seen += n;
            }
            prefix[tid] |= digit << sh;
            left[tid] = k - before;
        }
        __syncthreads();                // the scan has read the counts before the next digit zeroes them
        top = sh;
    }

    // prefix[] is the key of the N-th largest score, left[] = N - #{scores above it}
    const unsigned thr = prefix[c];
    double s1 = 0.0, s2 = 0.0;
    cos_tile::walk<long long>(qs, a.cu, C, D, 0, a.slabs, [&](long long r0, const cos_tile::f32x16& acc) {
        const long long rb = r0 + 4 * half;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            if (rb + 8 * (v >> 2) + (v & 3) >= C || vp_order_key(acc[v]) <= thr) continue;
            const double s = (double)acc[v];
            s1 += s;
            s2 += s * s;                // the square of an f32 is exact in float64
        }
    });
    s1 += __shfl_xor(s1, 32);
    s2 += __shfl_xor(s2, 32);
    double* part = reinterpret_cast<double*>(cnt);      // [wave][column][2]: the counts are done with
    if (half == 0) {
        part[(w * QT + c) * 2 + 0] = s1;
        part[(w * QT + c) * 2 + 1] = s2;
    }
    __syncthreads();
    const int q = blockIdx.x * QT + tid;
    if (tid < QT && q < a.Q) {
        double t1 = 0.0, t2 = 0.0;
        for (int i = 0; i < 4; ++i) {
            t1 += part[(i * QT + tid) * 2 + 0];
            t2 += part[(i * QT + tid) * 2 + 1];
        }
        const double t = (double)key_score(prefix[tid]), k = (double)left[tid];
        t1 += k * t;
        t2 += k * (t * t);
        float m, sd;
        score_norm::mean_std(t1, t2, a.N, m, sd);
        a.mean[q] = m;
        a.std[q] = sd;
    }
}

// ------------------------------------------------------------------------------------------------ the cohort split over workgroups
// vp_cohort_stats_split_f32: the same statistics for FEW rows (a search's queries), where one workgroup per tile leaves the chip idle.
// Grid (tiles of 32 rows, ranges): a workgroup walks SPLIT_SLABS-or-more slabs of the unit cohort, one launch per digit and one for the
// sums.  A digit's LDS histogram is added to the tile's global histogram of that pass (integer atomicAdd; one buffer per pass, all
// cleared by one memset in front).  The NEXT launch's prologue scans the finished histogram -- every workgroup of a tile finds the same
// (prefix, left) from the state the launch before it left in global memory, and the workgroup of range 0 leaves the new state for
// the launch after it (a buffer per pass: nobody reads what is being written).  The sum pass leaves (#above, sum, sum of squares) per
// (tile, range, column); the finalise kernel adds the ranges in ascending order.  No float atomics, no grid barrier, no spinning.
constexpr int SPLIT_SLABS = VP_COHORT_SPLIT_SLABS;
constexpr int SPLIT_MAX_RANGES = VP_COHORT_SPLIT_MAX_RANGES;
constexpr int SPLIT_MAX_Q = VP_COHORT_SPLIT_MAX_Q;

bool split_supported(int Q, int C, int D) { return supported(Q, C, D) && Q <= SPLIT_MAX_Q; }

struct SplitPlan {
    int qtiles, slabs_per_wg, ranges, digit_bits, passes;
    size_t lds, hist_words, hist_bytes, state_bytes, sums_bytes, above_bytes, bytes;     // hist_words: one (pass, tile) histogram
};

// ranges depends on C alone (vpmi.h states it): a row's statistics do not depend on the batch it came in
SplitPlan split_plan(int Q, int C, int D) {
    SplitPlan p{};
    const Plan u = plan(Q, C, D);
    p.qtiles = u.qtiles;
    p.digit_bits = u.digit_bits;
    p.lds = u.lds;
    p.passes = (32 + p.digit_bits - 1) / p.digit_bits;
    const int by_cap = (u.slabs + SPLIT_MAX_RANGES - 1) / SPLIT_MAX_RANGES;
    p.slabs_per_wg = by_cap > SPLIT_SLABS ? by_cap : SPLIT_SLABS;
    p.ranges = (u.slabs + p.slabs_per_wg - 1) / p.slabs_per_wg;
    p.hist_words = (size_t)QT << p.digit_bits;
    p.hist_bytes = (size_t)p.qtiles * p.passes * p.hist_words * 4;
    p.state_bytes = (size_t)p.qtiles * p.passes * 2 * QT * 4;
    p.sums_bytes = (size_t)p.qtiles * p.ranges * QT * 16;
    p.above_bytes = (size_t)p.qtiles * p.ranges * QT * 4;
    p.bytes = p.hist_bytes + p.state_bytes + p.sums_bytes + p.above_bytes;     // every part a multiple of 128 bytes
    return p;
}

struct SplitArgs {
    const float* x;                     // (Q, D) raw rows
    const float* cu;                    // (C, D) unit cohort rows
    int Q, C, D, N;                     // N = min(top_n, C)
    int slabs_per_wg, ranges, digit_bits, passes;
    int pass;                           // 0 .. passes - 1: count that digit; passes: the sums
    unsigned* hist;                     // [pass][tile][1 << digit_bits][32]
    unsigned* state;                    // [pass][tile][2][32]: prefix and left AFTER that pass
    double* sums;                       // [tile][range][32][2]
    unsigned* above;                    // [tile][range][32]
    float* mean;
    float* std;
};

// (prefix, left) after pass `done` from the state after the pass before it and the finished histogram of `done`, by all 256 threads:
// eight per column, each the total of an eighth of the digits; the one whose eighth holds the rank walks it from the largest digit down
// (cohort_stats_kernel's scan, cut in eight).  Leaves them in LDS; the caller's barrier follows.
__device__ __forceinline__ void split_pick(const SplitArgs& a, int done, int tile, unsigned* prefix, unsigned* left) {
    const int W = a.digit_bits, top = 32 - done * W, bits = W < top ? W : top, sh = top - bits, nb = 1 << bits;
    const int col = threadIdx.x >> 3, sub = threadIdx.x & 7, per = nb >> 3;        // nb is 256, 128 or 16
    const unsigned* h = a.hist + ((size_t)done * gridDim.x + tile) * ((size_t)QT << W);
    unsigned pre = 0u, k = (unsigned)a.N;
    if (done) {
        const unsigned* before = a.state + ((size_t)(done - 1) * gridDim.x + tile) * 2 * QT;
        pre = before[col];
        k = before[QT + col];
    }
    unsigned total = 0u;
    for (int d = sub * per; d < (sub + 1) * per; ++d) total += h[d * QT + col];
    unsigned higher = 0u;               // the counts of the eighths with larger digits
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const unsigned tj = __shfl(total, (threadIdx.x & 56) | j);
        higher += j > sub ? tj : 0u;
    }
    if (higher < k && k <= higher + total) {    // exactly one of the eight: k <= the number of candidates, always
        unsigned seen = higher;
        int d = (sub + 1) * per - 1;
        for (; d > sub * per; --d) {
            const unsigned n = h[d * QT + col];
            if (seen + n >= k) break;
            seen += n;
        }
        prefix[col] = pre | (unsigned)d << sh;
        left[col] = k - seen;
    }
}

// grid (tiles of 32 embeddings, ranges), 256 threads, dynamic LDS as cohort_stats_kernel's
__global__ __launch_bounds__(256) void cohort_split_pass_kernel(const SplitArgs a) {
    extern __shared__ __align__(16) float smem[];
    const int D = a.D, Dp = (D + 7) & ~7, W = a.digit_bits;
    float* qs = smem;
    unsigned* prefix = reinterpret_cast<unsigned*>(smem + (size_t)Dp * QT);
    unsigned* left = prefix + QT;
    unsigned* cnt = left + QT;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, half = lane >> 5;
    const int tile = blockIdx.x, range = blockIdx.y;
    const long long C = a.C;
    const bool sum_pass = a.pass == a.passes;

    cos_tile::load_tile<true>(qs, a.x, tile * QT, a.Q, D);
    if (a.pass == 0) {
        if (tid < QT) prefix[tid] = 0u;
    } else {
        split_pick(a, a.pass - 1, tile, prefix, left);
        __syncthreads();
        if (range == 0 && tid < 2 * QT) a.state[((size_t)(a.pass - 1) * gridDim.x + tile) * 2 * QT + tid] = prefix[tid];   // left follows
    }
    if (!sum_pass) {
        const int top = 32 - a.pass * W, bits = W < top ? W : top, sh = top - bits, nb = 1 << bits;
        const unsigned above_mask = top == 32 ? 0u : ~0u << top;
        for (int i = tid; i < nb * QT; i += 256) cnt[i] = 0u;
        __syncthreads();                // the tile, the prefix and the zeroed counts
        const unsigned mine = prefix[c];
        cos_tile::walk<long long>(qs, a.cu, C, D, range, a.slabs_per_wg, [&](long long r0, const cos_tile::f32x16& acc) {
            const long long rb = r0 + 4 * half;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                if (rb + 8 * (v >> 2) + (v & 3) >= C) continue;
                const unsigned key = vp_order_key(acc[v]);
                if ((key & above_mask) == mine) atomicAdd(&cnt[((key >> sh) & (nb - 1)) * QT + c], 1u);
            }
        });
        __syncthreads();
        unsigned* h = a.hist + ((size_t)a.pass * gridDim.x + tile) * ((size_t)QT << W);
        for (int i = tid; i < nb * QT; i += 256) {
            const unsigned n = cnt[i];
            if (n) atomicAdd(&h[i], n);
        }
        return;
    }
    __syncthreads();                    // the tile and the threshold keys
    const unsigned thr = prefix[c];
    double s1 = 0.0, s2 = 0.0;
    unsigned na = 0u;
    cos_tile::walk<long long>(qs, a.cu, C, D, range, a.slabs_per_wg, [&](long long r0, const cos_tile::f32x16& acc) {
        const long long rb = r0 + 4 * half;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            if (rb + 8 * (v >> 2) + (v & 3) >= C || vp_order_key(acc[v]) <= thr) continue;
            const double s = (double)acc[v];
            s1 += s;
            s2 += s * s;                // the square of an f32 is exact in float64
            ++na;
        }
    });
    s1 += __shfl_xor(s1, 32);
    s2 += __shfl_xor(s2, 32);
    na += __shfl_xor(na, 32);
    double* part = reinterpret_cast<double*>(cnt);      // [wave][column][2], then the counts [wave][column]
    unsigned* part_n = reinterpret_cast<unsigned*>(part + 4 * QT * 2);
    if (half == 0) {
        part[(w * QT + c) * 2 + 0] = s1;
        part[(w * QT + c) * 2 + 1] = s2;
        part_n[w * QT + c] = na;
    }
    __syncthreads();
    if (tid < QT) {
        double t1 = 0.0, t2 = 0.0;
        unsigned n = 0u;
        for (int i = 0; i < 4; ++i) {
            t1 += part[(i * QT + tid) * 2 + 0];
            t2 += part[(i * QT + tid) * 2 + 1];
            n += part_n[i * QT + tid];
        }
        const size_t at = ((size_t)tile * a.ranges + range) * QT + tid;
        a.sums[at * 2 + 0] = t1;
        a.sums[at * 2 + 1] = t2;
        a.above[at] = n;
    }
}

// a thread per row: the ranges in ascending order, the threshold score N - #above times, the float64 tail
__global__ __launch_bounds__(256) void cohort_split_finalise_kernel(const SplitArgs a) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= a.Q) return;
    const int tile = q / QT, col = q % QT, tiles = (a.Q + QT - 1) / QT;
    double t1 = 0.0, t2 = 0.0;
    unsigned n = 0u;
    for (int r = 0; r < a.ranges; ++r) {
        const size_t at = ((size_t)tile * a.ranges + r) * QT + col;
        t1 += a.sums[at * 2 + 0];
        t2 += a.sums[at * 2 + 1];
        n += a.above[at];
    }
    const unsigned thr = a.state[((size_t)(a.passes - 1) * tiles + tile) * 2 * QT + col];
    const double t = (double)key_score(thr), k = (double)((unsigned)a.N - n);
    t1 += k * t;
    t2 += k * (t * t);
    float m, sd;
    score_norm::mean_std(t1, t2, a.N, m, sd);
    a.mean[q] = m;
    a.std[q] = sd;
}

__global__ __launch_bounds__(256) void recip_std_kernel(const float* __restrict__ std, long long n, float* __restrict__ r) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        r[i] = score_norm::recip_std(std[i]);
}

// grid (column blocks, rows), both strided
__global__ __launch_bounds__(256) void score_norm_apply_kernel(float* __restrict__ s, int Nt, int Ne, const float* __restrict__ tmean,
                                                               const float* __restrict__ tr, const float* __restrict__ emean,
                                                               const float* __restrict__ er) {
    for (int i = blockIdx.y; i < Nt; i += gridDim.y) {
        const float mt = tmean[i], rt = tr[i];
        float* row = s + (size_t)i * Ne;
        for (int j = blockIdx.x * 256 + threadIdx.x; j < Ne; j += gridDim.x * 256) row[j] = score_norm::z(row[j], emean[j], er[j], mt, rt);
    }
}

}  // namespace

extern "C" {

size_t vp_cohort_stats_workspace_bytes(int Q, int C, int D) { return supported(Q, C, D) ? plan(Q, C, D).bytes : 0; }

int vp_cohort_stats_f32(vp_ctx* ctx, const float* x, int Q, const float* cohort, int C, int D, int top_n, float* mean, float* std,
                        void* ws, size_t ws_bytes, vp_stream stream) {
    if (!supported(Q, C, D) || top_n < 1)       // first, and without a context: needs no device
        VP_FAIL(ctx, VP_EUNSUP, "cohort_stats: Q, C, top_n >= 1, D %% 4 == 0, D <= %d", MAX_D);
    if (!ctx || !x || !cohort || !mean || !std || !ws) VP_FAIL(ctx, VP_EINVAL, "cohort_stats: null pointer");
    const Plan p = plan(Q, C, D);
    if (ws_bytes < p.bytes) VP_FAIL(ctx, VP_EWORKSPACE, "cohort_stats: workspace %zu < %zu bytes", ws_bytes, p.bytes);
    hipStream_t st = (hipStream_t)stream;
    static bool attr_dev[64] = {};              // the attribute is per device
    bool& attr_set = attr_dev[ctx->device & 63];
    if (!attr_set) {
        VP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(cohort_stats_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        MAX_LDS));
        attr_set = true;
    }
    hipLaunchKernelGGL(unit_rows_kernel, dim3((C + 3) / 4), dim3(256), 0, st, cohort, (long long)C, D, (float*)ws);
    VP_LAUNCH_CHECK(ctx, "unit_rows_kernel");
    StatsArgs a{};
    a.x = x;
    a.cu = (const float*)ws;
    a.Q = Q;
    a.C = C;
    a.D = D;
    a.N = top_n < C ? top_n : C;
    a.slabs = p.slabs;
    a.digit_bits = p.digit_bits;
    a.mean = mean;
    a.std = std;
    hipLaunchKernelGGL(cohort_stats_kernel, dim3(p.qtiles), dim3(256), p.lds, st, a);
    VP_LAUNCH_CHECK(ctx, "cohort_stats_kernel");
    return VP_OK;
}

int vp_unit_rows_f32(vp_ctx* ctx, const float* x, long long rows, int D, float* y, vp_stream stream) {
    if (rows < 1 || D < 4 || D % 4 != 0 || D > MAX_D || (rows + 3) / 4 > 0x7fffffffLL)
        VP_FAIL(ctx, VP_EUNSUP, "unit_rows: rows >= 1, D %% 4 == 0, D <= %d", MAX_D);
    if (!ctx || !x || !y) VP_FAIL(ctx, VP_EINVAL, "unit_rows: null pointer");
    hipLaunchKernelGGL(unit_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, rows, D, y);
    VP_LAUNCH_CHECK(ctx, "unit_rows_kernel");
    return VP_OK;
}

size_t vp_cohort_stats_split_workspace_bytes(int Q, int C, int D) { return split_supported(Q, C, D) ? split_plan(Q, C, D).bytes : 0; }

int vp_cohort_stats_split_f32(vp_ctx* ctx, const float* x, int Q, const float* cohort_unit, int C, int D, int top_n, float* mean,
                              float* std, void* ws, size_t ws_bytes, vp_stream stream) {
    if (!split_supported(Q, C, D) || top_n < 1)         // first, and without a context: needs no device
        VP_FAIL(ctx, VP_EUNSUP, "cohort_stats_split: 1 <= Q <= %d, C, top_n >= 1, D %% 4 == 0, D <= %d", SPLIT_MAX_Q, MAX_D);
    if (!ctx || !x || !cohort_unit || !mean || !std || !ws) VP_FAIL(ctx, VP_EINVAL, "cohort_stats_split: null pointer");
    const SplitPlan p = split_plan(Q, C, D);
    if (ws_bytes < p.bytes) VP_FAIL(ctx, VP_EWORKSPACE, "cohort_stats_split: workspace %zu < %zu bytes", ws_bytes, p.bytes);
    hipStream_t st = (hipStream_t)stream;
    static bool attr_dev[64] = {};              // the attribute is per device
    bool& attr_set = attr_dev[ctx->device & 63];
    if (!attr_set) {
        VP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(cohort_split_pass_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, MAX_LDS));
        attr_set = true;
    }
    SplitArgs a{};
    a.x = x;
    a.cu = cohort_unit;
    a.Q = Q;
    a.C = C;
    a.D = D;
    a.N = top_n < C ? top_n : C;
    a.slabs_per_wg = p.slabs_per_wg;
    a.ranges = p.ranges;
    a.digit_bits = p.digit_bits;
    a.passes = p.passes;
    a.hist = (unsigned*)ws;
    a.state = (unsigned*)((char*)ws + p.hist_bytes);
    a.sums = (double*)((char*)ws + p.hist_bytes + p.state_bytes);
    a.above = (unsigned*)((char*)ws + p.hist_bytes + p.state_bytes + p.sums_bytes);
    a.mean = mean;
    a.std = std;
    VP_HIP(ctx, hipMemsetAsync(a.hist, 0, p.hist_bytes, st));          // every pass's histograms, once
    for (a.pass = 0; a.pass <= p.passes; ++a.pass) {                    // the digits, then the sums
        hipLaunchKernelGGL(cohort_split_pass_kernel, dim3(p.qtiles, p.ranges), dim3(256), p.lds, st, a);
        VP_LAUNCH_CHECK(ctx, "cohort_split_pass_kernel");
    }
    hipLaunchKernelGGL(cohort_split_finalise_kernel, dim3((Q + 255) / 256), dim3(256), 0, st, a);
    VP_LAUNCH_CHECK(ctx, "cohort_split_finalise_kernel");
    return VP_OK;
}

int vp_score_norm_recip_f32(vp_ctx* ctx, const float* std, long long n, float* r, vp_stream stream) {
    if (n < 1) VP_FAIL(ctx, VP_EUNSUP, "score_norm_recip: n >= 1");
    if (!ctx || !std || !r) VP_FAIL(ctx, VP_EINVAL, "score_norm_recip: null pointer");
    hipLaunchKernelGGL(recip_std_kernel, dim3(grid1d(n)), dim3(256), 0, (hipStream_t)stream, std, n, r);
    VP_LAUNCH_CHECK(ctx, "recip_std_kernel");
    return VP_OK;
}

int vp_score_norm_apply_f32(vp_ctx* ctx, float* scores, int Nt, int Ne, const float* trial_mean, const float* trial_r,
                            const float* enroll_mean, const float* enroll_r, vp_stream stream) {
    if (Nt < 1 || Ne < 1) VP_FAIL(ctx, VP_EUNSUP, "score_norm_apply: Nt, Ne >= 1");
    if (!ctx || !scores || !trial_mean || !trial_r || !enroll_mean || !enroll_r) VP_FAIL(ctx, VP_EINVAL, "score_norm_apply: null pointer");
    const int gx = (Ne + 255) / 256;
    hipLaunchKernelGGL(score_norm_apply_kernel, dim3(gx < 64 ? gx : 64, Nt < 65535 ? Nt : 65535), dim3(256), 0, (hipStream_t)stream,
                       scores, Nt, Ne, trial_mean, trial_r, enroll_mean, enroll_r);
    VP_LAUNCH_CHECK(ctx, "score_norm_apply_kernel");
    return VP_OK;
}

}  // extern "C"
