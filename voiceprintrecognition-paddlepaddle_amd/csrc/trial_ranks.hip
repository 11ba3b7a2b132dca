// EER / minDCF without the (Nt, Ne) score matrix (PPVectorTrainer.evaluate, trainer.py:416-431, and metric/metrics.py:4-37): the sorted
// target scores and, for every gap between two of them, HOW MANY non-target scores fall into it.  docs/trial_ranks.md has the method.
//
// vp_trial_ranks_targets_f32  unit_rows_kernel writes both sides as unit rows into the workspace (a wave per row); then the targets pass.
// trial_pass_kernel<MODE, NORM>  a workgroup holds 32 unit trial rows in LDS and walks `slabs_per_wg` slabs of enrol rows with cos_tile.h's
//                             walk, which states how a score is summed and why a pair has the same bits in every pass.
//                             The passes differ in what a lane does with its 16 scores:
//   TARGETS  a pair with equal labels writes its score to targets[trial_offset[i] + enroll_rank[j]]: a place the labels alone fix.
//   COUNTS   a pair with different labels finds its bin #{j : t[j] < s} in the sorted targets -- all of them in LDS when they fit,
//            else `P` pivots (every stride-th target) in LDS and the `stride` targets between two pivots from global memory -- and
//            adds one to the workgroup's LDS count of that bin (bins past the LDS window: one global integer atomic each).  The
//            workgroup adds its non-zero counts to the 64-bit global histogram when its walk ends.
//   SELECT   a pair with different labels and lo < s <= hi whose order-preserving key agrees with `prefix` above the digit in hand
//            counts that digit (11, 11 and 10 bits: an LDS histogram of 2048 counters; 65 536 would not fit beside the tile).
// Integer counts only: no float atomics, no grid barrier, no spinning; the result does not depend on arrival order.
// NORM: the score every pass works on is score_norm.h's z of the cosine (adaptive score normalisation, docs/score_norm.md) -- the
// vp_trial_ranks_*_norm_f32 entry points; NORM = false is the cosine itself.
#include "cos_tile.h"
#include "score_norm.h"
#include "trial_plan.h"

namespace {

using cos_tile::SLAB;
using cos_tile::MAX_D;
constexpr int QT = cos_tile::COLS;      // trials of a tile
constexpr long long MAX_NT = 1LL << 24;
constexpr int MAX_LDS = 160 * 1024;
constexpr int PIVOTS = 2048;            // two-level search: at most this many pivots in LDS
constexpr int DIGIT_BINS = 2048;

enum { TARGETS = 0, COUNTS = 1, SELECT = 2 };

bool supported(int Nt, int Ne, int D, long long NT) {
    return trial_plan::shape_ok(Nt, Ne, D) && NT >= 1 && NT <= MAX_NT;
}

struct Plan {
    int qtiles, slabs_per_wg, ranges;
    int P, stride, H;                   // COUNTS: pivots in LDS, targets per pivot, bins of the LDS window
    size_t tile_lds, count_lds, unit_t, bytes;      // unit trial rows at ws + 0, unit enrol rows at ws + unit_t
};

Plan plan(int Nt, int Ne, int D, long long NT) {
    Plan p{};
    const trial_plan::Walk w = trial_plan::walk(Nt, Ne, D);
    p.qtiles = w.qtiles;
    p.slabs_per_wg = w.slabs_per_wg;
    p.ranges = w.ranges;
    p.tile_lds = w.tile_lds;
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
    p.unit_t = w.unit_t;
    p.bytes = w.bytes;
    return p;
}

// ------------------------------------------------------------------------------------------------ unit rows
// A wave per row, 16-byte loads; the length as cos_tile.h takes it, summed over the wave's lanes.
__global__ __launch_bounds__(256) void unit_rows_kernel(const float* __restrict__ x, long long rows, int D, float* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;              // wave-uniform
    cos_tile::unit_row(x + (size_t)r * D, y + (size_t)r * D, D, lane);
}

// ------------------------------------------------------------------------------------------------ the passes
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
    // NORM: per trial and per enrol row the mean of its top cohort scores and r = 1 / max(std, floor)
    const float* tmean;
    const float* tr;
    const float* emean;
    const float* er;
};

// #{i < n : a[i] < s}, a ascending
__device__ __forceinline__ int count_below(const float* a, int n, float s) {
    int lo = 0;
    while (n > 0) {
        const int h = n >> 1;
        if (a[lo + h] < s) { lo += h + 1; n -= h + 1; } else n = h;
    }
    return lo;
}

// grid (trial tiles, row ranges), 256 threads, dynamic LDS: qs [Dp][32] | COUNTS: pivots [P], counts [H] | SELECT: counts [DIGIT_BINS]
template <int MODE, bool NORM>
__global__ __launch_bounds__(256) void trial_pass_kernel(const PassArgs a) {
    extern __shared__ __align__(16) float smem[];
    const int D = a.D, Dp = (D + 7) & ~7;
    float* qs = smem;
    float* piv = smem + (size_t)Dp * QT;
    unsigned* cnt = reinterpret_cast<unsigned*>(piv + (MODE == COUNTS ? a.P : 0));
    const int nbins = MODE == COUNTS ? a.H : (MODE == SELECT ? DIGIT_BINS : 0);
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 31, half = lane >> 5;
    const int qt = blockIdx.x, range = blockIdx.y;

    cos_tile::load_tile<false>(qs, a.tu, qt * QT, a.Nt, D);
    if (MODE == COUNTS)
        for (int i = tid; i < a.P; i += 256) piv[i] = a.st[(size_t)i * a.stride];           // i stride < NT: P = ceil(NT / stride)
    for (int i = tid; i < nbins; i += 256) cnt[i] = 0u;
    __syncthreads();

    const int q = qt * QT + c;
    const bool my_q = q < a.Nt;         // the tile's columns past Nt are zero trials: nothing is kept for them
    const int lq = my_q ? a.tl[q] : 0;
    long long off = 0;
    if (MODE == TARGETS && my_q) off = a.toff[q];
    float mt = 0.f, rt = 0.f;
    if (NORM && my_q) { mt = a.tmean[q]; rt = a.tr[q]; }
    cos_tile::walk<long long>(qs, a.eu, a.Ne, D, range, a.slabs_per_wg, [&](long long r0, const cos_tile::f32x16& acc) {
        const long long rb = r0 + 4 * half;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const long long r = rb + 8 * (v >> 2) + (v & 3);
            if (!my_q || r >= a.Ne) continue;
            const bool same = a.el[r] == lq;
            const float s = NORM ? score_norm::z(acc[v], a.emean[r], a.er[r], mt, rt) : acc[v];
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
                const unsigned key = vp_order_key(s);
                if ((key & a.prefix_mask) == a.prefix) atomicAdd(&cnt[(key >> a.shift) & a.digit_mask], 1u);
            }
        }
    });
    if (MODE != TARGETS) {
        __syncthreads();
        for (int b = tid; b < nbins; b += 256) {
            const unsigned n = cnt[b];
            if (n) atomicAdd(&a.hist[b], (unsigned long long)n);
        }
    }
}

template <int MODE, bool NORM>
int launch_as(vp_ctx* ctx, const PassArgs& a, const Plan& p, size_t lds, hipStream_t st, const char* name) {
    static bool attr_dev[64] = {};              // the attribute is per device (and per instantiation)
    bool& attr_set = attr_dev[ctx->device & 63];
    if (!attr_set) {
        VP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(trial_pass_kernel<MODE, NORM>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, MAX_LDS));
        attr_set = true;
    }
    hipLaunchKernelGGL((trial_pass_kernel<MODE, NORM>), dim3(p.qtiles, p.ranges), dim3(256), lds, st, a);
    VP_LAUNCH_CHECK(ctx, name);
    return VP_OK;
}

// a.tmean set: the normalised pass
template <int MODE>
int launch(vp_ctx* ctx, const PassArgs& a, const Plan& p, size_t lds, hipStream_t st, const char* name) {
    return a.tmean ? launch_as<MODE, true>(ctx, a, p, lds, st, name) : launch_as<MODE, false>(ctx, a, p, lds, st, name);
}

// The four statistics arrays of a vp_trial_ranks_*_norm_f32 call; nullptr: the plain entry point.
struct Norm {
    const float *tmean, *tr, *emean, *er;
    bool complete() const { return tmean && tr && emean && er; }
};

PassArgs common_args(const Plan& p, const void* ws, const int* tl, int Nt, const int* el, int Ne, int D, long long NT, const Norm* nz) {
    PassArgs a{};
    if (nz) {
        a.tmean = nz->tmean;
        a.tr = nz->tr;
        a.emean = nz->emean;
        a.er = nz->er;
    }
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
    VP_FAIL(ctx, VP_EUNSUP, "%s: Nt, Ne >= 1, D %% 4 == 0, D <= %d, 1 <= NT <= %lld", what, MAX_D, MAX_NT)

// The three passes; nz = nullptr: on the cosines (vp_trial_ranks_*_f32), else on z (vp_trial_ranks_*_norm_f32).
int targets_pass(vp_ctx* ctx, const char* what, const float* trials, const int* trial_labels, const long long* trial_offsets, int Nt,
                 const float* enroll, const int* enroll_labels, const int* enroll_ranks, int Ne, int D, long long NT, float* targets,
                 const Norm* nz, void* ws, size_t ws_bytes, vp_stream stream) {
    if (!supported(Nt, Ne, D, NT)) TRIAL_UNSUP(ctx, what);       // first, and without a context: needs no device
    if (!ctx || !trials || !trial_labels || !trial_offsets || !enroll || !enroll_labels || !enroll_ranks || !targets || !ws ||
        (nz && !nz->complete()))
        VP_FAIL(ctx, VP_EINVAL, "%s: null pointer", what);
    const Plan p = plan(Nt, Ne, D, NT);
    if (ws_bytes < p.bytes) VP_FAIL(ctx, VP_EWORKSPACE, "%s: workspace %zu < %zu bytes", what, ws_bytes, p.bytes);
    hipStream_t st = (hipStream_t)stream;
    PassArgs a = common_args(p, ws, trial_labels, Nt, enroll_labels, Ne, D, NT, nz);
    hipLaunchKernelGGL(unit_rows_kernel, dim3((Nt + 3) / 4), dim3(256), 0, st, trials, (long long)Nt, D, (float*)ws);
    VP_LAUNCH_CHECK(ctx, "unit_rows_kernel");
    hipLaunchKernelGGL(unit_rows_kernel, dim3((Ne + 3) / 4), dim3(256), 0, st, enroll, (long long)Ne, D, (float*)((char*)ws + p.unit_t));
    VP_LAUNCH_CHECK(ctx, "unit_rows_kernel");
    a.toff = trial_offsets;
    a.erank = enroll_ranks;
    a.targets = targets;
    return launch<TARGETS>(ctx, a, p, p.tile_lds, st, "trial_pass_kernel<targets>");
}

int counts_pass(vp_ctx* ctx, const char* what, const int* trial_labels, int Nt, const int* enroll_labels, int Ne, int D,
                const float* sorted_targets, long long NT, long long* hist, const Norm* nz, const void* ws, size_t ws_bytes,
                vp_stream stream) {
    if (!supported(Nt, Ne, D, NT)) TRIAL_UNSUP(ctx, what);
    if (!ctx || !trial_labels || !enroll_labels || !sorted_targets || !hist || !ws || (nz && !nz->complete()))
        VP_FAIL(ctx, VP_EINVAL, "%s: null pointer", what);
    const Plan p = plan(Nt, Ne, D, NT);
    if (ws_bytes < p.bytes) VP_FAIL(ctx, VP_EWORKSPACE, "%s: workspace %zu < %zu bytes", what, ws_bytes, p.bytes);
    hipStream_t st = (hipStream_t)stream;
    PassArgs a = common_args(p, ws, trial_labels, Nt, enroll_labels, Ne, D, NT, nz);
    a.st = sorted_targets;
    a.P = p.P;
    a.stride = p.stride;
    a.H = p.H;
    a.hist = reinterpret_cast<unsigned long long*>(hist);
    VP_HIP(ctx, hipMemsetAsync(hist, 0, (size_t)(NT + 1) * 8, st));
    return launch<COUNTS>(ctx, a, p, p.count_lds, st, "trial_pass_kernel<counts>");
}

int select_pass(vp_ctx* ctx, const char* what, const int* trial_labels, int Nt, const int* enroll_labels, int Ne, int D, long long NT,
                float lo, float hi, int level, long long prefix, long long* digits, const Norm* nz, const void* ws, size_t ws_bytes,
                vp_stream stream) {
    if (!supported(Nt, Ne, D, NT)) TRIAL_UNSUP(ctx, what);
    if (!ctx || !trial_labels || !enroll_labels || !digits || !ws || (nz && !nz->complete()))
        VP_FAIL(ctx, VP_EINVAL, "%s: null pointer", what);
    if (level < 0 || level > 2 || prefix < 0 || prefix > 0xffffffffLL) VP_FAIL(ctx, VP_EINVAL, "%s: level, prefix", what);
    const Plan p = plan(Nt, Ne, D, NT);
    if (ws_bytes < p.bytes) VP_FAIL(ctx, VP_EWORKSPACE, "%s: workspace %zu < %zu bytes", what, ws_bytes, p.bytes);
    hipStream_t st = (hipStream_t)stream;
    PassArgs a = common_args(p, ws, trial_labels, Nt, enroll_labels, Ne, D, NT, nz);
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

}  // namespace

extern "C" {

size_t vp_trial_ranks_workspace_bytes(int Nt, int Ne, int D, long long NT) {
    return supported(Nt, Ne, D, NT) ? plan(Nt, Ne, D, NT).bytes : 0;
}

int vp_trial_ranks_targets_f32(vp_ctx* ctx, const float* trials, const int* trial_labels, const long long* trial_offsets, int Nt,
                               const float* enroll, const int* enroll_labels, const int* enroll_ranks, int Ne, int D, long long NT,
                               float* targets, void* ws, size_t ws_bytes, vp_stream stream) {
    return targets_pass(ctx, "trial_ranks_targets", trials, trial_labels, trial_offsets, Nt, enroll, enroll_labels, enroll_ranks, Ne, D,
                        NT, targets, nullptr, ws, ws_bytes, stream);
}

int vp_trial_ranks_counts_f32(vp_ctx* ctx, const int* trial_labels, int Nt, const int* enroll_labels, int Ne, int D,
                              const float* sorted_targets, long long NT, long long* hist, const void* ws, size_t ws_bytes,
                              vp_stream stream) {
    return counts_pass(ctx, "trial_ranks_counts", trial_labels, Nt, enroll_labels, Ne, D, sorted_targets, NT, hist, nullptr, ws,
                       ws_bytes, stream);
}

int vp_trial_ranks_select_f32(vp_ctx* ctx, const int* trial_labels, int Nt, const int* enroll_labels, int Ne, int D, long long NT,
                              float lo, float hi, int level, long long prefix, long long* digits, const void* ws, size_t ws_bytes,
                              vp_stream stream) {
    return select_pass(ctx, "trial_ranks_select", trial_labels, Nt, enroll_labels, Ne, D, NT, lo, hi, level, prefix, digits, nullptr,
                       ws, ws_bytes, stream);
}

int vp_trial_ranks_targets_norm_f32(vp_ctx* ctx, const float* trials, const int* trial_labels, const long long* trial_offsets, int Nt,
                                    const float* enroll, const int* enroll_labels, const int* enroll_ranks, int Ne, int D,
                                    long long NT, float* targets, const float* trial_mean, const float* trial_r,
                                    const float* enroll_mean, const float* enroll_r, void* ws, size_t ws_bytes, vp_stream stream) {
    const Norm nz{trial_mean, trial_r, enroll_mean, enroll_r};
    return targets_pass(ctx, "trial_ranks_targets_norm", trials, trial_labels, trial_offsets, Nt, enroll, enroll_labels, enroll_ranks,
                        Ne, D, NT, targets, &nz, ws, ws_bytes, stream);
}

int vp_trial_ranks_counts_norm_f32(vp_ctx* ctx, const int* trial_labels, int Nt, const int* enroll_labels, int Ne, int D,
                                   const float* sorted_targets, long long NT, long long* hist, const float* trial_mean,
                                   const float* trial_r, const float* enroll_mean, const float* enroll_r, const void* ws,
                                   size_t ws_bytes, vp_stream stream) {
    const Norm nz{trial_mean, trial_r, enroll_mean, enroll_r};
    return counts_pass(ctx, "trial_ranks_counts_norm", trial_labels, Nt, enroll_labels, Ne, D, sorted_targets, NT, hist, &nz, ws,
                       ws_bytes, stream);
}

int vp_trial_ranks_select_norm_f32(vp_ctx* ctx, const int* trial_labels, int Nt, const int* enroll_labels, int Ne, int D,
                                   long long NT, float lo, float hi, int level, long long prefix, long long* digits,
                                   const float* trial_mean, const float* trial_r, const float* enroll_mean, const float* enroll_r,
                                   const void* ws, size_t ws_bytes, vp_stream stream) {
    const Norm nz{trial_mean, trial_r, enroll_mean, enroll_r};
    return select_pass(ctx, "trial_ranks_select_norm", trial_labels, Nt, enroll_labels, Ne, D, NT, lo, hi, level, prefix, digits, &nz,
                       ws, ws_bytes, stream);
}

}  // extern "C"
