// 1:N speaker search over a resident gallery (PPVectorPredictor.__retrieval, predict.py:173-187, and the per-user means it searches,
// :154-164): unit centroids per user, and the k best centroids of every query without a (Q, U) score matrix in global memory.
//
// vp_gallery_centroids_f32   one workgroup per user: the user's rows added in ascending row order (a thread per column), divided by the
//                            count, scaled to unit length.  The same kernel rebuilds every row or one.
// vp_gallery_topk_f32        gallery_score_kernel: a workgroup normalises a tile of 32 queries into LDS and walks `slabs_per_wg` slabs
//                            of VP_GALLERY_SLAB centroid rows with cos_tile.h's walk, which states how a score is summed and why
//                            bit-identical rows get bit-identical scores.  Per wave and query a list of k (score, row) lives in LDS,
//                            unordered but for its worst entry at k - 1 (while places are empty: an empty one that counts the taken
//                            ones); a lane replaces that entry only when its score beats it.
//                            At the end eight lanes per query rank the entries of the four lists and write the best k as ONE
//                            sorted partial list per (query, workgroup).
//                            gallery_merge_kernel: a workgroup per query copies its partial lists to LDS and merges them (k rounds of a
//                            block-wide best-head selection over sorted lists).
// vp_gallery_topk_norm_f32   the same two kernels with gallery_score_kernel<true>: the value offered to the lists is score_norm.h's z of
//                            the cosine (the gallery row is the enrolment, the query the trial; docs/gallery.md, "Search on normalised
//                            scores"), so the selection itself is on z.  Nothing else differs: the lists, better(), the merge.
// Order everywhere: score descending, then row ascending.  No atomics, no grid barrier, fixed order of every sum: two runs give the
// same bits.  f32 throughout: a narrower gallery would change which rows win (the rule of diarize.hip's selection).
#include "cos_tile.h"
#include "score_norm.h"

namespace {

using cos_tile::SLAB;
using cos_tile::MAX_D;
constexpr int QT = cos_tile::COLS;      // queries of a tile
constexpr int MAX_K = 32;
constexpr int MAX_RANGES = 512;         // partial lists per query: 2 per thread of the merge kernel, 512 x 32 x 8 B = 128 KB of its LDS

struct Plan {
    int slabs_per_wg, ranges, qtiles;
    size_t lds, merge_lds, part_bytes, bytes;   // dynamic LDS of the two kernels; one of the two partial arrays; the workspace
};

bool supported(int Q, int U, int D, int k) {
    return Q >= 1 && U >= 1 && D >= 4 && D % 4 == 0 && D <= MAX_D && k >= 1 && k <= MAX_K && (long long)U * D < (1LL << 31) &&
           (Q + QT - 1) / QT <= 65535;
}

// A workgroup walks at least two slabs (the query tile's load and normalisation is paid once per workgroup) and as many as keep the
// partial lists of a query at MAX_RANGES.
Plan plan(int Q, int U, int D, int k) {
    Plan p{};
    const int slabs = (U + SLAB - 1) / SLAB;
    const int by_cap = (slabs + MAX_RANGES - 1) / MAX_RANGES, least = slabs < 2 ? slabs : 2;
    p.slabs_per_wg = by_cap > least ? by_cap : least;
    p.ranges = (slabs + p.slabs_per_wg - 1) / p.slabs_per_wg;
    p.qtiles = (Q + QT - 1) / QT;
    const int Dp = (D + 7) / 8 * 8;
    p.lds = (size_t)Dp * QT * 4 + (size_t)4 * QT * ((k + 7) / 8 * 8) * 8;
    p.merge_lds = (size_t)p.ranges * k * 8;
    p.part_bytes = vp_align_up((size_t)Q * p.ranges * k * 4, 256);
    p.bytes = 2 * p.part_bytes;
    return p;
}

__device__ __forceinline__ bool better(float s, int i, float ts, int ti) { return s > ts || (s == ts && i < ti); }

// ------------------------------------------------------------------------------------------------ centroids
__global__ __launch_bounds__(256) void gallery_centroid_kernel(const float* __restrict__ emb, const int* __restrict__ offsets,
                                                               const int* __restrict__ dst_rows, int D, float* __restrict__ cen) {
    __shared__ double red[256];
    const int tid = threadIdx.x, g = blockIdx.x;
    const int b = offsets[g], e = offsets[g + 1];
    float* out = cen + (size_t)dst_rows[g] * D;
    double ss = 0.0;                                         // the length in float64: the unit row is rounded once per element
    for (int col = tid; col < D; col += 256) {
        float acc = 0.f;
        for (int r = b; r < e; ++r) acc += emb[(size_t)r * D + col];
        const float m = e > b ? acc / (float)(e - b) : 0.f;
        out[col] = m;
        ss += (double)m * (double)m;
    }
    red[tid] = ss;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const double tot = red[0];
    const double inv = tot > 0.0 ? 1.0 / sqrt(tot) : 0.0;
    for (int col = tid; col < D; col += 256) out[col] = (float)((double)out[col] * inv);      // the element this thread wrote above
}

// ------------------------------------------------------------------------------------------------ scores and per-workgroup lists
// grid (query tiles, row ranges), 256 threads, dynamic LDS: qs [Dp][32] | list scores [4][32][kp] | list rows [4][32][kp]
// NORM: per query and per gallery row the mean of its top cohort scores and r = 1 / max(std, floor); the lists then hold z
struct NormStats {
    const float* qmean;
    const float* qr;
    const float* umean;
    const float* ur;
};

template <bool NORM>
__global__ __launch_bounds__(256) void gallery_score_kernel(const float* __restrict__ queries, int Q, const float* __restrict__ G, int U,
                                                            int D, int k, int slabs_per_wg, int ranges, float* __restrict__ part_s,
                                                            int* __restrict__ part_i, const NormStats nz) {
    extern __shared__ __align__(16) float smem[];
    const int Dp = (D + 7) & ~7;
    float* qs = smem;
    const int kp = (k + 7) & ~7;                // a list's stride: k entries and padding (+inf: never the worst) to whole 16-byte reads
    float* ls = smem + (size_t)Dp * QT;
    int* li = reinterpret_cast<int*>(ls + 4 * QT * kp);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, half = lane >> 5;
    const int qt = blockIdx.x, range = blockIdx.y;

    cos_tile::load_tile<true>(qs, queries, qt * QT, Q, D);      // raw queries in, unit rows out; a zero query is a zero row
    for (int i = tid; i < 4 * QT * kp; i += 256) { ls[i] = i % kp < k ? -INFINITY : INFINITY; li[i] = -1; }
    __syncthreads();

    float* my_s = ls + (w * QT + c) * kp;        // the list of (this wave, query c): shared by the lanes c and c + 32, which take turns
    const bool my_q = qt * QT + c < Q;           // the tile's columns past Q are zero queries: nothing is kept for them
    int* my_i = li + (w * QT + c) * kp;
    float mq = 0.f, rq = 0.f;
    if (NORM && my_q) { mq = nz.qmean[qt * QT + c]; rq = nz.qr[qt * QT + c]; }
    cos_tile::walk<int>(qs, G, U, D, range, slabs_per_wg, [&](int r0, const cos_tile::f32x16& cosines) {
        cos_tile::f32x16 acc = cosines;         // what is offered to the list: the cosine, or its z
        if (NORM) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int r = r0 + 4 * half + 8 * (v >> 2) + (v & 3);
                if (my_q && r < U) acc[v] = score_norm::z(cosines[v], nz.umean[r], nz.ur[r], mq, rq);
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (half == h) {
                float ts = my_s[k - 1];
                int ti = my_i[k - 1];
                const int rb = r0 + 4 * half;
                unsigned pending = 0;           // the scores that beat the list's worst entry as it stands (it only gets better)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int r = rb + 8 * (v >> 2) + (v & 3);
                    if (my_q && r < U && better(acc[v], r, ts, ti)) pending |= 1u << v;
                }
                // every lane works through ITS pending scores: the wave makes as many trips as the busiest lane has scores
                while (pending) {
                    const int v = __ffs(pending) - 1;
                    pending &= pending - 1;
                    float s = acc[0];
#pragma unroll
                    for (int u = 1; u < 16; ++u) s = v == u ? acc[u] : s;
                    const int r = rb + 8 * (v >> 2) + (v & 3);
                    if (!better(s, r, ts, ti)) continue;
                    // While the list has empty places its last entry is empty and carries their position: row -1 - n says that the
                    // entries 0 .. n - 1 are taken.  The new score goes to place n, no search; the place k - 1 itself goes last.
                    if (ti < 0 && -1 - ti < k - 1) {
                        my_s[-1 - ti] = s;
                        my_i[-1 - ti] = r;
                        --ti;
                        my_i[k - 1] = ti;
                        continue;
                    }
                    // the list is unordered but for its WORST entry, which sits at k - 1: the new score takes that place, the worst of
                    // the list is found again (16-byte reads, eight entries a trip; the padding entries are +inf) and put back at k - 1
                    my_s[k - 1] = s;
                    my_i[k - 1] = r;
                    float ws = s;
                    int wi = r, wp = k - 1;
                    for (int e = 0; e < kp && k > 1; e += 8) {
                        const float4 s0 = *reinterpret_cast<const float4*>(my_s + e), s1 = *reinterpret_cast<const float4*>(my_s + e + 4);
                        const int4 i0 = *reinterpret_cast<const int4*>(my_i + e), i1 = *reinterpret_cast<const int4*>(my_i + e + 4);
                        const float es[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
                        const int ei[8] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
#pragma unroll
                        for (int u = 0; u < 8; ++u)
                            if (better(ws, wi, es[u], ei[u])) { ws = es[u]; wi = ei[u]; wp = e + u; }
                    }
                    if (wp != k - 1) {
                        my_s[wp] = s;
                        my_i[wp] = r;
                        my_s[k - 1] = ws;
                        my_i[k - 1] = wi;
                    }
                    ts = ws;
                    ti = wi;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");     // the other half reads what this one wrote
            __builtin_amdgcn_wave_barrier();
        }
    });
    __syncthreads();
    {   // the query's 4 k entries (unordered) -> the workgroup's ONE list, in order.  Eight lanes per query; an entry's place is its RANK,
        // the number of entries that beat it (the order is total: rows are distinct), so nothing is exchanged between lanes or rounds
        const int j = tid >> 3, sub = tid & 7;
        const int q = qt * QT + j;
        const bool qv = q < Q;
        float* os = part_s + ((size_t)(qv ? q : 0) * ranges + range) * k;
        int* oi = part_i + ((size_t)(qv ? q : 0) * ranges + range) * k;
        int valid = 0;
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) {
            for (int e = sub; e < k; e += 8) {
                const float s = ls[(ww * QT + j) * kp + e];
                const int i = li[(ww * QT + j) * kp + e];
                if (i < 0 || !qv) continue;             // an empty place (any negative row), or a column past Q
                ++valid;
                int rank = 0;
#pragma unroll
                for (int w2 = 0; w2 < 4; ++w2) {
                    for (int e2 = 0; e2 < kp; e2 += 4) {    // the padding past k holds row -1 as the empty places do
                        const float4 s4 = *reinterpret_cast<const float4*>(ls + (w2 * QT + j) * kp + e2);
                        const int4 i4 = *reinterpret_cast<const int4*>(li + (w2 * QT + j) * kp + e2);
                        rank += (i4.x >= 0 && better(s4.x, i4.x, s, i)) + (i4.y >= 0 && better(s4.y, i4.y, s, i)) +
                                (i4.z >= 0 && better(s4.z, i4.z, s, i)) + (i4.w >= 0 && better(s4.w, i4.w, s, i));
                    }
                }
                if (rank < k && qv) { os[rank] = s; oi[rank] = i; }
            }
        }
        valid += __shfl_xor(valid, 1);
        valid += __shfl_xor(valid, 2);
        valid += __shfl_xor(valid, 4);
        for (int o = valid + sub; o < k; o += 8)
            if (qv) { os[o] = -INFINITY; oi[o] = -1; }
    }
}

// ------------------------------------------------------------------------------------------------ merge of the partial lists
// grid Q, 256 threads, dynamic LDS: the query's `ranges` sorted lists, scores then rows (one coalesced copy; the rounds then run out of
// LDS).  Thread t owns the lists t and t + 256 and a head in each.  A round: every thread's best head, the block's best of those (wave
// shuffles, then the four waves' through LDS), the owner of the winning row moves its head on.
__global__ __launch_bounds__(256) void gallery_merge_kernel(const float* __restrict__ part_s, const int* __restrict__ part_i, int ranges,
                                                            int k, int* __restrict__ out_idx, float* __restrict__ out_score) {
    extern __shared__ __align__(16) float smem[];
    __shared__ float red_s[2][4];
    __shared__ int red_i[2][4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = blockIdx.x;
    const int n = ranges * k;
    float* ps = smem;
    int* pi = reinterpret_cast<int*>(smem + n);
    for (int e = tid; e < n; e += 256) {
        ps[e] = part_s[(size_t)q * n + e];
        pi[e] = part_i[(size_t)q * n + e];
    }
    __syncthreads();
    int hd[2] = {0, 0};
    for (int o = 0; o < k; ++o) {
        float bs = -INFINITY;
        int bi = -1;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int l = tid + 256 * u;
            if (l < ranges && hd[u] < k) {
                const float s = ps[l * k + hd[u]];
                const int i = pi[l * k + hd[u]];
                if (i >= 0 && (bi < 0 || better(s, i, bs, bi))) { bs = s; bi = i; }
            }
        }
        const int mine = bi;
        float s = bs;
        int i = bi;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float os = __shfl_xor(s, off);
            const int oi = __shfl_xor(i, off);
            if (oi >= 0 && (i < 0 || better(os, oi, s, i))) { s = os; i = oi; }
        }
        if (lane == 0) { red_s[o & 1][w] = s; red_i[o & 1][w] = i; }
        __syncthreads();
        s = red_s[o & 1][0];
        i = red_i[o & 1][0];
#pragma unroll
        for (int ww = 1; ww < 4; ++ww) {
            const float os = red_s[o & 1][ww];
            const int oi = red_i[o & 1][ww];
            if (oi >= 0 && (i < 0 || better(os, oi, s, i))) { s = os; i = oi; }
        }
        if (i >= 0 && mine == i) {              // rows are disjoint between lists: exactly one thread owns the winner
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int l = tid + 256 * u;
                if (l < ranges && hd[u] < k && pi[l * k + hd[u]] == i) ++hd[u];
            }
        }
        if (tid == 0) {
            out_idx[(size_t)q * k + o] = i;
            out_score[(size_t)q * k + o] = i >= 0 ? s : -INFINITY;
        }
    }
}

// the two launches of a search; the callers have checked the shape and the pointers
template <bool NORM>
int topk(vp_ctx* ctx, const float* queries, int Q, const float* centroids, int U, int D, int k, const NormStats& nz, int* out_idx,
         float* out_score, void* ws, size_t ws_bytes, vp_stream stream) {
    const Plan p = plan(Q, U, D, k);
    if (ws_bytes < p.bytes) VP_FAIL(ctx, VP_EWORKSPACE, "gallery_topk: workspace %zu < %zu bytes", ws_bytes, p.bytes);
    hipStream_t st = (hipStream_t)stream;
    static bool attr_dev[64] = {};              // the attribute is per device (and per instantiation: the static is the template's)
    bool& attr_set = attr_dev[ctx->device & 63];
    if (!attr_set) {
        VP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(gallery_score_kernel<NORM>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, MAX_D * QT * 4 + 4 * QT * MAX_K * 8));
        VP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(gallery_merge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        MAX_RANGES * MAX_K * 8));
        attr_set = true;
    }
    float* part_s = (float*)ws;
    int* part_i = (int*)((char*)ws + p.part_bytes);
    hipLaunchKernelGGL(gallery_score_kernel<NORM>, dim3(p.qtiles, p.ranges), dim3(256), p.lds, st, queries, Q, centroids, U, D, k,
                       p.slabs_per_wg, p.ranges, part_s, part_i, nz);
    VP_LAUNCH_CHECK(ctx, "gallery_score_kernel");
    hipLaunchKernelGGL(gallery_merge_kernel, dim3(Q), dim3(256), p.merge_lds, st, part_s, part_i, p.ranges, k, out_idx, out_score);
    VP_LAUNCH_CHECK(ctx, "gallery_merge_kernel");
    return VP_OK;
}

}  // namespace

extern "C" {

int vp_gallery_centroids_f32(vp_ctx* ctx, const float* emb, const int* offsets, const int* dst_rows, int n, int D, float* centroids,
                             vp_stream stream) {
    if (!ctx || !emb || !offsets || !dst_rows || !centroids || n < 0 || D < 1) VP_FAIL(ctx, VP_EINVAL, "gallery_centroids: bad arguments");
    if (n == 0) return VP_OK;
    hipLaunchKernelGGL(gallery_centroid_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, emb, offsets, dst_rows, D, centroids);
    VP_LAUNCH_CHECK(ctx, "gallery_centroid_kernel");
    return VP_OK;
}

size_t vp_gallery_topk_workspace_bytes(int Q, int U, int D, int k) {
    return supported(Q, U, D, k) ? plan(Q, U, D, k).bytes : 0;
}

int vp_gallery_topk_f32(vp_ctx* ctx, const float* queries, int Q, const float* centroids, int U, int D, int k, int* out_idx,
                        float* out_score, void* ws, size_t ws_bytes, vp_stream stream) {
    if (!supported(Q, U, D, k))                 // first, and without a context: the refusal needs no device
        VP_FAIL(ctx, VP_EUNSUP, "gallery_topk: Q, U >= 1, D %% 4 == 0, D <= %d, 1 <= k <= %d, U D < 2^31", MAX_D, MAX_K);
    if (!ctx || !queries || !centroids || !out_idx || !out_score || !ws) VP_FAIL(ctx, VP_EINVAL, "gallery_topk: null pointer");
    return topk<false>(ctx, queries, Q, centroids, U, D, k, NormStats{}, out_idx, out_score, ws, ws_bytes, stream);
}

int vp_gallery_topk_norm_f32(vp_ctx* ctx, const float* queries, int Q, const float* centroids, int U, int D, int k,
                             const float* query_mean, const float* query_r, const float* user_mean, const float* user_r, int* out_idx,
                             float* out_score, void* ws, size_t ws_bytes, vp_stream stream) {
    if (!supported(Q, U, D, k))
        VP_FAIL(ctx, VP_EUNSUP, "gallery_topk_norm: Q, U >= 1, D %% 4 == 0, D <= %d, 1 <= k <= %d, U D < 2^31", MAX_D, MAX_K);
    if (!ctx || !queries || !centroids || !out_idx || !out_score || !ws) VP_FAIL(ctx, VP_EINVAL, "gallery_topk_norm: null pointer");
    if (!query_mean || !query_r || !user_mean || !user_r) VP_FAIL(ctx, VP_EINVAL, "gallery_topk_norm: null statistics pointer");
    return topk<true>(ctx, queries, Q, centroids, U, D, k, NormStats{query_mean, query_r, user_mean, user_r}, out_idx, out_score, ws,
                      ws_bytes, stream);
}

}  // extern "C"
