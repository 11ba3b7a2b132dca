// 1:N speaker search over a resident gallery (PPVectorPredictor.__retrieval, predict.py:173-187, and the per-user means it searches,
// :154-164): unit centroids per user, and the k best centroids of every query without a (Q, U) score matrix in global memory.
//
// vp_gallery_centroids_f32   one workgroup per user: the user's rows added in ascending row order (a thread per column), divided by the
//                            count, scaled to unit length.  The same kernel rebuilds every row or one.
// vp_gallery_topk_f32        gallery_score_kernel: a workgroup holds a tile of 32 normalised queries in LDS ([k][query], the B operand
//                            of v_mfma_f32_32x32x2_f32) and walks `slabs_per_wg` slabs of VP_GALLERY_SLAB = 128 centroid rows; each of
//                            its four waves owns 32 rows of a slab, reads them as 16-byte loads (lane (c, half) takes floats
//                            8g + 4 half .. + 3 of row c; a v_permlane32_swap pair puts k, k + 1 on the two halves) and keeps the
//                            32 x 32 scores in one accumulator over ALL of D.  A score is therefore one k-ordered fma chain
//                            (ascending k, the matrix core's own order inside a pair) whatever U, the slab, the wave or the grid:
//                            bit-identical rows get bit-identical scores.  Per wave and query a list of k (score, row) lives in LDS,
//                            unordered but for its worst entry at k - 1 (while places are empty: an empty one that counts the taken
//                            ones); a lane replaces that entry only when its score beats it.
//                            At the end eight lanes per query rank the entries of the four lists and write the best k as ONE
//                            sorted partial list per (query, workgroup).
//                            (The two normalisations take their lengths in float64, so a unit vector is rounded once per element.)
//                            gallery_merge_kernel: a workgroup per query copies its partial lists to LDS and merges them (k rounds of a
//                            block-wide best-head selection over sorted lists).
// Order everywhere: score descending, then row ascending.  No atomics, no grid barrier, fixed order of every sum: two runs give the
// same bits.  f32 throughout: a narrower gallery would change which rows win (the rule of diarize.hip's selection).
#include "common.h"

#include <math.h>

namespace {

constexpr int SLAB = VP_GALLERY_SLAB;   // 4 waves x 32 rows
constexpr int QT = 32;                  // queries of a tile = the matrix core's N
constexpr int MAX_K = 32, MAX_D = 1024;
constexpr int MAX_RANGES = 512;         // partial lists per query: 2 per thread of the merge kernel, 512 x 32 x 8 B = 128 KB of its LDS

typedef __attribute__((ext_vector_type(16))) float f32x16;

static_assert(SLAB == 128, "the score kernel's four waves take 32 rows each");

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
// Eight consecutive k of the wave's 32 rows x the tile's 32 queries.  In: lane (c, half) holds k0 + 4 half + {0, 1, 2, 3} of its row in
// v; the two swaps leave (k0, k0 + 1), (k0 + 2, k0 + 3), (k0 + 4, k0 + 5), (k0 + 6, k0 + 7) on (lower half, upper half) of x, z, y, w.
// FULL = false: the last four k of a D that is no multiple of 8 -- the upper half's v is zero and only x, z are used.
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

// grid (query tiles, row ranges), 256 threads, dynamic LDS: qs [Dp][32] | list scores [4][32][kp] | list rows [4][32][kp]
__global__ __launch_bounds__(256) void gallery_score_kernel(const float* __restrict__ queries, int Q, const float* __restrict__ G, int U,
                                                            int D, int k, int slabs_per_wg, int ranges, float* __restrict__ part_s,
                                                            int* __restrict__ part_i) {
    extern __shared__ __align__(16) float smem[];
    const int Dp = (D + 7) & ~7;
    float* qs = smem;
    const int kp = (k + 7) & ~7;                // a list's stride: k entries and padding (+inf: never the worst) to whole 16-byte reads
    float* ls = smem + (size_t)Dp * QT;
    int* li = reinterpret_cast<int*>(ls + 4 * QT * kp);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, half = lane >> 5;
    const int qt = blockIdx.x, range = blockIdx.y;

    {   // the query tile, normalised: eight threads per query, 16-byte loads; queries past Q and the k past D are zero
        const int j = tid >> 3, sub = tid & 7;
        const int q = qt * QT + j;
        const bool qv = q < Q;
        const float* src = queries + (size_t)(qv ? q : 0) * D;
        double ss = 0.0;                        // the length in float64 (32 x D elements per workgroup): one rounding per element
        for (int kk = sub * 4; kk < D; kk += 32) {
            const float4 v = *reinterpret_cast<const float4*>(src + kk);
            ss += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
        }
        ss += __shfl_xor(ss, 1);
        ss += __shfl_xor(ss, 2);
        ss += __shfl_xor(ss, 4);
        const double inv = (qv && ss > 0.0) ? 1.0 / sqrt(ss) : 0.0;
        for (int kk = sub * 4; kk < D; kk += 32) {
            const float4 v = *reinterpret_cast<const float4*>(src + kk);
            qs[(kk + 0) * QT + j] = qv ? (float)(v.x * inv) : 0.f;
            qs[(kk + 1) * QT + j] = qv ? (float)(v.y * inv) : 0.f;
            qs[(kk + 2) * QT + j] = qv ? (float)(v.z * inv) : 0.f;
            qs[(kk + 3) * QT + j] = qv ? (float)(v.w * inv) : 0.f;
        }
        if (sub == 0)
            for (int kk = D; kk < Dp; ++kk) qs[kk * QT + j] = 0.f;
        for (int i = tid; i < 4 * QT * kp; i += 256) { ls[i] = i % kp < k ? -INFINITY : INFINITY; li[i] = -1; }
    }
    __syncthreads();

    float* my_s = ls + (w * QT + c) * kp;        // the list of (this wave, query c): shared by the lanes c and c + 32, which take turns
    const bool my_q = qt * QT + c < Q;           // the tile's columns past Q are zero queries: nothing is kept for them
    int* my_i = li + (w * QT + c) * kp;
    const int ngroups = D >> 3;
    for (int sl = 0; sl < slabs_per_wg; ++sl) {
        const int r0 = (range * slabs_per_wg + sl) * SLAB + w * 32;
        if (r0 >= U) break;                     // wave-uniform
        const int row = r0 + c < U ? r0 + c : U - 1;       // rows past U are computed from row U - 1 and never inserted
        const float* a = G + (size_t)row * D + 4 * half;
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
            for (int u = 0; u < 8; ++u) mma_group<true>(v[u], qs + (size_t)(g + u) * 8 * QT, c, half, acc);
        }
        for (; g < ngroups; ++g) {
            const float4 v = *reinterpret_cast<const float4*>(a + (size_t)g * 8);
            mma_group<true>(v, qs + (size_t)g * 8 * QT, c, half, acc);
        }
        if (D & 4) {                            // the upper half's four k lie past the row: not read
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (half == 0) v = *reinterpret_cast<const float4*>(a + (size_t)ngroups * 8);
            mma_group<false>(v, qs + (size_t)ngroups * 8 * QT, c, half, acc);
        }
        // acc[v] = score of row r0 + 8 (v / 4) + 4 half + v % 4 against query c
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
    }
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
    const Plan p = plan(Q, U, D, k);
    if (ws_bytes < p.bytes) VP_FAIL(ctx, VP_EWORKSPACE, "gallery_topk: workspace %zu < %zu bytes", ws_bytes, p.bytes);
    hipStream_t st = (hipStream_t)stream;
    static bool attr_dev[64] = {};              // the attribute is per device
    bool& attr_set = attr_dev[ctx->device & 63];
    if (!attr_set) {
        VP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(gallery_score_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        MAX_D * QT * 4 + 4 * QT * MAX_K * 8));
        VP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(gallery_merge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        MAX_RANGES * MAX_K * 8));
        attr_set = true;
    }
    float* part_s = (float*)ws;
    int* part_i = (int*)((char*)ws + p.part_bytes);
    hipLaunchKernelGGL(gallery_score_kernel, dim3(p.qtiles, p.ranges), dim3(256), p.lds, st, queries, Q, centroids, U, D, k,
                       p.slabs_per_wg, p.ranges, part_s, part_i);
    VP_LAUNCH_CHECK(ctx, "gallery_score_kernel");
    hipLaunchKernelGGL(gallery_merge_kernel, dim3(Q), dim3(256), p.merge_lds, st, part_s, part_i, p.ranges, k, out_idx, out_score);
    VP_LAUNCH_CHECK(ctx, "gallery_merge_kernel");
    return VP_OK;
}

}  // extern "C"
