// Speaker diarization around the embedding forward (ppvector/infer_utils/speaker_diarization.py, predict.py:366-396):
//   * chunk_batch     -- the fixed-length windows of one recording as a batch: zero padding on the right (_chunk, :76-77), then the
//                        decibel normalisation _load_audio applies to every ndarray predict_batch is given (predict.py:213-215).
//   * affinity_prune  -- cosine affinity (get_sim_mat, :253-257) with the n_elems smallest entries of every row zeroed (p_pruning,
//                        :260-273): a row block's similarities live in LDS only, the row's n_elems-th smallest value is found there by an
//                        8-bit radix selection on the ordered-integer image of the floats (no sort, no unpruned matrix in memory).
//   * laplacian       -- M = (P + P^T) / 2 with a zero diagonal, L = diag(sum_j |M_ij|) - M (:246, :276-282).
// Everything is f32 whatever set_compute_dtype says (the pruning is a selection: a narrower format would change which entries survive);
// the chunk's mean square and its gain are carried in f64, as numpy carries them.  No float atomics anywhere: every sum has a fixed order,
// so two runs give the same bits.  The histogram of the selection uses integer LDS atomics, whose result does not depend on their order.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ chunk batch
struct ChunkArgs { const float* wave; const int* table; float* out; int wave_len, chunk_len, normalize; float target_db; };

// one workgroup per window.  The mean square is over the PADDED row (the reference pads before it normalises), the gain is
// AudioSegment.normalize's: min(target_db - 10 log10(max(mean x^2, 1e-20)), 300) dB.
__global__ __launch_bounds__(256) void chunk_batch_kernel(ChunkArgs a) {
    __shared__ double red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    int st = a.table[2 * b], ed = a.table[2 * b + 1];
    st = st < 0 ? 0 : (st > a.wave_len ? a.wave_len : st);
    ed = ed < st ? st : (ed > a.wave_len ? a.wave_len : ed);
    const int nv = ed - st < a.chunk_len ? ed - st : a.chunk_len;
    const float* s = a.wave + st;
    float gain = 1.f;
    if (a.normalize) {
        double ss = 0.0;
        for (int i = tid; i < nv; i += 256) { const double v = (double)s[i]; ss += v * v; }
        red[tid] = ss;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        double ms = red[0] / (double)a.chunk_len;
        ms = ms > 1e-20 ? ms : 1e-20;
        double g = (double)a.target_db - 10.0 * log10(ms);
        g = g < 300.0 ? g : 300.0;
        gain = (float)pow(10.0, g / 20.0);
    }
    float* o = a.out + (size_t)b * a.chunk_len;
    for (int i = tid; i < a.chunk_len; i += 256) o[i] = i < nv ? s[i] * gain : 0.f;
}

// ------------------------------------------------------------------------------------------------ affinity + pruning
// Normalised, transposed copy of the embeddings: xnT[k][i] = x[i][k] / |x_i| (so the affinity kernel's loads run along i), and the
// inverse norms themselves -- computed once.  A zero row keeps inverse norm 0 (its cosines are 0, as sklearn's normalize leaves them).
__global__ __launch_bounds__(256) void affinity_prep_kernel(const float* __restrict__ x, int N, int D, float* __restrict__ inv,
                                                            float* __restrict__ xnT) {
    __shared__ float tile[64][65];
    __shared__ float inv_s[64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i0 = blockIdx.x * 64;
    for (int r = w; r < 64; r += 4) {
        const int i = i0 + r;
        float ss = 0.f;
        if (i < N)
            for (int k = lane; k < D; k += 64) { const float v = x[(size_t)i * D + k]; ss += v * v; }
        ss = vp_wave_sum(ss);
        const float iv = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
        if (lane == 0) {
            inv_s[r] = iv;
            if (i < N) inv[i] = iv;
        }
    }
    __syncthreads();
    for (int k0 = 0; k0 < D; k0 += 64) {
        for (int r = w; r < 64; r += 4) {
            const int i = i0 + r, k = k0 + lane;
            tile[r][lane] = (i < N && k < D) ? x[(size_t)i * D + k] * inv_s[r] : 0.f;
        }
        __syncthreads();
        for (int c = w; c < 64; c += 4) {
            const int k = k0 + c, i = i0 + lane;
            if (k < D && i < N) xnT[(size_t)k * N + i] = tile[lane][c];
        }
        __syncthreads();
    }
}

// One workgroup per block of R rows.  Dynamic LDS: sims[R][N] | xs[R][Dp] (the block's own normalised rows, Dp = D rounded up to 4).
// Thread t owns columns t, t + 256, ... in every phase after the products, so the phases of one row need no barrier between them
// beyond the ones of the selection itself.
template <int R>
__global__ __launch_bounds__(256) void affinity_prune_kernel(const float* __restrict__ x, const float* __restrict__ xnT,
                                                             const float* __restrict__ inv, float* __restrict__ P, int N, int D, int Dp,
                                                             int n_elems) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ unsigned hist[256];
    __shared__ unsigned wtot[4];
    __shared__ unsigned sel[3];
    float* sims = (float*)smem;
    float* xs = sims + (size_t)R * N;                  // R * N * 4 is a multiple of 16 only if N % 4 == 0: xs is read as scalars below
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i0 = blockIdx.x * R;

    for (int idx = tid; idx < R * Dp; idx += 256) {
        const int r = idx / Dp, k = idx - r * Dp, i = i0 + r;
        xs[idx] = (i < N && k < D) ? x[(size_t)i * D + k] * inv[i] : 0.f;
    }
    __syncthreads();

    // products: four columns per thread and pass, the R rows of the block against each
    for (int jb = 0; jb < N; jb += 1024) {
        int jc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) { const int j = jb + tid + 256 * c; jc[c] = j < N ? j : N - 1; }
        float acc[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
        for (int k = 0; k < D; ++k) {
            float v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = xnT[(size_t)k * N + jc[c]];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float a = xs[r * Dp + k];
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = fmaf(a, v[c], acc[r][c]);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = jb + tid + 256 * c;
            if (j < N) {
#pragma unroll
                for (int r = 0; r < R; ++r) sims[(size_t)r * N + j] = acc[r][c] + 0.f;      // + 0: -0 becomes +0, one key per value
            }
        }
    }
    // no barrier: from here on a thread reads only the columns it wrote

    for (int r = 0; r < R; ++r) {
        const int i = i0 + r;
        if (i >= N) break;                               // uniform
        float* srow = sims + (size_t)r * N;
        if (n_elems > 0) {
            // the n_elems-th smallest key, 8 bits at a time from the top
            unsigned prefix = 0, kth = (unsigned)n_elems, cnt = 0;
            for (int pass = 0; pass < 4; ++pass) {
                const int shift = 24 - 8 * pass;
                hist[tid] = 0;
                __syncthreads();
                for (int j = tid; j < N; j += 256) {
                    const unsigned key = vp_order_key(srow[j]);
                    if (pass == 0 || ((key ^ prefix) >> (shift + 8)) == 0) atomicAdd(&hist[(key >> shift) & 255u], 1u);
                }
                __syncthreads();
                const unsigned c = hist[tid];
                unsigned incl = c;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned t = __shfl_up(incl, o);
                    if (lane >= o) incl += t;
                }
                if (lane == 63) wtot[w] = incl;
                __syncthreads();
                for (int q = 0; q < w; ++q) incl += wtot[q];
                const unsigned excl = incl - c;
                if (excl < kth && kth <= incl) { sel[0] = prefix | ((unsigned)tid << shift); sel[1] = kth - excl; sel[2] = c; }
                __syncthreads();
                prefix = sel[0]; kth = sel[1]; cnt = sel[2];
            }
            // prefix = key of the threshold value, cnt = how many entries of the row have it, kth of those are zeroed: the ones in the
            // lowest columns (the reference's argsort leaves the order of equal values undefined; this is the engine's rule)
            if (kth < cnt) {
                unsigned running = 0;
                for (int jb = 0; jb < N && running < kth; jb += 256) {
                    const int j = jb + tid;
                    const bool tie = j < N && vp_order_key(srow[j]) == prefix;
                    const unsigned long long m = __ballot(tie);
                    if (lane == 0) wtot[w] = (unsigned)__popcll(m);
                    __syncthreads();
                    unsigned rank = running + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
                    for (int q = 0; q < w; ++q) rank += wtot[q];
                    if (tie && rank < kth) srow[j] = 0.f;
                    running += wtot[0] + wtot[1] + wtot[2] + wtot[3];
                    __syncthreads();
                }
                for (int j = tid; j < N; j += 256)
                    if (vp_order_key(srow[j]) < prefix) srow[j] = 0.f;
            } else {
                for (int j = tid; j < N; j += 256)
                    if (vp_order_key(srow[j]) <= prefix) srow[j] = 0.f;
            }
        }
        float* prow = P + (size_t)i * N;
        for (int j = tid; j < N; j += 256) prow[j] = srow[j];
    }
}

// ------------------------------------------------------------------------------------------------ Laplacian
// One workgroup per 32 rows, walking the 32 x 32 tiles of those rows left to right: the tile of P is read directly, its transpose
// partner is read along ITS rows (coalesced) and turned in LDS.  Each thread keeps the |M| sums of its four rows over its column of
// every tile; the 32 partials of a row are added in lane order at the end -- a fixed order.  Out of place only: the partner tile of a
// later workgroup would already be overwritten.
__global__ __launch_bounds__(256) void laplacian_kernel(const float* __restrict__ P, float* __restrict__ L, int N) {
    __shared__ float tile[32][33];
    __shared__ float part[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8
    const int r0 = blockIdx.x * 32;
    float deg[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < N; c0 += 32) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ly = ty + 8 * q, gr = c0 + ly, gc = r0 + tx;
            tile[ly][tx] = (gr < N && gc < N) ? P[(size_t)gr * N + gc] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = r0 + ty + 8 * q, col = c0 + tx;
            if (row < N && col < N && row != col) {
                const float m = 0.5f * (P[(size_t)row * N + col] + tile[tx][ty + 8 * q]);
                deg[q] += fabsf(m);
                L[(size_t)row * N + col] = 0.f - m;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) part[ty + 8 * q][tx] = deg[q];
    __syncthreads();
    if (threadIdx.x < 32) {
        const int row = r0 + threadIdx.x;
        if (row < N) {
            float d = 0.f;
            for (int t = 0; t < 32; ++t) d += part[threadIdx.x][t];
            L[(size_t)row * N + row] = d;
        }
    }
}

template <int R>
int launch_affinity(vp_ctx* ctx, const float* x, const float* xnT, const float* inv, float* P, int N, int D, int n_elems, hipStream_t st) {
    const int Dp = (D + 3) / 4 * 4;
    const size_t smem = ((size_t)R * N + (size_t)R * Dp) * 4;
    VP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(affinity_prune_kernel<R>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)smem));
    hipLaunchKernelGGL(affinity_prune_kernel<R>, dim3((N + R - 1) / R), dim3(256), smem, st, x, xnT, inv, P, N, D, Dp, n_elems);
    VP_LAUNCH_CHECK(ctx, "affinity_prune");
    return VP_OK;
}

}  // namespace

extern "C" {

int vp_chunk_batch_f32(vp_ctx* ctx, const float* wave, int wave_len, const int32_t* table, int N, int chunk_len, int normalize,
                       float target_db, float* out, vp_stream stream) {
    if (!ctx || !wave || !table || !out || wave_len <= 0 || N <= 0 || chunk_len <= 0) VP_FAIL(ctx, VP_EINVAL, "chunk_batch: bad arguments");
    ChunkArgs a{wave, table, out, wave_len, chunk_len, normalize, target_db};
    hipLaunchKernelGGL(chunk_batch_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, a);
    VP_LAUNCH_CHECK(ctx, "chunk_batch");
    return VP_OK;
}

size_t vp_affinity_prune_workspace_bytes(int N, int D) {
    if (N <= 0 || D <= 0) return 0;
    return vp_align_up((size_t)N * 4, 256) + vp_align_up((size_t)N * D * 4, 256);
}

int vp_affinity_prune_f32(vp_ctx* ctx, const float* emb, int N, int D, int n_elems, float* P, void* ws, size_t ws_bytes,
                          vp_stream stream) {
    if (!ctx || !emb || !P || N < 2 || N > 16384 || D < 1 || D > 1024 || n_elems < 0 || n_elems >= N)
        VP_FAIL(ctx, VP_EINVAL, "affinity_prune: bad arguments (2 <= N <= 16384, 1 <= D <= 1024, 0 <= n_elems < N)");
    if (!ws || ws_bytes < vp_affinity_prune_workspace_bytes(N, D)) VP_FAIL(ctx, VP_EWORKSPACE, "affinity_prune: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float* inv = (float*)ws;
    float* xnT = (float*)((char*)ws + vp_align_up((size_t)N * 4, 256));
    hipLaunchKernelGGL(affinity_prep_kernel, dim3((N + 63) / 64), dim3(256), 0, st, emb, N, D, inv, xnT);
    VP_LAUNCH_CHECK(ctx, "affinity_prep");
    // rows per workgroup: as many as keep the block's similarities within 64 KB of LDS
    if (N <= 2048) return launch_affinity<8>(ctx, emb, xnT, inv, P, N, D, n_elems, st);
    if (N <= 4096) return launch_affinity<4>(ctx, emb, xnT, inv, P, N, D, n_elems, st);
    if (N <= 8192) return launch_affinity<2>(ctx, emb, xnT, inv, P, N, D, n_elems, st);
    return launch_affinity<1>(ctx, emb, xnT, inv, P, N, D, n_elems, st);
}

int vp_laplacian_f32(vp_ctx* ctx, const float* P, int N, float* L, vp_stream stream) {
    if (!ctx || !P || !L || P == L || N < 1 || N > 16384) VP_FAIL(ctx, VP_EINVAL, "laplacian: bad arguments (out of place, 1 <= N <= 16384)");
    hipLaunchKernelGGL(laplacian_kernel, dim3((N + 31) / 32), dim3(256), 0, (hipStream_t)stream, P, L, N);
    VP_LAUNCH_CHECK(ctx, "laplacian");
    return VP_OK;
}

}  // extern "C"
