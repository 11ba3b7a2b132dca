// The k smallest eigenpairs of the diarization Laplacian (SpectralCluster.get_spec_embs: scipy.linalg.eigh of the whole N x N matrix, of
// which the eigen-gap rule reads 16 values and k-means at most 15 vectors) by Chebyshev-filtered subspace iteration on a block of
// P = 32 vectors.  L = diag(sum |M|) - M is symmetric positive semi-definite with its spectrum inside [0, sigma], sigma = 2 max L_ii
// (Gershgorin).  One round:
//   filter         Y = p_m(L) X, p_m the degree-m Chebyshev polynomial that is small on [a, sigma] (a = the block's largest Ritz value)
//                  and 1 at 0, by the three-term recurrence Y' = alpha L Y + beta Y + gamma Y_prev: per step one product kernel (L Y in
//                  slices of k) and one combine kernel (the slices added in order, then the recurrence);
//   Rayleigh-Ritz  W = L Y; G = Y^T Y and H = Y^T W as float64 partial sums per block of 128 rows, added in block order; in ONE
//                  workgroup: Cholesky G = C C^T, H' = C^-1 H C^-T, cyclic Jacobi on H' (31 steps of 16 disjoint rotations per sweep),
//                  eigenvalues ascending, T = C^-T Q; then X = Y T (float64 sums, rounded once: X^T X = I to f32 rounding) and the
//                  residuals |W T - lambda Y T|_2 from the same float64 sums.
// Products: the exact-f32 matrix cores (v_mfma_f32_32x32x2_f32), f32 in and out.  float64 only in the 32 x 32 problem, the Gram sums and
// the rotation.  No float atomics, no grid barrier, no host synchronisation: every global step is a launch, every sum has a fixed order,
// two runs give the same bits.  The convergence loop is the caller's (ppvector/infer_utils/speaker_diarization.py: smallest_eigenpairs).
#include "common.h"

namespace {

constexpr int P = 32;              // block size: k <= 24 wanted vectors and at least 8 guard vectors
constexpr int GRAM_ROWS = 128;     // rows of one Gram / rotation workgroup
constexpr int MAX_STEPS = 64;      // filter degree of one iterate call
constexpr int JACOBI_SWEEPS = 16;

typedef __attribute__((ext_vector_type(16))) float f32x16;

// A product L Y is cut along k into slices so that about 1024 workgroups stream L at once (N / 32 row blocks alone leave most of the
// 256 CUs waiting on their own loads); the slices' partial products are added in slice order by the combine kernel.
struct Slices { int count, len; };
Slices slices(int N) {
    const int row_blocks = (N + 31) / 32;
    int s = 1024 / row_blocks;
    s = s < 1 ? 1 : (s > 16 ? 16 : s);
    const int len = ((N + s - 1) / s + 7) / 8 * 8;                    // whole groups of the four waves' k pairs
    return Slices{(N + len - 1) / len, len};
}

// workspace: | State | X (home) | S0 | S1 | S2 | partial products | Gram partials | residual partials |
struct State {
    double sigma, upper;           // Gershgorin bound; largest Ritz value of the block (the filter's lower interval end)
    double lam[P];
    double T[P * P];               // row-major, column j belongs to the j-th smallest Ritz value
    float coef[MAX_STEPS * 4];     // alpha, beta, gamma of every filter step
};

struct Layout {
    State* st;
    float* X;
    float* S[3];
    float* part;                   // [slices][N][P]
    double* gram;                  // [blocks][2][P][P]
    double* rpart;                 // [blocks][P]
    size_t bytes;
};

// ws == nullptr: only `bytes` is filled in (the workspace query)
Layout layout(void* ws, int N) {
    const size_t blocks = (size_t)(N + GRAM_ROWS - 1) / GRAM_ROWS, vec = vp_align_up((size_t)N * P * 4, 256);
    Layout l{};
    size_t o = 0;
    auto take = [&](size_t bytes) {
        void* at = ws ? (void*)((char*)ws + o) : nullptr;
        o += bytes;
        return at;
    };
    l.st = (State*)take(vp_align_up(sizeof(State), 256));
    l.X = (float*)take(vec);
    for (int i = 0; i < 3; ++i) l.S[i] = (float*)take(vec);
    l.part = (float*)take(vec * (size_t)slices(N).count);
    l.gram = (double*)take(vp_align_up(blocks * 2 * P * P * 8, 256));
    l.rpart = (double*)take(vp_align_up(blocks * P * 8, 256));
    l.bytes = o;
    return l;
}

// ------------------------------------------------------------------------------------------------ bound and start block
__global__ __launch_bounds__(256) void eigs_bound_kernel(const float* __restrict__ L, int N, State* st) {
    __shared__ float red[256];
    float m = 0.f;
    for (int i = threadIdx.x; i < N; i += 256) m = fmaxf(m, L[(size_t)i * N + i]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) { st->sigma = 2.0 * (double)red[0]; st->upper = st->sigma; }
}

// X[i][j] = a hash of (i, j) in [-0.5, 0.5): no RNG state, the same block on every call
__global__ __launch_bounds__(256) void eigs_start_kernel(float* __restrict__ X, int N) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= N * P) return;
    unsigned h = (unsigned)(idx / P) * 0x9E3779B1u + (unsigned)(idx % P) * 0x85EBCA77u + 0x165667B1u;
    h ^= h >> 15; h *= 0x2C1B3C6Du;
    h ^= h >> 12; h *= 0x297A2D39u;
    h ^= h >> 15;
    X[idx] = (float)(h >> 8) * (1.0f / 16777216.0f) - 0.5f;
}

// The scaled Chebyshev recurrence on [a, b] = [upper, sigma], normalised to 1 at 0 (Zhou & Saad's filter with a0 = 0):
//   e = (b - a) / 2, c = (b + a) / 2, s_1 = -e / c, Y_1 = (s_1 / e) (L - c) X, s_{i+1} = 1 / (2 / s_1 - s_i),
//   Y_{i+1} = (2 s_{i+1} / e) (L - c) Y_i - s_i s_{i+1} Y_{i-1}.
// A degenerate interval (L = 0, or a block that already reaches sigma) makes every step the identity.
__global__ void eigs_coef_kernel(State* st, int steps) {
    if (threadIdx.x != 0) return;
    const double a = st->upper, b = st->sigma;
    const bool ok = b > 0.0 && b - a > 1e-6 * b && a >= 0.0;
    const double e = 0.5 * (b - a), c = 0.5 * (b + a), s1 = ok ? -e / c : 0.0;
    double s = s1;
    for (int i = 0; i < steps; ++i) {
        float* q = st->coef + 4 * i;
        if (!ok) { q[0] = 0.f; q[1] = 1.f; q[2] = 0.f; continue; }
        if (i == 0) { q[0] = (float)(s1 / e); q[1] = (float)(-c * s1 / e); q[2] = 0.f; continue; }
        const double s2 = 1.0 / (2.0 / s1 - s);
        q[0] = (float)(2.0 * s2 / e); q[1] = (float)(-2.0 * s2 * c / e); q[2] = (float)(-s * s2);
        s = s2;
    }
}

// ------------------------------------------------------------------------------------------------ L times a block
// part[slice] = L[:, slice's k] Y[slice's k].  One workgroup per 32 rows of the result and slice of k; L is exactly symmetric
// (vp_laplacian_f32), so the A operand A[i][k] = L[r0 + i][k] is read as L[k][r0 + i]: 32 consecutive floats of one row per half wave.
// The four waves take the slice's k pairs (2w, 2w + 1), (2w + 8, 2w + 9), ... and their 32 x 32 partial sums are added in wave order
// in LDS.
__global__ __launch_bounds__(256) void eigs_block_product_kernel(const float* __restrict__ L, int N, const float* __restrict__ Y,
                                                                 float* __restrict__ part, int slice_len) {
    __shared__ float red[4][16][64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r0 = blockIdx.x * 32, c = lane & 31, half = lane >> 5;
    const int r = r0 + c;
    const bool rv = r < N;
    const int rc = rv ? r : N - 1;
    const int kb = blockIdx.y * slice_len, ke = kb + slice_len < N ? kb + slice_len : N;
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    int k0 = kb + 2 * w;
    constexpr int U = 8;                                            // k pairs in flight per wave: 16 loads before the first MFMA
    for (; k0 + 8 * (U - 1) + 1 < ke; k0 += 8 * U) {                // every k of the U pairs is a row of the slice
        float a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = k0 + 8 * u + half;
            a[u] = L[(size_t)k * N + rc];
            b[u] = Y[(size_t)k * P + c];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(rv ? a[u] : 0.f, b[u], acc, 0, 0, 0);
    }
    for (; k0 < ke; k0 += 8) {
        const int k = k0 + half;
        const bool kv = k < ke;
        const int kc = kv ? k : N - 1;
        float a = L[(size_t)kc * N + rc];
        float b = Y[(size_t)kc * P + c];
        a = (kv && rv) ? a : 0.f;
        b = kv ? b : 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) red[w][v][lane] = acc[v];
    __syncthreads();
    float* o = part + (size_t)blockIdx.y * N * P;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int v = w + 4 * q;                                    // D[i][j]: j = lane & 31, i = 8 (v / 4) + 4 (lane / 32) + v % 4
        const int row = r0 + 8 * (v >> 2) + 4 * half + (v & 3);
        if (row < N) o[(size_t)row * P + c] = ((red[0][v][lane] + red[1][v][lane]) + red[2][v][lane]) + red[3][v][lane];
    }
}

// out = alpha (sum of the slices) + beta Y + gamma Yp (coef == nullptr: out = the sum), four elements per thread; n = N * 32
__global__ __launch_bounds__(256) void eigs_combine_kernel(const float* __restrict__ part, int count, int n, const float* __restrict__ Y,
                                                           const float* __restrict__ Yp, float* __restrict__ out,
                                                           const float* __restrict__ coef) {
    const int idx = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (idx >= n) return;                                            // n is a multiple of 32
    float s[4], y[4];
    vp_load4(part + idx, s);
    for (int i = 1; i < count; ++i) {
        vp_load4(part + (size_t)i * n + idx, y);
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] += y[q];
    }
    if (coef) {
        const float al = coef[0], be = coef[1], ga = coef[2];
        vp_load4(Y + idx, y);
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] = al * s[q] + be * y[q];
        if (ga != 0.f) {
            vp_load4(Yp + idx, y);
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] += ga * y[q];
        }
    }
    vp_store4(out + idx, s);
}

// ------------------------------------------------------------------------------------------------ Gram matrices
// part[block][0] = Y^T Y, part[block][1] = Y^T W over the block's rows, float64 (a product of two f32 is exact in it).
// Thread t: row a = t / 8 of both matrices, columns 4 (t % 8) .. + 3.
__global__ __launch_bounds__(256) void eigs_gram_kernel(const float* __restrict__ Y, const float* __restrict__ W, int N,
                                                        double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float ys[GRAM_ROWS][P];
    __shared__ __attribute__((aligned(16))) float wsh[GRAM_ROWS][P];
    const int tid = threadIdx.x, r0 = blockIdx.x * GRAM_ROWS;
    for (int idx = tid; idx < GRAM_ROWS * P; idx += 256) {
        const int row = r0 + idx / P;
        ys[idx / P][idx % P] = row < N ? Y[(size_t)r0 * P + idx] : 0.f;
        wsh[idx / P][idx % P] = row < N ? W[(size_t)r0 * P + idx] : 0.f;
    }
    __syncthreads();
    const int a = tid >> 3, b0 = 4 * (tid & 7);
    double g[4] = {0, 0, 0, 0}, h[4] = {0, 0, 0, 0};
    for (int r = 0; r < GRAM_ROWS; ++r) {
        const double ya = (double)ys[r][a];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            g[q] = fma(ya, (double)ys[r][b0 + q], g[q]);
            h[q] = fma(ya, (double)wsh[r][b0 + q], h[q]);
        }
    }
    double* o = part + (size_t)blockIdx.x * 2 * P * P;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        o[a * P + b0 + q] = g[q];
        o[P * P + a * P + b0 + q] = h[q];
    }
}

// ------------------------------------------------------------------------------------------------ the 32 x 32 problem
// One workgroup.  G, H from the partials (block order), Cholesky, whitening, Jacobi, sort, T = C^-T Q.
__global__ __launch_bounds__(256) void eigs_ritz_kernel(const double* __restrict__ part, int blocks, State* st) {
    __shared__ double G[P][P + 1], H[P][P + 1], V[P][P + 1], Ci[P][P + 1];
    __shared__ double rc[16], rs[16], sq[2][256];
    __shared__ int rp[16], rq[16], order[P];
    const int tid = threadIdx.x;
    for (int e = tid; e < P * P; e += 256) {
        double g = 0.0, h = 0.0;
        for (int b = 0; b < blocks; ++b) {
            g += part[(size_t)b * 2 * P * P + e];
            h += part[(size_t)b * 2 * P * P + P * P + e];
        }
        G[e / P][e % P] = g;
        V[e / P][e % P] = h;
    }
    __syncthreads();
    for (int e = tid; e < P * P; e += 256) {
        const int i = e / P, j = e % P;
        H[i][j] = 0.5 * (V[i][j] + V[j][i]);
        Ci[i][j] = 0.0;
    }
    __syncthreads();
    // Cholesky, lower factor in place (right-looking); the strict upper triangle of G is not read again
    for (int j = 0; j < P; ++j) {
        const double d = G[j][j];
        const double piv = d > 1e-300 ? sqrt(d) : 1e-150;          // a rank-deficient block: the caller sees residuals that do not fall
        __syncthreads();
        if (tid >= j && tid < P) G[tid][j] = tid == j ? piv : G[tid][j] / piv;
        __syncthreads();
        for (int e = tid; e < P * P; e += 256) {
            const int i = e / P, k = e % P;
            if (k > j && i >= k) G[i][k] -= G[i][j] * G[k][j];
        }
        __syncthreads();
    }
    // Ci = C^-1 (lower), one column per thread
    if (tid < P) {
        const int j = tid;
        Ci[j][j] = 1.0 / G[j][j];
        for (int i = j + 1; i < P; ++i) {
            double s = 0.0;
            for (int k = j; k < i; ++k) s += G[i][k] * Ci[k][j];
            Ci[i][j] = -s / G[i][i];
        }
    }
    __syncthreads();
    // V = Ci H;  G = sym(V Ci^T) = H'
    for (int e = tid; e < P * P; e += 256) {
        const int i = e / P, j = e % P;
        double s = 0.0;
        for (int k = 0; k <= i; ++k) s += Ci[i][k] * H[k][j];
        V[i][j] = s;
    }
    __syncthreads();
    for (int e = tid; e < P * P; e += 256) {
        const int i = e / P, j = e % P;
        double s = 0.0;
        for (int k = 0; k <= j; ++k) s += V[i][k] * Ci[j][k];
        H[i][j] = s;
    }
    __syncthreads();
    for (int e = tid; e < P * P; e += 256) {
        const int i = e / P, j = e % P;
        G[i][j] = 0.5 * (H[i][j] + H[j][i]);
        V[i][j] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    // cyclic Jacobi, round-robin order: step s pairs (31, s) and ((s + i) % 31, (s - i) % 31), i = 1..15 -- 16 disjoint rotations
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        double off = 0.0, dia = 0.0;                                  // sums of squares: four entries per thread, then a fixed tree
        for (int e = tid; e < P * P; e += 256) {
            const double v = G[e / P][e % P];
            (e / P == e % P ? dia : off) += v * v;
        }
        sq[0][tid] = off; sq[1][tid] = dia;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) { sq[0][tid] += sq[0][tid + o]; sq[1][tid] += sq[1][tid + o]; }
            __syncthreads();
        }
        const bool done = sq[0][0] <= 1e-28 * sq[1][0];
        __syncthreads();
        if (done) break;                                              // uniform
        for (int s = 0; s < P - 1; ++s) {
            if (tid < 16) {
                int p = tid == 0 ? P - 1 : (s + tid) % (P - 1), q = tid == 0 ? s : (s - tid + (P - 1)) % (P - 1);
                if (p > q) { const int t = p; p = q; q = t; }
                const double apq = G[p][q];
                double cs = 1.0, sn = 0.0;
                if (apq != 0.0) {
                    const double th = (G[q][q] - G[p][p]) / (2.0 * apq);
                    const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                    cs = 1.0 / sqrt(t * t + 1.0);
                    sn = t * cs;
                }
                rp[tid] = p; rq[tid] = q; rc[tid] = cs; rs[tid] = sn;
            }
            __syncthreads();
            for (int e = tid; e < 16 * P; e += 256) {                 // columns: G <- G J, V <- V J
                const int pr = e / P, i = e % P, p = rp[pr], q = rq[pr];
                const double cs = rc[pr], sn = rs[pr];
                const double gp = G[i][p], gq = G[i][q], vp = V[i][p], vq = V[i][q];
                G[i][p] = cs * gp - sn * gq; G[i][q] = sn * gp + cs * gq;
                V[i][p] = cs * vp - sn * vq; V[i][q] = sn * vp + cs * vq;
            }
            __syncthreads();
            for (int e = tid; e < 16 * P; e += 256) {                 // rows: G <- J^T G
                const int pr = e / P, i = e % P, p = rp[pr], q = rq[pr];
                const double cs = rc[pr], sn = rs[pr];
                const double gp = G[p][i], gq = G[q][i];
                G[p][i] = cs * gp - sn * gq; G[q][i] = sn * gp + cs * gq;
            }
            __syncthreads();
        }
    }
    // ascending order (equal values: lower index first)
    if (tid < P) {
        const double d = G[tid][tid];
        int rank = 0;
        for (int j = 0; j < P; ++j) {
            const double o = G[j][j];
            rank += (o < d || (o == d && j < tid)) ? 1 : 0;
        }
        order[rank] = tid;
        st->lam[rank] = d;
    }
    __syncthreads();
    if (tid == 0) st->upper = G[order[P - 1]][order[P - 1]];
    for (int e = tid; e < P * P; e += 256) {                          // T = Ci^T Q
        const int i = e / P, j = e % P, src = order[j];
        double s = 0.0;
        for (int k = i; k < P; ++k) s += Ci[k][i] * V[k][src];
        st->T[e] = s;
    }
}

// ------------------------------------------------------------------------------------------------ rotation, vectors, residuals
// X = Y T (rounded once), vecs = its first k columns, rpart[block][j] = sum over the block's rows of ((W T)_j - lambda_j (Y T)_j)^2.
// sigma == 0 (L = 0): the first k unit vectors.  256 threads = 8 rows x 32 columns per pass.
__global__ __launch_bounds__(256) void eigs_rotate_kernel(const float* __restrict__ Y, const float* __restrict__ W, int N, int k,
                                                          const State* __restrict__ st, float* __restrict__ X, float* __restrict__ vecs,
                                                          double* __restrict__ rpart) {
    __shared__ double T[P][P];
    __shared__ float ys[8][P], wsh[8][P];
    __shared__ double rr[8][P];
    const int tid = threadIdx.x, j = tid & 31, g = tid >> 5;
    for (int e = tid; e < P * P; e += 256) T[e / P][e % P] = st->T[e];
    const double lam = st->lam[j];
    const bool zero = !(st->sigma > 0.0);
    double acc = 0.0;
    for (int pass = 0; pass < GRAM_ROWS / 8; ++pass) {
        const int row = blockIdx.x * GRAM_ROWS + pass * 8 + g;
        __syncthreads();
        ys[g][j] = row < N ? Y[(size_t)row * P + j] : 0.f;
        wsh[g][j] = row < N ? W[(size_t)row * P + j] : 0.f;
        __syncthreads();
        double x = 0.0, wv = 0.0;
#pragma unroll 8
        for (int i = 0; i < P; ++i) {
            x = fma((double)ys[g][i], T[i][j], x);
            wv = fma((double)wsh[g][i], T[i][j], wv);
        }
        if (row < N) {
            X[(size_t)row * P + j] = (float)x;
            if (j < k) vecs[(size_t)row * k + j] = zero ? (row == j ? 1.f : 0.f) : (float)x;
            const double d = wv - lam * x;
            acc += d * d;
        }
    }
    rr[g][j] = acc;
    __syncthreads();
    if (tid < P) {
        double s = 0.0;
        for (int q = 0; q < 8; ++q) s += rr[q][tid];
        rpart[(size_t)blockIdx.x * P + tid] = s;
    }
}

// evals, resid (k each) and bounds = (sigma, the block's largest Ritz value): what the caller reads back once per round
__global__ void eigs_report_kernel(const State* __restrict__ st, const double* __restrict__ rpart, int blocks, int k,
                                   float* __restrict__ evals, float* __restrict__ resid, float* __restrict__ bounds) {
    const int j = threadIdx.x;
    const bool zero = !(st->sigma > 0.0);
    if (j < k) {
        double s = 0.0;
        for (int b = 0; b < blocks; ++b) s += rpart[(size_t)b * P + j];
        evals[j] = zero ? 0.f : (float)st->lam[j];
        resid[j] = zero ? 0.f : (float)sqrt(s);
    }
    if (j == 0) { bounds[0] = (float)st->sigma; bounds[1] = zero ? 0.f : (float)st->upper; }
}

int check_args(vp_ctx* ctx, const float* L, int N, int k, void* ws, size_t ws_bytes, float* evals, float* evecs, float* resid,
               float* bounds) {
    if (!ctx) return VP_EINVAL;
    if (k < 1 || k > 24) VP_FAIL(ctx, VP_EINVAL, "eigs: 1 <= k <= 24");
    if (N < 64 || N > 16384) VP_FAIL(ctx, VP_EUNSUP, "eigs: 64 <= N <= 16384");
    if (!L || !evals || !evecs || !resid || !bounds) VP_FAIL(ctx, VP_EINVAL, "eigs: null pointer");
    if (!ws || ws_bytes < vp_eigs_workspace_bytes(N, k)) VP_FAIL(ctx, VP_EWORKSPACE, "eigs: workspace too small");
    return VP_OK;
}

// out = alpha L Y + beta Y + gamma Yp (coef == nullptr: out = L Y); out is neither Y nor Yp
int product(vp_ctx* ctx, const float* L, int N, const Layout& l, const float* Y, const float* Yp, float* out, const float* coef,
            hipStream_t s) {
    const Slices sl = slices(N);
    hipLaunchKernelGGL(eigs_block_product_kernel, dim3((N + 31) / 32, sl.count), dim3(256), 0, s, L, N, Y, l.part, sl.len);
    VP_LAUNCH_CHECK(ctx, "eigs_block_product");
    hipLaunchKernelGGL(eigs_combine_kernel, dim3((N * P / 4 + 255) / 256), dim3(256), 0, s, (const float*)l.part, sl.count, N * P, Y, Yp,
                       out, coef);
    VP_LAUNCH_CHECK(ctx, "eigs_combine");
    return VP_OK;
}

// Rayleigh-Ritz on the block Y (W: a free buffer for L Y); the rotated block goes to `to`, which is neither
int rayleigh_ritz(vp_ctx* ctx, const float* L, int N, int k, const Layout& l, const float* Y, float* W, float* to, float* evals,
                  float* evecs, float* resid, float* bounds, hipStream_t s) {
    const int blocks = (N + GRAM_ROWS - 1) / GRAM_ROWS;
    if (int rc = product(ctx, L, N, l, Y, nullptr, W, nullptr, s)) return rc;
    hipLaunchKernelGGL(eigs_gram_kernel, dim3(blocks), dim3(256), 0, s, Y, (const float*)W, N, l.gram);
    VP_LAUNCH_CHECK(ctx, "eigs_gram");
    hipLaunchKernelGGL(eigs_ritz_kernel, dim3(1), dim3(256), 0, s, (const double*)l.gram, blocks, l.st);
    VP_LAUNCH_CHECK(ctx, "eigs_ritz");
    hipLaunchKernelGGL(eigs_rotate_kernel, dim3(blocks), dim3(256), 0, s, Y, (const float*)W, N, k, (const State*)l.st, to, evecs, l.rpart);
    VP_LAUNCH_CHECK(ctx, "eigs_rotate");
    hipLaunchKernelGGL(eigs_report_kernel, dim3(1), dim3(64), 0, s, (const State*)l.st, (const double*)l.rpart, blocks, k, evals, resid,
                       bounds);
    VP_LAUNCH_CHECK(ctx, "eigs_report");
    return VP_OK;
}

}  // namespace

extern "C" {

size_t vp_eigs_workspace_bytes(int N, int k) {
    if (N < 64 || N > 16384 || k < 1 || k > 24) return 0;
    return layout(nullptr, N).bytes;
}

int vp_eigs_init_f32(vp_ctx* ctx, const float* L, int N, int k, void* ws, size_t ws_bytes, float* evals, float* evecs, float* resid,
                     float* bounds, vp_stream stream) {
    if (int rc = check_args(ctx, L, N, k, ws, ws_bytes, evals, evecs, resid, bounds)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Layout l = layout(ws, N);
    hipLaunchKernelGGL(eigs_bound_kernel, dim3(1), dim3(256), 0, s, L, N, l.st);
    VP_LAUNCH_CHECK(ctx, "eigs_bound");
    hipLaunchKernelGGL(eigs_start_kernel, dim3((N * P + 255) / 256), dim3(256), 0, s, l.S[0], N);
    VP_LAUNCH_CHECK(ctx, "eigs_start");
    // orthonormalised by the Rayleigh-Ritz step itself, which also gives the first filter its interval
    return rayleigh_ritz(ctx, L, N, k, l, l.S[0], l.S[1], l.X, evals, evecs, resid, bounds, s);
}

int vp_eigs_iterate_f32(vp_ctx* ctx, const float* L, int N, int k, int steps, void* ws, size_t ws_bytes, float* evals, float* evecs,
                        float* resid, float* bounds, vp_stream stream) {
    if (int rc = check_args(ctx, L, N, k, ws, ws_bytes, evals, evecs, resid, bounds)) return rc;
    if (steps < 1 || steps > MAX_STEPS) VP_FAIL(ctx, VP_EINVAL, "eigs_iterate: 1 <= steps <= 64");
    hipStream_t s = (hipStream_t)stream;
    const Layout l = layout(ws, N);
    hipLaunchKernelGGL(eigs_coef_kernel, dim3(1), dim3(64), 0, s, l.st, steps);
    VP_LAUNCH_CHECK(ctx, "eigs_coef");
    // step i reads Y_i-1 (and Y_i-2) and writes S[i % 3]; the home block X is Y_0 and is free again after step 2
    const float* prev = nullptr;
    const float* cur = l.X;
    for (int i = 0; i < steps; ++i) {
        float* out = l.S[i % 3];
        if (int rc = product(ctx, L, N, l, cur, prev ? prev : cur, out, l.st->coef + 4 * i, s)) return rc;
        prev = cur;
        cur = out;
    }
    // cur = S[(steps - 1) % 3]; S[steps % 3] holds Y_steps-3 or nothing: free for W.  With steps == 1, prev is X itself, which the
    // rotation may overwrite only because it does not read it: it reads cur and W.
    return rayleigh_ritz(ctx, L, N, k, l, cur, l.S[steps % 3], l.X, evals, evecs, resid, bounds, s);
}

}  // extern "C"
