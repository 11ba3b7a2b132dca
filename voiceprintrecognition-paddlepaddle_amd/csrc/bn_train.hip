// The BatchNorm training unit (f32 engine and the wide mixed-precision layers): column sums over rows, the finalise of batch statistics,
// the apply pass y = z scale + shift, and the backward passes with the ReLU / Hardtanh masks and the fused bias gradient.  Who calls what,
// the argument contracts and the measured error: docs/bn_train.md.
//
// Reference: BatchNorm1D / BatchNorm2D in train mode (models/utils.py:96-119: batch statistics over (B, T); running = 0.9 running + 0.1
// batch) and their autograd.  Activations are position-major (M rows, C contiguous); every reduction is two-stage and fixed-order (no
// atomics, the partials summed by vp_launch_sum_partials of train_ops.hip): results are bit-reproducible run to run.
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------- column sums over rows
// part[chunk][which][c]: which 0 = sum_m a[m][c], 1 = sum_m a[m][c] * (b[m][c] - bmean[c]) * bscale[c]  (second only when b)
struct ColSumArgs { const float* a; const float* b; const float* bmean; const float* bscale; float* part; int lda, ldb, M, C, rows_per_chunk; };

__global__ __launch_bounds__(256) void col_sums_kernel(ColSumArgs p) {
    __shared__ float sm[2][4][64];
    const int lc = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lc;
    const int m0 = blockIdx.y * p.rows_per_chunk, m1 = min(p.M, m0 + p.rows_per_chunk);
    float s1 = 0.f, s2 = 0.f;
    if (c < p.C) {
        const float mu = p.b ? p.bmean[c] : 0.f, sc = p.b ? p.bscale[c] : 0.f;
        for (int m = m0 + rg; m < m1; m += 4) {
            const float av = p.a[(size_t)m * p.lda + c];
            s1 += av;
            if (p.b) s2 += av * (p.b[(size_t)m * p.ldb + c] - mu) * sc;
        }
    }
    sm[0][rg][lc] = s1; sm[1][rg][lc] = s2;
    __syncthreads();
    if (rg == 0 && c < p.C) {
        float* o = p.part + (size_t)blockIdx.y * 2 * p.C;
        o[c] = sm[0][0][lc] + sm[0][1][lc] + sm[0][2][lc] + sm[0][3][lc];
        o[p.C + c] = sm[1][0][lc] + sm[1][1][lc] + sm[1][2][lc] + sm[1][3][lc];
    }
}

// Four channels per lane (C and the row pitches multiples of 4, 16-byte aligned bases): a wave-instruction moves 1 KB of a row
// instead of 256 B, and four rows' loads are issued before the first add.  Workgroup = CL column lanes x (256 / CL) row groups
// over rows_per_chunk rows; CL = 64 / 32 / 16 by width so that 64-channel tensors (the Res2 convs) still fill the lanes.
#ifndef VP_BNBWD_ROWS
// rows in flight per thread of the BatchNorm-backward passes.  Round 5 A/B (tools/build_variant.sh u8 -DVP_BNBWD_ROWS=8, one box, one
// session): 8 rows 8.043 ms per ECAPA B = 256 training step, 4 rows 8.011 ms -- the passes are not short of loads in flight; 4 it stays
#define VP_BNBWD_ROWS 4
#endif
struct ColSum4Args { const float* a; const float* b; const float* bmean; const float* bscale; float* part; int lda, ldb, M, C4, rows_per_chunk, cl_shift;
                     const float* ms; const float* mh;      // optional: a counts only where b * ms + mh > 0 (a ReLU BEHIND the BatchNorm, resnet_se.py:72-74)
                     // UTT: the summed tensor is a * us[b] + um[b] * inv_t per utterance b = row / T -- the SE block's input gradient
                     // dh = dout * s + dmean / T (ecapa_tdnn.py:50-82 backward) formed on the fly, never stored
                     const float* us; const float* um; int T; float inv_t;
                     // UTT == 2: the summed tensor is a + us[b] + um[b] * bf16(b * xsc + xsh) -- the gradient that reaches a TDNNBlock's output y = BN(z)
                     // through its consumer's context statistics [mean_t y | std_t y] (pooling.py:97-104), affine in y per utterance and
                     // channel: us = alpha, um = beta of vp_time_stats_bwd_coeffs; y re-formed from the bf16 z the pass reads anyway
                     const float* xsc; const float* xsh;
                     float mask_hi; };     // with ms / mh: a also counts only where b * ms + mh < mask_hi (0: no upper bound) -- Hardtanh(0, 20) behind the BatchNorm (eres2net.py)

template <int UTT>
__device__ __forceinline__ void utt_affine4(float (&v)[4], const float* us, const float* um, int T, float inv_t, int C, int m, int c) {
    if constexpr (UTT == 1) {
        const size_t o = (size_t)(m / T) * C + c;
        float sv[4], dv[4];
        vp_load4(us + o, sv); vp_load4(um + o, dv);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __fmaf_rn(v[e], sv[e], dv[e] * inv_t);
    }
}

// UTT == 2: v += alpha[b] + beta[b] * bf16(z * xsc + xsh)
template <int UTT>
__device__ __forceinline__ void ctx_affine4(float (&v)[4], const float (&zv)[4], const float* ua, const float* ub, const float (&xsc)[4],
                                            const float (&xsh)[4], int T, int C, int m, int c) {
    if constexpr (UTT == 2) {
        const size_t o = (size_t)(m / T) * C + c;
        float al[4], be[4];
        vp_load4(ua + o, al); vp_load4(ub + o, be);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += __fmaf_rn(be[e], (float)(bf16_t)__fmaf_rn(zv[e], xsc[e], xsh[e]), al[e]);
    }
}

template <bool HASB, typename TB = float, int UTT = 0>
__global__ __launch_bounds__(256) void col_sums4_kernel(ColSum4Args p) {
    const TB* __restrict__ gb = reinterpret_cast<const TB*>(p.b);
    __shared__ float sm[2][256][4];
    const int CL = 1 << p.cl_shift, RG = 256 >> p.cl_shift;
    const int lc = threadIdx.x & (CL - 1), rg = threadIdx.x >> p.cl_shift;
    const int c4 = blockIdx.x * CL + lc, c = c4 * 4;
    const int m0 = blockIdx.y * p.rows_per_chunk, m1 = min(p.M, m0 + p.rows_per_chunk);
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    if (c4 < p.C4) {
        float mu[4] = {0.f, 0.f, 0.f, 0.f}, sc[4] = {0.f, 0.f, 0.f, 0.f};
        if (HASB) { vp_load4(p.bmean + c, mu); vp_load4(p.bscale + c, sc); }
        float ms[4] = {0.f, 0.f, 0.f, 0.f}, mh[4] = {1.f, 1.f, 1.f, 1.f};          // (no mask: 0 * b + 1 > 0 always)
        if (HASB && p.ms) { vp_load4(p.ms + c, ms); vp_load4(p.mh + c, mh); }
        float xsc[4] = {0.f, 0.f, 0.f, 0.f}, xsh[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (UTT == 2) { vp_load4(p.xsc + c, xsc); vp_load4(p.xsh + c, xsh); }
        int m = m0 + rg;
        // VP_BNBWD_ROWS rows per trip, their loads issued together, summed in row order
        constexpr int U = UTT ? 4 : VP_BNBWD_ROWS;              // (the per-utterance operands cost the registers of four rows)
        for (; m + (U - 1) * RG < m1; m += U * RG) {
            float av[U][4], bv[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                vp_load4(p.a + (size_t)(m + u * RG) * p.lda + c, av[u]);
                if (HASB) vp_load4(gb + (size_t)(m + u * RG) * p.ldb + c, bv[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                utt_affine4<UTT>(av[u], p.us, p.um, p.T, p.inv_t, p.C4 * 4, m + u * RG, c);
                if constexpr (HASB) ctx_affine4<UTT>(av[u], bv[u], p.us, p.um, xsc, xsh, p.T, p.C4 * 4, m + u * RG, c);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float g = av[u][e];
                    if constexpr (HASB) {
                        const float mv = (float)bv[u][e] * ms[e] + mh[e];
                        g = (mv > 0.f && (p.mask_hi == 0.f || mv < p.mask_hi)) ? g : 0.f;
                    }
                    s1[e] += g;
                    if (HASB) s2[e] += g * (bv[u][e] - mu[e]) * sc[e];
                }
        }
        for (; m < m1; m += RG) {
            float av[4], bv[4];
            vp_load4(p.a + (size_t)m * p.lda + c, av);
            if (HASB) vp_load4(gb + (size_t)m * p.ldb + c, bv);
            utt_affine4<UTT>(av, p.us, p.um, p.T, p.inv_t, p.C4 * 4, m, c);
            if constexpr (HASB) ctx_affine4<UTT>(av, bv, p.us, p.um, xsc, xsh, p.T, p.C4 * 4, m, c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float g = av[e];
                if constexpr (HASB) {
                    const float mv = (float)bv[e] * ms[e] + mh[e];
                    g = (mv > 0.f && (p.mask_hi == 0.f || mv < p.mask_hi)) ? g : 0.f;
                }
                s1[e] += g;
                if (HASB) s2[e] += g * (bv[e] - mu[e]) * sc[e];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { sm[0][threadIdx.x][e] = s1[e]; sm[1][threadIdx.x][e] = s2[e]; }
    __syncthreads();
    if (rg == 0 && c4 < p.C4) {
        float t1[4] = {0.f, 0.f, 0.f, 0.f}, t2[4] = {0.f, 0.f, 0.f, 0.f};
        for (int r = 0; r < RG; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) { t1[e] += sm[0][r * CL + lc][e]; t2[e] += sm[1][r * CL + lc][e]; }
        float* o = p.part + (size_t)blockIdx.y * 8 * p.C4;
        vp_store4(o + c, t1); vp_store4(o + 4 * p.C4 + c, t2);
    }
}

// ---------------------------------------------------------------------------------------------- BatchNorm, batch statistics
// from the producing conv's fused sums: mean / biased variance over all M rows, the folded affine for the apply pass,
// the saved mean / inverse std for backward, and the running statistics (Paddle: running = mom * running + (1 - mom) * batch).
struct BnFinArgs {
    const float* psum; const float* psumsq; int nparts; int M, C;
    const float* gamma; const float* beta; float* run_mean; float* run_var; float momentum, eps;
    float* mean; float* invstd; float* scale; float* shift;
    const unsigned* fault;      // the context's grid-barrier bail-out word: while it is set the running statistics are left untouched
};

// One workgroup = 16 channels x 16 part-lanes: the nparts partial rows (tiles x segments: ~1200 at B = 256 x 3 s) are
// summed 16 at a time with independent loads, then across the 16 lanes in fixed order.  (One thread per channel walking all
// the parts serially took 336 us per call -- 10 ms of a 54 ms training step.)
__global__ __launch_bounds__(256) void bn_train_finalize_kernel(BnFinArgs a) {
    __shared__ float sm[2][16][17];
    const int cl = threadIdx.x & 15, pl = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    float s1 = 0.f, s2 = 0.f;
    if (c < a.C) {
        // four partial rows per trip with their eight loads issued together (one load latency per trip instead of per row: the
        // ~75 rows per thread made this 25 us per call), summed in row order
        int k = pl;
        for (; k + 48 < a.nparts; k += 64) {
            float p[4], q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { p[u] = a.psum[(size_t)(k + 16 * u) * a.C + c]; q[u] = a.psumsq[(size_t)(k + 16 * u) * a.C + c]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) { s1 += p[u]; s2 += q[u]; }
        }
        for (; k < a.nparts; k += 16) { s1 += a.psum[(size_t)k * a.C + c]; s2 += a.psumsq[(size_t)k * a.C + c]; }
    }
    sm[0][pl][cl] = s1; sm[1][pl][cl] = s2;
    __syncthreads();
    if (pl != 0 || c >= a.C) return;
    s1 = 0.f; s2 = 0.f;
    for (int k = 0; k < 16; ++k) { s1 += sm[0][k][cl]; s2 += sm[1][k][cl]; }
    const float mu = s1 / (float)a.M;
    const float var = fmaxf(s2 / (float)a.M - mu * mu, 0.f);
    const float is = rsqrtf(var + a.eps);
    a.mean[c] = mu; a.invstd[c] = is;
    const float g = a.gamma ? a.gamma[c] : 1.f, be = a.beta ? a.beta[c] : 0.f;
    a.scale[c] = g * is;
    a.shift[c] = be - mu * g * is;
    // a fused training kernel upstream gave up at its grid barrier: this layer's batch statistics come from incomplete sums.  The step is
    // dropped by the optimiser kernels; the PERSISTENT state written here (the running statistics) must not see it either
    if (a.fault && __hip_atomic_load(a.fault, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;
    if (a.run_mean) a.run_mean[c] = a.momentum * a.run_mean[c] + (1.f - a.momentum) * mu;
    if (a.run_var) a.run_var[c] = a.momentum * a.run_var[c] + (1.f - a.momentum) * var;
}

// y = z * scale + shift
template <typename TZ, typename TY = float>
__global__ __launch_bounds__(256) void affine_rows_kernel(const TZ* z, int ldz, const float* scale, const float* shift, long long M,
                                                          int C4, TY* y, int ldy, int relu) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < M * C4; i += (long long)gridDim.x * 256) {
        const long long m = i / C4;
        const int c = (int)(i - m * C4) * 4;
        float v[4], s[4], h[4];
        vp_load4(z + m * ldz + c, v); vp_load4(scale + c, s); vp_load4(shift + c, h);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = __fmaf_rn(v[e], s[e], h[e]);
            if (relu) v[e] = fmaxf(v[e], 0.f);
            if (relu == 2) v[e] = fminf(v[e], 20.f);          // Hardtanh(0, 20)
        }
        vp_store4(y + m * ldy + c, v);
    }
}

// y = z * scale + shift into a channel slice of a wider tensor (ldy), and aux = y + add (add: another slice of a wider tensor):
// a Res2Net chunk's output written where the concatenation wants it, and the next chunk's input y_i + x_{i+1} from the same pass
struct AffAuxArgs { const float* z; const float* scale; const float* shift; float* y; const float* add; float* aux;
                    int ldz, ldy, ld_add, ld_aux, C4; long long M; };
__global__ __launch_bounds__(256) void affine_rows_aux_kernel(AffAuxArgs a) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.M * a.C4; i += (long long)gridDim.x * 256) {
        const long long m = i / a.C4;
        const int c = (int)(i - m * a.C4) * 4;
        float v[4], s[4], h[4];
        vp_load4(a.z + m * a.ldz + c, v); vp_load4(a.scale + c, s); vp_load4(a.shift + c, h);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] * s[e] + h[e];
        vp_store4(a.y + m * a.ldy + c, v);
        if (a.aux) {
            float ad[4];
            vp_load4(a.add + m * a.ld_add + c, ad);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += ad[e];
            vp_store4(a.aux + m * a.ld_aux + c, v);
        }
    }
}

// dz = [z > 0] * gamma * invstd * (dy - sum_dy / M - zhat * sum_dy_zhat / M),  zhat = (z - mean) * invstd
// (BatchNorm backward through y = BN(z), then the ReLU that produced z; relu_mask = 0 skips the mask)
struct BnBwdArgs {
    const float* dy; const float* z; const float* mean; const float* invstd; const float* gamma; const float* sums;   // sums [2][C]
    float* dz; int lddy, ldz, lddz, C4, relu_mask; long long M;
    const float* ms; const float* mh;       // optional: d y counts only where z * ms + mh > 0 (a ReLU BEHIND the BatchNorm)
    const float* us; const float* um; int T; float inv_t;      // bn_relu_bwd_dbias_kernel<.., UTT>: d y = dy * us[b] + um[b] * inv_t, b = row / T
    const float* xsc; const float* xsh;                        // UTT == 2: d y = dy + us[b] + um[b] * bf16(z * xsc + xsh) (see ColSum4Args)
    float mask_hi;                                             // with ms / mh: ... and z * ms + mh < mask_hi (0: no upper bound)
    int accumulate;                                            // bn_relu_bwd_kernel: dz += (a DenseNet block's shared gradient buffer, campplus.py:168-171)
};

__global__ __launch_bounds__(256) void bn_relu_bwd_kernel(BnBwdArgs a) {
    const float invM = 1.f / (float)a.M;
    const int C = a.C4 * 4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.M * a.C4; i += (long long)gridDim.x * 256) {
        const long long m = i / a.C4;
        const int c = (int)(i - m * a.C4) * 4;
        float dy[4], z[4], mu[4], is[4], g[4], s1[4], s2[4], o[4];
        vp_load4(a.dy + m * a.lddy + c, dy); vp_load4(a.z + m * a.ldz + c, z);
        vp_load4(a.mean + c, mu); vp_load4(a.invstd + c, is); vp_load4(a.sums + c, s1); vp_load4(a.sums + C + c, s2);
        if (a.gamma) vp_load4(a.gamma + c, g); else { g[0] = g[1] = g[2] = g[3] = 1.f; }
        if (a.ms) {
            float ms[4], mh[4];
            vp_load4(a.ms + c, ms); vp_load4(a.mh + c, mh);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float mv = z[e] * ms[e] + mh[e];
                dy[e] = (mv > 0.f && (a.mask_hi == 0.f || mv < a.mask_hi)) ? dy[e] : 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float zh = (z[e] - mu[e]) * is[e];
            const float v = g[e] * is[e] * (dy[e] - s1[e] * invM - zh * s2[e] * invM);
            o[e] = (a.relu_mask && !(z[e] > 0.f)) ? 0.f : v;
        }
        if (a.accumulate) {
            float old[4];
            vp_load4(a.dz + m * a.lddz + c, old);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] += old[e];
        }
        vp_store4(a.dz + m * a.lddz + c, o);
    }
}

// The same dz, laid out like col_sums4_kernel so that a lane keeps its four channels: the column sums of dz (the bias gradient of
// the conv in front of the ReLU) come out of the pass that writes dz instead of a second read of it.  part[chunk][C].
struct BnBwdSumArgs { BnBwdArgs b; float* part; int M, rows_per_chunk, cl_shift; };

// TO = bf16_t: dz leaves as bf16 (b.dz reinterpreted, lddz in elements) -- the operand the wide layers' data- and weight-gradient
// GEMMs read (they would round it to bf16 anyway); the column sums are of the unrounded values.
template <typename TO, typename TZ = float, int UTT = 0>
__global__ __launch_bounds__(256) void bn_relu_bwd_dbias_kernel(BnBwdSumArgs p) {
    __shared__ float sm[256][4];
    const BnBwdArgs& a = p.b;
    TO* __restrict__ gdz = reinterpret_cast<TO*>(a.dz);
    const TZ* __restrict__ gz = reinterpret_cast<const TZ*>(a.z);
    const int CL = 1 << p.cl_shift, RG = 256 >> p.cl_shift;
    const int lc = threadIdx.x & (CL - 1), rg = threadIdx.x >> p.cl_shift;
    const int c4 = blockIdx.x * CL + lc, c = c4 * 4, C = a.C4 * 4;
    const int m0 = blockIdx.y * p.rows_per_chunk, m1 = min(p.M, m0 + p.rows_per_chunk);
    const float invM = 1.f / (float)a.M;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (c4 < a.C4) {
        float mu[4], is[4], g[4], s1[4], s2[4];
        vp_load4(a.mean + c, mu); vp_load4(a.invstd + c, is); vp_load4(a.sums + c, s1); vp_load4(a.sums + C + c, s2);
        if (a.gamma) vp_load4(a.gamma + c, g); else { g[0] = g[1] = g[2] = g[3] = 1.f; }
        float xsc[4] = {0.f, 0.f, 0.f, 0.f}, xsh[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (UTT == 2) { vp_load4(a.xsc + c, xsc); vp_load4(a.xsh + c, xsh); }
        auto one = [&](const float* dy, const float* z, float* o) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float zh = (z[e] - mu[e]) * is[e];
                const float v = g[e] * is[e] * (dy[e] - s1[e] * invM - zh * s2[e] * invM);
                o[e] = (a.relu_mask && !(z[e] > 0.f)) ? 0.f : v;
                acc[e] += o[e];
            }
        };
        int m = m0 + rg;
        constexpr int U = UTT ? 4 : VP_BNBWD_ROWS;               // (rows in flight per thread: see col_sums4_kernel)
        for (; m + (U - 1) * RG < m1; m += U * RG) {
            float dy[U][4], z[U][4], o[4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                vp_load4(a.dy + (size_t)(m + u * RG) * a.lddy + c, dy[u]);
                vp_load4(gz + (size_t)(m + u * RG) * a.ldz + c, z[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                utt_affine4<UTT>(dy[u], a.us, a.um, a.T, a.inv_t, C, m + u * RG, c);
                ctx_affine4<UTT>(dy[u], z[u], a.us, a.um, xsc, xsh, a.T, C, m + u * RG, c);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) { one(dy[u], z[u], o); vp_store4(gdz + (size_t)(m + u * RG) * a.lddz + c, o); }
        }
        for (; m < m1; m += RG) {
            float dy[4], z[4], o[4];
            vp_load4(a.dy + (size_t)m * a.lddy + c, dy); vp_load4(gz + (size_t)m * a.ldz + c, z);
            utt_affine4<UTT>(dy, a.us, a.um, a.T, a.inv_t, C, m, c);
            ctx_affine4<UTT>(dy, z, a.us, a.um, xsc, xsh, a.T, C, m, c);
            one(dy, z, o);
            vp_store4(gdz + (size_t)m * a.lddz + c, o);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sm[threadIdx.x][e] = acc[e];
    __syncthreads();
    if (rg == 0 && c4 < a.C4) {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        for (int r = 0; r < RG; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] += sm[r * CL + lc][e];
        vp_store4(p.part + (size_t)blockIdx.y * C + c, t);
    }
}

// rows per chunk / chunks / lane split of the four-channels-per-lane kernels: ~1024 workgroups, at most 512 chunks
void colsum4_geometry(long long M, int C4, int& cl_shift, int& colblocks, int& rpc, int& chunks) {
    cl_shift = C4 >= 64 ? 6 : (C4 >= 32 ? 5 : 4);
    const int CL = 1 << cl_shift, RG = 256 >> cl_shift;
    colblocks = (C4 + CL - 1) / CL;
    long long ch = 1024 / colblocks;              // (more chunks cost more in the partial-sum reduce than they gain here)
    if (ch < 1) ch = 1;
    if (ch > 512) ch = 512;
    long long r = (M + ch - 1) / ch;
    if (r < 4 * RG) r = 4 * RG;
    rpc = (int)r;
    chunks = (int)((M + r - 1) / r);
}

// The optional per-utterance term of the bf16 forms (utterance = row / T; u0, u1 (M / T, C) f32, 16-byte aligned):
// kind 1 (_utt): the gradient is dy * u0 + u1 / T (in front of an SE block); kind 2 (_ctx): dy + u0 + u1 * bf16(z * bn_scale + bn_shift)
// (in front of context statistics: u0 = alpha, u1 = beta of vp_time_stats_bwd_coeffs); kind 0: none
struct UttTerm { int kind; const float* u0; const float* u1; int T; const float* bn_scale; const float* bn_shift; };

bool utt_term_ok(const UttTerm& u, long long M) {
    if (!u.kind) return true;
    return u.u0 && u.u1 && u.T > 0 && M % u.T == 0 && (((uintptr_t)u.u0 | (uintptr_t)u.u1) & 15) == 0 && (u.kind != 2 || (u.bn_scale && u.bn_shift));
}

// sums [2][C]: sum_m a[m][c] and (when b) sum_m a[m][c] * (b[m][c] - bmean[c]) * bscale[c]
int col_sums_impl(vp_ctx* ctx, const float* a, int lda, const float* b, int ldb, const float* bmean, const float* bscale,
                  const float* mask_scale, const float* mask_shift, long long M, int C, float* sums, void* ws, size_t ws_bytes,
                  vp_stream stream, float mask_hi = 0.f) {
    if (!ctx || !a || !sums || M <= 0 || C <= 0 || (b && (!bmean || !bscale))) VP_FAIL(ctx, VP_EINVAL, "col_sums: bad arguments");
    if (!ws || ws_bytes < vp_col_sums_workspace_bytes(M, C)) VP_FAIL(ctx, VP_EWORKSPACE, "col_sums: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    long long chunks;
    if (M > 0x7fffffffLL) VP_FAIL(ctx, VP_EINVAL, "col_sums: more than 2^31 rows");
    if (((C | lda | (b ? ldb : 0)) & 3) == 0 && (((uintptr_t)a | (uintptr_t)(b ? b : a)) & 15) == 0) {
        int cl_shift, colblocks, rpc, ch;
        colsum4_geometry(M, C / 4, cl_shift, colblocks, rpc, ch);
        chunks = ch;
        ColSum4Args p{a, b, bmean, bscale, (float*)ws, lda, ldb, (int)M, C / 4, rpc, cl_shift, mask_scale, mask_shift};
        p.mask_hi = mask_hi;
        if (b) hipLaunchKernelGGL(col_sums4_kernel<true>, dim3(colblocks, (unsigned)chunks), dim3(256), 0, st, p);
        else hipLaunchKernelGGL(col_sums4_kernel<false>, dim3(colblocks, (unsigned)chunks), dim3(256), 0, st, p);
    } else {
        chunks = (M + 511) / 512;
        if (chunks > 1024) chunks = 1024;
        const int rpc = (int)((M + chunks - 1) / chunks);
        chunks = (M + rpc - 1) / rpc;
        ColSumArgs p{a, b, bmean, bscale, (float*)ws, lda, ldb, (int)M, C, rpc};
        hipLaunchKernelGGL(col_sums_kernel, dim3((C + 63) / 64, (unsigned)chunks), dim3(256), 0, st, p);
    }
    VP_LAUNCH_CHECK(ctx, "col_sums");
    vp_launch_sum_partials((const float*)ws, (int)chunks, (long long)2 * C, sums, st);
    VP_LAUNCH_CHECK(ctx, "col_sums_reduce");
    return VP_OK;
}

// the same two sums with b stored as bf16 (ldb in elements) and the optional per-utterance term on a; `who` names the entry point
int col_sums_b16_impl(vp_ctx* ctx, const char* who, const float* a, int lda, const UttTerm& u, const void* b, int ldb, const float* bmean,
                      const float* bscale, long long M, int C, float* sums, void* ws, size_t ws_bytes, vp_stream stream) {
    if (!ctx || !a || !b || !bmean || !bscale || !sums || M <= 0 || M > 0x7fffffffLL || C <= 0 || (C | lda | ldb) & 3 ||
        ((uintptr_t)a & 15) || ((uintptr_t)b & 7) || !utt_term_ok(u, M))
        VP_FAIL(ctx, VP_EINVAL, "%s: bad arguments", who);
    if (!ws || ws_bytes < vp_col_sums_workspace_bytes(M, C)) VP_FAIL(ctx, VP_EWORKSPACE, "%s: workspace too small", who);
    int cl_shift, colblocks, rpc, chunks;
    colsum4_geometry(M, C / 4, cl_shift, colblocks, rpc, chunks);
    ColSum4Args p{a, (const float*)b, bmean, bscale, (float*)ws, lda, ldb, (int)M, C / 4, rpc, cl_shift, nullptr, nullptr, u.u0, u.u1,
                  u.kind ? u.T : 1, u.kind == 1 ? 1.f / (float)u.T : 0.f, u.bn_scale, u.bn_shift};
    const dim3 grid(colblocks, (unsigned)chunks);
    hipStream_t st = (hipStream_t)stream;
    if (u.kind == 2) hipLaunchKernelGGL((col_sums4_kernel<true, bf16_t, 2>), grid, dim3(256), 0, st, p);
    else if (u.kind == 1) hipLaunchKernelGGL((col_sums4_kernel<true, bf16_t, 1>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((col_sums4_kernel<true, bf16_t>), grid, dim3(256), 0, st, p);
    VP_LAUNCH_CHECK(ctx, "col_sums_b16");
    vp_launch_sum_partials((const float*)ws, chunks, (long long)2 * C, sums, st);
    VP_LAUNCH_CHECK(ctx, "col_sums_b16_reduce");
    return VP_OK;
}

template <typename TZ, typename TY>
int affine_rows_impl(vp_ctx* ctx, const char* who, const void* z, int ldz, const float* scale, const float* shift, long long M, int C,
                     void* y, int ldy, int relu, vp_stream stream) {
    if (!ctx || !z || !scale || !shift || !y || M <= 0 || C <= 0 || (C | ldz | ldy) & 3) VP_FAIL(ctx, VP_EINVAL, "%s: bad arguments", who);
    hipLaunchKernelGGL((affine_rows_kernel<TZ, TY>), dim3(grid1d(M * (C / 4))), dim3(256), 0, (hipStream_t)stream, (const TZ*)z, ldz, scale,
                       shift, M, C / 4, (TY*)y, ldy, relu);
    VP_LAUNCH_CHECK(ctx, "affine_rows");
    return VP_OK;
}

// dz and dbias = sum_m dz in one pass; z and dz f32 or bf16 (f32 operands 16-byte, bf16 8-byte aligned), the optional per-utterance
// term on dy (bf16 z and dz only); `who` names the entry point
int bn_bwd_dbias_impl(vp_ctx* ctx, const char* who, const float* dy, int lddy, const UttTerm& u, const void* z, int ldz, bool z_bf16,
                      const float* mean, const float* invstd, const float* gamma, const float* sums, long long M, int C, int relu_mask,
                      void* dz, int lddz, bool dz_bf16, float* dbias, void* ws, size_t ws_bytes, vp_stream stream) {
    if (!ctx || !dy || !z || !mean || !invstd || !sums || !dz || !dbias || M <= 0 || M > 0x7fffffffLL || C <= 0 ||
        (C | lddy | ldz | lddz) & 3 || ((uintptr_t)dy & 15) || ((uintptr_t)z & (z_bf16 ? 7 : 15)) || ((uintptr_t)dz & (dz_bf16 ? 7 : 15)) ||
        (z_bf16 && !dz_bf16) || !utt_term_ok(u, M))
        VP_FAIL(ctx, VP_EINVAL, "%s: bad arguments", who);
    if (!ws || ws_bytes < vp_bn_relu_bwd_dbias_workspace_bytes(M, C)) VP_FAIL(ctx, VP_EWORKSPACE, "%s: workspace too small", who);
    int cl_shift, colblocks, rpc, chunks;
    colsum4_geometry(M, C / 4, cl_shift, colblocks, rpc, chunks);
    BnBwdSumArgs p{{dy, (const float*)z, mean, invstd, gamma, sums, (float*)dz, lddy, ldz, lddz, C / 4, relu_mask, M, nullptr, nullptr,
                    u.u0, u.u1, u.kind ? u.T : 0, u.kind == 1 ? 1.f / (float)u.T : 0.f, u.bn_scale, u.bn_shift}, (float*)ws, (int)M, rpc, cl_shift};
    const dim3 grid(colblocks, (unsigned)chunks);
    hipStream_t st = (hipStream_t)stream;
    if (u.kind == 2) hipLaunchKernelGGL((bn_relu_bwd_dbias_kernel<bf16_t, bf16_t, 2>), grid, dim3(256), 0, st, p);
    else if (u.kind == 1) hipLaunchKernelGGL((bn_relu_bwd_dbias_kernel<bf16_t, bf16_t, 1>), grid, dim3(256), 0, st, p);
    else if (z_bf16) hipLaunchKernelGGL((bn_relu_bwd_dbias_kernel<bf16_t, bf16_t>), grid, dim3(256), 0, st, p);
    else if (dz_bf16) hipLaunchKernelGGL(bn_relu_bwd_dbias_kernel<bf16_t>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(bn_relu_bwd_dbias_kernel<float>, grid, dim3(256), 0, st, p);
    VP_LAUNCH_CHECK(ctx, "bn_relu_bwd_dbias");
    vp_launch_sum_partials((const float*)ws, chunks, (long long)C, dbias, st);
    VP_LAUNCH_CHECK(ctx, "bn_relu_bwd_dbias_reduce");
    return VP_OK;
}

}  // namespace

extern "C" {

size_t vp_col_sums_workspace_bytes(long long M, int C) {
    (void)M;
    return (size_t)1024 * 2 * C * sizeof(float) + 256;
}

int vp_col_sums_f32(vp_ctx* ctx, const float* a, int lda, const float* b, int ldb, const float* bmean, const float* bscale,
                    long long M, int C, float* sums, void* ws, size_t ws_bytes, vp_stream stream) {
    return col_sums_impl(ctx, a, lda, b, ldb, bmean, bscale, nullptr, nullptr, M, C, sums, ws, ws_bytes, stream);
}

// BatchNorm -> ReLU units (resnet_se.py:72-74, eres2net.py): the ReLU's backward folded into the two BatchNorm-backward passes.  a (= d y)
// counts only where the unit's output b * mask_scale + mask_shift (the BatchNorm affine of the saved pre-BN tensor b) was positive -- the
// same expression the forward's vp_affine_rows_f32 evaluates.  C % 4 == 0, 16-byte aligned; else VP_EUNSUP.
int vp_col_sums_masked_f32(vp_ctx* ctx, const float* a, int lda, const float* b, int ldb, const float* bmean, const float* bscale,
                           const float* mask_scale, const float* mask_shift, float mask_hi, long long M, int C, float* sums, void* ws,
                           size_t ws_bytes, vp_stream stream) {
    if (!b || !mask_scale || !mask_shift || mask_hi < 0.f) VP_FAIL(ctx, VP_EINVAL, "col_sums_masked: bad arguments");
    if (((C | lda | ldb) & 3) || (((uintptr_t)a | (uintptr_t)b) & 15)) return VP_EUNSUP;
    return col_sums_impl(ctx, a, lda, b, ldb, bmean, bscale, mask_scale, mask_shift, M, C, sums, ws, ws_bytes, stream, mask_hi);
}

// b stored as bf16: the BatchNorm-backward reductions over a bf16 pre-BN activation
int vp_col_sums_f32_b16(vp_ctx* ctx, const float* a, int lda, const void* b, int ldb, const float* bmean, const float* bscale, long long M,
                        int C, float* sums, void* ws, size_t ws_bytes, vp_stream stream) {
    return col_sums_b16_impl(ctx, "col_sums_b16", a, lda, UttTerm{}, b, ldb, bmean, bscale, M, C, sums, ws, ws_bytes, stream);
}

// the same sums of a * us[b] + um[b] / T (b = row / T): the BatchNorm-backward reductions of the conv in front of an SE block, with the
// SE block's input gradient dh = dout * s + dmean / T formed on the fly (vp_scale_shift_rows_f32 never runs)
int vp_col_sums_f32_b16_utt(vp_ctx* ctx, const float* a, int lda, const float* utt_scale, const float* utt_shift, int T, const void* b, int ldb,
                            const float* bmean, const float* bscale, long long M, int C, float* sums, void* ws, size_t ws_bytes, vp_stream stream) {
    return col_sums_b16_impl(ctx, "col_sums_b16_utt", a, lda, UttTerm{1, utt_scale, utt_shift, T, nullptr, nullptr}, b, ldb, bmean, bscale, M, C,
                             sums, ws, ws_bytes, stream);
}

// The BatchNorm-backward reductions of a TDNNBlock whose output y = BN(z) is consumed by a pooling layer's context statistics: d y =
// dy + alpha[b] + beta[b] * bf16(z * bn_scale + bn_shift) (vp_time_stats_bwd_coeffs), y re-formed from the bf16 z the passes read anyway --
// vp_time_stats_bwd_add_x16's pass over the (B*T, C) tensors never runs
int vp_col_sums_f32_b16_ctx(vp_ctx* ctx, const float* a, int lda, const float* alpha, const float* beta, int T, const float* bn_scale,
                            const float* bn_shift, const void* b, int ldb, const float* bmean, const float* bscale, long long M, int C, float* sums,
                            void* ws, size_t ws_bytes, vp_stream stream) {
    return col_sums_b16_impl(ctx, "col_sums_b16_ctx", a, lda, UttTerm{2, alpha, beta, T, bn_scale, bn_shift}, b, ldb, bmean, bscale, M, C, sums,
                             ws, ws_bytes, stream);
}

int vp_bn_train_finalize(vp_ctx* ctx, const float* psum, const float* psumsq, int nparts, long long M, int C, const float* gamma,
                         const float* beta, float* running_mean, float* running_var, float momentum, float eps, float* mean,
                         float* invstd, float* scale, float* shift, vp_stream stream) {
    if (!ctx || !psum || !psumsq || nparts <= 0 || M <= 0 || C <= 0 || !mean || !invstd || !scale || !shift)
        VP_FAIL(ctx, VP_EINVAL, "bn_finalize: bad arguments");
    BnFinArgs a{psum, psumsq, nparts, (int)M, C, gamma, beta, running_mean, running_var, momentum, eps, mean, invstd, scale, shift, vp_fault_word(ctx)};
    hipLaunchKernelGGL(bn_train_finalize_kernel, dim3((C + 15) / 16), dim3(256), 0, (hipStream_t)stream, a);
    VP_LAUNCH_CHECK(ctx, "bn_train_finalize");
    return VP_OK;
}

// the apply pass y = z scale + shift [relu 1: max(., 0); 2: Hardtanh(0, 20)]
int vp_affine_rows_f32(vp_ctx* ctx, const float* z, int ldz, const float* scale, const float* shift, long long M, int C, float* y,
                       int ldy, int relu, vp_stream stream) {
    return affine_rows_impl<float, float>(ctx, "affine_rows", z, ldz, scale, shift, M, C, y, ldy, relu, stream);
}

// z stored as bf16 (the wide mixed-precision layers keep the conv output in the low precision, as Paddle's O1 does): y f32
int vp_affine_rows_b16_f32(vp_ctx* ctx, const void* z, int ldz, const float* scale, const float* shift, long long M, int C, float* y,
                           int ldy, int relu, vp_stream stream) {
    return affine_rows_impl<bf16_t, float>(ctx, "affine_rows_b16", z, ldz, scale, shift, M, C, y, ldy, relu, stream);
}

// z AND y bf16: a layer output whose only consumers read it as bf16 (ECAPA's MFA output under enable_amp: ASP's GEMM operand and statistics)
int vp_affine_rows_b16_b16(vp_ctx* ctx, const void* z, int ldz, const float* scale, const float* shift, long long M, int C, void* y,
                           int ldy, int relu, vp_stream stream) {
    return affine_rows_impl<bf16_t, bf16_t>(ctx, "affine_rows_b16_b16", z, ldz, scale, shift, M, C, y, ldy, relu, stream);
}

// z f32, y bf16 (a layer outside the wide set whose only consumers read bf16: ECAPA's block 0 under enable_amp)
int vp_affine_rows_f32_b16(vp_ctx* ctx, const float* z, int ldz, const float* scale, const float* shift, long long M, int C, void* y,
                           int ldy, int relu, vp_stream stream) {
    return affine_rows_impl<float, bf16_t>(ctx, "affine_rows_f32_b16", z, ldz, scale, shift, M, C, y, ldy, relu, stream);
}

int vp_affine_rows_aux_f32(vp_ctx* ctx, const float* z, int ldz, const float* scale, const float* shift, long long M, int C, float* y, int ldy,
                           const float* add, int ld_add, float* aux, int ld_aux, vp_stream stream) {
    if (!ctx || !z || !scale || !shift || !y || M <= 0 || C <= 0 || (C | ldz | ldy) & 3 || (aux && (!add || (ld_add | ld_aux) & 3)) ||
        (((uintptr_t)z | (uintptr_t)y | (uintptr_t)add | (uintptr_t)aux) & 15))
        VP_FAIL(ctx, VP_EINVAL, "affine_rows_aux: bad arguments");
    AffAuxArgs a{z, scale, shift, y, add, aux, ldz, ldy, ld_add, ld_aux, C / 4, M};
    hipLaunchKernelGGL(affine_rows_aux_kernel, dim3(grid1d(M * (C / 4))), dim3(256), 0, (hipStream_t)stream, a);
    VP_LAUNCH_CHECK(ctx, "affine_rows_aux");
    return VP_OK;
}

int vp_bn_relu_bwd_f32(vp_ctx* ctx, const float* dy, int lddy, const float* z, int ldz, const float* mean, const float* invstd,
                       const float* gamma, const float* sums, long long M, int C, int relu_mask, float* dz, int lddz,
                       vp_stream stream) {
    if (!ctx || !dy || !z || !mean || !invstd || !sums || !dz || M <= 0 || C <= 0 || (C | lddy | ldz | lddz) & 3)
        VP_FAIL(ctx, VP_EINVAL, "bn_relu_bwd: bad arguments");
    BnBwdArgs a{dy, z, mean, invstd, gamma, sums, dz, lddy, ldz, lddz, C / 4, relu_mask, M, nullptr, nullptr};
    hipLaunchKernelGGL(bn_relu_bwd_kernel, dim3(grid1d(M * (C / 4))), dim3(256), 0, (hipStream_t)stream, a);
    VP_LAUNCH_CHECK(ctx, "bn_relu_bwd");
    return VP_OK;
}

// BatchNorm backward with a ReLU BEHIND the BatchNorm folded in (see vp_col_sums_masked_f32): d y counts only where z * mask_scale + mask_shift > 0
int vp_bn_relu_bwd_masked_f32(vp_ctx* ctx, const float* dy, int lddy, const float* z, int ldz, const float* mean, const float* invstd,
                              const float* gamma, const float* sums, const float* mask_scale, const float* mask_shift, float mask_hi,
                              long long M, int C, float* dz, int lddz, int accumulate, vp_stream stream) {
    if (!ctx || !dy || !z || !mean || !invstd || !sums || !dz || !mask_scale || !mask_shift || mask_hi < 0.f || M <= 0 || C <= 0 ||
        (C | lddy | ldz | lddz) & 3)
        VP_FAIL(ctx, VP_EINVAL, "bn_relu_bwd_masked: bad arguments");
    BnBwdArgs a{dy, z, mean, invstd, gamma, sums, dz, lddy, ldz, lddz, C / 4, 0, M, mask_scale, mask_shift};
    a.mask_hi = mask_hi;
    a.accumulate = accumulate != 0;
    hipLaunchKernelGGL(bn_relu_bwd_kernel, dim3(grid1d(M * (C / 4))), dim3(256), 0, (hipStream_t)stream, a);
    VP_LAUNCH_CHECK(ctx, "bn_relu_bwd_masked");
    return VP_OK;
}

size_t vp_bn_relu_bwd_dbias_workspace_bytes(long long M, int C) {
    (void)M;
    return (size_t)1024 * C * sizeof(float) + 256;
}

int vp_bn_relu_bwd_dbias_f32(vp_ctx* ctx, const float* dy, int lddy, const float* z, int ldz, const float* mean, const float* invstd,
                             const float* gamma, const float* sums, long long M, int C, int relu_mask, float* dz, int lddz,
                             float* dbias, void* ws, size_t ws_bytes, vp_stream stream) {
    return bn_bwd_dbias_impl(ctx, "bn_relu_bwd_dbias", dy, lddy, UttTerm{}, z, ldz, false, mean, invstd, gamma, sums, M, C, relu_mask, dz, lddz,
                             false, dbias, ws, ws_bytes, stream);
}

// the same with dz written as bf16 (lddz in elements): see bn_relu_bwd_dbias_kernel
int vp_bn_relu_bwd_dbias_bf16out(vp_ctx* ctx, const float* dy, int lddy, const float* z, int ldz, const float* mean, const float* invstd,
                                 const float* gamma, const float* sums, long long M, int C, int relu_mask, void* dz, int lddz,
                                 float* dbias, void* ws, size_t ws_bytes, vp_stream stream) {
    return bn_bwd_dbias_impl(ctx, "bn_relu_bwd_dbias_bf16out", dy, lddy, UttTerm{}, z, ldz, false, mean, invstd, gamma, sums, M, C, relu_mask,
                             dz, lddz, true, dbias, ws, ws_bytes, stream);
}

// z AND dz bf16: the wide layers with the pre-BN activation kept in the low precision
int vp_bn_relu_bwd_dbias_b16(vp_ctx* ctx, const float* dy, int lddy, const void* z, int ldz, const float* mean, const float* invstd,
                             const float* gamma, const float* sums, long long M, int C, int relu_mask, void* dz, int lddz,
                             float* dbias, void* ws, size_t ws_bytes, vp_stream stream) {
    return bn_bwd_dbias_impl(ctx, "bn_relu_bwd_dbias_b16", dy, lddy, UttTerm{}, z, ldz, true, mean, invstd, gamma, sums, M, C, relu_mask, dz,
                             lddz, true, dbias, ws, ws_bytes, stream);
}

// z AND dz bf16, d y = dy * utt_scale[b] + utt_shift[b] / T (b = row / T) formed on the fly: BatchNorm + ReLU backward of the conv in
// front of an SE block straight from the block's OUTPUT gradient (see vp_col_sums_f32_b16_utt)
int vp_bn_relu_bwd_dbias_b16_utt(vp_ctx* ctx, const float* dy, int lddy, const float* utt_scale, const float* utt_shift, int T, const void* z,
                                 int ldz, const float* mean, const float* invstd, const float* gamma, const float* sums, long long M, int C,
                                 int relu_mask, void* dz, int lddz, float* dbias, void* ws, size_t ws_bytes, vp_stream stream) {
    return bn_bwd_dbias_impl(ctx, "bn_relu_bwd_dbias_utt", dy, lddy, UttTerm{1, utt_scale, utt_shift, T, nullptr, nullptr}, z, ldz, true, mean,
                             invstd, gamma, sums, M, C, relu_mask, dz, lddz, true, dbias, ws, ws_bytes, stream);
}

// the same for d y = dy + alpha[b] + beta[b] * bf16(z * bn_scale + bn_shift) (see vp_col_sums_f32_b16_ctx)
int vp_bn_relu_bwd_dbias_b16_ctx(vp_ctx* ctx, const float* dy, int lddy, const float* alpha, const float* beta, int T, const float* bn_scale,
                                 const float* bn_shift, const void* z, int ldz, const float* mean, const float* invstd, const float* gamma,
                                 const float* sums, long long M, int C, int relu_mask, void* dz, int lddz, float* dbias, void* ws,
                                 size_t ws_bytes, vp_stream stream) {
    return bn_bwd_dbias_impl(ctx, "bn_relu_bwd_dbias_ctx", dy, lddy, UttTerm{2, alpha, beta, T, bn_scale, bn_shift}, z, ldz, true, mean, invstd,
                             gamma, sums, M, C, relu_mask, dz, lddz, true, dbias, ws, ws_bytes, stream);
}

}  // extern "C"
