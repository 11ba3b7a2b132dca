// Training-side kernels (f32 engine): the conv weight layouts and bf16 weight panels, Adam, momentum, gradient packing, the
// per-utterance (ASP) and CAM++ context pieces and the activations.  The conv weight gradient (and the partial-sum reducer other
// files borrow) is in wgrad.hip; BatchNorm with batch statistics and the column sums are in bn_train.hip.
//
// Reference: what paddle's autograd + optimiser run for PPVectorTrainer.__train_epoch (ppvector/trainer.py:202-274):
// the layers of models/utils.py:65-148, ReLU, and Adam with coupled L2 (optimizer/__init__.py:12-18, configs/*.yml weight_decay
// 1e-6).  Activations are position-major (M = B*T rows, C contiguous) like everywhere else; every reduction is two-stage and
// fixed-order (no atomics): results are bit-reproducible run to run.
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------- conv weight layouts
// wp[o][tap * Cin + c] = w[o][c][tap] (the forward kernel's weight panel) and w2[c][(KW - 1 - tap) * Cout + o] = w[o][c][tap]
// (the data-gradient conv's: taps reversed, channel roles swapped) from the model's (Cout, Cin, KW) tensor in one launch.
// 2-D (KF > 1): the model stores (Cout, Cin, KF, KT), tap kf * KT + kt; the kernels' tap order is kt * KF + kf (KW = KF * KT taps).
__global__ __launch_bounds__(256) void weight_layouts_kernel(const float* w, int Cout, int Cin, int KW, int KF, float* wp, float* w2) {
    const long long n = (long long)Cout * Cin * KW;
    const int KT = KW / KF;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int o = (int)(i / ((long long)Cin * KW));
        const int r = (int)(i - (long long)o * Cin * KW);
        const int c = r / KW;
        int j = r - c * KW;
        if (KF > 1) j = (j % KT) * KF + j / KT;
        const float v = w[i];
        if (wp) wp[((size_t)o * KW + j) * Cin + c] = v;
        if (w2) w2[((size_t)c * KW + (KW - 1 - j)) * Cout + o] = v;
    }
}

// ---------------------------------------------------------------------------------------------- bf16 weight panels, all layers at once
// For up to WPREP_MAX f32 matrices w_e (rows_e x cols_e, row pitch ld_e: a column slice of a wider tensor is allowed): the bf16 copy
// w16_e [rows][cols] (the forward GEMM's panel) and the bf16 TRANSPOSE wt16_e [cols][rows] (the data-gradient GEMM's panel) in ONE
// launch -- what a mixed-precision step used to do with two conversion launches per wide layer (auto_cast casts every conv's weight per
// call in the reference, trainer.py:209-213).  64 x 64 tiles through LDS: both outputs leave as 128-byte rows.
constexpr int WPREP_MAX = 24;
struct WPrepArgs {
    const float* w[WPREP_MAX]; bf16_t* w16[WPREP_MAX]; bf16_t* wt16[WPREP_MAX];
    int rows[WPREP_MAX], cols[WPREP_MAX], ld[WPREP_MAX], tile0[WPREP_MAX + 1];
    int n;
};
__global__ __launch_bounds__(256) void weight_prep_kernel(WPrepArgs a) {
    __shared__ float sm[64][65];
    int e = 0;
    while (e + 1 < a.n && (int)blockIdx.x >= a.tile0[e + 1]) ++e;
    const int t = blockIdx.x - a.tile0[e];
    const int rows = a.rows[e], cols = a.cols[e], ld = a.ld[e];
    const int tc = (cols + 63) / 64;
    const int r0 = (t / tc) * 64, c0 = (t % tc) * 64;
    const float* __restrict__ w = a.w[e];
    bf16_t* __restrict__ w16 = a.w16[e];
    bf16_t* __restrict__ wt = a.wt16[e];
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
#pragma unroll 4
    for (int i = ly; i < 64; i += 4) {
        const int r = r0 + i, c = c0 + lx;
        const float v = (r < rows && c < cols) ? w[(size_t)r * ld + c] : 0.f;
        sm[i][lx] = v;
        if (w16 && r < rows && c < cols) w16[(size_t)r * cols + c] = (bf16_t)v;
    }
    if (!wt) return;
    __syncthreads();
#pragma unroll 4
    for (int i = ly; i < 64; i += 4) {
        const int c = c0 + i, r = r0 + lx;
        if (c < cols && r < rows) wt[(size_t)c * rows + r] = (bf16_t)sm[lx][i];
    }
}

// ---------------------------------------------------------------------------------------------- Adam (coupled L2)
// paddle.optimizer.Adam(weight_decay=L2Decay-style float): g += wd * p;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
// p -= lr * (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps)
// keep = 1 - lr * coeff for paddle.optimizer.AdamW's DECOUPLED decay (the parameter shrinks first, the moments never see the decay);
// 1 for Adam.
// fault: the context's grid-barrier bail-out word (csrc/res2_train.hip).  A fused training kernel whose grid barrier timed out has
// produced statistics from incomplete sums: the update of that step is DROPPED on the device -- the host polls the word only every
// few steps (a D2H sync per step would stall the launch pipeline) and must not find the bad step in the weights or Adam's moments.
__global__ __launch_bounds__(256) void adam_kernel(float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2,
                                                   float eps, float wd, float c1, float c2, float gscale, float keep, const unsigned* fault) {
    if (fault && __hip_atomic_load(fault, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float pv = p[i];
        const float gr = g[i] * gscale + wd * pv;
        const float mn = b1 * m[i] + (1.f - b1) * gr;
        const float vn = b2 * v[i] + (1.f - b2) * gr * gr;
        m[i] = mn; v[i] = vn;
        p[i] = pv * keep - lr * (mn / c1) / (sqrtf(vn / c2) + eps);
    }
}

// paddle.optimizer.Momentum (and SGD = momentum 0): g += wd * p (L2Decay-style float);  vel = mu * vel + g;
// p -= lr * vel, or with use_nesterov p -= lr * (g + mu * vel)
__global__ __launch_bounds__(256) void momentum_kernel(float* p, const float* g, float* vel, long long n, float lr, float mu, float wd,
                                                       float gscale, int nesterov, const unsigned* fault) {
    if (fault && __hip_atomic_load(fault, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float pv = p[i];
        const float gr = g[i] * gscale + wd * pv;
        const float vn = mu * vel[i] + gr;
        vel[i] = vn;
        p[i] = pv - lr * (nesterov ? gr + mu * vn : vn);
    }
}

// ---------------------------------------------------------------------------------------------- gradient packing
// dst[off_i .. off_i + n_i) = src_i (or zeros when src_i is NULL) for up to 128 segments per launch: the parameters' gradient
// tensors, as autograd left them, into the optimiser's flat gradient buffer.  (With .grad bound to views of the flat buffer
// autograd accumulates in place: one add_ launch per parameter, 148 per ECAPA step -- a seventh of all launches.)
constexpr int PACK_MAX = 128;
struct PackArgs { const float* src[PACK_MAX]; long long off[PACK_MAX]; long long n[PACK_MAX]; float* dst; };

__global__ __launch_bounds__(256) void pack_segments_kernel(const PackArgs a) {
    const int sgm = blockIdx.y;
    const float* __restrict__ src = a.src[sgm];
    float* __restrict__ dst = a.dst + a.off[sgm];
    const long long n = a.n[sgm];
    // 16 bytes per lane where the segment allows it (the 9.4 MB MFA weight gradient took 63 us at 4 bytes per lane on 64 workgroups)
    if (src && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        const long long n4 = n >> 2;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256)
            reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
        for (long long i = (n4 << 2) + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dst[i] = src[i];
        return;
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dst[i] = src ? src[i] : 0.f;
}

// ---------------------------------------------------------------------------------------------- per-utterance pieces (ASP)
// Adjoint of reflect padding: dxp (B, T + 2p, C) is the gradient w.r.t. the reflect-padded input (from the zero-padded
// "full" data-gradient conv); frames 1..p and T-1-p..T-2 also receive their mirror images' gradients.
struct FoldArgs { const float* dxp; float* dx; int T, p, C4; long long total;
                  int lddx; const float* add; int ld_add; float* sum; };     // dx rows lddx apart; sum = folded + add (dense), when add
__global__ __launch_bounds__(256) void reflect_fold_kernel(FoldArgs a) {
    const int Tp = a.T + 2 * a.p;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (long long)gridDim.x * 256) {
        const long long m = i / a.C4;
        const int c = (int)(i - m * a.C4) * 4;
        const long long b = m / a.T;
        const int t = (int)(m - b * a.T);
        const float* base = a.dxp + (size_t)b * Tp * a.C4 * 4 + c;
        float v[4], w[4];
        vp_load4(base + (size_t)(t + a.p) * a.C4 * 4, v);
        if (t >= 1 && t <= a.p) {
            vp_load4(base + (size_t)(a.p - t) * a.C4 * 4, w);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += w[e];
        }
        if (t <= a.T - 2 && t >= a.T - 1 - a.p) {
            vp_load4(base + (size_t)(2 * (a.T - 1) - t + a.p) * a.C4 * 4, w);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += w[e];
        }
        vp_store4(a.dx + m * a.lddx + c, v);
        if (a.add) {
            vp_load4(a.add + m * a.ld_add + c, w);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += w[e];
            vp_store4(a.sum + m * a.C4 * 4 + c, v);
        }
    }
}

// Backward of out[b,t,c] = x[b,t,c] * s[b,c] (+ res): dx = dy * s;  ds[b,c] = sum_t dy * x.  One workgroup = 64 channels
// of one utterance.
__global__ __launch_bounds__(256) void scale_rows_bwd_kernel(const float* dy, const float* x, const float* s, int T, int C, float* dx,
                                                             float* ds) {
    __shared__ float sm[4][64];
    const int lc = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int b = blockIdx.y, c = blockIdx.x * 64 + lc;
    float acc = 0.f;
    if (c < C) {
        const float sv = s[(size_t)b * C + c];
        for (int t = rg; t < T; t += 4) {
            const size_t o = ((size_t)b * T + t) * C + c;
            const float g = dy[o];
            acc += g * x[o];
            dx[o] = g * sv;
        }
    }
    sm[rg][lc] = acc;
    __syncthreads();
    if (rg == 0 && c < C) ds[(size_t)b * C + c] = sm[0][lc] + sm[1][lc] + sm[2][lc] + sm[3][lc];
}

// The same for utterances of MANY positions (ResNetSE / ERes2Net feature maps: T x F' = 10^4 positions of 32-256 channels): the kernel
// above gives one workgroup per (utterance, 64 channels) -- 32 workgroups walking 19 072 rows each on the stage-1 maps, 574 us per call
// and a quarter of the ResNetSE training step.  Here the positions are cut into chunks (grid = chunks x B), four channels per lane,
// partial sums per chunk reduced by sum_partials (fixed order).  part: [B][chunks][C].
struct SrbArgs { const float* dy; const float* x; const float* s; float* dx; float* part; int T, C4, chunks, rows_per_chunk, cl_shift; };
__global__ __launch_bounds__(256) void scale_rows_bwd_chunk_kernel(SrbArgs a) {
    __shared__ float sm[256][4];
    const int CL = 1 << a.cl_shift, RG = 256 >> a.cl_shift;
    const int lc = threadIdx.x & (CL - 1), rg = threadIdx.x >> a.cl_shift;
    const int b = blockIdx.y, ch = blockIdx.x;
    const int p0 = ch * a.rows_per_chunk, p1 = min(a.T, p0 + a.rows_per_chunk);
    const int C = a.C4 * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (lc < a.C4) {
        float sv[4];
        vp_load4(a.s + (size_t)b * C + 4 * lc, sv);
        int p = p0 + rg;
        for (; p + 3 * RG < p1; p += 4 * RG) {                   // four rows of loads in flight
            float g[4][4], xv[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t o = ((size_t)b * a.T + p + u * RG) * C + 4 * lc;
                vp_load4(a.dy + o, g[u]); vp_load4(a.x + o, xv[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float o4[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) { acc[e] += g[u][e] * xv[u][e]; o4[e] = g[u][e] * sv[e]; }
                vp_store4(a.dx + ((size_t)b * a.T + p + u * RG) * C + 4 * lc, o4);
            }
        }
        for (; p < p1; p += RG) {
            const size_t o = ((size_t)b * a.T + p) * C + 4 * lc;
            float g[4], xv[4], o4[4];
            vp_load4(a.dy + o, g); vp_load4(a.x + o, xv);
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc[e] += g[e] * xv[e]; o4[e] = g[e] * sv[e]; }
            vp_store4(a.dx + o, o4);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sm[threadIdx.x][e] = acc[e];
    __syncthreads();
    if (rg == 0 && lc < a.C4) {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        for (int q = 0; q < RG; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] += sm[q * CL + lc][e];
        vp_store4(a.part + ((size_t)b * a.chunks + ch) * C + 4 * lc, t);
    }
}

// The SE gate's backward in two passes (see SEBlockFn in train/functions.py): ds[b,c] = sum_t dy * x first -- the squeeze path's
// gradient dm[b,c] (through the two dense layers) depends on it -- then dx = dy * s[b,c] + dm[b,c] / T in one write of dx, instead
// of dx = dy * s, a separate mean-backward tensor and their sum.  Four channels per lane; 32 lanes x 8 frame groups per utterance.
// AFF: x is the PRE-BatchNorm activation z (bf16); the SE block's input h = bf16(z * bsc + bsh) is formed on the fly -- the same values
// the BatchNorm apply pass (vp_affine_rows_b16_b16) would have stored
template <bool AFF>
__device__ __forceinline__ void bn_affine4_b16(float (&v)[4], const float (&sc)[4], const float (&sh)[4]) {
    if constexpr (AFF) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (float)(bf16_t)__fmaf_rn(v[e], sc[e], sh[e]);
    }
}

template <typename TX = float, bool AFF = false>
__global__ __launch_bounds__(256) void utt_dot4_kernel(const float* dy, const TX* x, int T, int C, float* ds, const float* bsc = nullptr,
                                                       const float* bsh = nullptr) {
    __shared__ float sm[256][4];
    const int lc = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int b = blockIdx.y, c4 = blockIdx.x * 32 + lc;
    const bool ok = c4 < (C >> 2);
    const int c = ok ? c4 * 4 : 0;
    const float* gb = dy + (size_t)b * T * C + c;
    const TX* xb = x + (size_t)b * T * C + c;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float sc[4] = {1.f, 1.f, 1.f, 1.f}, sh[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (AFF) { vp_load4(bsc + c, sc); vp_load4(bsh + c, sh); }
    int t = rg;
    for (; t + 24 < T; t += 32) {
        float g[4][4], v[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { vp_load4(gb + (size_t)(t + 8 * u) * C, g[u]); vp_load4(xb + (size_t)(t + 8 * u) * C, v[u]); }
#pragma unroll
        for (int u = 0; u < 4; ++u) bn_affine4_b16<AFF>(v[u], sc, sh);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += g[u][e] * v[u][e];
    }
    for (; t < T; t += 8) {
        float g[4], v[4];
        vp_load4(gb + (size_t)t * C, g); vp_load4(xb + (size_t)t * C, v);
        bn_affine4_b16<AFF>(v, sc, sh);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += g[e] * v[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sm[threadIdx.x][e] = acc[e];
    __syncthreads();
    if (rg != 0 || !ok) return;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] += sm[r * 32 + lc][e];
    vp_store4(ds + (size_t)b * C + c, o);
}

__global__ __launch_bounds__(256) void scale_shift_rows4_kernel(const float* dy, const float* s, const float* dm, int T, int C4, float inv_t,
                                                                long long total, float* dx) {
    const int C = C4 * 4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long m = i / C4;
        const int c = (int)(i - m * C4) * 4;
        const long long b = m / T;
        float g[4], sv[4], d[4], o[4];
        vp_load4(dy + m * C + c, g); vp_load4(s + b * C + c, sv); vp_load4(dm + b * C + c, d);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = __fmaf_rn(g[e], sv[e], d[e] * inv_t);       // (the form utt_affine4 evaluates: bit-identical A/B)
        vp_store4(dx + m * C + c, o);
    }
}

// up[b, t, f, :] = dz[b, t / s, f / s, :] when t and f are multiples of s (and in range), else 0: the zero-insertion that turns
// the data gradient of a stride-s conv into a stride-1 conv over `up` (T_in x F_in positions).
struct ZiArgs { const float* dz; float* up; int T_out, F_out, T_in, F_in, st, sf, C4; long long total; };
__global__ __launch_bounds__(256) void zero_insert_kernel(ZiArgs a) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (long long)gridDim.x * 256) {
        const long long pos = i / a.C4;
        const int c = (int)(i - pos * a.C4) * 4;
        const long long bt = pos / a.F_in;
        const int f = (int)(pos - bt * a.F_in);
        const long long b = bt / a.T_in;
        const int t = (int)(bt - b * a.T_in);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (t % a.st == 0 && f % a.sf == 0 && t / a.st < a.T_out && f / a.sf < a.F_out)
            vp_load4(a.dz + (((size_t)b * a.T_out + t / a.st) * a.F_out + f / a.sf) * a.C4 * 4 + c, v);
        vp_store4(a.up + pos * a.C4 * 4 + c, v);
    }
}

// dz = [y > 0] * dy   (ReLU backward from its output)
__global__ __launch_bounds__(256) void relu_mask_kernel(const float* dy, const float* y, long long n4, float* dz) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        float g[4], v[4];
        vp_load4(dy + i * 4, g); vp_load4(y + i * 4, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = v[e] > 0.f ? g[e] : 0.f;
        vp_store4(dz + i * 4, g);
    }
}

// Backward of the AFF output o = x (1 + t) + y (1 - t) (eres2net.py:48-51, t = tanh(local_att)): dx = g (1 + t), dy = g (1 - t), dt = g (x - y)
__global__ __launch_bounds__(256) void aff_combine_bwd_kernel(const float* g, const float* t, const float* x, const float* y, long long n4,
                                                              float* dx, float* dy, float* dt) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        float gv[4], tv[4], xv[4], yv[4], a[4], b[4], c[4];
        vp_load4(g + i * 4, gv); vp_load4(t + i * 4, tv); vp_load4(x + i * 4, xv); vp_load4(y + i * 4, yv);
#pragma unroll
        for (int e = 0; e < 4; ++e) { a[e] = gv[e] * (1.f + tv[e]); b[e] = gv[e] * (1.f - tv[e]); c[e] = gv[e] * (xv[e] - yv[e]); }
        vp_store4(dx + i * 4, a); vp_store4(dy + i * 4, b); vp_store4(dt + i * 4, c);
    }
}

// ---------------------------------------------------------------------------------------------- CAM++ context (campplus.py:88-106)
// ctx[b, s, c] = mean_t x[b, t, c] + mean_{t in segment s} x[b, t, c]  (100-frame segments, the last one over its valid frames);
// backward: dx[b, t, c] = sum_s dctx[b, s, c] / T + dctx[b, seg(t), c] / len(seg(t)).  One workgroup = 64 channels of one utterance.
__global__ __launch_bounds__(256) void seg_ctx_kernel(const float* x, int T, int C, int seg_len, int nseg, float* ctx) {
    __shared__ float sm[4][64];
    const int lc = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int b = blockIdx.y, c = blockIdx.x * 64 + lc;
    const bool ok = c < C;
    float tot = 0.f;
    for (int s = 0; s < nseg; ++s) {
        const int t0 = s * seg_len, t1 = min(T, t0 + seg_len);
        float acc = 0.f;
        if (ok) for (int t = t0 + rg; t < t1; t += 4) acc += x[((size_t)b * T + t) * C + c];
        sm[rg][lc] = acc;
        __syncthreads();
        const float ssum = sm[0][lc] + sm[1][lc] + sm[2][lc] + sm[3][lc];
        __syncthreads();
        tot += ssum;
        if (rg == 0 && ok) ctx[((size_t)b * nseg + s) * C + c] = ssum / (float)(t1 - t0);
    }
    if (rg == 0 && ok)
        for (int s = 0; s < nseg; ++s) ctx[((size_t)b * nseg + s) * C + c] += tot / (float)T;
}

__global__ __launch_bounds__(256) void seg_ctx_bwd_kernel(const float* dctx, int T, int C, int seg_len, int nseg, float* dx) {
    const int lc = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int b = blockIdx.y, c = blockIdx.x * 64 + lc;
    if (c >= C) return;
    float tot = 0.f;
    for (int s = 0; s < nseg; ++s) tot += dctx[((size_t)b * nseg + s) * C + c];
    tot /= (float)T;
    for (int t = rg; t < T; t += 4) {
        const int s = t / seg_len;
        const int len = min(T, (s + 1) * seg_len) - s * seg_len;
        dx[((size_t)b * T + t) * C + c] = tot + dctx[((size_t)b * nseg + s) * C + c] / (float)len;
    }
}

// out[b, t, c] = y[b, t, c] * m[b, seg(t), c];  backward: dy = g * m,  dm[b, s, c] = sum_{t in s} g * y
__global__ __launch_bounds__(256) void seg_scale_kernel(const float* y, const float* m, int T, int C4, int seg_len, int nseg, long long total,
                                                        float* out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / C4;
        const int c = (int)(i - r * C4) * 4;
        const long long b = r / T;
        const int t = (int)(r - b * T);
        float v[4], g[4];
        vp_load4(y + r * C4 * 4 + c, v);
        vp_load4(m + (b * nseg + t / seg_len) * C4 * 4 + c, g);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= g[e];
        vp_store4(out + r * C4 * 4 + c, v);
    }
}

__global__ __launch_bounds__(256) void seg_scale_bwd_kernel(const float* g, const float* y, const float* m, int T, int C, int seg_len, int nseg,
                                                            float* dy, float* dm) {
    __shared__ float sm[4][64];
    const int lc = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int b = blockIdx.y, c = blockIdx.x * 64 + lc;
    const bool ok = c < C;
    for (int s = 0; s < nseg; ++s) {
        const int t0 = s * seg_len, t1 = min(T, t0 + seg_len);
        const float mv = ok ? m[((size_t)b * nseg + s) * C + c] : 0.f;
        float acc = 0.f;
        if (ok)
            for (int t = t0 + rg; t < t1; t += 4) {
                const size_t o = ((size_t)b * T + t) * C + c;
                const float gv = g[o];
                acc += gv * y[o];
                dy[o] = gv * mv;
            }
        sm[rg][lc] = acc;
        __syncthreads();
        if (rg == 0 && ok) dm[((size_t)b * nseg + s) * C + c] = sm[0][lc] + sm[1][lc] + sm[2][lc] + sm[3][lc];
        __syncthreads();
    }
}

// dz = dy * (1 - y^2)   (tanh backward from its output)
__global__ __launch_bounds__(256) void tanh_bwd_kernel(const float* dy, const float* y, long long n4, float* dz, int sigmoid) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        float g[4], v[4];
        vp_load4(dy + i * 4, g); vp_load4(y + i * 4, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float d;
            if (sigmoid == 2) d = v[e] > 0.f ? 1.f : 0.f;
            else if (sigmoid == 3) d = (v[e] > 0.f && v[e] < 20.f) ? 1.f : 0.f;
            else if (sigmoid == 4) { const float sg = 1.f / (1.f + expf(-v[e])); d = sg * (1.f + v[e] * (1.f - sg)); }   // v = the INPUT
            else d = sigmoid ? v[e] * (1.f - v[e]) : 1.f - v[e] * v[e];
            g[e] *= d;
        }
        vp_store4(dz + i * 4, g);
    }
}
__global__ __launch_bounds__(256) void tanh_fwd_kernel(const float* x, long long n4, float* y, int sigmoid) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        float v[4];
        vp_load4(x + i * 4, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (sigmoid == 2) v[e] = fmaxf(v[e], 0.f);
            else if (sigmoid == 3) v[e] = fminf(fmaxf(v[e], 0.f), 20.f);
            else if (sigmoid == 4) v[e] = v[e] / (1.f + expf(-v[e]));
            else v[e] = sigmoid ? 1.f / (1.f + expf(-v[e])) : tanhf(v[e]);
        }
        vp_store4(y + i * 4, v);
    }
}

int act_kind(int act) {
    return act == VP_ACT_SIGMOID ? 1 : act == VP_ACT_RELU ? 2 : act == VP_ACT_HARDTANH20 ? 3 : act == VP_ACT_SILU ? 4 : 0;
}

}  // namespace

extern "C" {

int vp_conv_weight_layouts_f32(vp_ctx* ctx, const float* w, int Cout, int Cin, int KW, float* wp, float* w2, vp_stream stream) {
    if (!ctx || !w || (!wp && !w2) || Cout <= 0 || Cin <= 0 || KW <= 0) VP_FAIL(ctx, VP_EINVAL, "weight_layouts: bad arguments");
    hipLaunchKernelGGL(weight_layouts_kernel, dim3(grid1d((long long)Cout * Cin * KW)), dim3(256), 0, (hipStream_t)stream, w, Cout, Cin, KW, 1,
                       wp, w2);
    VP_LAUNCH_CHECK(ctx, "weight_layouts");
    return VP_OK;
}

int vp_conv2d_weight_layouts_f32(vp_ctx* ctx, const float* w, int Cout, int Cin, int KF, int KT, float* wp, float* w2, vp_stream stream) {
    if (!ctx || !w || (!wp && !w2) || Cout <= 0 || Cin <= 0 || KF <= 0 || KT <= 0) VP_FAIL(ctx, VP_EINVAL, "weight_layouts_2d: bad arguments");
    hipLaunchKernelGGL(weight_layouts_kernel, dim3(grid1d((long long)Cout * Cin * KF * KT)), dim3(256), 0, (hipStream_t)stream, w, Cout, Cin,
                       KF * KT, KF, wp, w2);
    VP_LAUNCH_CHECK(ctx, "weight_layouts_2d");
    return VP_OK;
}

int vp_prep_weights_bf16(vp_ctx* ctx, const void* const* w, void* const* w16, void* const* wt16, const int* rows, const int* cols,
                         const int* ld, int n, vp_stream stream) {
    if (!ctx || !w || !w16 || !wt16 || !rows || !cols || !ld || n <= 0) VP_FAIL(ctx, VP_EINVAL, "prep_weights: bad arguments");
    for (int i0 = 0; i0 < n; i0 += WPREP_MAX) {
        WPrepArgs a;
        memset(&a, 0, sizeof(a));
        const int m = n - i0 < WPREP_MAX ? n - i0 : WPREP_MAX;
        int tiles = 0;
        for (int i = 0; i < m; ++i) {
            const int k = i0 + i;
            if (!w[k] || (!w16[k] && !wt16[k]) || rows[k] <= 0 || cols[k] <= 0 || ld[k] < cols[k]) VP_FAIL(ctx, VP_EINVAL, "prep_weights: bad entry %d", k);
            a.w[i] = (const float*)w[k]; a.w16[i] = (bf16_t*)w16[k]; a.wt16[i] = (bf16_t*)wt16[k];
            a.rows[i] = rows[k]; a.cols[i] = cols[k]; a.ld[i] = ld[k]; a.tile0[i] = tiles;
            tiles += ((rows[k] + 63) / 64) * ((cols[k] + 63) / 64);
        }
        a.tile0[m] = tiles; a.n = m;
        hipLaunchKernelGGL(weight_prep_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream, a);
        VP_LAUNCH_CHECK(ctx, "weight_prep");
    }
    return VP_OK;
}

int vp_adam_step_f32(vp_ctx* ctx, float* param, const float* grad, float* m, float* v, long long n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int step, float grad_scale, vp_stream stream) {
    if (!ctx || !param || !grad || !m || !v || n <= 0 || step < 1) VP_FAIL(ctx, VP_EINVAL, "adam: bad arguments");
    const float c1 = 1.f - powf(beta1, (float)step), c2 = 1.f - powf(beta2, (float)step);
    hipLaunchKernelGGL(adam_kernel, dim3(grid1d(n)), dim3(256), 0, (hipStream_t)stream, param, grad, m, v, n, lr, beta1, beta2, eps,
                       weight_decay, c1, c2, grad_scale, 1.f, vp_fault_word(ctx));
    VP_LAUNCH_CHECK(ctx, "adam");
    return VP_OK;
}

int vp_adamw_step_f32(vp_ctx* ctx, float* param, const float* grad, float* m, float* v, long long n, float lr, float beta1, float beta2,
                      float eps, float coeff, int step, float grad_scale, vp_stream stream) {
    if (!ctx || !param || !grad || !m || !v || n <= 0 || step < 1) VP_FAIL(ctx, VP_EINVAL, "adamw: bad arguments");
    const float c1 = 1.f - powf(beta1, (float)step), c2 = 1.f - powf(beta2, (float)step);
    hipLaunchKernelGGL(adam_kernel, dim3(grid1d(n)), dim3(256), 0, (hipStream_t)stream, param, grad, m, v, n, lr, beta1, beta2, eps,
                       0.f, c1, c2, grad_scale, 1.f - lr * coeff, vp_fault_word(ctx));
    VP_LAUNCH_CHECK(ctx, "adamw");
    return VP_OK;
}

int vp_momentum_step_f32(vp_ctx* ctx, float* param, const float* grad, float* velocity, long long n, float lr, float momentum,
                         float weight_decay, int use_nesterov, float grad_scale, vp_stream stream) {
    if (!ctx || !param || !grad || !velocity || n <= 0) VP_FAIL(ctx, VP_EINVAL, "momentum: bad arguments");
    hipLaunchKernelGGL(momentum_kernel, dim3(grid1d(n)), dim3(256), 0, (hipStream_t)stream, param, grad, velocity, n, lr, momentum,
                       weight_decay, grad_scale, use_nesterov, vp_fault_word(ctx));
    VP_LAUNCH_CHECK(ctx, "momentum");
    return VP_OK;
}

int vp_pack_segments_f32(vp_ctx* ctx, const void* const* srcs, const long long* offs, const long long* sizes, int n, float* dst,
                         vp_stream stream) {
    if (!ctx || !srcs || !offs || !sizes || !dst || n <= 0) VP_FAIL(ctx, VP_EINVAL, "pack_segments: bad arguments");
    for (int i0 = 0; i0 < n; i0 += PACK_MAX) {
        PackArgs a;
        const int cnt = n - i0 < PACK_MAX ? n - i0 : PACK_MAX;
        long long big = 0;
        for (int i = 0; i < cnt; ++i) {
            if (offs[i0 + i] < 0 || sizes[i0 + i] < 0) VP_FAIL(ctx, VP_EINVAL, "pack_segments: negative offset / size");
            a.src[i] = (const float*)srcs[i0 + i]; a.off[i] = offs[i0 + i]; a.n[i] = sizes[i0 + i];
            if (sizes[i0 + i] > big) big = sizes[i0 + i];
        }
        a.dst = dst;
        long long bx = (big + 4 * 256 - 1) / (4 * 256);
        if (bx < 1) bx = 1;
        if (bx > 512) bx = 512;
        hipLaunchKernelGGL(pack_segments_kernel, dim3((unsigned)bx, cnt), dim3(256), 0, (hipStream_t)stream, a);
        VP_LAUNCH_CHECK(ctx, "pack_segments");
    }
    return VP_OK;
}

int vp_act_f32(vp_ctx* ctx, int act, const float* x, long long n, float* y, vp_stream stream) {
    if (!ctx || !x || !y || n <= 0 || n & 3 || act < VP_ACT_RELU || act > VP_ACT_SILU) VP_FAIL(ctx, VP_EINVAL, "act: bad arguments");
    hipLaunchKernelGGL(tanh_fwd_kernel, dim3(grid1d(n / 4)), dim3(256), 0, (hipStream_t)stream, x, n / 4, y, act_kind(act));
    VP_LAUNCH_CHECK(ctx, "act");
    return VP_OK;
}

int vp_act_bwd_f32(vp_ctx* ctx, int act, const float* dy, const float* y, long long n, float* dz, vp_stream stream) {
    if (!ctx || !dy || !y || !dz || n <= 0 || n & 3 || act < VP_ACT_RELU || act > VP_ACT_SILU) VP_FAIL(ctx, VP_EINVAL, "act_bwd: bad arguments");
    hipLaunchKernelGGL(tanh_bwd_kernel, dim3(grid1d(n / 4)), dim3(256), 0, (hipStream_t)stream, dy, y, n / 4, dz, act_kind(act));
    VP_LAUNCH_CHECK(ctx, "act_bwd");
    return VP_OK;
}

int vp_reflect_fold_f32(vp_ctx* ctx, const float* dxp, int B, int T, int pad, int C, float* dx, vp_stream stream) {
    if (!ctx || !dxp || !dx || B <= 0 || T <= 0 || pad < 0 || pad >= T || C <= 0 || C & 3) VP_FAIL(ctx, VP_EINVAL, "reflect_fold: bad arguments");
    FoldArgs a{dxp, dx, T, pad, C / 4, (long long)B * T * (C / 4), C, nullptr, 0, nullptr};
    hipLaunchKernelGGL(reflect_fold_kernel, dim3(grid1d(a.total)), dim3(256), 0, (hipStream_t)stream, a);
    VP_LAUNCH_CHECK(ctx, "reflect_fold");
    return VP_OK;
}

// the same fold written into a channel slice of a wider gradient tensor (rows lddx apart), and sum = folded + add (dense (B*T, C))
// when add is given: a Res2Net chunk's input gradient goes to its slice of d x, and, summed with the concatenation's gradient
// of the previous chunk's output, becomes that chunk's output gradient (ecapa_tdnn.py:36-46), in the pass that folds
int vp_reflect_fold_into_f32(vp_ctx* ctx, const float* dxp, int B, int T, int pad, int C, float* dx, int lddx, const float* add, int ld_add,
                             float* sum, vp_stream stream) {
    if (!ctx || !dxp || !dx || B <= 0 || T <= 0 || pad < 0 || pad >= T || C <= 0 || (C | lddx | ld_add) & 3 || (add && !sum) ||
        (((uintptr_t)dx | (uintptr_t)add | (uintptr_t)sum) & 15))
        VP_FAIL(ctx, VP_EINVAL, "reflect_fold_into: bad arguments");
    FoldArgs a{dxp, dx, T, pad, C / 4, (long long)B * T * (C / 4), lddx, add, ld_add, sum};
    hipLaunchKernelGGL(reflect_fold_kernel, dim3(grid1d(a.total)), dim3(256), 0, (hipStream_t)stream, a);
    VP_LAUNCH_CHECK(ctx, "reflect_fold_into");
    return VP_OK;
}

static void srb_geometry(int B, int T, int C, int& cl_shift, int& chunks, int& rpc) {
    const int C4 = C / 4;
    cl_shift = 0;
    while ((1 << cl_shift) < C4 && cl_shift < 8) ++cl_shift;
    const int RG = 256 >> cl_shift;
    long long ch = 2048 / (B > 0 ? B : 1);                      // ~2048 workgroups
    if (ch < 1) ch = 1;
    long long r = (T + ch - 1) / ch;
    if (r < 8LL * RG) r = 8LL * RG;                              // at least two four-row trips per thread
    rpc = (int)r;
    chunks = (T + rpc - 1) / rpc;
}

size_t vp_scale_rows_bwd_workspace_bytes(int B, int T, int C) {
    if (B <= 0 || T <= 0 || C <= 0 || (C & 3) || C > 1024) return 0;
    int cl, chunks, rpc;
    srb_geometry(B, T, C, cl, chunks, rpc);
    return (size_t)B * chunks * C * sizeof(float) + 256;
}

// out = x * s[b] (+ res) backward with the positions of an utterance spread over many workgroups (ws from vp_scale_rows_bwd_workspace_bytes;
// C % 4 == 0, C <= 1024, 16-byte aligned tensors -- otherwise, or for few positions, callers use vp_scale_rows_bwd_f32)
int vp_scale_rows_bwd_ws_f32(vp_ctx* ctx, const float* dy, const float* x, const float* s, int B, int T, int C, float* dx, float* ds, void* ws,
                             size_t ws_bytes, vp_stream stream) {
    if (!ctx || !dy || !x || !s || !dx || !ds || B <= 0 || T <= 0 || C <= 0 || B > 65535) VP_FAIL(ctx, VP_EINVAL, "scale_rows_bwd: bad arguments");
    if ((C & 3) || C > 1024 || (((uintptr_t)dy | (uintptr_t)x | (uintptr_t)s | (uintptr_t)dx) & 15)) return VP_EUNSUP;
    const size_t need = vp_scale_rows_bwd_workspace_bytes(B, T, C);
    if (!ws || ws_bytes < need) VP_FAIL(ctx, VP_EWORKSPACE, "scale_rows_bwd: workspace %zu < %zu", ws_bytes, need);
    int cl, chunks, rpc;
    srb_geometry(B, T, C, cl, chunks, rpc);
    SrbArgs a{dy, x, s, dx, (float*)ws, T, C / 4, chunks, rpc, cl};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(scale_rows_bwd_chunk_kernel, dim3(chunks, B), dim3(256), 0, st, a);
    VP_LAUNCH_CHECK(ctx, "scale_rows_bwd_chunk");
    vp_launch_sum_partials((const float*)ws, chunks, C, ds, st, 1, 1, B);
    VP_LAUNCH_CHECK(ctx, "scale_rows_bwd_reduce");
    return VP_OK;
}

int vp_scale_rows_bwd_f32(vp_ctx* ctx, const float* dy, const float* x, const float* s, int B, int T, int C, float* dx, float* ds,
                          vp_stream stream) {
    if (!ctx || !dy || !x || !s || !dx || !ds || B <= 0 || T <= 0 || C <= 0 || B > 65535) VP_FAIL(ctx, VP_EINVAL, "scale_rows_bwd: bad arguments");
    hipLaunchKernelGGL(scale_rows_bwd_kernel, dim3((C + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, dy, x, s, T, C, dx, ds);
    VP_LAUNCH_CHECK(ctx, "scale_rows_bwd");
    return VP_OK;
}

int vp_utt_dot_f32(vp_ctx* ctx, const float* dy, const float* x, int B, int T, int C, float* ds, vp_stream stream) {
    if (!ctx || !dy || !x || !ds || B <= 0 || T <= 0 || C <= 0 || (C & 3) || B > 65535 || (((uintptr_t)dy | (uintptr_t)x | (uintptr_t)ds) & 15))
        VP_FAIL(ctx, VP_EINVAL, "utt_dot: bad arguments");
    hipLaunchKernelGGL(utt_dot4_kernel<float>, dim3((C / 4 + 31) / 32, B), dim3(256), 0, (hipStream_t)stream, dy, x, T, C, ds);
    VP_LAUNCH_CHECK(ctx, "utt_dot");
    return VP_OK;
}

// x stored as bf16 (the SE block's input kept in the low precision: its gate's gradient ds[b,c] = sum_t dy * x)
int vp_utt_dot_x16(vp_ctx* ctx, const float* dy, const void* x_bf16, int B, int T, int C, float* ds, vp_stream stream) {
    if (!ctx || !dy || !x_bf16 || !ds || B <= 0 || T <= 0 || C <= 0 || (C & 3) || B > 65535 || (((uintptr_t)dy | (uintptr_t)ds) & 15) || ((uintptr_t)x_bf16 & 7))
        VP_FAIL(ctx, VP_EINVAL, "utt_dot_x16: bad arguments");
    hipLaunchKernelGGL(utt_dot4_kernel<bf16_t>, dim3((C / 4 + 31) / 32, B), dim3(256), 0, (hipStream_t)stream, dy, (const bf16_t*)x_bf16, T, C, ds);
    VP_LAUNCH_CHECK(ctx, "utt_dot_x16");
    return VP_OK;
}

// ds[b][c] = sum_t dy * bf16(z * bn_scale + bn_shift): the SE gate's gradient over the PRE-BatchNorm activation of the conv in front of
// it (bf16), the BatchNorm apply pass folded into the read (the block's input h is never stored)
int vp_utt_dot_z16(vp_ctx* ctx, const float* dy, const void* z_bf16, const float* bn_scale, const float* bn_shift, int B, int T, int C,
                   float* ds, vp_stream stream) {
    if (!ctx || !dy || !z_bf16 || !bn_scale || !bn_shift || !ds || B <= 0 || T <= 0 || C <= 0 || (C & 3) || B > 65535 ||
        (((uintptr_t)dy | (uintptr_t)ds | (uintptr_t)bn_scale | (uintptr_t)bn_shift) & 15) || ((uintptr_t)z_bf16 & 7))
        VP_FAIL(ctx, VP_EINVAL, "utt_dot_z16: bad arguments");
    hipLaunchKernelGGL((utt_dot4_kernel<bf16_t, true>), dim3((C / 4 + 31) / 32, B), dim3(256), 0, (hipStream_t)stream, dy, (const bf16_t*)z_bf16, T, C,
                       ds, bn_scale, bn_shift);
    VP_LAUNCH_CHECK(ctx, "utt_dot_z16");
    return VP_OK;
}

int vp_scale_shift_rows_f32(vp_ctx* ctx, const float* dy, const float* s, const float* dm, int B, int T, int C, float* dx, vp_stream stream) {
    if (!ctx || !dy || !s || !dm || !dx || B <= 0 || T <= 0 || C <= 0 || (C & 3) ||
        (((uintptr_t)dy | (uintptr_t)s | (uintptr_t)dm | (uintptr_t)dx) & 15))
        VP_FAIL(ctx, VP_EINVAL, "scale_shift_rows: bad arguments");
    const long long total = (long long)B * T * (C / 4);
    hipLaunchKernelGGL(scale_shift_rows4_kernel, dim3(grid1d(total)), dim3(256), 0, (hipStream_t)stream, dy, s, dm, T, C / 4, 1.f / (float)T,
                       total, dx);
    VP_LAUNCH_CHECK(ctx, "scale_shift_rows");
    return VP_OK;
}

int vp_zero_insert_2d_f32(vp_ctx* ctx, const float* dz, int B, int T_out, int F_out, int C, int T_in, int F_in, int stride_t, int stride_f,
                          float* up, vp_stream stream) {
    if (!ctx || !dz || !up || B <= 0 || T_out <= 0 || F_out <= 0 || T_in <= 0 || F_in <= 0 || stride_t < 1 || stride_f < 1 || C <= 0 || C & 3)
        VP_FAIL(ctx, VP_EINVAL, "zero_insert: bad arguments");
    ZiArgs a{dz, up, T_out, F_out, T_in, F_in, stride_t, stride_f, C / 4, (long long)B * T_in * F_in * (C / 4)};
    hipLaunchKernelGGL(zero_insert_kernel, dim3(grid1d(a.total)), dim3(256), 0, (hipStream_t)stream, a);
    VP_LAUNCH_CHECK(ctx, "zero_insert");
    return VP_OK;
}

int vp_relu_bwd_f32(vp_ctx* ctx, const float* dy, const float* y, long long n, float* dz, vp_stream stream) {
    if (!ctx || !dy || !y || !dz || n <= 0 || n & 3) VP_FAIL(ctx, VP_EINVAL, "relu_bwd: bad arguments");
    hipLaunchKernelGGL(relu_mask_kernel, dim3(grid1d(n / 4)), dim3(256), 0, (hipStream_t)stream, dy, y, n / 4, dz);
    VP_LAUNCH_CHECK(ctx, "relu_bwd");
    return VP_OK;
}

int vp_aff_combine_f32(vp_ctx* ctx, const float* t, const float* x, const float* y, long long rows, int C, float* out, vp_stream stream) {
    if (!ctx || !t || !x || !y || !out || rows <= 0 || C <= 0 || C & 3) VP_FAIL(ctx, VP_EINVAL, "aff_combine: bad arguments");
    return vp_aff_combine(ctx, VP_F32, t, C, x, C, 0, y, C, 0, out, C, 0, rows, C, (hipStream_t)stream);
}

int vp_aff_combine_bwd_f32(vp_ctx* ctx, const float* g, const float* t, const float* x, const float* y, long long n, float* dx, float* dy,
                           float* dt, vp_stream stream) {
    if (!ctx || !g || !t || !x || !y || !dx || !dy || !dt || n <= 0 || n & 3) VP_FAIL(ctx, VP_EINVAL, "aff_combine_bwd: bad arguments");
    hipLaunchKernelGGL(aff_combine_bwd_kernel, dim3(grid1d(n / 4)), dim3(256), 0, (hipStream_t)stream, g, t, x, y, n / 4, dx, dy, dt);
    VP_LAUNCH_CHECK(ctx, "aff_combine_bwd");
    return VP_OK;
}

int vp_seg_ctx_f32(vp_ctx* ctx, const float* x, int B, int T, int C, int seg_len, float* out, vp_stream stream) {
    if (!ctx || !x || !out || B <= 0 || T <= 0 || C <= 0 || seg_len <= 0 || B > 65535) VP_FAIL(ctx, VP_EINVAL, "seg_ctx: bad arguments");
    hipLaunchKernelGGL(seg_ctx_kernel, dim3((C + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, x, T, C, seg_len, (T + seg_len - 1) / seg_len, out);
    VP_LAUNCH_CHECK(ctx, "seg_ctx");
    return VP_OK;
}

int vp_seg_ctx_bwd_f32(vp_ctx* ctx, const float* dctx, int B, int T, int C, int seg_len, float* dx, vp_stream stream) {
    if (!ctx || !dctx || !dx || B <= 0 || T <= 0 || C <= 0 || seg_len <= 0 || B > 65535) VP_FAIL(ctx, VP_EINVAL, "seg_ctx_bwd: bad arguments");
    hipLaunchKernelGGL(seg_ctx_bwd_kernel, dim3((C + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, dctx, T, C, seg_len, (T + seg_len - 1) / seg_len, dx);
    VP_LAUNCH_CHECK(ctx, "seg_ctx_bwd");
    return VP_OK;
}

int vp_seg_scale_f32(vp_ctx* ctx, const float* y, const float* m, int B, int T, int C, int seg_len, float* out, vp_stream stream) {
    if (!ctx || !y || !m || !out || B <= 0 || T <= 0 || C <= 0 || C & 3 || seg_len <= 0) VP_FAIL(ctx, VP_EINVAL, "seg_scale: bad arguments");
    const long long total = (long long)B * T * (C / 4);
    hipLaunchKernelGGL(seg_scale_kernel, dim3(grid1d(total)), dim3(256), 0, (hipStream_t)stream, y, m, T, C / 4, seg_len, (T + seg_len - 1) / seg_len, total, out);
    VP_LAUNCH_CHECK(ctx, "seg_scale");
    return VP_OK;
}

int vp_seg_scale_bwd_f32(vp_ctx* ctx, const float* g, const float* y, const float* m, int B, int T, int C, int seg_len, float* dy, float* dm,
                         vp_stream stream) {
    if (!ctx || !g || !y || !m || !dy || !dm || B <= 0 || T <= 0 || C <= 0 || seg_len <= 0 || B > 65535) VP_FAIL(ctx, VP_EINVAL, "seg_scale_bwd: bad arguments");
    hipLaunchKernelGGL(seg_scale_bwd_kernel, dim3((C + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, g, y, m, T, C, seg_len, (T + seg_len - 1) / seg_len, dy, dm);
    VP_LAUNCH_CHECK(ctx, "seg_scale_bwd");
    return VP_OK;
}

}  // extern "C"
