// Pooling statistics, forward and backward, of the inference engines and the training step:
//   attentive statistics (ASP, pooling.py:114-123): al = softmax_t(e), [mu | sd] = [sum al x | sqrt(max(sum al (x - mu)^2, eps))]
//   time statistics (pooling.py:97-104, 141):       [mean | std] over an utterance's frames, biased + clamp (ASP context) or TSTP
//   utt_sums:                                       sum over an utterance's frames (gradient of a per-utterance bias)
// All HBM/L2-bound or tiny; kept in f32 so that they add no error on top of the f32 reference.  docs/pooling_stats.md: which kernel
// runs when, the three contracts (tail predication, the clamp's subgradient, conditioning: each written once below), measured error.
#include "common.h"

#include <stdlib.h>

namespace {

// ---------------------------------------------------------------- the pieces, each defined once
// The clamp's subgradient: the forwards store sd = sqrtf(max(var, eps)) and the backwards infer "the clamp did not hold" from it.
// Sound at eps = 1e-12f and 1e-8f (the two in use) only because sqrtf is correctly rounded and, for these two, the rounded root of
// eps squares back to no more than eps; at 1e-6f it does not (tests/test_pooling_oracle_cpu.py).  Were it to break,
// dv = dsd / 2e-6 on a clamped channel.
__device__ __forceinline__ bool clamp_open(float sd, float eps) { return sd * sd > eps; }

// Sums t1, t2 of (x - c0) and its square over T frames -> md = mean - c0 and the std.
// ASP context: sqrt(clip(var_biased, eps)) (pooling.py:97-104); TSTP: sqrt(var_unbiased + eps) (pooling.py:141)
__device__ __forceinline__ void moments_finish(float t1, float t2, int T, int unbiased, float eps, float& md, float& sd) {
    md = t1 / (float)T;
    const float ss = fmaxf(t2 - (float)T * md * md, 0.f);
    sd = unbiased ? sqrtf(ss / (float)(T > 1 ? T - 1 : 1) + eps) : sqrtf(fmaxf(ss / (float)T, eps));
}

// pooled[b] = [mu0 + md | sqrt(max(var, eps))]
__device__ __forceinline__ void asp_store(float* pooled, int b, int C, int c, float mu0, float md, float var, float eps) {
    pooled[(size_t)b * 2 * C + c] = mu0 + md;
    pooled[(size_t)b * 2 * C + C + c] = sqrtf(fmaxf(var, eps));
}

// Frame groups of the register kernels: 512 threads = 64 channels x 8 groups, thread (lane, rg) holds frames rg + 8 i, i < NT, of
// its channel.  Tail predication: it LOADS frame min(rg + 8 i, T - 1) unconditionally (all loads issued up front, none out of
// bounds) and every USE is predicated with rg + 8 i < T.  A lost predicate counts the last frame several times; a dispatch that
// hands T > 8 NT to a kernel drops frames.  e, x: the thread's channel in row 0, rows lde / ldx apart; row0: the utterance's first frame.
template <int NT, typename TL, typename TX>
__device__ __forceinline__ void fg_load(const TL* e, int lde, const TX* x, int ldx, size_t row0, int rg, int T, float (&ev)[NT], float (&xv)[NT]) {
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int t = min(rg + 8 * i, T - 1);
        ev[i] = vp_to_f32(e[(row0 + t) * lde]);
        xv[i] = vp_to_f32(x[(row0 + t) * ldx]);
    }
}
__device__ __forceinline__ bool fg_has(int rg, int i, int T) { return rg + 8 * i < T; }
// the channel's maximum over the T frames: the group's own (predicated), then the 8 groups' through LDS
template <int NT>
__device__ __forceinline__ float fg_max(const float (&ev)[NT], int rg, int T, float (*sm)[64], int lane) {
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NT; ++i) if (fg_has(rg, i, T)) mx = fmaxf(mx, ev[i]);
    sm[rg][lane] = mx;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) mx = fmaxf(mx, sm[q][lane]);
    return mx;
}
// the 8 groups' partial sums of K quantities, each in group order (after the caller's barrier).  One loop over the groups for all
// K: two loops read LDS in another order, and the register kernels schedule -- and time -- differently
template <int K>
__device__ __forceinline__ void fg_sums(float (*sm)[8][64], int lane, float (&s)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] += sm[k][q][lane];
}

// Four channels per lane (32 lanes x 8 frame groups, four frames' loads in flight): sums of (x - c0) and its square over the frames
// [t0, t1) of the utterance at xb, c0 = the utterance's first frame; every thread's sums are left in LDS, behind a barrier.
__device__ __forceinline__ void moments4_accumulate(const float* xb, int ldx, int t0, int t1, float (*sm)[256][4], float c0[4]) {
    const int rg = threadIdx.x >> 5;
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    vp_load4(xb, c0);
    int t = t0 + rg;
    for (; t + 24 < t1; t += 32) {
        float v[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) vp_load4(xb + (size_t)(t + 8 * u) * ldx, v[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = v[u][e] - c0[e]; s1[e] += d; s2[e] += d * d; }
    }
    for (; t < t1; t += 8) {
        float v[4];
        vp_load4(xb + (size_t)t * ldx, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float d = v[e] - c0[e]; s1[e] += d; s2[e] += d * d; }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { sm[0][threadIdx.x][e] = s1[e]; sm[1][threadIdx.x][e] = s2[e]; }
    __syncthreads();
}
// channel e of lane lc's quad: the 8 groups' sums, in group order
__device__ __forceinline__ void moments4_total(float (*sm)[256][4], int lc, int e, float& t1, float& t2) {
    t1 = 0.f; t2 = 0.f;
    for (int r = 0; r < 8; ++r) { t1 += sm[0][r * 32 + lc][e]; t2 += sm[1][r * 32 + lc][e]; }
}

// ---------------------------------------------------------------- ASP forward
// x is centred on `center` (the plain time mean; the inference engines) or, with none given (the training entry points), on the
// utterance's first frame of the channel, to keep the sums well conditioned in f32: raw E[x^2] - E[x]^2 loses (mean / std)^2 of
// the std's relative precision.  With no centre given the variance comes from a second pass about the mean just found: sum p (x - mu)^2
// has no cancellation left, whatever the softmax weighs (a peaked one puts mu far from any fixed centre: var << (mu - centre)^2, and
// s2 / s0 - md^2 loses var's leading digits).  logits, x: f32 or bf16 as the kernel's template arguments say.
struct AspArgs {
    const void* logits; const void* x; const float* center; float* pooled;
    int ldx, xoff, ldc, B, T_, C; float eps;
};

// the four waves' online-softmax states (max, s0, s1[, s2]) of the streaming kernel -> the channel's max and sums
template <bool S2>
__device__ __forceinline__ float asp_merge4(float (*sm)[4][64], int lane, float& t0, float& t1, float& t2) {
    const float M = fmaxf(fmaxf(sm[0][0][lane], sm[1][0][lane]), fmaxf(sm[2][0][lane], sm[3][0][lane]));
    t0 = 0.f; t1 = 0.f; t2 = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const float mw = sm[w][0][lane];
        const float f = (mw == -INFINITY) ? 0.f : expf(mw - M);
        t0 += sm[w][1][lane] * f; t1 += sm[w][2][lane] * f;
        if (S2) t2 += sm[w][3][lane] * f;
    }
    return M;
}

// Streaming: one workgroup = 64 channels of one utterance; the 4 waves split the frames, online softmax per lane, merged through
// LDS.  f32 logits, any T.
template <typename TX>
__global__ __launch_bounds__(256) void asp_softmax_stats_kernel(AspArgs a) {
    const float* lg = static_cast<const float*>(a.logits);
    const TX* xg = static_cast<const TX*>(a.x);
    __shared__ float sm[4][4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int c = blockIdx.x * 64 + lane;
    const bool ok = c < a.C;
    const int cc = ok ? c : 0;
    const size_t row0 = (size_t)b * a.T_;
    const float mu0 = a.center ? a.center[(size_t)b * a.ldc + cc] : vp_to_f32(xg[row0 * a.ldx + a.xoff + cc]);
    float mx = -INFINITY, s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int t = wv; t < a.T_; t += 4) {
        const float e = lg[(row0 + t) * a.C + cc];
        const float xv = vp_to_f32(xg[(row0 + t) * a.ldx + a.xoff + cc]) - mu0;
        if (e > mx) {
            const float f = expf(mx - e);       // exp(-inf) = 0 on the first frame
            s0 = s0 * f + 1.f; s1 = s1 * f + xv; s2 = s2 * f + xv * xv; mx = e;
        } else {
            const float p = expf(e - mx);
            s0 += p; s1 += p * xv; s2 += p * xv * xv;
        }
    }
    sm[wv][0][lane] = mx; sm[wv][1][lane] = s0; sm[wv][2][lane] = s1; sm[wv][3][lane] = s2;
    __syncthreads();
    float t0, t1, t2;
    if (!a.center) {
        // second pass about the mean just found, reading the utterance's slice again
        const float M = asp_merge4<false>(sm, lane, t0, t1, t2);
        const float md = t1 / t0;
        float v = 0.f;
        for (int t = wv; t < a.T_; t += 4) {
            const float p = expf(lg[(row0 + t) * a.C + cc] - M);
            const float d = vp_to_f32(xg[(row0 + t) * a.ldx + a.xoff + cc]) - mu0 - md;
            v += p * d * d;
        }
        sm[wv][3][lane] = v;                    // (the first pass's s2: not read on this path)
        __syncthreads();
        if (wv == 0 && ok) asp_store(a.pooled, b, a.C, c, mu0, md, (sm[0][3][lane] + sm[1][3][lane] + sm[2][3][lane] + sm[3][3][lane]) / t0, a.eps);
        return;
    }
    if (wv == 0 && ok) {
        asp_merge4<true>(sm, lane, t0, t1, t2);
        const float md = t1 / t0;
        asp_store(a.pooled, b, a.C, c, mu0, md, t2 / t0 - md * md, a.eps);
    }
}

// T <= 8 NT: a thread keeps its share of an utterance's logits and x in registers -- all loads issued up front (the streaming kernel
// above has two loads in flight per thread and a divergent branch per frame: 4.2 TB/s) -- then max, then the sums.
// TL: the logits as stored -- float, or bf16 under enable_amp (what Paddle's O1 hands the softmax is the bf16 output of the logits
// conv, cast up); TX: x as its producer stored it.
template <int NT, typename TL, typename TX>
__global__ __launch_bounds__(512) void asp_softmax_stats_reg_kernel(AspArgs a) {
    const TL* __restrict__ lg = static_cast<const TL*>(a.logits);
    const TX* __restrict__ xg = static_cast<const TX*>(a.x);
    __shared__ float sm[4][8][64];
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int c = blockIdx.x * 64 + lane;
    const bool ok = c < a.C;
    const int cc = ok ? c : 0;
    const size_t row0 = (size_t)b * a.T_;
    const float mu0 = a.center ? a.center[(size_t)b * a.ldc + cc] : vp_to_f32(xg[row0 * a.ldx + a.xoff + cc]);    // (as in the streaming kernel)
    float ev[NT], xv[NT];
    fg_load<NT>(lg + cc, a.C, xg + a.xoff + cc, a.ldx, row0, rg, a.T_, ev, xv);
    const float mx = fg_max<NT>(ev, rg, a.T_, sm[0], lane);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        if (fg_has(rg, i, a.T_)) {
            const float p = expf(ev[i] - mx), d = xv[i] - mu0;
            s0 += p; s1 += p * d; s2 += p * d * d;
        }
    }
    sm[1][rg][lane] = s0; sm[2][rg][lane] = s1; sm[3][rg][lane] = s2;
    __syncthreads();
    if (!a.center) {
        // the second pass runs over the registers
        float s01[2];                            // sum p, sum p (x - mu0)
        fg_sums(sm + 1, lane, s01);
        const float t0 = s01[0], md = s01[1] / t0;
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            if (fg_has(rg, i, a.T_)) {
                const float p = expf(ev[i] - mx), d = xv[i] - mu0 - md;
                v += p * d * d;
            }
        }
        sm[0][rg][lane] = v;                    // (the maxima were last read before the barrier above)
        __syncthreads();
        if (rg == 0 && ok) {
            float sv[1];
            fg_sums(sm, lane, sv);
            asp_store(a.pooled, b, a.C, c, mu0, md, sv[0] / t0, a.eps);
        }
        return;
    }
    if (rg == 0 && ok) {
        float t[3];
        fg_sums(sm + 1, lane, t);
        const float md = t[1] / t[0];
        asp_store(a.pooled, b, a.C, c, mu0, md, t[2] / t[0] - md * md, a.eps);
    }
}

// ---------------------------------------------------------------- ASP backward
//   dv = [sd^2 > eps] dsd / (2 sd);  dalpha_t = dmu x_t + dv (x_t - mu)^2;  S = sum_t alpha_t dalpha_t
//   de_t = alpha_t (dalpha_t - S);   dx_t = alpha_t (dmu + 2 dv (x_t - mu))
// e, x, de: f32 or bf16 as the kernel's template arguments say (TE = bf16_t: d e leaves as bf16 -- the operand the logits conv's two
// backward GEMMs would round it to anyway)
struct AsBwdArgs { const void* e; const void* x; const float* pooled; const float* dpooled; void* de; float* dx; int ldx, lddx, T, C; float eps; };

// Streaming: one workgroup = 64 channels of one utterance, three passes over its frames (max; normaliser and S; outputs).  f32 e and x.
template <typename TE>
__global__ __launch_bounds__(256) void attn_stats_bwd_kernel(AsBwdArgs a) {
    __shared__ float sm[2][4][64];
    const int lc = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int b = blockIdx.y, c = blockIdx.x * 64 + lc;
    const bool ok = c < a.C;
    const int cc = ok ? c : 0;
    const float* eb = static_cast<const float*>(a.e) + (size_t)b * a.T * a.C + cc;
    const float* xb = static_cast<const float*>(a.x) + (size_t)b * a.T * a.ldx + cc;
    TE* de = static_cast<TE*>(a.de);
    const float mu = a.pooled[(size_t)b * 2 * a.C + cc], sd = a.pooled[(size_t)b * 2 * a.C + a.C + cc];
    const float dmu = a.dpooled[(size_t)b * 2 * a.C + cc], dsd = a.dpooled[(size_t)b * 2 * a.C + a.C + cc];
    const float dv = clamp_open(sd, a.eps) ? dsd / (2.f * sd) : 0.f;
    float mx = -INFINITY;
    for (int t = rg; t < a.T; t += 4) mx = fmaxf(mx, eb[(size_t)t * a.C]);
    sm[0][rg][lc] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sm[0][0][lc], sm[0][1][lc]), fmaxf(sm[0][2][lc], sm[0][3][lc]));
    __syncthreads();
    float z = 0.f, u = 0.f;
    for (int t = rg; t < a.T; t += 4) {
        const float p = expf(eb[(size_t)t * a.C] - mx);
        const float xv = xb[(size_t)t * a.ldx], d = xv - mu;
        z += p; u += p * (dmu * xv + dv * d * d);
    }
    sm[0][rg][lc] = z; sm[1][rg][lc] = u;
    __syncthreads();
    z = sm[0][0][lc] + sm[0][1][lc] + sm[0][2][lc] + sm[0][3][lc];
    u = sm[1][0][lc] + sm[1][1][lc] + sm[1][2][lc] + sm[1][3][lc];
    const float S = u / z;
    if (!ok) return;
    for (int t = rg; t < a.T; t += 4) {
        const float al = expf(eb[(size_t)t * a.C] - mx) / z;
        const float xv = xb[(size_t)t * a.ldx], d = xv - mu;
        de[((size_t)b * a.T + t) * a.C + c] = (TE)(al * (dmu * xv + dv * d * d - S));
        a.dx[((size_t)b * a.T + t) * a.lddx + c] = al * (dmu + 2.f * dv * d);
    }
}

// The same with the thread's share of e and x kept in REGISTERS between the passes (T <= 8 NT).  The plain kernel above re-reads both
// slices from HBM in its second and third pass (PMC: 2.35 GB read per launch at B = 256 for 0.94 GB of inputs -- 552 us, the largest
// kernel of the backward pass bar the weight gradients); here every input byte is read once.  (An LDS-resident variant -- 76 KB per
// workgroup, two per CU -- measured SLOWER than the plain kernel: 8 waves per CU cannot keep enough loads in flight.)
// TL = bf16: the logits as the forward stored them; TX = bf16: x as its producer stored it.
template <typename TE, int NT, typename TL, typename TX>
__global__ __launch_bounds__(512) void attn_stats_bwd_reg_kernel(AsBwdArgs a) {
    __shared__ float sm[2][8][64];
    const int lc = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int b = blockIdx.y, c = blockIdx.x * 64 + lc;
    const bool ok = c < a.C;
    const int cc = ok ? c : 0;
    TE* de = static_cast<TE*>(a.de);
    const float mu = a.pooled[(size_t)b * 2 * a.C + cc], sd = a.pooled[(size_t)b * 2 * a.C + a.C + cc];
    const float dmu = a.dpooled[(size_t)b * 2 * a.C + cc], dsd = a.dpooled[(size_t)b * 2 * a.C + a.C + cc];
    const float dv = clamp_open(sd, a.eps) ? dsd / (2.f * sd) : 0.f;
    float ev[NT], xv[NT];
    fg_load<NT>(static_cast<const TL*>(a.e) + (size_t)b * a.T * a.C + cc, a.C, static_cast<const TX*>(a.x) + (size_t)b * a.T * a.ldx + cc, a.ldx,
                0, rg, a.T, ev, xv);
    const float mx = fg_max<NT>(ev, rg, a.T, sm[0], lc);
    __syncthreads();
    float z = 0.f, u = 0.f;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const float p = fg_has(rg, i, a.T) ? expf(ev[i] - mx) : 0.f;
        const float d = xv[i] - mu;
        ev[i] = p;                                  // exp(e - max): the third pass needs nothing else of e
        z += p; u += p * (dmu * xv[i] + dv * d * d);
    }
    sm[0][rg][lc] = z; sm[1][rg][lc] = u;
    __syncthreads();
    float zu[2];
    fg_sums(sm, lc, zu);
    z = zu[0];
    const float S = zu[1] / z;
    if (!ok) return;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        if (fg_has(rg, i, a.T)) {
            const int t = rg + 8 * i;
            const float al = ev[i] / z;
            const float d = xv[i] - mu;
            de[((size_t)b * a.T + t) * a.C + c] = (TE)(al * (dmu * xv[i] + dv * d * d - S));
            a.dx[((size_t)b * a.T + t) * a.lddx + c] = al * (dmu + 2.f * dv * d);
        }
    }
}

// ---------------------------------------------------------------- ASP dispatch, both directions
// T -> the register kernel whose 8 NT frames hold it, else streaming.  bf16 logits have no streaming kernel on either side, so the
// forward that accepted a T and the backward that is handed its logits must agree on these edges: both ask here.
constexpr int ASP_NT_SHORT = 20, ASP_NT_LONG = 40;
enum AspPath { ASP_REG_SHORT, ASP_REG_LONG, ASP_STREAMING };
AspPath asp_path(int T) { return T <= 8 * ASP_NT_SHORT ? ASP_REG_SHORT : T <= 8 * ASP_NT_LONG ? ASP_REG_LONG : ASP_STREAMING; }

// One dtype combination's kernels: reg[ASP_REG_SHORT], reg[ASP_REG_LONG] and the streaming one; nullptr where none is built.
template <typename Args>
struct AspKernels { void (*reg[2])(Args); void (*streaming)(Args); };

// The kernel asp_path(T) names; the streaming one instead where the combination has no register kernels or the direction's A/B
// switch (plain) is set.  No streaming kernel to fall to: VP_EUNSUP, nothing launched.
template <typename Args>
int asp_launch(vp_ctx* ctx, const char* name, const AspKernels<Args>& k, bool plain, const Args& a, int B, int T, hipStream_t st) {
    const AspPath p = plain ? ASP_STREAMING : asp_path(T);
    void (*const fn)(Args) = p != ASP_STREAMING && k.reg[p] ? k.reg[p] : k.streaming;
    if (!fn) return VP_EUNSUP;
    hipLaunchKernelGGL(fn, dim3((a.C + 63) / 64, B), dim3(fn == k.streaming ? 256 : 512), 0, st, a);
    VP_LAUNCH_CHECK(ctx, name);
    return VP_OK;
}

int asp_fwd(vp_ctx* ctx, bool l16, bool x16, const AspArgs& a, const char* name, hipStream_t st) {
    using K = AspKernels<AspArgs>;
    static const K f32_x32{{asp_softmax_stats_reg_kernel<ASP_NT_SHORT, float, float>, asp_softmax_stats_reg_kernel<ASP_NT_LONG, float, float>},
                           asp_softmax_stats_kernel<float>};
    static const K f32_x16{{nullptr, nullptr}, asp_softmax_stats_kernel<bf16_t>};        // the bf16 inference engine: streaming at every T
    static const K l16_x32{{asp_softmax_stats_reg_kernel<ASP_NT_SHORT, bf16_t, float>, asp_softmax_stats_reg_kernel<ASP_NT_LONG, bf16_t, float>}, nullptr};
    static const K l16_x16{{asp_softmax_stats_reg_kernel<ASP_NT_SHORT, bf16_t, bf16_t>, asp_softmax_stats_reg_kernel<ASP_NT_LONG, bf16_t, bf16_t>}, nullptr};
    static const bool plain = getenv("VPMI_ASP_STATS_PLAIN") != nullptr;          // A/B switch of the f32 logits, read once per process
    return asp_launch(ctx, name, l16 ? (x16 ? l16_x16 : l16_x32) : (x16 ? f32_x16 : f32_x32), plain && !l16, a, a.B, a.T_, st);
}

// e16: e and d e bf16, x f32 or bf16 (x16); else e and x f32, d e f32 or bf16 (de16)
int attn_stats_bwd(vp_ctx* ctx, bool e16, bool x16, bool de16, const AsBwdArgs& a, int B, const char* name, hipStream_t st) {
    using K = AspKernels<AsBwdArgs>;
    static const K f32_de32{{attn_stats_bwd_reg_kernel<float, ASP_NT_SHORT, float, float>, attn_stats_bwd_reg_kernel<float, ASP_NT_LONG, float, float>},
                            attn_stats_bwd_kernel<float>};
    static const K f32_de16{{attn_stats_bwd_reg_kernel<bf16_t, ASP_NT_SHORT, float, float>, attn_stats_bwd_reg_kernel<bf16_t, ASP_NT_LONG, float, float>},
                            attn_stats_bwd_kernel<bf16_t>};
    static const K e16_x32{{attn_stats_bwd_reg_kernel<bf16_t, ASP_NT_SHORT, bf16_t, float>, attn_stats_bwd_reg_kernel<bf16_t, ASP_NT_LONG, bf16_t, float>}, nullptr};
    static const K e16_x16{{attn_stats_bwd_reg_kernel<bf16_t, ASP_NT_SHORT, bf16_t, bf16_t>, attn_stats_bwd_reg_kernel<bf16_t, ASP_NT_LONG, bf16_t, bf16_t>}, nullptr};
    static const bool plain = getenv("VPMI_ASB_PLAIN") != nullptr;      // A/B switch of the f32 logits, read once per process
    return asp_launch(ctx, name, e16 ? (x16 ? e16_x16 : e16_x32) : (de16 ? f32_de16 : f32_de32), plain && !e16, a, B, a.T, st);
}

// ---------------------------------------------------------------- time statistics, forward
// mean / std over time straight from the activations (small T): stats[b] = [mean(C) | std(C)] (moments_finish), sums about the
// utterance's first frame of the channel
struct TmArgs { const void* x; float* stats; int ldx, Tn, C; float eps; int unbiased; };      // x: f32 or bf16 as the kernel says

template <typename T>
__global__ __launch_bounds__(256) void time_moments_kernel(TmArgs a) {
    __shared__ float sm[2][4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y, c = blockIdx.x * 64 + lane;
    const bool ok = c < a.C;
    const int cc = ok ? c : 0;
    const T* xb = static_cast<const T*>(a.x) + (size_t)b * a.Tn * a.ldx;
    const float c0 = vp_to_f32(xb[cc]);
    float s1 = 0.f, s2 = 0.f;
    for (int t = wv; t < a.Tn; t += 4) {
        const float v = vp_to_f32(xb[(size_t)t * a.ldx + cc]) - c0;
        s1 += v; s2 += v * v;
    }
    sm[0][wv][lane] = s1; sm[1][wv][lane] = s2;
    __syncthreads();
    if (wv == 0 && ok) {
        const float t1 = sm[0][0][lane] + sm[0][1][lane] + sm[0][2][lane] + sm[0][3][lane];
        const float t2 = sm[1][0][lane] + sm[1][1][lane] + sm[1][2][lane] + sm[1][3][lane];
        float md, sd;
        moments_finish(t1, t2, a.Tn, a.unbiased, a.eps, md, sd);
        a.stats[(size_t)b * 2 * a.C + c] = c0 + md;
        a.stats[(size_t)b * 2 * a.C + a.C + c] = sd;
    }
}

// f32 activations (the training path), four channels per lane
__global__ __launch_bounds__(256) void time_moments4_kernel(TmArgs a) {
    __shared__ float sm[2][256][4];
    const int lc = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int b = blockIdx.y, c4 = blockIdx.x * 32 + lc;
    const bool ok = c4 < (a.C >> 2);
    const int c = ok ? c4 * 4 : 0;
    float c0[4], m[4], sd[4];
    moments4_accumulate(static_cast<const float*>(a.x) + (size_t)b * a.Tn * a.ldx + c, a.ldx, 0, a.Tn, sm, c0);
    if (rg != 0 || !ok) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float t1, t2, md;
        moments4_total(sm, lc, e, t1, t2);
        moments_finish(t1, t2, a.Tn, a.unbiased, a.eps, md, sd[e]);
        m[e] = c0[e] + md;
    }
    vp_store4(a.stats + (size_t)b * 2 * a.C + c, m);
    vp_store4(a.stats + (size_t)b * 2 * a.C + a.C + c, sd);
}

// Many positions per utterance (2-D feature maps): the frames are cut into chunks (grid = channel blocks x B x chunks), partial
// sums of (x - x[first frame]) and its square per chunk, then a finalize over the chunks in order.  part: [B][chunks][2][C].
struct TmChunkArgs { const float* x; float* part; int ldx, Tn, C, chunks, rows_per_chunk; };
__global__ __launch_bounds__(256) void time_moments_chunk_kernel(TmChunkArgs a) {
    __shared__ float sm[2][256][4];
    const int lc = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int b = blockIdx.y, ch = blockIdx.z, c4 = blockIdx.x * 32 + lc;
    const bool ok = c4 < (a.C >> 2);
    const int c = ok ? c4 * 4 : 0;
    const int t0 = ch * a.rows_per_chunk;
    float c0[4], t1[4], t2[4];
    moments4_accumulate(a.x + (size_t)b * a.Tn * a.ldx + c, a.ldx, t0, min(a.Tn, t0 + a.rows_per_chunk), sm, c0);
    if (rg != 0 || !ok) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) moments4_total(sm, lc, e, t1[e], t2[e]);
    float* p = a.part + ((size_t)b * a.chunks + ch) * 2 * a.C;
    vp_store4(p + c, t1);
    vp_store4(p + a.C + c, t2);
}
struct TmFinArgs { const float* x; const float* part; float* stats; int ldx, Tn, C, chunks, unbiased; float eps; };
__global__ __launch_bounds__(256) void time_moments_fin_kernel(TmFinArgs a) {
    const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    float t1 = 0.f, t2 = 0.f;
    for (int ch = 0; ch < a.chunks; ++ch) {
        const float* p = a.part + ((size_t)b * a.chunks + ch) * 2 * a.C;
        t1 += p[c]; t2 += p[a.C + c];
    }
    const float c0 = a.x[(size_t)b * a.Tn * a.ldx + c];
    float md, sd;
    moments_finish(t1, t2, a.Tn, a.unbiased, a.eps, md, sd);
    a.stats[(size_t)b * 2 * a.C + c] = c0 + md;
    a.stats[(size_t)b * 2 * a.C + a.C + c] = sd;
}
void tm_geometry(int B, int T, int C, int& chunks, int& rpc) {
    const int cblocks = (C / 4 + 31) / 32;
    long long ch = 2048 / ((long long)B * cblocks > 0 ? (long long)B * cblocks : 1);
    if (ch < 1) ch = 1;
    long long r = (T + ch - 1) / ch;
    if (r < 64) r = 64;
    rpc = (int)r;
    chunks = (T + rpc - 1) / rpc;
}

// ---------------------------------------------------------------- time statistics, backward
// Backward of stats[b] = [mean_t x | sqrt(max(var_biased_t x, eps))] (pooling.py:97-104 with a mask of ones):
// dx[b,t,c] = dmean / T + [var > eps] * dstd / std * (x - mean) / T
struct TsBwdArgs { const void* x; const float* stats; const float* dstats; float* dx; int ldx, lddx, T, C4; float eps; long long total; int unbiased;
                   const float* add; int ldadd; };     // x: TX (f32 or bf16); add: other gradients of x summed in the same pass (may alias dx)
template <typename TX>
__global__ __launch_bounds__(256) void time_stats_bwd_kernel(TsBwdArgs a) {
    const TX* xg = static_cast<const TX*>(a.x);
    const int C = a.C4 * 4;
    const float invT = 1.f / (float)a.T;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (long long)gridDim.x * 256) {
        const long long m = i / a.C4;
        const int c = (int)(i - m * a.C4) * 4;
        const long long b = m / a.T;
        float x[4], mu[4], sd[4], dm[4], ds[4], o[4];
        vp_load4(xg + m * a.ldx + c, x);
        vp_load4(a.stats + b * 2 * C + c, mu); vp_load4(a.stats + b * 2 * C + C + c, sd);
        vp_load4(a.dstats + b * 2 * C + c, dm); vp_load4(a.dstats + b * 2 * C + C + c, ds);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            // sd = sqrt(var_unbiased + eps).  eps = 0 (CAM++'s statistics pooling, campplus.py:24-30) and a channel that is constant over an
            // utterance's frames (a ReLU output that is zero throughout) give sd = 0: the term is 0 / 0.  Its limit -- and what autograd
            // frameworks return for d sqrt(var) at var = 0 (torch masks it; round 5: this NaN reached Adam ~200 steps into a CAM++ run and
            // killed the model, tools/train_dynamics_ab.py) -- is no contribution from the std
            o[e] = a.unbiased ? dm[e] * invT + (sd[e] > 0.f ? ds[e] / sd[e] * (x[e] - mu[e]) / (float)(a.T > 1 ? a.T - 1 : 1) : 0.f)
                              : dm[e] * invT + (clamp_open(sd[e], a.eps) ? ds[e] / sd[e] * (x[e] - mu[e]) * invT : 0.f);
        if (a.add) {
            float ad[4];
            vp_load4(a.add + m * a.ldadd + c, ad);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] += ad[e];
        }
        vp_store4(a.dx + m * a.lddx + c, o);
    }
}

// The same gradient as per-utterance coefficients: dx[b,t,c] = alpha[b,c] + beta[b,c] * x[b,t,c] with beta = [var > eps] dstd / (std T),
// alpha = dmean / T - beta * mean -- what the BatchNorm-backward passes of the producing layer add to their d y on the fly
// (ColSum4Args UTT == 2, csrc/bn_train.hip) instead of a pass over the (B*T, C) tensor.  ab: [2][B][C]
__global__ __launch_bounds__(256) void time_stats_bwd_coeffs_kernel(const float* stats, const float* dstats, int B, int C, int T, float eps, float* ab) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, c = i - b * C;
    const float invT = 1.f / (float)T;
    const float mu = stats[(size_t)b * 2 * C + c], sd = stats[(size_t)b * 2 * C + C + c];
    const float dm = dstats[(size_t)b * 2 * C + c], ds = dstats[(size_t)b * 2 * C + C + c];
    const float be = clamp_open(sd, eps) ? ds / sd * invT : 0.f;
    ab[i] = __fmaf_rn(-be, mu, dm * invT);
    ab[(size_t)B * C + i] = be;
}

// x f32 or bf16 (ldx in elements); add (with_add): the other consumers' gradients of x folded into this pass (add may be dx)
template <typename TX>
int time_stats_bwd(vp_ctx* ctx, const char* name, const void* x, int ldx, const float* stats, const float* dstats, int B, int T, int C, float eps,
                   int unbiased, bool with_add, const float* add, int ldadd, float* dx, int lddx, vp_stream stream) {
    if (!ctx || !x || !stats || !dstats || !dx || (with_add && !add) || B <= 0 || T <= 0 || C <= 0 || (C | ldx | lddx | ldadd) & 3)
        VP_FAIL(ctx, VP_EINVAL, "%s: bad arguments", name);
    TsBwdArgs a{x, stats, dstats, dx, ldx, lddx, T, C / 4, eps, (long long)B * T * (C / 4), unbiased, add, ldadd};
    const long long blocks = (a.total + 255) / 256;
    hipLaunchKernelGGL(time_stats_bwd_kernel<TX>, dim3((unsigned)(blocks > 256 * 64 ? 256 * 64 : blocks)), dim3(256), 0, (hipStream_t)stream, a);
    VP_LAUNCH_CHECK(ctx, name);
    return VP_OK;
}

// ---------------------------------------------------------------- per-utterance sums
// out[b][c] = sum_t a[b, t, c]   (gradient of a per-utterance bias; one workgroup = 64 channels of one utterance)
template <typename TA>
__global__ __launch_bounds__(256) void utt_sums_kernel(const TA* a, int lda, int T, int C, float* out) {
    __shared__ float sm[4][64];
    const int lc = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int b = blockIdx.y, c = blockIdx.x * 64 + lc;
    float s = 0.f;
    if (c < C)
        for (int t = rg; t < T; t += 4) s += vp_to_f32(a[((size_t)b * T + t) * lda + c]);
    sm[rg][lc] = s;
    __syncthreads();
    if (rg == 0 && c < C) out[(size_t)b * C + c] = sm[0][lc] + sm[1][lc] + sm[2][lc] + sm[3][lc];
}

template <typename TA>
int utt_sums(vp_ctx* ctx, const char* name, const void* a, int lda, int B, int T, int C, float* out, vp_stream stream) {
    if (!ctx || !a || !out || B <= 0 || T <= 0 || C <= 0 || B > 65535) VP_FAIL(ctx, VP_EINVAL, "%s: bad arguments", name);
    hipLaunchKernelGGL(utt_sums_kernel<TA>, dim3((C + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, static_cast<const TA*>(a), lda, T, C, out);
    VP_LAUNCH_CHECK(ctx, name);
    return VP_OK;
}

}  // namespace

// ---------------------------------------------------------------- entry points
int vp_asp_softmax_stats_ex(vp_ctx* ctx, int dtype, const float* logits, const void* x, int ldx, int xoff,
                            const float* center, int ldc, int B, int T, int C, float eps, float* pooled, hipStream_t st) {
    if (!ctx || !logits || !x || !pooled || B <= 0 || T <= 0 || C <= 0) VP_FAIL(ctx, VP_EINVAL, "asp: bad arguments");
    if (B > 65535) VP_FAIL(ctx, VP_EINVAL, "asp: batch too large");
    if (dtype != VP_BF16 && dtype != VP_F32) VP_FAIL(ctx, VP_EINVAL, "asp: bad dtype");
    return asp_fwd(ctx, false, dtype == VP_BF16, AspArgs{logits, x, center, pooled, ldx, xoff, ldc, B, T, C, eps}, "asp_softmax_stats", st);
}

int vp_time_moments(vp_ctx* ctx, int dtype, const void* x, int ldx, int B, int T, int C, float eps, int unbiased,
                    float* stats, hipStream_t st) {
    if (B > 65535) VP_FAIL(ctx, VP_EINVAL, "time_moments: batch too large");
    const dim3 grid((C + 63) / 64, B);
    const TmArgs a{x, stats, ldx, T, C, eps, unbiased};
    if (dtype != VP_BF16 && ((C | ldx) & 3) == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)stats & 15) == 0)
        hipLaunchKernelGGL(time_moments4_kernel, dim3((C / 4 + 31) / 32, B), dim3(256), 0, st, a);
    else if (dtype == VP_BF16) hipLaunchKernelGGL(time_moments_kernel<bf16_t>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(time_moments_kernel<float>, grid, dim3(256), 0, st, a);
    VP_LAUNCH_CHECK(ctx, "time_moments");
    return VP_OK;
}

extern "C" {

int vp_asp_softmax_stats(vp_ctx* ctx, int dtype, const float* logits, const void* x, int ldx, int xoff,
                         int B, int T, int C, float eps, float* pooled, vp_stream stream) {
    return vp_asp_softmax_stats_ex(ctx, dtype, logits, x, ldx, xoff, nullptr, 0, B, T, C, eps, pooled, (hipStream_t)stream);
}

// f32 or bf16 x, logits stored as bf16 (the training engine under enable_amp; T <= 320, else VP_EUNSUP: the caller keeps f32 logits)
int vp_asp_softmax_stats_l16(vp_ctx* ctx, const void* logits_bf16, const void* x, int x_dtype, int ldx, int xoff, int B, int T, int C, float eps,
                             float* pooled, vp_stream stream) {
    if (!ctx || !logits_bf16 || !x || !pooled || B <= 0 || T <= 0 || C <= 0 || B > 65535 || (x_dtype != VP_F32 && x_dtype != VP_BF16))
        VP_FAIL(ctx, VP_EINVAL, "asp_l16: bad arguments");
    return asp_fwd(ctx, true, x_dtype == VP_BF16, AspArgs{logits_bf16, x, nullptr, pooled, ldx, xoff, 0, B, T, C, eps}, "asp_softmax_stats_l16",
                   (hipStream_t)stream);
}

int vp_attn_stats_bwd_f32(vp_ctx* ctx, const float* e, const float* x, int ldx, const float* pooled, const float* dpooled, int B, int T,
                          int C, float eps, float* de, float* dx, int lddx, vp_stream stream) {
    if (!ctx || !e || !x || !pooled || !dpooled || !de || !dx || B <= 0 || T <= 0 || C <= 0 || B > 65535) VP_FAIL(ctx, VP_EINVAL, "attn_stats_bwd: bad arguments");
    return attn_stats_bwd(ctx, false, false, false, AsBwdArgs{e, x, pooled, dpooled, de, dx, ldx, lddx, T, C, eps}, B, "attn_stats_bwd", (hipStream_t)stream);
}

// d e written as bf16 ((B*T, C) dense): mixed precision, the logits conv's backward GEMMs then read bf16 operands
int vp_attn_stats_bwd_de16(vp_ctx* ctx, const float* e, const float* x, int ldx, const float* pooled, const float* dpooled, int B, int T,
                           int C, float eps, void* de, float* dx, int lddx, vp_stream stream) {
    if (!ctx || !e || !x || !pooled || !dpooled || !de || !dx || B <= 0 || T <= 0 || C <= 0 || B > 65535) VP_FAIL(ctx, VP_EINVAL, "attn_stats_bwd: bad arguments");
    return attn_stats_bwd(ctx, false, false, true, AsBwdArgs{e, x, pooled, dpooled, de, dx, ldx, lddx, T, C, eps}, B, "attn_stats_bwd_de16", (hipStream_t)stream);
}

// d e bf16 AND e stored as bf16 (vp_asp_softmax_stats_l16's logits); T <= 320, else VP_EUNSUP
int vp_attn_stats_bwd_e16(vp_ctx* ctx, const void* e_bf16, const void* x, int x_dtype, int ldx, const float* pooled, const float* dpooled, int B,
                          int T, int C, float eps, void* de_bf16, float* dx, int lddx, vp_stream stream) {
    if (!ctx || !e_bf16 || !x || !pooled || !dpooled || !de_bf16 || !dx || B <= 0 || T <= 0 || C <= 0 || B > 65535 ||
        (x_dtype != VP_F32 && x_dtype != VP_BF16))
        VP_FAIL(ctx, VP_EINVAL, "attn_stats_bwd_e16: bad arguments");
    return attn_stats_bwd(ctx, true, x_dtype == VP_BF16, true, AsBwdArgs{e_bf16, x, pooled, dpooled, de_bf16, dx, ldx, lddx, T, C, eps}, B,
                          "attn_stats_bwd_e16", (hipStream_t)stream);
}

int vp_time_stats_f32(vp_ctx* ctx, const float* x, int ldx, int B, int T, int C, float eps, int unbiased, float* stats, vp_stream stream) {
    if (!ctx || !x || !stats || B <= 0 || T <= 0 || C <= 0) VP_FAIL(ctx, VP_EINVAL, "time_stats: bad arguments");
    return vp_time_moments(ctx, VP_F32, x, ldx, B, T, C, eps, unbiased, stats, (hipStream_t)stream);
}

size_t vp_time_stats_workspace_bytes(int B, int T, int C) {
    if (B <= 0 || T <= 0 || C <= 0) return 0;
    int chunks, rpc;
    tm_geometry(B, T, C, chunks, rpc);
    return (size_t)B * chunks * 2 * C * sizeof(float) + 256;
}

// f32 (B, T, C) with MANY frames per utterance (ResNetSE / ERes2Net feature maps as (B, T*F', C)): [mean | std] with the frames spread over
// ~2048 workgroups.  C % 4 == 0, ldx % 4 == 0, 16-byte aligned; else VP_EUNSUP (callers use vp_time_stats_f32).
int vp_time_stats_ws_f32(vp_ctx* ctx, const float* x, int ldx, int B, int T, int C, float eps, int unbiased, float* stats, void* ws,
                         size_t ws_bytes, vp_stream stream) {
    if (!ctx || !x || !stats || B <= 0 || T <= 0 || C <= 0 || B > 65535) VP_FAIL(ctx, VP_EINVAL, "time_stats_ws: bad arguments");
    if (((C | ldx) & 3) || ((uintptr_t)x & 15)) return VP_EUNSUP;
    if (!ws || ws_bytes < vp_time_stats_workspace_bytes(B, T, C)) VP_FAIL(ctx, VP_EWORKSPACE, "time_stats_ws: workspace too small");
    int chunks, rpc;
    tm_geometry(B, T, C, chunks, rpc);
    hipStream_t st = (hipStream_t)stream;
    TmChunkArgs a{x, (float*)ws, ldx, T, C, chunks, rpc};
    hipLaunchKernelGGL(time_moments_chunk_kernel, dim3((C / 4 + 31) / 32, B, chunks), dim3(256), 0, st, a);
    VP_LAUNCH_CHECK(ctx, "time_moments_chunk");
    TmFinArgs f{x, (const float*)ws, stats, ldx, T, C, chunks, unbiased, eps};
    hipLaunchKernelGGL(time_moments_fin_kernel, dim3((C + 255) / 256, B), dim3(256), 0, st, f);
    VP_LAUNCH_CHECK(ctx, "time_moments_fin");
    return VP_OK;
}

int vp_time_stats_bwd_f32(vp_ctx* ctx, const float* x, int ldx, const float* stats, const float* dstats, int B, int T, int C, float eps,
                          int unbiased, float* dx, int lddx, vp_stream stream) {
    return time_stats_bwd<float>(ctx, "time_stats_bwd", x, ldx, stats, dstats, B, T, C, eps, unbiased, false, nullptr, 0, dx, lddx, stream);
}

int vp_time_stats_bwd_add_f32(vp_ctx* ctx, const float* x, int ldx, const float* stats, const float* dstats, int B, int T, int C, float eps,
                              int unbiased, const float* add, int ldadd, float* dx, int lddx, vp_stream stream) {
    return time_stats_bwd<float>(ctx, "time_stats_bwd_add", x, ldx, stats, dstats, B, T, C, eps, unbiased, true, add, ldadd, dx, lddx, stream);
}

int vp_time_stats_bwd_add_x16(vp_ctx* ctx, const void* x_bf16, int ldx, const float* stats, const float* dstats, int B, int T, int C, float eps,
                              int unbiased, const float* add, int ldadd, float* dx, int lddx, vp_stream stream) {
    return time_stats_bwd<bf16_t>(ctx, "time_stats_bwd_add_x16", x_bf16, ldx, stats, dstats, B, T, C, eps, unbiased, true, add, ldadd, dx, lddx, stream);
}

// alpha / beta of the context-statistics gradient (time_stats_bwd_coeffs_kernel): ab [2][B][C]
int vp_time_stats_bwd_coeffs(vp_ctx* ctx, const float* stats, const float* dstats, int B, int T, int C, float eps, float* ab, vp_stream stream) {
    if (!ctx || !stats || !dstats || !ab || B <= 0 || T <= 0 || C <= 0) VP_FAIL(ctx, VP_EINVAL, "time_stats_bwd_coeffs: bad arguments");
    hipLaunchKernelGGL(time_stats_bwd_coeffs_kernel, dim3((B * C + 255) / 256), dim3(256), 0, (hipStream_t)stream, stats, dstats, B, C, T, eps, ab);
    VP_LAUNCH_CHECK(ctx, "time_stats_bwd_coeffs");
    return VP_OK;
}

int vp_utt_sums_f32(vp_ctx* ctx, const float* a, int lda, int B, int T, int C, float* out, vp_stream stream) {
    return utt_sums<float>(ctx, "utt_sums", a, lda, B, T, C, out, stream);
}

int vp_utt_sums_b16(vp_ctx* ctx, const void* a_bf16, int lda, int B, int T, int C, float* out, vp_stream stream) {
    return utt_sums<bf16_t>(ctx, "utt_sums_b16", a_bf16, lda, B, T, C, out, stream);
}

}  // extern "C"
