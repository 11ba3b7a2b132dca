// What the classifier head (head.hip, head_tiled.hip) and the loss family (losses.hip) share: the AAM margin and its constants, and the
// per-row log-sum-exp of a 256-thread workgroup.  Each piece is defined here once; the kernels keep their own loops.
#pragma once
#include "common.h"

#include <math.h>

// the five margin values, in the order of the device margin table (vp_set_margin_table)
struct VpMargin { float m, cos_m, sin_m, th, mmm; };          // m, cos m, sin m, cos(pi - m), 1 + cos(pi - m)

static inline VpMargin vp_margin_of(float margin) {
    VpMargin g;
    g.m = margin;
    g.cos_m = (float)cos((double)margin); g.sin_m = (float)sin((double)margin);
    g.th = (float)cos(M_PI - (double)margin); g.mmm = (float)(1.0 + cos(M_PI - (double)margin));
    return g;
}

// the table, when one is set, wins over the launch scalars.  take_m: AM, ARM and SphereFace2 read the margin itself as well; the
// AAM kernels only its four derived values
__device__ __forceinline__ void vp_margin_override(VpMargin& g, const float* mt, bool take_m) {
    if (!mt) return;
    if (take_m) g.m = mt[0];
    g.cos_m = mt[1]; g.sin_m = mt[2]; g.th = mt[3]; g.mmm = mt[4];
}

// the reference (aamloss.py:34) has no clamp and returns NaN when an f32 cosine rounds above 1; identical wherever |cos| <= 1
__device__ __forceinline__ float vp_clamped_sine(float cs) { return sqrtf(fmaxf(1.f - cs * cs, 0.f)); }

// AAM margin on a target cosine: phi = cos(theta + m) where the hard / easy select takes it, else cos - mmm (hard) / cos (easy).
// VpMargin travels by value and each form keeps the select of the kernels it came from: with that head_tile_bwd_kernel (256 VGPRs,
// scratch in use) compiles to the instructions it had with the arithmetic written in place; a by-reference helper gave it other code,
// 1 % slower at 200 000 classes (docs/training_step.md).
__device__ __forceinline__ float vp_aam_phi(const VpMargin g, const float cs, const float sine) { return cs * g.cos_m - sine * g.sin_m; }
__device__ __forceinline__ float vp_aam_margin(const VpMargin g, const int easy, const float cs) {
    const float phi = vp_aam_phi(g, cs, vp_clamped_sine(cs));
    return easy ? (cs > 0.f ? phi : cs) : (cs > g.th ? phi : cs - g.mmm);
}
// the same, and dm = d margin / d cos: 1 where phi is not taken (the division stays under that condition)
__device__ __forceinline__ float vp_aam_margin(const VpMargin g, const int easy, const float cs, float& dm) {
    const float sine = vp_clamped_sine(cs);
    const float phi = vp_aam_phi(g, cs, sine);
    const bool use_phi = easy ? (cs > 0.f) : (cs > g.th);
    dm = 1.f;
    const float o = use_phi ? phi : (easy ? cs : cs - g.mmm);
    if (use_phi) dm = g.cos_m + cs * g.sin_m / sine;
    return o;
}

// online log-sum-exp, one more value: mx = running max, se = sum exp(. - mx)
__device__ __forceinline__ void vp_lse_step(float o, float& mx, float& se) {
    if (o > mx) { se = se * expf(mx - o) + 1.f; mx = o; }
    else se += expf(o - mx);
}

// the 256 threads' (mx, se, so = sum of the values) -> lse and O = sum of the values, valid in thread 0 only: wave merge, then the
// four waves in fixed order.  sm: [3][4] floats of LDS.  Every thread of the workgroup calls it (it holds a barrier).
__device__ __forceinline__ void vp_lse_merge(float mx, float se, float so, float (*sm)[4], float& lse, float& O) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float wmx = vp_wave_max(mx);
    se = vp_wave_sum(mx == -INFINITY ? 0.f : se * expf(mx - wmx));
    so = vp_wave_sum(so);
    if (lane == 0) { sm[0][wv] = wmx; sm[1][wv] = se; sm[2][wv] = so; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float M = fmaxf(fmaxf(sm[0][0], sm[0][1]), fmaxf(sm[0][2], sm[0][3]));
        float S = 0.f;
        O = 0.f;
        for (int w = 0; w < 4; ++w) {
            S += (sm[0][w] == -INFINITY) ? 0.f : sm[1][w] * expf(sm[0][w] - M);
            O += sm[2][w];
        }
        lse = M + logf(S);
    }
}
