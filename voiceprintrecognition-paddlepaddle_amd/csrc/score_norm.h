// Adaptive score normalisation (AS-norm, docs/score_norm.md): the arithmetic every kernel that normalises a score shares -- the
// statistics' float64 tail (cohort_stats.hip), r = 1 / max(std, floor), and z (trial_pass_kernel<MODE, true> of trial_ranks.hip and
// score_norm_apply_kernel of cohort_stats.hip).  Device code, included by both.
//
// THE CONTRACT.  Every operation below is rounded on its own (to nearest even), in the order written: tests/score_norm_oracle.py
// restates them in NumPy, one operation per line, and gets the same bits.  hipcc contracts a * b + c into an fma by default.  The
// __fmul_rn / __fadd_rn / __dmul_rn / __dsub_rn of this toolchain are plain operators compiled under that default, so they fuse like
// any other once inlined; what keeps the operations apart is `fp contract(off)` over plain operators written HERE.  Division and
// square root are the correctly rounded ones (hipcc's default for f32, always for f64).
#pragma once
#include "common.h"

#include <math.h>

namespace score_norm {

constexpr float STD_FLOOR = 1e-6f;      // the tolerance on one cosine (TOL of tests/trial_ranks_oracle.py): a spread below it is noise

// sum and sum of squares (float64) of the N kept scores -> mean, std (population form), each rounded once to f32
__device__ __forceinline__ void mean_std(double s1, double s2, int N, float& mean, float& std) {
#pragma clang fp contract(off)
    const double n = (double)N;
    const double m = s1 / n;
    const double m2 = s2 / n;
    const double mm = m * m;
    const double var = m2 - mm;
    mean = (float)m;
    std = (float)__builtin_sqrt(var > 0.0 ? var : 0.0);
}

__device__ __forceinline__ float recip_std(float std) {
    return 1.f / (std > STD_FLOOR ? std : STD_FLOOR);
}

// z = 0.5 ((s - mean_e) r_e + (s - mean_t) r_t): sub, mul, sub, mul, add, mul
__device__ __forceinline__ float z(float s, float mean_e, float r_e, float mean_t, float r_t) {
#pragma clang fp contract(off)
    const float de = s - mean_e;
    const float pe = de * r_e;
    const float dt = s - mean_t;
    const float pt = dt * r_t;
    const float sum = pe + pt;
    return 0.5f * sum;
}

}  // namespace score_norm
