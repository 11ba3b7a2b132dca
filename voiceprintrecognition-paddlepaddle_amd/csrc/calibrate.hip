// Score calibration (docs/calibration.md; no reference call site: an extension): the twelve float64 sums from which the host takes the
// value, the gradient and the Hessian of the logistic objective of llr = a s + b over ALL (trial, enrol) pairs, without the (Nt, Ne)
// score matrix.
//
// calib_pass_kernel<NORM>  shaped like trial_pass_kernel of trial_ranks.hip: a workgroup holds 32 unit trial rows in LDS and walks
//                          `slabs_per_wg` slabs of unit enrol rows with cos_tile.h's walk -- the unit rows the targets pass of the trial
//                          scorer left in its workspace, so a pair has the bits it has in the ranks.  NORM: the score is
//                          score_norm.h's z of the cosine.  A lane widens each of its 16 scores to float64, takes the six terms of
//                          the pair's class (labels equal: target) and adds them to twelve float64 registers.  At the end of the walk
//                          the lanes of a wave are folded with __shfl_xor (32, 16, .. 1), the four waves through LDS in wave order,
//                          and one thread per sum writes the workgroup's twelve doubles to partials[workgroup].
// calib_fold_kernel        one workgroup: sum k is the partials' k-th doubles added in workgroup order.
// Every term and every sum is float64; the order of every addition is fixed by the shape alone: no float atomics, no grid barrier, no
// spinning; two runs give the same bits.  Every partial is written by the pass, so the buffers need no clearing.
#include "cos_tile.h"
#include "score_norm.h"
#include "trial_plan.h"

namespace {

constexpr int QT = cos_tile::COLS;
constexpr int NSUMS = 12;               // targets S0 .. S5, then non-targets S0 .. S5

struct CalibArgs {
    const float* tu;                    // (Nt, D) unit trial rows
    const float* eu;                    // (Ne, D) unit enrol rows
    const int* tl;                      // (Nt) ids
    const int* el;                      // (Ne)
    int Nt, Ne, D, slabs_per_wg;
    double a, b;                        // llr + tau = a s + b
    double* partials;                   // (workgroups, 12)
    // NORM: per trial and per enrol row the mean of its top cohort scores and r = 1 / max(std, floor)
    const float* tmean;
    const float* tr;
    const float* emean;
    const float* er;
};

// a s + b as two operations, each rounded on its own: tests/calibration_oracle.py restates it and gets the same bits
__device__ __forceinline__ double affine(double a, double s, double b) {
#pragma clang fp contract(off)
    const double p = a * s;
    return p + b;
}

// grid (trial tiles, row ranges), 256 threads, dynamic LDS: qs [Dp][32] | wave sums [4][12] float64
template <bool NORM>
__global__ __launch_bounds__(256) void calib_pass_kernel(const CalibArgs a) {
    extern __shared__ __align__(16) float smem[];
    const int D = a.D, Dp = (D + 7) & ~7;
    float* qs = smem;
    double* wsum = reinterpret_cast<double*>(smem + (size_t)Dp * QT);          // Dp QT 4 bytes: a multiple of 1024
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 31, half = lane >> 5;
    const int qt = blockIdx.x, range = blockIdx.y;

    cos_tile::load_tile<false>(qs, a.tu, qt * QT, a.Nt, D);
    __syncthreads();

    const int q = qt * QT + c;
    const bool my_q = q < a.Nt;         // the tile's columns past Nt are zero trials: no pair
    const int lq = my_q ? a.tl[q] : 0;
    float mt = 0.f, rt = 0.f;
    if (NORM && my_q) { mt = a.tmean[q]; rt = a.tr[q]; }
    double sum[NSUMS];
#pragma unroll
    for (int k = 0; k < NSUMS; ++k) sum[k] = 0.0;
    cos_tile::walk<long long>(qs, a.eu, a.Ne, D, range, a.slabs_per_wg, [&](long long r0, const cos_tile::f32x16& acc) {
        const long long rb = r0 + 4 * half;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const long long r = rb + 8 * (v >> 2) + (v & 3);
            const bool pair = my_q && r < a.Ne;
            const long long rr = pair ? r : 0;              // a row that exists; what it gives is left out below
            const bool tar = pair && a.el[rr] == lq, non = pair && !tar;
            const double s = NORM ? (double)score_norm::z(acc[v], a.emean[rr], a.er[rr], mt, rt) : (double)acc[v];
            const double y = affine(a.a, s, a.b);
            const double u = tar ? -y : y;
            // e = exp(-|u|) <= 1: softplus(u) = max(u, 0) + log1p(e); sigma(|u|) = 1 / (1 + e), sigma(-|u|) = e / (1 + e);
            // w = sigma(u) (1 - sigma(u)) = sigma(|u|) sigma(-|u|), which keeps its relative precision at large |u|
            const double e = exp(-fabs(u));
            const double hi = 1.0 / (1.0 + e), lo = e * hi;
            const double t0 = fmax(u, 0.0) + log1p(e);
            const double t1 = u >= 0.0 ? hi : lo;
            const double t3 = hi * lo;
            const double t2 = t1 * s, t4 = t3 * s, t5 = t4 * s;
            sum[0] += tar ? t0 : 0.0;
            sum[1] += tar ? t1 : 0.0;
            sum[2] += tar ? t2 : 0.0;
            sum[3] += tar ? t3 : 0.0;
            sum[4] += tar ? t4 : 0.0;
            sum[5] += tar ? t5 : 0.0;
            sum[6] += non ? t0 : 0.0;
            sum[7] += non ? t1 : 0.0;
            sum[8] += non ? t2 : 0.0;
            sum[9] += non ? t3 : 0.0;
            sum[10] += non ? t4 : 0.0;
            sum[11] += non ? t5 : 0.0;
        }
    });
#pragma unroll
    for (int k = 0; k < NSUMS; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum[k] += __shfl_xor(sum[k], o);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < NSUMS; ++k) wsum[(tid >> 6) * NSUMS + k] = sum[k];
    __syncthreads();
    if (tid < NSUMS) {
        const double t = ((wsum[tid] + wsum[NSUMS + tid]) + wsum[2 * NSUMS + tid]) + wsum[3 * NSUMS + tid];
        a.partials[((size_t)range * gridDim.x + qt) * NSUMS + tid] = t;
    }
}

__global__ __launch_bounds__(64) void calib_fold_kernel(const double* __restrict__ partials, int n, double* __restrict__ sums) {
    const int k = threadIdx.x;
    if (k >= NSUMS) return;
    double t = 0.0;
    for (int i = 0; i < n; ++i) t += partials[(size_t)i * NSUMS + k];
    sums[k] = t;
}

struct Norm {
    const float *tmean, *tr, *emean, *er;
    bool complete() const { return tmean && tr && emean && er; }
};

size_t partials_bytes(const trial_plan::Walk& p) { return (size_t)p.qtiles * p.ranges * NSUMS * sizeof(double); }

template <bool NORM>
int launch_pass(vp_ctx* ctx, const CalibArgs& a, const trial_plan::Walk& p, size_t lds, hipStream_t st) {
    static bool attr_dev[64] = {};              // the attribute is per device (and per instantiation)
    bool& attr_set = attr_dev[ctx->device & 63];
    if (!attr_set) {
        VP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(calib_pass_kernel<NORM>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)(cos_tile::MAX_D * QT * 4 + 4 * NSUMS * 8)));
        attr_set = true;
    }
    hipLaunchKernelGGL((calib_pass_kernel<NORM>), dim3(p.qtiles, p.ranges), dim3(256), lds, st, a);
    VP_LAUNCH_CHECK(ctx, "calib_pass_kernel");
    return VP_OK;
}

// nz = nullptr: on the cosines (vp_trial_calib_sums_f32), else on z (vp_trial_calib_sums_norm_f32)
// ab: (a, b) on the HOST
int sums_pass(vp_ctx* ctx, const char* what, const int* trial_ids, int Nt, const int* enroll_ids, int Ne, int D, const double* ab,
              double* sums, void* partials, size_t partials_size, const Norm* nz, const void* ws, size_t ws_bytes, vp_stream stream) {
    if (!trial_plan::shape_ok(Nt, Ne, D))       // first, and without a context: needs no device
        VP_FAIL(ctx, VP_EUNSUP, "%s: Nt, Ne >= 1, D %% 4 == 0, D <= %d", what, cos_tile::MAX_D);
    if (!ctx || !trial_ids || !enroll_ids || !ab || !sums || !partials || !ws || (nz && !nz->complete()))
        VP_FAIL(ctx, VP_EINVAL, "%s: null pointer", what);
    const double a = ab[0], b = ab[1];
    if (!isfinite(a) || !isfinite(b)) VP_FAIL(ctx, VP_EINVAL, "%s: a = %g, b = %g", what, a, b);
    const trial_plan::Walk p = trial_plan::walk(Nt, Ne, D);
    if (ws_bytes < p.bytes) VP_FAIL(ctx, VP_EINVAL, "%s: workspace %zu < %zu bytes", what, ws_bytes, p.bytes);
    if (partials_size < partials_bytes(p))
        VP_FAIL(ctx, VP_EINVAL, "%s: partials %zu < %zu bytes", what, partials_size, partials_bytes(p));
    hipStream_t st = (hipStream_t)stream;
    CalibArgs k{};
    k.tu = (const float*)ws;
    k.eu = (const float*)((const char*)ws + p.unit_t);
    k.tl = trial_ids;
    k.el = enroll_ids;
    k.Nt = Nt;
    k.Ne = Ne;
    k.D = D;
    k.slabs_per_wg = p.slabs_per_wg;
    k.a = a;
    k.b = b;
    k.partials = (double*)partials;
    if (nz) {
        k.tmean = nz->tmean;
        k.tr = nz->tr;
        k.emean = nz->emean;
        k.er = nz->er;
    }
    const size_t lds = p.tile_lds + 4 * NSUMS * sizeof(double);
    const int rc = nz ? launch_pass<true>(ctx, k, p, lds, st) : launch_pass<false>(ctx, k, p, lds, st);
    if (rc != VP_OK) return rc;
    hipLaunchKernelGGL(calib_fold_kernel, dim3(1), dim3(64), 0, st, (const double*)partials, p.qtiles * p.ranges, sums);
    VP_LAUNCH_CHECK(ctx, "calib_fold_kernel");
    return VP_OK;
}

}  // namespace

extern "C" {

size_t vp_trial_calib_partials_bytes(int Nt, int Ne, int D) {
    return trial_plan::shape_ok(Nt, Ne, D) ? partials_bytes(trial_plan::walk(Nt, Ne, D)) : 0;
}

int vp_trial_calib_sums_f32(vp_ctx* ctx, const int* trial_ids, int Nt, const int* enroll_ids, int Ne, int D, const double* ab,
                            double* sums, void* partials, size_t partials_bytes, const void* ws, size_t ws_bytes, vp_stream stream) {
    return sums_pass(ctx, "trial_calib_sums", trial_ids, Nt, enroll_ids, Ne, D, ab, sums, partials, partials_bytes, nullptr, ws,
                     ws_bytes, stream);
}

int vp_trial_calib_sums_norm_f32(vp_ctx* ctx, const int* trial_ids, int Nt, const int* enroll_ids, int Ne, int D, const double* ab,
                                 double* sums, void* partials, size_t partials_bytes, const float* trial_mean, const float* trial_r,
                                 const float* enroll_mean, const float* enroll_r, const void* ws, size_t ws_bytes, vp_stream stream) {
    const Norm nz{trial_mean, trial_r, enroll_mean, enroll_r};
    return sums_pass(ctx, "trial_calib_sums_norm", trial_ids, Nt, enroll_ids, Ne, D, ab, sums, partials, partials_bytes, &nz, ws,
                     ws_bytes, stream);
}

}  // extern "C"
