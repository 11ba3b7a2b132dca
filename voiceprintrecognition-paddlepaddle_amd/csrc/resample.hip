// Sample-rate conversion of a ragged batch on the GPU: the polyphase FIR of scipy.signal.resample_poly(x, up, down) with its defaults
// (window ('kaiser', 5.0), padtype 'constant') -- what AudioSegment.resample (ppvector/predict.py) computes on the host for every file
// that is not at the dataset's rate (data_utils/reader.py _decode, PPVectorPredictor._load_audio).  docs/resample.md has the method.
//
// With half = 10 max(up, down), the filter h (2 half + 1 taps, designed on the host in float64, scaled by up) and the phase-major
// table P[p][j] = h[p + j up] zero-padded to J = ceil((2 half + 1) / up) taps per phase, output m of an utterance of n samples is
//     c = m down + half,  p = c mod up,  q = c div up,      y[m] = sum_{j < J} P[p][j] x[q - j],      x = 0 outside [0, n)
// one f32 fma chain over j = 0 .. J - 1 whatever the tile, the batch or the grid, so a row's bits do not depend on its neighbours.
//
// resample_kernel: grid (tile slots, utterances), 256 threads; a workgroup walks tiles of `tile` outputs of its utterance.
//   * the input span of a tile -- x[q(first) - (J - 1) .. q(last)], at most (tile - 1) down / up + 1 + J samples -- is staged in LDS
//     once, zeros where the index is outside [0, n): every sample is read from memory once per tile although J outputs' sums use it,
//     and nothing outside the row is ever read.
//   * up > 1: neighbouring outputs sit on different phases, so a wave reads 64 different table rows at once.  From memory that is
//     64 cache lines per load instruction; the table (up rows of J floats, at most 84 KB, 36 KB at 44.1 kHz -> 16 kHz) is therefore
//     copied to LDS once per workgroup, its rows padded to an odd stride so that the rows of a wave start on different banks.
//   * up == 1 (integer decimation): every output uses the one row, the address is the same in all lanes and the loads are scalar --
//     the table stays where it is and LDS holds the span alone (at 1:1024 a span and a table of 80 KB each would not both fit).
//   * the tile is 1024 outputs unless table + span would pass the 160 KB of a CU; then it is the largest that fits
//     (vp_resample_tile).  At 48 kHz -> 16 kHz a workgroup holds 12.5 KB, at 44.1 kHz -> 16 kHz 48 KB: 8 and 3 workgroups per CU.
//   * m down passes 2^31 after five minutes at 44.1 kHz: c and q0 are 64-bit, once per tile; inside a tile the offsets fit 32 bits.
#include "common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_TILE = 1024;
constexpr int RS_MAX_RATE = 1024;           // of max(up, down)
constexpr int RS_LDS_FLOATS = 40960;        // 160 KB
constexpr int RS_MAX_B = 65535;             // grid.y

struct ResamplePlan { int J, half, row, table_floats, tile, span_floats; };

// false when the pair is out of range
bool resample_plan(int up, int down, ResamplePlan& p) {
    if (up <= 0 || down <= 0 || up > RS_MAX_RATE || down > RS_MAX_RATE) return false;
    p.half = 10 * (up > down ? up : down);
    p.J = (2 * p.half + 1 + up - 1) / up;
    p.row = p.J | 1;
    p.table_floats = up == 1 ? 0 : up * p.row;
    const long long budget = RS_LDS_FLOATS - p.table_floats - 1 - p.J;      // > 0 for every pair in range (docs/resample.md)
    long long tile = RS_TILE;
    if ((tile - 1) * down / up > budget) tile = 1 + budget * up / down;     // then (tile - 1) down / up <= budget
    p.tile = (int)tile;
    p.span_floats = (int)((tile - 1) * down / up) + 1 + p.J;
    return true;
}

struct ResampleArgs {
    const float* const* src; const int* lens; const int* new_lens; float* const* dst; const float* table;
    int up, down, J, half, row, tile;
};

template <bool UP1>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = a.lens[b], M = a.new_lens[b];
    if (n <= 0 || M <= 0) return;                               // uniform per workgroup
    const float* __restrict__ x = a.src[b];
    float* __restrict__ o = a.dst[b];
    const float* __restrict__ table = a.table;
    float* tab = sm;
    float* xs = sm + (UP1 ? 0 : a.up * a.row);
    if (!UP1) {
        for (int p = tid / 64; p < a.up; p += RS_THREADS / 64)                          // a wave per row
            for (int j = tid & 63; j < a.J; j += 64) tab[p * a.row + j] = table[(size_t)p * a.J + j];
    }
    for (long long m0 = (long long)blockIdx.x * a.tile; m0 < M; m0 += (long long)gridDim.x * a.tile) {
        const int nt = M - m0 < a.tile ? (int)(M - m0) : a.tile;
        const long long c0 = m0 * a.down + a.half;
        const long long q0 = c0 / a.up;
        const int p0 = (int)(c0 - q0 * a.up);
        const long long lo = q0 - (a.J - 1);                                            // first input index of the span, may be < 0
        const int span = (p0 + (nt - 1) * a.down) / a.up + a.J;                         // q(last) - lo + 1 <= span_floats of the plan
        __syncthreads();                                                                // the tile before is done with xs
        for (int i = tid; i < span; i += RS_THREADS) {
            const long long g = lo + i;
            xs[i] = g >= 0 && g < n ? x[g] : 0.f;
        }
        __syncthreads();                                                                // and, the first time, the table
        for (int r = tid; r < nt; r += RS_THREADS) {
            const int t = p0 + r * a.down;                                              // < 1024 + 1023 * 1024
            const int dq = t / a.up, p = t - dq * a.up;
            const float* xp = xs + (a.J - 1) + dq;                                      // xp[-j] = x[q - j]
            const float* cp = UP1 ? table : tab + p * a.row;
            float acc = 0.f;
#pragma unroll 4
            for (int j = 0; j < a.J; ++j) acc = fmaf(cp[j], xp[-j], acc);
            o[m0 + r] = acc;
        }
    }
}

}  // namespace

extern "C" {

int vp_resample_tile(int up, int down) {
    ResamplePlan p;
    return resample_plan(up, down, p) ? p.tile : 0;
}

int vp_resample_poly_f32(vp_ctx* ctx, const float* const* srcs, const int32_t* lens, const int32_t* new_lens, float* const* dsts, int B,
                         int max_new_len, int up, int down, const float* phase_table, int taps_per_phase, vp_stream stream) {
    if (!ctx || !srcs || !lens || !new_lens || !dsts || !phase_table) VP_FAIL(ctx, VP_EINVAL, "resample_poly: null pointer");
    ResamplePlan p;
    if (B <= 0 || B > RS_MAX_B || max_new_len <= 0 || !resample_plan(up, down, p))
        VP_FAIL(ctx, VP_EINVAL, "resample_poly: 1 <= B <= %d, max_new_len >= 1, 1 <= up, down <= %d", RS_MAX_B, RS_MAX_RATE);
    if (taps_per_phase != p.J)
        VP_FAIL(ctx, VP_EINVAL, "resample_poly: taps_per_phase %d, ceil((20 max(up, down) + 1) / up) = %d", taps_per_phase, p.J);
    const int lds_bytes = (p.table_floats + p.span_floats) * (int)sizeof(float);
    static bool attr_dev[64] = {};                    // the attribute is per DEVICE (a process may drive several GPUs)
    bool& attr_set = attr_dev[ctx->device & 63];
    if (!attr_set) {
        VP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(resample_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        RS_LDS_FLOATS * (int)sizeof(float)));
        VP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(resample_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        RS_LDS_FLOATS * (int)sizeof(float)));
        attr_set = true;
    }
    ResampleArgs a{srcs, lens, new_lens, dsts, phase_table, up, down, p.J, p.half, p.row, p.tile};
    // tile slots: every tile of the longest row, or as many as keep about 2048 workgroups in the launch -- a workgroup that walks
    // several tiles copies the table once
    const int tiles = (int)(((long long)max_new_len + p.tile - 1) / p.tile);
    const int slots = 2048 / B > 1 ? 2048 / B : 1;
    const dim3 grid(tiles < slots ? tiles : slots, B);
    if (up == 1) hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(RS_THREADS), lds_bytes, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(RS_THREADS), lds_bytes, (hipStream_t)stream, a);
    VP_LAUNCH_CHECK(ctx, "resample_kernel");
    return VP_OK;
}

}  // extern "C"
