// Reverberation of a ragged batch on gfx950: dst[b] = convolve(src[b], rir[b], 'full')[:len(src[b])].
//
// Replaces ReverbPerturbAugmentor.__call__ -> AudioSegment.reverb (call site ppvector/data_utils/reader.py:161-162; yeaudio is
// third party, restated [3P-memory]: the impulse response scaled to unit energy -- done by the host when it decodes the file --
// then a full convolution cut to the utterance's length).  An impulse response is 0.5-3 s = 8 000-48 000 taps, so the direct
// form costs ~1e10 multiply-adds per utterance; this is a uniformly partitioned overlap-save FFT convolution:
//   partition P = 2048 samples, transform N = 2P = 4096 points (complex f32 Stockham radix-4 in LDS, the melspec.hip scheme with
//   one workgroup per transform: two 4096-point buffers = 68 KB of LDS);
//   kernel 1: X[k] = FFT(x[(k-1)P .. (k+1)P)) for every input block (hop P, zeros outside the utterance) and
//             H[p] = FFT(h[pP .. (p+1)P) | P zeros) for every partition of the impulse response -> workspace.  Both signals are
//             real, so only bins 0 .. N/2 are kept;
//   kernel 2: per output block k: S = sum_{p <= k} X[k-p] H[p] in f32 (p ascending: a fixed order), its Hermitian upper half
//             restored, inverse transform (as the forward one of the conjugate; only the real part is needed), samples
//             P .. 2P-1 are y[kP .. (k+1)P), cut at the utterance's length.
// Every workspace element kernel 2 reads was written by kernel 1 of the same call.  dst[b] must not alias src[b].
#include "common.h"

#include <math.h>
#include <vector>

namespace {

constexpr int RV_P = 2048;                   // partition (samples)
constexpr int RV_N = 2 * RV_P;               // transform size
constexpr int RV_THREADS = 256;
constexpr int RV_BINS = RV_N / 2 + 1;        // bins kept of a real signal's spectrum
constexpr int RV_STRIDE = RV_N / 2 + 8;      // float2 per stored spectrum (a multiple of 64 bytes)
constexpr int RV_LDS = RV_N + RV_N / 16;     // one padded transform buffer (float2)
constexpr size_t RV_SMEM = (size_t)2 * RV_LDS * sizeof(float2);

struct ReverbArgs {
    const float* const* src; const float* const* rir; float* const* dst;
    const int* lens; const int* rir_lens;
    const float2* tw;         // [RV_N] e^{-2 pi i k / RV_N}
    float2* ws;               // [B][max_nb + max_np][RV_STRIDE]
    int max_len, max_rir_len, max_nb, max_np;
};

__device__ __forceinline__ int pidx(int i) { return i + (i >> 4); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// Forward RV_N-point transform of `a` (filled, barrier passed) by the whole workgroup: six radix-4 Stockham stages ping-pong
// between a and b; the result is back in `a`, in natural order, after the last barrier.
__device__ __forceinline__ void rv_fft(float2* a, float2* b, const float2* __restrict__ tw, int tid) {
    float2* src = a;
    float2* dst = b;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const int Ns = 1 << (2 * s);
        const int twstep = RV_N >> (2 * s + 2);                       // N / (4 Ns)
#pragma unroll
        for (int u = 0; u < RV_N / 4 / RV_THREADS; ++u) {
            const int j = tid + RV_THREADS * u;
            const int jm = j & (Ns - 1);
            float2 v0 = src[pidx(j)];
            float2 v1 = cmul(src[pidx(j + RV_N / 4)], tw[(jm * twstep) & (RV_N - 1)]);
            float2 v2 = cmul(src[pidx(j + RV_N / 2)], tw[(2 * jm * twstep) & (RV_N - 1)]);
            float2 v3 = cmul(src[pidx(j + 3 * RV_N / 4)], tw[(3 * jm * twstep) & (RV_N - 1)]);
            const float2 s02 = make_float2(v0.x + v2.x, v0.y + v2.y), d02 = make_float2(v0.x - v2.x, v0.y - v2.y);
            const float2 s13 = make_float2(v1.x + v3.x, v1.y + v3.y), d13 = make_float2(v1.x - v3.x, v1.y - v3.y);
            const int idx = ((j >> (2 * s)) << (2 * s + 2)) + jm;
            dst[pidx(idx)] = make_float2(s02.x + s13.x, s02.y + s13.y);
            dst[pidx(idx + Ns)] = make_float2(d02.x + d13.y, d02.y - d13.x);
            dst[pidx(idx + 2 * Ns)] = make_float2(s02.x - s13.x, s02.y - s13.y);
            dst[pidx(idx + 3 * Ns)] = make_float2(d02.x - d13.y, d02.y + d13.x);
        }
        __syncthreads();
        float2* tmp = src; src = dst; dst = tmp;
    }
}

// lengths of utterance b as both kernels see them: never past what the workspace was sized for
__device__ __forceinline__ bool rv_shape(const ReverbArgs& a, int b, int& n, int& Lr, int& nb, int& np) {
    n = min(a.lens[b], a.max_len);
    Lr = min(a.rir_lens[b], a.max_rir_len);
    if (n <= 0 || Lr <= 0) return false;
    nb = (n + RV_P - 1) / RV_P;
    np = (Lr + RV_P - 1) / RV_P;
    return true;
}

// grid (max_nb + max_np, B): x < max_nb transforms input block x of the utterance, the rest partition x - max_nb of its impulse response
__global__ __launch_bounds__(RV_THREADS) void reverb_spectra_kernel(ReverbArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* d0 = reinterpret_cast<float2*>(smem);
    float2* d1 = d0 + RV_LDS;
    const int tid = threadIdx.x, b = blockIdx.y;
    int n, Lr, nb, np;
    if (!rv_shape(a, b, n, Lr, nb, np)) return;                      // uniform per workgroup, as every return below
    int k = blockIdx.x;
    const float* s;
    int base, len, take;
    if (k < a.max_nb) {
        if (k >= nb) return;
        s = a.src[b]; base = (k - 1) * RV_P; len = n; take = RV_N;
    } else {
        const int p = k - a.max_nb;
        if (p >= np) return;
        s = a.rir[b]; base = p * RV_P; len = Lr; take = RV_P;
        k = a.max_nb + p;
    }
    float2* out = a.ws + ((size_t)b * (a.max_nb + a.max_np) + k) * RV_STRIDE;
    for (int i = tid; i < RV_N; i += RV_THREADS) {
        const int g = base + i;
        d0[pidx(i)] = make_float2(i < take && g >= 0 && g < len ? s[g] : 0.f, 0.f);
    }
    __syncthreads();
    rv_fft(d0, d1, a.tw, tid);
    for (int f = tid; f < RV_BINS; f += RV_THREADS) out[f] = d0[pidx(f)];
}

// grid (max_nb, B): output block x of the utterance
__global__ __launch_bounds__(RV_THREADS) void reverb_block_kernel(ReverbArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* d0 = reinterpret_cast<float2*>(smem);
    float2* d1 = d0 + RV_LDS;
    const int tid = threadIdx.x, b = blockIdx.y, k = blockIdx.x;
    int n, Lr, nb, np;
    if (!rv_shape(a, b, n, Lr, nb, np) || k >= nb) return;           // uniform per workgroup
    const float2* X = a.ws + (size_t)b * (a.max_nb + a.max_np) * RV_STRIDE;
    const float2* H = X + (size_t)a.max_nb * RV_STRIDE;
    const int cnt = k + 1 < np ? k + 1 : np;
    constexpr int PER = RV_N / 2 / RV_THREADS;                        // bins 0 .. N/2 - 1 over the lanes; bin N/2 on thread 0
    float2 acc[PER], accn = make_float2(0.f, 0.f);
#pragma unroll
    for (int u = 0; u < PER; ++u) acc[u] = make_float2(0.f, 0.f);
    for (int p = 0; p < cnt; ++p) {
        const float2* xs = X + (size_t)(k - p) * RV_STRIDE;
        const float2* hs = H + (size_t)p * RV_STRIDE;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int f = tid + RV_THREADS * u;
            const float2 t = cmul(xs[f], hs[f]);
            acc[u].x += t.x; acc[u].y += t.y;
        }
        if (tid == 0) {
            const float2 t = cmul(xs[RV_N / 2], hs[RV_N / 2]);
            accn.x += t.x; accn.y += t.y;
        }
    }
    // inverse transform = conjugate of the forward transform of the conjugate; the upper half is the mirror of the lower one
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int f = tid + RV_THREADS * u;
        d0[pidx(f)] = make_float2(acc[u].x, -acc[u].y);
        if (f > 0) d0[pidx(RV_N - f)] = acc[u];
    }
    if (tid == 0) d0[pidx(RV_N / 2)] = make_float2(accn.x, -accn.y);
    __syncthreads();
    rv_fft(d0, d1, a.tw, tid);
    float* o = a.dst[b];
    for (int i = tid; i < RV_P; i += RV_THREADS) {
        const int g = k * RV_P + i;
        if (g < n) o[g] = d0[pidx(RV_P + i)].x * (1.f / RV_N);
    }
}

int rv_tables(vp_ctx* ctx) {
    if (ctx->rv_twiddle) return VP_OK;
    std::vector<float2> tw(RV_N);
    for (int k = 0; k < RV_N; ++k) tw[k] = make_float2((float)cos(-2.0 * M_PI * k / RV_N), (float)sin(-2.0 * M_PI * k / RV_N));
    float2* d = nullptr;
    VP_HIP(ctx, hipMalloc(&d, RV_N * sizeof(float2)));
    hipError_t e = hipMemcpy(d, tw.data(), RV_N * sizeof(float2), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        VP_FAIL(ctx, VP_EHIP, "reverb: twiddle upload: %s", hipGetErrorString(e));
    }
    ctx->rv_twiddle = d;
    return VP_OK;
}

}  // namespace

int vp_reverb_release_tables(vp_ctx* ctx) {
    if (!ctx) return VP_OK;
    if (ctx->rv_twiddle) (void)hipFree(ctx->rv_twiddle);
    ctx->rv_twiddle = nullptr;
    return VP_OK;
}

extern "C" {

size_t vp_reverb_workspace_bytes(int B, int max_len, int max_rir_len) {
    if (B <= 0 || max_len <= 0 || max_rir_len <= 0 || max_len > (1 << 30) || max_rir_len > (1 << 30)) return 0;
    const size_t blocks = (size_t)(max_len + RV_P - 1) / RV_P + (size_t)(max_rir_len + RV_P - 1) / RV_P;
    return (size_t)B * blocks * RV_STRIDE * sizeof(float2);
}

int vp_reverb_f32(vp_ctx* ctx, const float* const* srcs, const int32_t* lens, const float* const* rirs, const int32_t* rir_lens,
                  float* const* dsts, int B, int max_len, int max_rir_len, void* ws, size_t ws_bytes, vp_stream stream) {
    if (!ctx || !srcs || !lens || !rirs || !rir_lens || !dsts || B <= 0 || B > 65535 || max_len <= 0 || max_rir_len <= 0 ||
        max_len > (1 << 30) || max_rir_len > (1 << 30))
        VP_FAIL(ctx, VP_EINVAL, "reverb: bad arguments");
    if (!ws || ws_bytes < vp_reverb_workspace_bytes(B, max_len, max_rir_len)) VP_FAIL(ctx, VP_EINVAL, "reverb: workspace too small");
    int rc = rv_tables(ctx);
    if (rc) return rc;
    static bool attr_dev[64] = {};                    // the attribute is per DEVICE (a process may drive several GPUs)
    bool& attr_set = attr_dev[ctx->device & 63];
    if (!attr_set) {
        VP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(reverb_spectra_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)RV_SMEM));
        VP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(reverb_block_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)RV_SMEM));
        attr_set = true;
    }
    ReverbArgs a;
    a.src = srcs; a.rir = rirs; a.dst = dsts; a.lens = lens; a.rir_lens = rir_lens; a.tw = ctx->rv_twiddle; a.ws = (float2*)ws;
    a.max_len = max_len; a.max_rir_len = max_rir_len;
    a.max_nb = (max_len + RV_P - 1) / RV_P; a.max_np = (max_rir_len + RV_P - 1) / RV_P;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(reverb_spectra_kernel, dim3(a.max_nb + a.max_np, B), dim3(RV_THREADS), RV_SMEM, st, a);
    VP_LAUNCH_CHECK(ctx, "reverb_spectra");
    hipLaunchKernelGGL(reverb_block_kernel, dim3(a.max_nb, B), dim3(RV_THREADS), RV_SMEM, st, a);
    VP_LAUNCH_CHECK(ctx, "reverb_block");
    return VP_OK;
}

}  // extern "C"
