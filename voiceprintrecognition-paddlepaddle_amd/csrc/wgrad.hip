// The conv weight gradient, whole: dW[n][j*Cin + c] = sum_{b,t} dz[b, t, n] * x[b, src(t, j), c], src = the forward's tap index
// (reflect / zero / none) -- Conv1D / Conv2D backward of models/utils.py:65-93 under PPVectorTrainer.__train_epoch (trainer.py:202-274).
// Rows are cut into S splits; a kernel of one of five families (VP_WGRAD_* of vpmi.h) writes the partials [S][Cout][K] and a fixed-order
// reducer sums them into dW (no atomics: bit-reproducible).  Host: wgrad_validate -> wgrad_plan (the ONLY place that picks the family
// and S) -> wgrad_launch; vp_conv1d_wgrad_workspace_bytes from the same split helpers.  docs/wgrad.md has the rules in order.
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------- 64 x 64 tiles, exact f32
// One workgroup = a 64 (n) x 64 (k-column) tile of dW over a slice of the rows; 4 waves of 32 x 32; v_mfma_f32_16x16x4_f32
// with dz^T as the A operand and the shifted x rows as B -- both operands are read row-wise (16 lanes = 64 contiguous
// bytes), the reduction dimension (rows) is the MFMA k.
struct WgradArgs {
    const float* x; const float* dz; float* part;
    int ldx, xoff, lddz, M, N, K, Cin, T_in, T_out, dilation, stride, pad_left, pad_mode, rows_per_split;
    int F_in, F_out, KF, stride_f, pad_f;        // 2-D convs (zero padding): rows are (b, t, f), taps (kt, kf); F_in = F_out = KF = 1 for 1-D
    // batched launch (amp kernel): blockIdx.z = conv * splits + split; conv c reads x + c * xb, dz + c * dzb (elements of their dtype)
    int splits; long long xb, dzb;
};

// The tap-to-source-row rule.  Output row m is position (b, t, f); under the tap of a k-column (tapoff = kt * dilation - pad_left,
// tapf = kf - pad_f) it reads input row (b, ts, fs): nothing when that lies in the zero padding, else load(src), src = the element
// offset of the row's channel 0 from x (reflect padding mirrors the frame index; the f axis is zero-padded only).  Row decoded apart
// from the tap, load handed in: in this form the 64 x 64 and 64 x 256 kernels keep the instructions they had (docs/wgrad.md).
struct WgradRow { int b, t, f; };
__device__ __forceinline__ WgradRow wgrad_row(const WgradArgs& a, int m) {
    const int bt = m / a.F_out, f = m - bt * a.F_out;
    const int b = bt / a.T_out, t = bt - b * a.T_out;
    return {b, t, f};
}
template <typename F>
__device__ __forceinline__ void wgrad_tap_src(const WgradArgs& a, const WgradRow& row, int tapoff, int tapf, F&& load) {
    const int traw = row.t * a.stride + tapoff, fs = row.f * a.stride_f + tapf;
    int ts = traw;
    bool ok = fs >= 0 && fs < a.F_in;
    if (a.pad_mode == VP_PAD_REFLECT) {
        ts = ts < 0 ? -ts : ts;
        ts = ts >= a.T_in ? 2 * (a.T_in - 1) - ts : ts;
    } else {
        ok = ok && traw >= 0 && traw < a.T_in;
    }
    if (ok) load((((size_t)row.b * a.T_in + ts) * a.F_in + fs) * a.ldx + a.xoff);
}

// LDS-tiled: per 32-row chunk the workgroup stages dz[32][64 n] and the tap-shifted x[32][64 k-columns] with 16-byte loads
// (16 lanes per row, prefetched one chunk ahead in registers), then every wave reads its MFMA operands from LDS
// (row stride 80 floats: the four k-rows of a fragment land on disjoint banks).  The first version fetched every
// fragment straight from global memory, 4 bytes per lane: 53 TFLOP/s on the 1536 x 1536 layer.
constexpr int WG_RC = 32;              // rows per staged chunk
constexpr int WG_LD = 80;              // floats per staged row (64 + 16 pad)

__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradArgs a) {
    __shared__ __attribute__((aligned(16))) float dzs[WG_RC * WG_LD];
    __shared__ __attribute__((aligned(16))) float xs[WG_RC * WG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int i = lane & 15, kk = lane >> 4;
    const int wn = wv & 1, wk = wv >> 1;
    const int nb = blockIdx.y * 64, kb = blockIdx.x * 64;
    const int m_begin = blockIdx.z * a.rows_per_split;
    const int m_end = min(a.M, m_begin + a.rows_per_split);
    // staging role: rows srow and srow + 16 of the chunk, 4 consecutive columns starting at scol
    const int srow = tid >> 4, scol = (tid & 15) * 4;
    const int ncol = nb + scol;                       // dz column (4 consecutive n; N % 4 == 0 -> all or none valid)
    const bool nvalid = ncol < a.N;
    const int kcol = kb + scol;                       // k-column = tap * Cin + c (Cin % 4 == 0: the 4 stay inside one tap)
    const bool kvalid = kcol < a.K;
    const int j = kvalid ? kcol / a.Cin : 0;
    const int cc = kvalid ? kcol - j * a.Cin : 0;
    const int kt = j / a.KF;
    const int tapoff = kt * a.dilation - a.pad_left, tapf = (j - kt * a.KF) - a.pad_f;
    const bool vec_ok = (a.Cin & 3) == 0 && ((a.ldx | a.xoff) & 3) == 0 && (a.lddz & 3) == 0;

    float4 rdz[2], rx[2];
    auto gload = [&](int mbase) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int m = mbase + srow + 16 * h;
            rdz[h] = make_float4(0.f, 0.f, 0.f, 0.f);
            rx[h] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m >= m_end) continue;
            if (nvalid) rdz[h] = *reinterpret_cast<const float4*>(a.dz + (size_t)m * a.lddz + ncol);
            if (kvalid) wgrad_tap_src(a, wgrad_row(a, m), tapoff, tapf, [&](size_t src) { rx[h] = *reinterpret_cast<const float4*>(a.x + (src + cc)); });
        }
    };
    auto swrite = [&]() {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<float4*>(dzs + (srow + 16 * h) * WG_LD + scol) = rdz[h];
            *reinterpret_cast<float4*>(xs + (srow + 16 * h) * WG_LD + scol) = rx[h];
        }
    };
    f32x4 acc[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[p][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!vec_ok) return;                              // host refuses these shapes (kept so the kernel cannot misread)
    gload(m_begin);
    for (int mb = m_begin; mb < m_end; mb += WG_RC) {
        swrite();
        __syncthreads();
        gload(mb + WG_RC);                            // rows past m_end come back as zeros
#pragma unroll
        for (int r = 0; r < WG_RC; r += 4) {
            float av[2], bv[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                av[q] = dzs[(r + kk) * WG_LD + wn * 32 + q * 16 + i];
                bv[q] = xs[(r + kk) * WG_LD + wk * 32 + q * 16 + i];
            }
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int q = 0; q < 2; ++q) acc[p][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[p], bv[q], acc[p][q], 0, 0, 0);
        }
        __syncthreads();
    }
    const int n0 = nb + wn * 32, k0 = kb + wk * 32;
    float* out = a.part + (size_t)blockIdx.z * a.N * a.K;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int col = k0 + q * 16 + i;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + p * 16 + kk * 4 + r;
                if (n < a.N && col < a.K) out[(size_t)n * a.K + col] = acc[p][q][r];
            }
        }
}

// ---------------------------------------------------------------------------------------------- 128 x 128 tiles, bf16 matrix cores
// Mixed precision (vp_conv1d_desc.mfma_bf16): the same contraction on the bf16 matrix cores.  One workgroup = a 128 (n) x 128
// (k-column) tile of dW over a slice of the rows, 4 waves of 64 x 64 (v_mfma_f32_16x16x32_bf16, f32 accumulate).  The reduction
// index is the ROW, along which both operands are strided in memory: a thread loads 8 rows x 4 consecutive columns (16-byte
// loads, a half-wave = 512 contiguous bytes of a row), rounds to bf16 and writes the four 8-row column pieces TRANSPOSED into
// LDS ([column][64 rows], 128 B per column), where a fragment is one ds_read_b128.  The 16-byte chunk q of column R sits at
// position q ^ L(R), L(R) = ((R >> 1) & 7) ^ ((R >> 4) & 1): conflict-free for the transposed writes (8 lanes = columns 4
// apart) AND for the fragment reads (searched exhaustively over XOR-linear maps against the ds_read_b128 lane groups).
constexpr int WA_T = 128;              // tile edge of dW
constexpr int WA_RC = 64;              // rows per staged chunk = two MFMA k-steps
__device__ __forceinline__ int wa_L(int R) { return ((R >> 1) & 7) ^ ((R >> 4) & 1); }

// BF: x and dz are already bf16 in memory (the wide layers' operands, see ConvBlock): 8-byte loads of four bf16, no rounding here.
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

// X3 (f32 operands only): split precision -- each operand is staged as TWO transposed bf16 planes (hi = bf16(v), lo = bf16(v - hi)) and
// the contraction is lo*hi + hi*lo + hi*hi (conv_gemm_impl.h: x3_t): the weight gradient of the 'float32x3' training mode, ~2^-17 per
// product.  Twice the LDS (128 KB: one workgroup per CU) and three MFMAs per fragment pair.
template <bool BF, bool X3 = false>
__global__ __launch_bounds__(256, X3 ? 1 : 2) void conv_wgrad_amp_kernel(WgradArgs a) {
    static_assert(!(BF && X3), "split precision takes f32 operands");
    constexpr int PLANES = X3 ? 2 : 1;
    constexpr int STG = PLANES * 2 * WA_T * 128;                       // bytes per stage
    extern __shared__ __attribute__((aligned(16))) char wsm[];        // [2 stages][dz^T 16 KB | x^T 16 KB] (x3: + the two lo planes)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int wn = wv & 1, wk = wv >> 1;
    const int nb = blockIdx.y * WA_T, kb = blockIdx.x * WA_T;
    const int zb = blockIdx.z / a.splits, sp = blockIdx.z - zb * a.splits;
    const int m_begin = sp * a.rows_per_split;
    const int m_end = min(a.M, m_begin + a.rows_per_split);
    // staging role: rows 8 rg .. 8 rg + 7 of the chunk, columns 4 cg .. 4 cg + 3 of the tile
    const int cg = tid & 31, rg = tid >> 5;
    const int ncol = nb + 4 * cg;
    const bool nvalid = ncol < a.N;
    const int kcol = kb + 4 * cg;                     // k-column = tap * Cin + c (Cin % 4 == 0: the 4 stay inside one tap)
    const bool kvalid = kcol < a.K;
    const int j = kvalid ? kcol / a.Cin : 0;
    const int cc = kvalid ? kcol - j * a.Cin : 0;
    const int kt = j / a.KF;
    const int tapoff = kt * a.dilation - a.pad_left, tapf = (j - kt * a.KF) - a.pad_f;
    // 1x1 convs with identical input / output geometry (the wide layers): source row = output row
    const bool simple = a.K == a.Cin && a.stride == 1 && a.pad_left == 0 && a.T_in == a.T_out && a.F_in == 1 && a.F_out == 1;

    using ld_t = typename std::conditional<BF, uint2, float4>::type;
    using el_t = typename std::conditional<BF, bf16_t, float>::type;
    const el_t* __restrict__ gdz = reinterpret_cast<const el_t*>(a.dz) + zb * a.dzb;
    const el_t* __restrict__ gx = reinterpret_cast<const el_t*>(a.x) + zb * a.xb;
    ld_t rdz[8], rx[8];
    auto gload = [&](int mbase) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int m = mbase + 8 * rg + r;
            rdz[r] = ld_t{};
            rx[r] = ld_t{};
            if (m >= m_end) continue;
            if (nvalid) rdz[r] = *reinterpret_cast<const ld_t*>(gdz + (size_t)m * a.lddz + ncol);
            if (!kvalid) continue;
            if (simple) {
                rx[r] = *reinterpret_cast<const ld_t*>(gx + (size_t)m * a.ldx + a.xoff + cc);
            } else {
                // wgrad_row + wgrad_tap_src written out: through the helper this kernel's code moves, so its body stays (docs/wgrad.md)
                const int bt = m / a.F_out, f = m - bt * a.F_out;
                const int b = bt / a.T_out, t = bt - b * a.T_out;
                const int traw = t * a.stride + tapoff, fs = f * a.stride_f + tapf;
                int ts = traw;
                bool ok = fs >= 0 && fs < a.F_in;
                if (a.pad_mode == VP_PAD_REFLECT) {
                    ts = ts < 0 ? -ts : ts;
                    ts = ts >= a.T_in ? 2 * (a.T_in - 1) - ts : ts;
                } else {
                    ok = ok && traw >= 0 && traw < a.T_in;
                }
                if (ok) rx[r] = *reinterpret_cast<const ld_t*>(gx + (((size_t)b * a.T_in + ts) * a.F_in + fs) * a.ldx + a.xoff + cc);
            }
        }
    };
    auto swrite = [&](int s) {
        char* dzs = wsm + s * STG;
        char* xs = dzs + WA_T * 128;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int R = 4 * cg + e;
            const int pos = (rg ^ wa_L(R)) << 4;
            if constexpr (BF) {
                u16x8 vd, vx;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const unsigned wd = e < 2 ? rdz[r].x : rdz[r].y, wx = e < 2 ? rx[r].x : rx[r].y;
                    vd[r] = (unsigned short)((e & 1) ? (wd >> 16) : (wd & 0xffffu));
                    vx[r] = (unsigned short)((e & 1) ? (wx >> 16) : (wx & 0xffffu));
                }
                *reinterpret_cast<u16x8*>(dzs + R * 128 + pos) = vd;
                *reinterpret_cast<u16x8*>(xs + R * 128 + pos) = vx;
            } else {
                bf16x8 vd, vx;
                [[maybe_unused]] bf16x8 ld, lx;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const float d = e == 0 ? rdz[r].x : (e == 1 ? rdz[r].y : (e == 2 ? rdz[r].z : rdz[r].w));
                    const float xv = e == 0 ? rx[r].x : (e == 1 ? rx[r].y : (e == 2 ? rx[r].z : rx[r].w));
                    vd[r] = (bf16_t)d;
                    vx[r] = (bf16_t)xv;
                    if constexpr (X3) {
                        ld[r] = (bf16_t)(d - (float)vd[r]);
                        lx[r] = (bf16_t)(xv - (float)vx[r]);
                    }
                }
                *reinterpret_cast<bf16x8*>(dzs + R * 128 + pos) = vd;
                *reinterpret_cast<bf16x8*>(xs + R * 128 + pos) = vx;
                if constexpr (X3) {
                    *reinterpret_cast<bf16x8*>(dzs + 2 * WA_T * 128 + R * 128 + pos) = ld;
                    *reinterpret_cast<bf16x8*>(xs + 2 * WA_T * 128 + R * 128 + pos) = lx;
                }
            }
        }
    };
    f32x4 acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    gload(m_begin);
    int s = 0;
    for (int mb = m_begin; mb < m_end; mb += WA_RC) {
        swrite(s);
        __syncthreads();
        gload(mb + WA_RC);                            // rows past m_end come back as zeros
        const char* dzs = wsm + s * STG;
        const char* xs = dzs + WA_T * 128;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 af[4], bf[4];
            [[maybe_unused]] bf16x8 al[4], bl[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int R = wn * 64 + p * 16 + i;
                af[p] = *reinterpret_cast<const bf16x8*>(dzs + R * 128 + (((ks * 4 + g) ^ wa_L(R)) << 4));
                if constexpr (X3) al[p] = *reinterpret_cast<const bf16x8*>(dzs + 2 * WA_T * 128 + R * 128 + (((ks * 4 + g) ^ wa_L(R)) << 4));
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int R = wk * 64 + q * 16 + i;
                bf[q] = *reinterpret_cast<const bf16x8*>(xs + R * 128 + (((ks * 4 + g) ^ wa_L(R)) << 4));
                if constexpr (X3) bl[q] = *reinterpret_cast<const bf16x8*>(xs + 2 * WA_T * 128 + R * 128 + (((ks * 4 + g) ^ wa_L(R)) << 4));
            }
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if constexpr (X3) {
                        acc[p][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[p], bf[q], acc[p][q], 0, 0, 0);
                        acc[p][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[p], bl[q], acc[p][q], 0, 0, 0);
                    }
                    acc[p][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[p], bf[q], acc[p][q], 0, 0, 0);
                }
        }
        s ^= 1;
    }
    const int n0 = nb + wn * 64, k0 = kb + wk * 64;
    float* out = a.part + (size_t)blockIdx.z * a.N * a.K;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = k0 + q * 16 + i;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + p * 16 + g * 4 + r;
                if (n < a.N && col < a.K) out[(size_t)n * a.K + col] = acc[p][q][r];
            }
        }
}

// ---------------------------------------------------------------------------------------------- 64 x 256 tiles, narrow layers
// The same contraction for a NARROW layer: N <= 64 outputs (the Res2Net chunk convs: 64 x 192).  The square 128 x 128 tile above spends
// up to 3/4 of its MFMAs and LDS traffic on output rows that do not exist there; here a workgroup takes all N <= 64 outputs x 256
// k-columns (blockIdx.x), the four waves 64 each.  LDS: 2 stages x (dz^T 64 x 128 B | x^T 256 x 128 B).  bf16 operands in memory, 1-D
// stride-1 layers only (an f32-operand flavour was slower than the square tile -- ResNetSE step 22.7 -> 23.8 ms -- and is not built).
__global__ __launch_bounds__(256, 2) void conv_wgrad_n64_kernel(WgradArgs a) {
    extern __shared__ __attribute__((aligned(16))) char wsm[];
    constexpr int STAGE = (64 + 256) * 128;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int kb = blockIdx.x * 256;
    const int zb = blockIdx.z / a.splits, sp = blockIdx.z - zb * a.splits;
    const int m_begin = sp * a.rows_per_split;
    const int m_end = min(a.M, m_begin + a.rows_per_split);
    const int cg = tid & 31, rg = tid >> 5;
    const bool nvalid = cg < 16 && 4 * cg < a.N;
    int cc[2], tapoff[2], tapf[2];
    bool kvalid[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int kcol = kb + 128 * u + 4 * cg;
        kvalid[u] = kcol < a.K;
        const int j = kvalid[u] ? kcol / a.Cin : 0;
        cc[u] = kvalid[u] ? kcol - j * a.Cin : 0;
        const int kt = j / a.KF;
        tapoff[u] = kt * a.dilation - a.pad_left;
        tapf[u] = (j - kt * a.KF) - a.pad_f;
    }
    uint2 rdz[8], rx[2][8];
    auto gload = [&](int mbase) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int m = mbase + 8 * rg + r;
            rdz[r] = uint2{0u, 0u}; rx[0][r] = uint2{0u, 0u}; rx[1][r] = uint2{0u, 0u};
            if (m >= m_end) continue;
            if (nvalid) rdz[r] = *reinterpret_cast<const uint2*>(reinterpret_cast<const bf16_t*>(a.dz) + zb * a.dzb + (size_t)m * a.lddz + 4 * cg);
            const WgradRow row = wgrad_row(a, m);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (!kvalid[u]) continue;
                wgrad_tap_src(a, row, tapoff[u], tapf[u], [&](size_t src) {
                    rx[u][r] = *reinterpret_cast<const uint2*>(reinterpret_cast<const bf16_t*>(a.x) + zb * a.xb + (src + cc[u]));
                });
            }
        }
    };
    auto put = [&](char* base, int R, int e, const uint2 (&v)[8]) {
        u16x8 o;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const unsigned w = e < 2 ? v[r].x : v[r].y;
            o[r] = (unsigned short)((e & 1) ? (w >> 16) : (w & 0xffffu));
        }
        *reinterpret_cast<u16x8*>(base + R * 128 + ((rg ^ wa_L(R)) << 4)) = o;
    };
    auto swrite = [&](int s) {
        char* dzs = wsm + s * STAGE;
        char* xs = dzs + 64 * 128;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (cg < 16) put(dzs, 4 * cg + e, e, rdz);
            put(xs, 4 * cg + e, e, rx[0]);
            put(xs, 128 + 4 * cg + e, e, rx[1]);
        }
    };
    f32x4 acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    gload(m_begin);
    int s = 0;
    for (int mb = m_begin; mb < m_end; mb += WA_RC) {
        swrite(s);
        __syncthreads();
        gload(mb + WA_RC);
        const char* dzs = wsm + s * STAGE;
        const char* xs = dzs + 64 * 128;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 af[4], bf[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int R = p * 16 + i;
                af[p] = *reinterpret_cast<const bf16x8*>(dzs + R * 128 + (((ks * 4 + g) ^ wa_L(R)) << 4));
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int R = wv * 64 + q * 16 + i;
                bf[q] = *reinterpret_cast<const bf16x8*>(xs + R * 128 + (((ks * 4 + g) ^ wa_L(R)) << 4));
            }
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[p], bf[q], acc[p][q], 0, 0, 0);
        }
        s ^= 1;
    }
    float* out = a.part + (size_t)blockIdx.z * a.N * a.K;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = kb + wv * 64 + q * 16 + i;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = p * 16 + g * 4 + r;
                if (n < a.N && col < a.K) out[(size_t)n * a.K + col] = acc[p][q][r];
            }
        }
}

// ---------------------------------------------------------------------------------------------- the partial-sum reducers
// out[i] = sum_k part[k][i]: 16 outputs x 16 partial-lanes per workgroup, fixed order (one thread walking all S partials
// serially took 33 us per call -- 3.6 ms of a 39 ms training step over ~110 calls)
// (KW > 1: the weight gradient leaves in the model's (Cout, Cin, KW) layout: partial index (o, tap, c) -> (o, c, tap))
// (2-D convs, KF > 1: the partial's tap index is kt * KF + kf -- the forward kernel's order -- the model's is kf * KT + kt)
__device__ __forceinline__ long long oik_index(long long idx, int Cin, int KW, int KF = 1) {
    if (KW <= 1) return idx;
    const long long o = idx / ((long long)KW * Cin);
    const int r = (int)(idx - o * KW * Cin);
    int j = r / Cin;
    const int c = r - j * Cin;
    if (KF > 1) j = (j % KF) * (KW / KF) + j / KF;
    return (o * Cin + c) * KW + j;
}
// both reducers: batched weight gradients have one (S, n) slab of partials and one output of n per blockIdx.y
__device__ __forceinline__ const float* sp_slab(const float* part, int S, long long n) { return part + (size_t)blockIdx.y * S * n; }
__device__ __forceinline__ void sp_store(float* out, long long n, long long idx, float v, int Cin, int KW, int KF) {
    out[(size_t)blockIdx.y * n + oik_index(idx, Cin, KW, KF)] = v;
}

__global__ __launch_bounds__(256) void sum_partials_kernel(const float* part, int S, long long n, float* out, int Cin, int KW, int KF) {
    __shared__ float sm[16][17];
    part = sp_slab(part, S, n);
    const int ol = threadIdx.x & 15, pl = threadIdx.x >> 4;
    const long long idx = (long long)blockIdx.x * 16 + ol;
    float s = 0.f;
    if (idx < n) {
        int k = pl;
        for (; k + 48 < S; k += 64) {             // four partial rows per trip, their loads issued together, summed in row order
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = part[(size_t)(k + 16 * u) * n + idx];
#pragma unroll
            for (int u = 0; u < 4; ++u) s += v[u];
        }
        for (; k < S; k += 16) s += part[(size_t)k * n + idx];
    }
    sm[pl][ol] = s;
    __syncthreads();
    if (pl == 0 && idx < n) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += sm[k][ol];
        sp_store(out, n, idx, t, Cin, KW, KF);
    }
}

// Many outputs (a weight gradient of >= 32 768 elements): 64 consecutive outputs per workgroup, the S partial rows dealt to the four
// waves (row k to wave k % 4, four loads in flight per lane) and the four wave sums added in wave order -- a fixed order.  (One thread
// walking all S rows of its output: 0.97 TB/s on a 33 MB partial slab, 37 us per call and 3-5 % of the 2-D backbones' training steps.)
__global__ __launch_bounds__(256) void sum_partials_wide_kernel(const float* part, int S, long long n, float* out, int Cin, int KW, int KF) {
    __shared__ float sm[3][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * 64 + lane;
    part = sp_slab(part, S, n);
    float s = 0.f;
    if (i < n) {
        int k = w;
        for (; k + 12 < S; k += 16) {
            const float v0 = part[(size_t)k * n + i], v1 = part[(size_t)(k + 4) * n + i];
            const float v2 = part[(size_t)(k + 8) * n + i], v3 = part[(size_t)(k + 12) * n + i];
            s += v0; s += v1; s += v2; s += v3;
        }
        for (; k < S; k += 4) s += part[(size_t)k * n + i];
    }
    if (w) sm[w - 1][lane] = s;
    __syncthreads();
    if (w == 0 && i < n) sp_store(out, n, i, ((s + sm[0][lane]) + sm[1][lane]) + sm[2][lane], Cin, KW, KF);
}

// ---------------------------------------------------------------------------------------------- 256 x 256 tiles, wide 1x1 layers
// The WIDE 1x1 layers (ECAPA tdnn1 / tdnn2: 512 x 512, MFA: 1536 x 1536, ASP's 128 x 1536 and 1536 x 128) on bf16 operands:
// dW[n][c] = sum_m dz[m][n] * x[m][c], both MFMA operands "k-major" in memory.  conv_wgrad_amp_kernel transposes them through registers
// (bit surgery per element, 128 x 128 tiles: on the MFA layer every operand byte is fetched twelve times, 816 us); here
//   * tiles are 256 (n) x 256 (c): eight waves of 64 x 128, one workgroup per CU -- the most a CU's accumulators hold;
//   * the operand rows go to LDS AS THEY LIE in memory (LDS-DMA, 16 B per lane, no VGPRs, no VALU), 32 rows per stage, four stages in
//     flight (128 KB), one counted s_waitcnt vmcnt + one barrier per stage;
//   * fragments come out of that row-major image with gfx950's transposing LDS read: ds_read_b64_tr_b16 hands lane i of a 16-lane group
//     COLUMN i of the 4 (rows) x 16 (columns) block the group's sixteen 8-byte addresses describe (lanes 4 r .. 4 r + 3 address row r) --
//     two reads = the eight k of a 16x16x32 operand.  A and B are read the same way, so the k order inside an MFMA is whatever the
//     hardware makes it for both.
// LDS image of a stage: [dz 32 rows x 512 B | x 32 rows x 512 B].  The 32-byte segment s (16 columns) of row r sits at segment
// s ^ f(r), f(r) = (r & 3) | ((r >> 3) & 1) << 2: the 32 lanes the LDS serves together read rows {8 g .. 8 g + 3} of two g, one segment
// each -- eight different f, 256 distinct bytes.  The DMA lands lane-linear, so the swizzle is applied to the SOURCE chunk.
// Rows past the split's end and stages past its last are beyond the buffer descriptors' num_records: they arrive as zeros.
constexpr int WT = 256;                    // tile edge of dW
constexpr int WT_KS = 32;                  // operand rows per stage = one MFMA k
constexpr int WT_ROWB = 512;               // bytes of an LDS row (256 bf16)
constexpr int WT_HALF = WT_KS * WT_ROWB;   // one operand of a stage
constexpr int WT_STAGE = 2 * WT_HALF;
constexpr int WT_NST = 4;
constexpr int WT_SMEM = WT_NST * WT_STAGE; // 131,072 B

typedef __attribute__((address_space(3))) void* wt_lds_t;
typedef __attribute__((ext_vector_type(4))) short s16x4;

struct WgradTrArgs {
    const bf16_t* x; const bf16_t* dz; float* part;
    int ldx, lddz, M, N, K, rows_per_split;
};

__device__ __forceinline__ bf16x8 wt_frag(const char* p) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p + 4 * WT_ROWB));
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

__global__ __launch_bounds__(512, 1) void conv_wgrad_tr256_kernel(const WgradTrArgs a) {
    extern __shared__ __attribute__((aligned(16))) char wsm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int wn = wv & 3, wc = wv >> 2;                                 // the wave's 64 outputs (n) x 128 inputs (c) of the tile
    // Workgroup -> (split, n tile, c tile), XCD-aware: the hardware deals consecutive workgroup ids round-robin to the eight XCDs, so id
    // bid runs logical tile (bid & 7) x (blocks per XCD) + (bid >> 3) -- an XCD's resident workgroups are CONSECUTIVE logical tiles:
    // the tiles of one or two row splits, which share their operand rows in that XCD's L2.  (With the plain order every XCD held tiles
    // of every split: 2.8 GB came over the fabric for the MFA layer's 0.47 GB of operands, 5.2 TB/s, and that was the kernel's time.)
    const int nblk = gridDim.x, bid = blockIdx.x;
    const int qq = nblk >> 3, rr = nblk & 7, xcd = bid & 7;
    const int swz = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (bid >> 3);
    const int tx = (a.K + WT - 1) / WT, ty = (a.N + WT - 1) / WT;       // (N or K = 128: one half-used tile on that side, see the host)
    const int split = swz / (tx * ty), rem = swz - split * (tx * ty);
    const int nb = (rem / tx) * WT, cb = (rem % tx) * WT;
    const int m_begin = split * a.rows_per_split;
    const int rows = min(a.M, m_begin + a.rows_per_split) - m_begin;
    float* out = a.part + (size_t)split * a.N * a.K;
    if (rows <= 0) return;                                               // (the host sizes the splits so that none is empty)
    const unsigned lddzb = (unsigned)a.lddz * 2u, ldxb = (unsigned)a.ldx * 2u;
    // A 128-column operand (ASP's attention TDNN: 128 outputs; its logits conv: 128 inputs) takes the same 256-wide tile: the descriptor
    // ends with the operand's LAST valid element, so the missing columns of the last row read as zeros and those of every other row read
    // the next row's first columns -- finite values that only reach accumulators the store below leaves out
    const int ncn = min(WT, a.N - nb), ncc = min(WT, a.K - cb);
    const __amdgpu_buffer_rsrc_t dzr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<bf16_t*>(a.dz + (size_t)m_begin * a.lddz + nb), 0, (unsigned)(((size_t)(rows - 1) * a.lddz + ncn) * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<bf16_t*>(a.x + (size_t)m_begin * a.ldx + cb), 0, (unsigned)(((size_t)(rows - 1) * a.ldx + ncc) * 2), 0x00020000);

    // staging: a DMA instruction fills two LDS rows (64 lanes x 16 B); wave wv owns rows 4 wv .. 4 wv + 3 of both operands
    unsigned vdz[2], vx[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int rl = 2 * k + (lane >> 5), r = 4 * wv + rl;
        const int f = (r & 3) | (((r >> 3) & 1) << 2);
        const unsigned chunk = (unsigned)((lane & 31) ^ (f << 1)) << 4;
        vdz[k] = (unsigned)r * lddzb + chunk;
        vx[k] = (unsigned)r * ldxb + chunk;
    }
    const int KT = (rows + WT_KS - 1) / WT_KS;
    auto issue = [&](int t, int slot) {
        char* st = wsm + slot * WT_STAGE + 4 * wv * WT_ROWB;
        // stages past the last: any offset past num_records (the row term alone is, for t >= KT)
        const unsigned rdz = (unsigned)t * (WT_KS * lddzb), rx = (unsigned)t * (WT_KS * ldxb);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(dzr, (wt_lds_t)(st + k * 2 * WT_ROWB), 16, vdz[k] + rdz, 0, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (wt_lds_t)(st + WT_HALF + k * 2 * WT_ROWB), 16, vx[k] + rx, 0, 0, 0);
        }
    };

    // fragment addresses inside a stage: row 8 g + (i >> 2) (+ 4 for the second read), segment (block ^ f), 8 bytes at (i & 3)
    const int fl = (i >> 2) | ((g & 1) << 2);
    const int rowoff = (8 * g + (i >> 2)) * WT_ROWB + (i & 3) * 8;
    int aoff[4], boff[8];
#pragma unroll
    for (int p = 0; p < 4; ++p) aoff[p] = rowoff + (((wn * 4 + p) ^ fl) << 5);
#pragma unroll
    for (int q = 0; q < 8; ++q) boff[q] = WT_HALF + rowoff + (((wc * 8 + q) ^ fl) << 5);

    f32x4 acc[4][8];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[p][q] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Software pipeline inside every wave: iteration t multiplies the fragments of stage t (read during iteration t - 1) while the
    // transposing reads of stage t + 1 are in flight; the DMA runs three stages ahead of the reads.  (Reads and MFMAs of ONE stage back
    // to back left the matrix cores idle through every read burst: all eight waves sit in the same phase between two barriers.)
    auto read = [&](int slot, bf16x8 (&af)[4], bf16x8 (&bf)[8]) {
        const char* st = wsm + slot * WT_STAGE;
#pragma unroll
        for (int p = 0; p < 4; ++p) af[p] = wt_frag(st + aoff[p]);
#pragma unroll
        for (int q = 0; q < 8; ++q) bf[q] = wt_frag(st + boff[q]);
    };
    auto mma = [&](const bf16x8 (&af)[4], const bf16x8 (&bf)[8]) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[p][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[p], bf[q], acc[p][q], 0, 0, 0);
    };
    // top of iteration t: stage t + 1 has landed when at most the two younger stages' pieces (4 each) are outstanding; past the barrier
    // everyone's pieces of it are in and everyone holds stage t in registers (lgkmcnt: its reads, issued a whole MFMA block ago, have
    // returned -- a raw s_barrier does not wait for them), so stage t's slot takes stage t + 4
    auto top = [&](int t, int slot) {
        asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        issue(t + 4, slot);
    };
    bf16x8 afA[4], bfA[8], afB[4], bfB[8];
    issue(0, 0); issue(1, 1); issue(2, 2); issue(3, 3);
    asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    read(0, afA, bfA);
    int t = 0;
    for (; t + 1 < KT; t += 2) {                                         // slots: stage t in t & 3
        top(t, t & 3);
        read((t + 1) & 3, afB, bfB);
        mma(afA, bfA);
        top(t + 1, (t + 1) & 3);
        read((t + 2) & 3, afA, bfA);                                     // (stage KT, when t + 2 == KT: zeros, not used)
        mma(afB, bfB);
    }
    if (t < KT) mma(afA, bfA);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                    // the zero-fill DMAs of the stages past the end

    const int n0 = nb + wn * 64, c0 = cb + wc * 128;
    if (n0 >= a.N || c0 >= a.K) return;                                 // (wave-uniform: the unused half of a 128-column side)
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(size_t)(n0 + p * 16 + g * 4 + r) * a.K + c0 + q * 16 + i] = acc[p][q][r];
}

// ---------------------------------------------------------------------------------------------- host: families, plan, launch
// One row per kernel (the AMP family has two: f32 operands rounded while staging, and WG_AMP_BF, bf16 operands in memory): LDS bytes (the
// exact-f32 kernel declares its own, the others ask for them at launch), tile of dW (outputs x k-columns), rows per staged chunk, block.
struct WgradKernel { const void* fn; int lds_bytes; bool lds_dynamic; int tile_n, tile_k, chunk, block; };
enum { WG_AMP_BF = VP_WGRAD_TR256 + 1, WG_KERNELS };
constexpr int WA_SMEM = 2 * 2 * WA_T * 128;       // two stages of (dz^T | x^T)
const WgradKernel& wgrad_kernel(int row) {
    static const WgradKernel table[WG_KERNELS] = {
        /* VP_WGRAD_F32   */ {reinterpret_cast<const void*>(conv_wgrad_kernel), 2 * WG_RC * WG_LD * 4, false, 64, 64, WG_RC, 256},
        /* VP_WGRAD_AMP   */ {reinterpret_cast<const void*>(conv_wgrad_amp_kernel<false>), WA_SMEM, true, WA_T, WA_T, WA_RC, 256},
        /* VP_WGRAD_X3    */ {reinterpret_cast<const void*>(conv_wgrad_amp_kernel<false, true>), 2 * WA_SMEM, true, WA_T, WA_T, WA_RC, 256},
        /* VP_WGRAD_N64   */ {reinterpret_cast<const void*>(conv_wgrad_n64_kernel), 2 * (64 + 256) * 128, true, 64, 256, WA_RC, 256},
        /* VP_WGRAD_TR256 */ {reinterpret_cast<const void*>(conv_wgrad_tr256_kernel), WT_SMEM, true, WT, WT, WT_KS, 512},
        /* WG_AMP_BF      */ {reinterpret_cast<const void*>(conv_wgrad_amp_kernel<true>), WA_SMEM, true, WA_T, WA_T, WA_RC, 256},
    };
    return table[row];
}
// more than 64 KB of dynamic LDS must be allowed once per kernel and DEVICE (a process may drive several GPUs)
int wgrad_allow_lds(vp_ctx* ctx, int row) {
    static bool done[64][WG_KERNELS] = {};
    bool& set = done[ctx->device & 63][row];
    if (!set && wgrad_kernel(row).lds_dynamic) {
        VP_HIP(ctx, hipFuncSetAttribute(wgrad_kernel(row).fn, hipFuncAttributeMaxDynamicSharedMemorySize, wgrad_kernel(row).lds_bytes));
        set = true;
    }
    return VP_OK;
}
int wgrad_cus(int device) {
    static int cus_dev[64] = {};
    int& cus = cus_dev[device & 63];
    if (!cus && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) cus = 256;
    return cus;
}
// M rows in S splits of whole staged chunks, none of them empty
struct WgradSplit { int S; long long rps; };
WgradSplit wgrad_whole_chunks(long long M, int S, int chunk) {
    const long long rps = ((M + S - 1) / S + chunk - 1) / chunk * chunk;
    return {(int)((M + rps - 1) / rps), rps};
}
// The 64-tile rule: ~2048 workgroups of 64 x 64 tiles, <= 256 splits of >= 64 rows; a batch fills the chip itself: fewer, longer splits
int wgrad_splits64(long long M, int Cout, int K, int nbatch) {
    int S = 2048 / (((Cout + 63) / 64) * ((K + 63) / 64));
    S = S < 1 ? 1 : (S > 256 ? 256 : S);
    if (nbatch > 1 && S > 512 / nbatch) S = 512 / nbatch > 1 ? 512 / nbatch : 1;
    return (long long)S * 64 > M ? (int)((M + 63) / 64) : S;
}
// The 256-tile kernel: sides of multiples of 256, or exactly 128 (a half-used tile: 64 x 128 per wave, so 128 is the one narrower width
// whose valid part is whole waves on either side); one workgroup per CU of a 256-CU chip, no split shorter than a stage.
bool wgrad_tr256_sides(int N, int K) { return (N % WT == 0 || N == 128) && (K % WT == 0 || K == 128); }
WgradSplit wgrad_tr256_split(long long M, int N, int K) {
    const int tiles = ((N + WT - 1) / WT) * ((K + WT - 1) / WT);
    int S = tiles < 256 ? 256 / tiles : 1;
    if ((long long)S * WT_KS > M) S = (int)((M + WT_KS - 1) / WT_KS);
    return wgrad_whole_chunks(M, S, WT_KS);
}
// The most splits any plan of this GEOMETRY has (M, Cout, K = KW * Cin, KW): the 64-tile rule unbatched -- every later step of the plan
// only takes splits away -- or the 256-tile count where the geometry admits that kernel.  The workspace is this many [Cout][K] partials.
int wgrad_splits_bound(long long M, int Cout, int K, int KW) {
    const int S = wgrad_splits64(M, Cout, K, 1);
    const int s2 = KW == 1 && wgrad_tr256_sides(Cout, K) && M >= WT_KS ? wgrad_tr256_split(M, Cout, K).S : 0;
    return s2 > S ? s2 : S;
}
bool wgrad_two_d(const vp_conv1d_desc* d) { return d->KF > 1 || d->F_in > 1 || d->F_out > 1; }
long long wgrad_rows(const vp_conv1d_desc* d) { return (long long)d->B * d->T_out * (wgrad_two_d(d) ? d->F_out : 1); }

// d: the FORWARD conv's descriptor (x / ldx / xoff and the geometry; w, y, epilogue fields ignored).  ws_bytes NULL: the plan query
int wgrad_validate(vp_ctx* ctx, const vp_conv1d_desc* d, const void* dz, int lddz, int nbatch, const void* ws, const size_t* ws_bytes) {
    if (!d || !d->x || !dz) VP_FAIL(ctx, VP_EINVAL, "wgrad: null argument");
    if (d->dtype_in != VP_F32 && d->dtype_in != VP_BF16) VP_FAIL(ctx, VP_EUNSUP, "wgrad: f32 or bf16 tensors");
    if (d->mfma_bf16 < 0 || d->mfma_bf16 > 3) VP_FAIL(ctx, VP_EINVAL, "wgrad: mfma_bf16 %d outside 0..3", d->mfma_bf16);
    if (wgrad_two_d(d) && (d->KF < 1 || d->KW % d->KF || d->F_in < 1 || d->F_out < 1 || d->stride_f < 1 || d->pad_mode != VP_PAD_ZERO))
        VP_FAIL(ctx, VP_EINVAL, "wgrad: bad 2-D geometry (zero padding only)");
    if (d->B <= 0 || d->T_in <= 0 || d->T_out <= 0 || d->Cin <= 0 || d->Cout <= 0 || d->KW <= 0 || d->stride <= 0 || d->dilation <= 0)
        VP_FAIL(ctx, VP_EINVAL, "wgrad: bad shape");
    const size_t need = vp_conv1d_wgrad_workspace_bytes(d) * (size_t)nbatch;
    if (ws_bytes && (!ws || *ws_bytes < need)) VP_FAIL(ctx, VP_EWORKSPACE, "wgrad: workspace %zu < %zu", *ws_bytes, need);
    if (nbatch < 1 || (nbatch > 1 && d->dtype_in != VP_BF16)) VP_FAIL(ctx, VP_EINVAL, "wgrad: batched launches take bf16 operands");
    if (wgrad_rows(d) > 0x7fffffffLL / 2) VP_FAIL(ctx, VP_EINVAL, "wgrad: too many rows");
    if ((d->Cin | d->Cout | d->ldx | d->xoff | lddz) & 3) VP_FAIL(ctx, VP_EINVAL, "wgrad: Cin / Cout / ldx / xoff / lddz must be multiples of 4");
    return VP_OK;
}
struct WgradPlan { int family, row, splits, rows_per_split; };       // row: of wgrad_kernel (tile edges, LDS bytes)
// Family and row splits of one launch (a validated descriptor), on a chip of `cus` CUs.  Pure host code.
int wgrad_plan(vp_ctx* ctx, const vp_conv1d_desc* d, const void* dz, int lddz, int nbatch, int cus, WgradPlan& p) {
    static const bool no_tr256 = getenv("VPMI_WGRAD_TR256_OFF") != nullptr;      // A/B switch (tools/wgrad_probe.py)
    const long long M = wgrad_rows(d);
    const int N = d->Cout, K = d->KW * d->Cin;
    const bool bf_in = d->dtype_in == VP_BF16, two_d = wgrad_two_d(d);      // bf_in: x AND dz bf16 in memory, bf16 matrix cores only
    const bool mc = d->mfma_bf16 || bf_in;            // the bf16 matrix cores
    // split precision (f32 operands).  Mode 3 (pre-split forward weights) is mode 2 here: the weights are not an operand of their own gradient
    const bool x3 = (d->mfma_bf16 == 2 || d->mfma_bf16 == 3) && !bf_in;
    int S = wgrad_splits64(M, N, K, nbatch);
    if (mc && nbatch == 1) {
        // The 128 x 128 kernel keeps two workgroups per CU resident (split precision: one).  1.5 rounds of them cost two rounds of time
        // (a 3 x 3 conv of 32 channels: 3 tiles x 256 splits = 768 workgroups on 512 slots): take the largest split count that fills
        // WHOLE rounds instead (3 x 170 = 510: the same rows in one round, and a third fewer partial rows).
        const long long slots = (x3 ? 1LL : 2LL) * cus;
        const long long tiles128 = (long long)((K + 127) / 128) * ((N + 127) / 128);
        const long long W = tiles128 * S, S2 = slots * (W / slots) / tiles128;
        if (W > slots && S2 >= 1 && S2 < S) S = (int)S2;
    }
    p.family = !mc ? VP_WGRAD_F32 : x3 ? VP_WGRAD_X3 : (bf_in && N <= 64 && K > 128 && !two_d && d->stride == 1) ? VP_WGRAD_N64 : VP_WGRAD_AMP;
    WgradSplit sp = wgrad_whole_chunks(M, S, wgrad_kernel(p.family).chunk);
    // The 256-tile kernel: plain wide 1x1 layers (source row = output row) on bf16 operands whose rows the LDS-DMA can fetch 16 bytes
    // at a time.  Small problems stay on the 128-tile kernel: one workgroup per CU leaves each split a handful of stages and the partial
    // sums cost more than the GEMM (512 x 512 over 9536 rows: 37 us against 28 us).  A 128-column side executes a 256-wide tile and is
    // counted as such (ASP's 128 x 1536 over 76 288 rows is 2.9998e10 flop as stated); a 128 x 128 layer would use a quarter of its tile.
    const bool simple = K == d->Cin && d->stride == 1 && d->pad_left == 0 && d->T_in == d->T_out && !two_d;
    if (bf_in && simple && nbatch == 1 && !no_tr256 && wgrad_tr256_sides(N, K) && !(N == 128 && K == 128) && (d->ldx | d->xoff | lddz) % 8 == 0 &&
        M >= WT_KS && 2.0 * (double)M * (N < WT ? WT : N) * (K < WT ? WT : K) >= 3e10 && !(((uintptr_t)d->x | (uintptr_t)dz) & 15)) {
        const WgradSplit t = wgrad_tr256_split(M, N, K);
        if (t.rps * (long long)(lddz > d->ldx ? lddz : d->ldx) * 2 < 0x70000000LL) { p.family = VP_WGRAD_TR256; sp = t; }      // 32-bit buffer offsets
    }
    const int bound = wgrad_splits_bound(M, N, K, d->KW);
    if (sp.S > bound) VP_FAIL(ctx, VP_EWORKSPACE, "wgrad: a plan of %d splits is past the workspace bound of %d", sp.S, bound);
    p.row = p.family == VP_WGRAD_AMP && bf_in ? WG_AMP_BF : p.family;
    p.splits = sp.S; p.rows_per_split = (int)sp.rps;
    return VP_OK;
}

int wgrad_launch(vp_ctx* ctx, const vp_conv1d_desc* d, const void* dz, int lddz, float* dW, void* ws, size_t ws_bytes, vp_stream stream,
                 bool oik, int nbatch = 1, long long x_bstride = 0, long long dz_bstride = 0) {
    if (!ctx || !dW) VP_FAIL(ctx, VP_EINVAL, "wgrad: null argument");
    WgradPlan p;
    int rc = wgrad_validate(ctx, d, dz, lddz, nbatch, ws, &ws_bytes);
    if (!rc) rc = wgrad_plan(ctx, d, dz, lddz, nbatch, wgrad_cus(ctx->device), p);
    if (!rc) rc = wgrad_allow_lds(ctx, p.row);
    if (rc) return rc;
    const WgradKernel& k = wgrad_kernel(p.row);
    const int N = d->Cout, K = d->KW * d->Cin, M = (int)wgrad_rows(d), two_d = wgrad_two_d(d);
    WgradArgs a;
    WgradTrArgs t;
    void* arg = &a;      // (the kernel's one by-value parameter)
    dim3 grid((K + k.tile_k - 1) / k.tile_k, (N + k.tile_n - 1) / k.tile_n, p.splits * nbatch);
    switch (p.family) {
    case VP_WGRAD_TR256:                               // its own argument block; a flat grid it orders itself (XCD-aware)
        t.x = static_cast<const bf16_t*>(d->x) + d->xoff; t.dz = static_cast<const bf16_t*>(dz); t.part = (float*)ws;
        t.ldx = d->ldx; t.lddz = lddz; t.M = M; t.N = N; t.K = K; t.rows_per_split = p.rows_per_split;
        arg = &t;
        grid = dim3(grid.x * grid.y * p.splits);
        break;
    default:
        a.x = (const float*)d->x; a.dz = (const float*)dz; a.part = (float*)ws;
        a.ldx = d->ldx; a.xoff = d->xoff; a.lddz = lddz; a.M = M; a.N = N; a.K = K; a.Cin = d->Cin;
        a.T_in = d->T_in; a.T_out = d->T_out; a.dilation = d->dilation; a.stride = d->stride; a.pad_left = d->pad_left;
        a.pad_mode = d->pad_mode; a.rows_per_split = p.rows_per_split;
        a.F_in = two_d ? d->F_in : 1; a.F_out = two_d ? d->F_out : 1; a.KF = two_d ? d->KF : 1;
        a.stride_f = two_d ? d->stride_f : 1; a.pad_f = two_d ? d->pad_f : 0;
        a.splits = p.splits; a.xb = x_bstride; a.dzb = dz_bstride;
    }
    hipStream_t st = (hipStream_t)stream;
    (void)hipLaunchKernel(k.fn, grid, dim3(k.block), &arg, k.lds_dynamic ? k.lds_bytes : 0, st);
    VP_LAUNCH_CHECK(ctx, "conv_wgrad");
    vp_launch_sum_partials((const float*)ws, p.splits, (long long)N * K, dW, st, d->Cin, oik ? d->KW : 1, nbatch, (oik && two_d) ? d->KF : 1);
    VP_LAUNCH_CHECK(ctx, "wgrad_reduce");
    return VP_OK;
}

}  // namespace

// many outputs: 64 per workgroup; few outputs, many partials: 16 x 16 (declared in common.h: bn_train.hip and train_ops.hip use it)
void vp_launch_sum_partials(const float* part, int S, long long n, float* out, hipStream_t st, int Cin, int KW, int batch, int KF) {
    if (n >= 32768) hipLaunchKernelGGL(sum_partials_wide_kernel, dim3((unsigned)((n + 63) / 64), batch), dim3(256), 0, st, part, S, n, out, Cin, KW, KF);
    else hipLaunchKernelGGL(sum_partials_kernel, dim3((unsigned)((n + 15) / 16), batch), dim3(256), 0, st, part, S, n, out, Cin, KW, KF);
}

extern "C" {

size_t vp_conv1d_wgrad_workspace_bytes(const vp_conv1d_desc* d) {
    if (!d || d->Cout <= 0 || d->KW <= 0 || d->Cin <= 0) return 0;
    const int K = d->KW * d->Cin;
    return (size_t)wgrad_splits_bound(wgrad_rows(d), d->Cout, K, d->KW) * d->Cout * K * sizeof(float) + 256;
}

int vp_conv1d_wgrad_plan(const vp_conv1d_desc* d, const void* dz, int lddz, int nbatch, int cus, int* kernel, int* tile_n, int* tile_k,
                         int* splits, int* rows_per_split) {
    WgradPlan p;
    int rc = wgrad_validate(nullptr, d, dz, lddz, nbatch, nullptr, nullptr);
    if (!rc) rc = wgrad_plan(nullptr, d, dz, lddz, nbatch, cus > 0 ? cus : 256, p);
    if (rc) return rc;
    if (kernel) *kernel = p.family;
    if (tile_n) *tile_n = wgrad_kernel(p.row).tile_n;
    if (tile_k) *tile_k = wgrad_kernel(p.row).tile_k;
    if (splits) *splits = p.splits;
    if (rows_per_split) *rows_per_split = p.rows_per_split;
    return VP_OK;
}

int vp_conv1d_wgrad_f32(vp_ctx* ctx, const vp_conv1d_desc* d, const float* dz, int lddz, float* dW, void* ws, size_t ws_bytes, vp_stream stream) {
    return wgrad_launch(ctx, d, dz, lddz, dW, ws, ws_bytes, stream, false);
}

// the same gradient in the model's own (Cout, Cin, KW) layout (KW = KT * KF taps for the 2-D convs): no permute copy afterwards
int vp_conv1d_wgrad_oik_f32(vp_ctx* ctx, const vp_conv1d_desc* d, const float* dz, int lddz, float* dW, void* ws, size_t ws_bytes, vp_stream stream) {
    return wgrad_launch(ctx, d, dz, lddz, dW, ws, ws_bytes, stream, true);
}

// x (d->x, d->dtype_in == VP_BF16) and dz both bf16 in memory; dW f32 in the model's (Cout, Cin, KW) layout
int vp_conv1d_wgrad_bf16_oik(vp_ctx* ctx, const vp_conv1d_desc* d, const void* dz, int lddz, float* dW, void* ws, size_t ws_bytes, vp_stream stream) {
    if (!d || d->dtype_in != VP_BF16) VP_FAIL(ctx, VP_EINVAL, "wgrad_bf16: the descriptor's dtype_in must be bf16");
    return wgrad_launch(ctx, d, dz, lddz, dW, ws, ws_bytes, stream, true);
}

// nbatch convs of identical geometry in ONE launch: conv c reads x + c * x_bstride and dz + c * dz_bstride (bf16 elements) and writes
// dW + c * Cout * Cin * KW; ws = nbatch x vp_conv1d_wgrad_workspace_bytes(d).  (The seven chunk convs of a Res2Net block.)
int vp_conv1d_wgrad_bf16_oik_batched(vp_ctx* ctx, const vp_conv1d_desc* d, const void* dz, int lddz, float* dW, int nbatch, long long x_bstride,
                                     long long dz_bstride, void* ws, size_t ws_bytes, vp_stream stream) {
    if (!d || d->dtype_in != VP_BF16) VP_FAIL(ctx, VP_EINVAL, "wgrad_bf16: the descriptor's dtype_in must be bf16");
    return wgrad_launch(ctx, d, dz, lddz, dW, ws, ws_bytes, stream, true, nbatch, x_bstride, dz_bstride);
}

}  // extern "C"
