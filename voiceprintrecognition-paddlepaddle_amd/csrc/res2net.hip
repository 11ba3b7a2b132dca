// Res2Net backbone forward (eval mode): the stem kernel, the two pooling kernels and the launch graph.
//
// Reference: Res2Net.forward (ppvector/models/res2net.py) = Conv2D(1 -> m, 7x7, stride 3, pad 1) + BN + ReLU -> MaxPool2D(3, 2, 1)
// -> 4 layers of Bottle2neck blocks (1x1 -> split into `scale` chunks -> 3x3 convs (stride, chained in 'normal' blocks) -> concat with
// the last chunk (passed through, or AvgPool2D(3, stride, 1, exclusive) in the 'stage' block) -> 1x1 -> BN + residual -> ReLU)
// -> reshape (B, C*F', T') -> AttentiveStatisticsPooling -> BN -> Linear -> BN.
// Layout: (B, T, F, C) position-major, as ResNetSE (resnet_se.hip).  The concat buffer of a block holds [last chunk | sp_0 | ... |
// sp_{nums-1}]: the host permutes conv1's output channels and conv3's input channels to that order, so the pass-through chunk of a
// 'normal' block is stored there by conv1's epilogue (y2 / ysplit) and the split convs write their column slices in place.  The
// chain sp_{i+1} = sp_i + spx[i+1] comes from the conv epilogue's aux = y + add_in.  The final reshape is a permutation of the ASP /
// Linear weights done at pack time (channel index f*C + c instead of c*F + f).  Descriptors are built by launch.h (vp_layer_desc +
// geometry); a call site sets only what is its own.
#include <math.h>

#include "launch.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------------
// Stem: conv 7x7 stride 3 pad 1 (one input channel) + bias + folded BN + ReLU, then max pool 3x3 stride 2 pad 1, in one kernel.  A
// workgroup owns PT pooled frames x all pooled bins x CG channels of one utterance: it stages the (6 PT + 7) x (F + 2) input patch (zero-padded) and
// the weights in LDS, computes the 2 PT + 1 conv rows the tile's pooling windows cover, and pools them.  The conv map never reaches HBM.
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
struct StemArgs {
    const T* x; T* y;
    const float* w; const float* bias; const float* scale; const float* shift;
    int T_, F, C, CG, Tc, Fc, Tp, Fp, PT, tiles;       // CG: the channels one workgroup computes (C / CG groups)
};

constexpr int STEM_K = 7;
constexpr int STEM_LDS_MAX = 48 * 1024;

int stem_out(int v) { return v >= 5 ? (v - 5) / 3 + 1 : 0; }     // conv 7, stride 3, pad 1
int pool_out(int v) { return v >= 1 ? (v - 1) / 2 + 1 : 0; }     // pool 3, stride 2, pad 1 (also a 3x3 / 1x1 stride-2 conv)
// (not launch.h's vp_down: this one maps an empty axis to 0, which the plan of a too-short input relies on; equal for v >= 1)
int down(int v, int s) { return s == 2 ? pool_out(v) : v; }

size_t stem_lds_bytes(int PT, int F, int CG, int Fc) {
    return ((size_t)(6 * PT + 7) * (F + 2) + (size_t)STEM_K * STEM_K * CG + 3 * (size_t)CG + (size_t)(2 * PT + 1) * Fc * CG) * 4;
}

// tile: PT pooled frames x CG channels per workgroup -- the most channels (a divisor of C, multiple of 4) that fit with PT >= 2 frames, else
// with one frame; 0 when not even 4 channels of one frame fit (F beyond ~1500 bins)
void stem_tile(int F, int C, int Fc, int& PT, int& CG) {
    for (int minpt = 2; minpt >= 1; --minpt)
        for (int cg = C; cg >= 4; cg -= 4) {
            if (C % cg) continue;
            for (int pt = 8; pt >= minpt; --pt)
                if (stem_lds_bytes(pt, F, cg, Fc) <= STEM_LDS_MAX) { PT = pt; CG = cg; return; }
        }
    PT = CG = 0;
}

template <typename T>
__global__ __launch_bounds__(256) void r2n_stem_kernel(StemArgs<T> a) {
    extern __shared__ float lds[];
    const int PT = a.PT, NR = 6 * PT + 7, NCR = 2 * PT + 1, FW = a.F + 2, C = a.CG;     // C: this workgroup's channels c0 .. c0 + CG - 1
    float* patch = lds;                                // [NR][FW]: input rows t0 .. t0 + NR - 1, columns f = -1 .. F
    float* wl = patch + NR * FW;                       // [49][CG]
    float* ep = wl + STEM_K * STEM_K * C;              // bias, scale, shift: [3][CG]
    float* cv = ep + 3 * C;                            // [NCR][Fc][CG] post-ReLU conv rows tc0 .. tc0 + NCR - 1 (-inf outside the map)
    const int ngroups = a.C / a.CG;
    const int b = blockIdx.x / (a.tiles * ngroups), rem = blockIdx.x - b * a.tiles * ngroups;
    const int tile = rem / ngroups, c0 = (rem - tile * ngroups) * a.CG;
    const int tp0 = tile * PT, tc0 = 2 * tp0 - 1, t0 = 3 * tc0 - 1;
    const T* xb = a.x + (size_t)b * a.T_ * a.F;
    for (int i = threadIdx.x; i < NR * FW; i += 256) {
        const int r = i / FW, col = i - r * FW;
        const int t = t0 + r, f = col - 1;
        patch[i] = (t >= 0 && t < a.T_ && f >= 0 && f < a.F) ? vp_to_f32(xb[(size_t)t * a.F + f]) : 0.f;
    }
    for (int i = threadIdx.x; i < STEM_K * STEM_K * C; i += 256) {
        const int tap = i / C, c = i - tap * C;
        wl[i] = a.w[(c0 + c) * STEM_K * STEM_K + tap];
    }
    for (int i = threadIdx.x; i < C; i += 256) {
        ep[i] = a.bias ? a.bias[c0 + i] : 0.f;
        ep[C + i] = a.scale ? a.scale[c0 + i] : 1.f;
        ep[2 * C + i] = a.shift ? a.shift[c0 + i] : 0.f;
    }
    __syncthreads();
    const int nconv = NCR * a.Fc * C;
    for (int i = threadIdx.x; i < nconv; i += 256) {
        const int c = i % C, rest = i / C;
        const int fc = rest % a.Fc, r = rest / a.Fc;
        const int tc = tc0 + r;
        float v = -INFINITY;
        if (tc >= 0 && tc < a.Tc) {
            const float* p = patch + 3 * r * FW + 3 * fc;          // t = 3 tc - 1 + kt, column = f + 1 = 3 fc + kf
            float acc = 0.f;
#pragma unroll
            for (int kt = 0; kt < STEM_K; ++kt)
#pragma unroll
                for (int kf = 0; kf < STEM_K; ++kf) acc = fmaf(p[kt * FW + kf], wl[(kt * STEM_K + kf) * C + c], acc);
            v = fmaxf((acc + ep[c]) * ep[C + c] + ep[2 * C + c], 0.f);
        }
        cv[i] = v;
    }
    __syncthreads();
    const int C4 = C / 4, npool = PT * a.Fp * C4;
    for (int i = threadIdx.x; i < npool; i += 256) {
        const int c4 = i % C4, rest = i / C4;
        const int fp = rest % a.Fp, q = rest / a.Fp;
        const int tp = tp0 + q;
        if (tp >= a.Tp) continue;
        float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int dr = 0; dr < 3; ++dr) {
            const int r = 2 * q + dr;                               // tc = 2 tp - 1 + dr
#pragma unroll
            for (int df = 0; df < 3; ++df) {
                const int fc = 2 * fp - 1 + df;
                if (fc < 0 || fc >= a.Fc) continue;
                const float* s = cv + ((size_t)r * a.Fc + fc) * C + 4 * c4;
#pragma unroll
                for (int j = 0; j < 4; ++j) m[j] = fmaxf(m[j], s[j]);
            }
        }
        vp_store4(a.y + (((size_t)b * a.Tp + tp) * a.Fp + fp) * a.C + c0 + 4 * c4, m);
    }
}

int r2n_stem(vp_ctx* ctx, int dt, const void* x, void* y, const float* w, const float* bias, const float* scale, const float* shift,
             int B, int T, int F, int C, hipStream_t st) {
    if (dt != VP_F32 && dt != VP_BF16) VP_FAIL(ctx, VP_EINVAL, "res2net stem: bad dtype");
    if (C < 4 || C % 4 || C > 256) VP_FAIL(ctx, VP_EUNSUP, "res2net stem: %d channels (4..256, multiple of 4)", C);
    const int Tc = stem_out(T), Fc = stem_out(F);
    if (Tc < 1 || Fc < 1) VP_FAIL(ctx, VP_EINVAL, "res2net stem: %d x %d input is smaller than the 7x7 stride-3 window", T, F);
    int PT, CG;
    stem_tile(F, C, Fc, PT, CG);
    if (PT < 1) VP_FAIL(ctx, VP_EUNSUP, "res2net stem: %d bins do not fit the LDS tile", F);
    const int Tp = pool_out(Tc), Fp = pool_out(Fc);
    const int tiles = (Tp + PT - 1) / PT;
    const long long grid = (long long)B * tiles * (C / CG);
    if (grid > 0x7fffffffLL) VP_FAIL(ctx, VP_EINVAL, "res2net stem: batch too large");
    const size_t lds = stem_lds_bytes(PT, F, CG, Fc);
    if (dt == VP_BF16) {
        StemArgs<bf16_t> a{(const bf16_t*)x, (bf16_t*)y, w, bias, scale, shift, T, F, C, CG, Tc, Fc, Tp, Fp, PT, tiles};
        hipLaunchKernelGGL(r2n_stem_kernel<bf16_t>, dim3((unsigned)grid), dim3(256), lds, st, a);
    } else {
        StemArgs<float> a{(const float*)x, (float*)y, w, bias, scale, shift, T, F, C, CG, Tc, Fc, Tp, Fp, PT, tiles};
        hipLaunchKernelGGL(r2n_stem_kernel<float>, dim3((unsigned)grid), dim3(256), lds, st, a);
    }
    VP_LAUNCH_CHECK(ctx, "res2net_stem");
    return VP_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 3x3 pooling over (B, T, F, C) maps with channel slices (rows ld apart, columns from off): exclusive average (stride 1 or 2, pad 1:
// the divisor counts only the window's elements inside the map -- Paddle's AvgPool2D default) and max (stride 2, pad 1, padding
// excluded).  Four channels per thread.  The backward kernels gather over the outputs whose windows cover an input element: no
// atomics, deterministic.
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
struct PoolArgs {
    const T* x; T* y; const T* x2;                   // x2: the max pool's forward input (backward only)
    int ldx, xoff, ldy, yoff;
    int Ti, Fi, To, Fo, C4, stride;
    long long total;
};

__device__ __forceinline__ int win_lo(int v, int s) { return v == 0 ? 0 : (v + s - 2) / s; }   // first output whose window holds v

template <typename T>
__global__ __launch_bounds__(256) void r2n_avgpool_kernel(PoolArgs<T> a) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (long long)gridDim.x * 256) {
        const int c4 = (int)(i % a.C4);
        long long r = i / a.C4;
        const int fo = (int)(r % a.Fo); r /= a.Fo;
        const int to = (int)(r % a.To);
        const long long b = r / a.To;
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        int cnt = 0;
        for (int dt = 0; dt < 3; ++dt) {
            const int t = to * a.stride - 1 + dt;
            if (t < 0 || t >= a.Ti) continue;
            for (int df = 0; df < 3; ++df) {
                const int f = fo * a.stride - 1 + df;
                if (f < 0 || f >= a.Fi) continue;
                float v[4];
                vp_load4(a.x + ((b * a.Ti + t) * a.Fi + f) * a.ldx + a.xoff + 4 * c4, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) s[j] += v[j];
                ++cnt;
            }
        }
        const float inv = 1.f / (float)cnt;
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] *= inv;
        vp_store4(a.y + ((b * a.To + to) * a.Fo + fo) * a.ldy + a.yoff + 4 * c4, s);
    }
}

// x = d out (To x Fo), y = d in (Ti x Fi)
__global__ __launch_bounds__(256) void r2n_avgpool_bwd_kernel(PoolArgs<float> a) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (long long)gridDim.x * 256) {
        const int c4 = (int)(i % a.C4);
        long long r = i / a.C4;
        const int f = (int)(r % a.Fi); r /= a.Fi;
        const int t = (int)(r % a.Ti);
        const long long b = r / a.Ti;
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        const int to1 = min((t + 1) / a.stride, a.To - 1), fo1 = min((f + 1) / a.stride, a.Fo - 1);
        for (int to = win_lo(t, a.stride); to <= to1; ++to) {
            const int nt = min(to * a.stride + 1, a.Ti - 1) - max(to * a.stride - 1, 0) + 1;
            for (int fo = win_lo(f, a.stride); fo <= fo1; ++fo) {
                const int nf = min(fo * a.stride + 1, a.Fi - 1) - max(fo * a.stride - 1, 0) + 1;
                float v[4];
                vp_load4(a.x + ((b * a.To + to) * a.Fo + fo) * a.ldx + a.xoff + 4 * c4, v);
                const float inv = 1.f / (float)(nt * nf);
#pragma unroll
                for (int j = 0; j < 4; ++j) s[j] += v[j] * inv;
            }
        }
        vp_store4(a.y + ((b * a.Ti + t) * a.Fi + f) * a.ldy + a.yoff + 4 * c4, s);
    }
}

__global__ __launch_bounds__(256) void r2n_maxpool_kernel(PoolArgs<float> a) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (long long)gridDim.x * 256) {
        const int c4 = (int)(i % a.C4);
        long long r = i / a.C4;
        const int fo = (int)(r % a.Fo); r /= a.Fo;
        const int to = (int)(r % a.To);
        const long long b = r / a.To;
        float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        for (int dt = 0; dt < 3; ++dt) {
            const int t = 2 * to - 1 + dt;
            if (t < 0 || t >= a.Ti) continue;
            for (int df = 0; df < 3; ++df) {
                const int f = 2 * fo - 1 + df;
                if (f < 0 || f >= a.Fi) continue;
                float v[4];
                vp_load4(a.x + ((b * a.Ti + t) * a.Fi + f) * a.ldx + a.xoff + 4 * c4, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) m[j] = fmaxf(m[j], v[j]);
            }
        }
        vp_store4(a.y + ((b * a.To + to) * a.Fo + fo) * a.ldy + a.yoff + 4 * c4, m);
    }
}

// x = d out, x2 = forward input, y = d in: each output's gradient goes to the FIRST maximum of its window in row-major scan order
__global__ __launch_bounds__(256) void r2n_maxpool_bwd_kernel(PoolArgs<float> a) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (long long)gridDim.x * 256) {
        const int c4 = (int)(i % a.C4);
        long long r = i / a.C4;
        const int f = (int)(r % a.Fi); r /= a.Fi;
        const int t = (int)(r % a.Ti);
        const long long b = r / a.Ti;
        const float* xin = a.x2 + b * a.Ti * a.Fi * (long long)a.C4 * 4 + 4 * c4;
        const long long ldin = (long long)a.C4 * 4;
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        const int to1 = min((t + 1) / 2, a.To - 1), fo1 = min((f + 1) / 2, a.Fo - 1);
        for (int to = win_lo(t, 2); to <= to1; ++to) {
            for (int fo = win_lo(f, 2); fo <= fo1; ++fo) {
                float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                int at[4] = {-1, -1, -1, -1};
                for (int dt = 0; dt < 3; ++dt) {
                    const int ts = 2 * to - 1 + dt;
                    if (ts < 0 || ts >= a.Ti) continue;
                    for (int df = 0; df < 3; ++df) {
                        const int fs = 2 * fo - 1 + df;
                        if (fs < 0 || fs >= a.Fi) continue;
                        float v[4];
                        vp_load4(xin + ((long long)ts * a.Fi + fs) * ldin, v);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (v[j] > m[j] || at[j] < 0) { m[j] = v[j]; at[j] = ts * a.Fi + fs; }
                    }
                }
                float g[4];
                vp_load4(a.x + ((b * a.To + to) * a.Fo + fo) * a.ldx + a.xoff + 4 * c4, g);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (at[j] == t * a.Fi + f) s[j] += g[j];
            }
        }
        vp_store4(a.y + ((b * a.Ti + t) * a.Fi + f) * a.ldy + a.yoff + 4 * c4, s);
    }
}

unsigned pool_blocks(long long total) {
    long long blocks = (total + 255) / 256;
    return (unsigned)(blocks > 256 * 64 ? 256 * 64 : (blocks < 1 ? 1 : blocks));
}

bool slices_ok(int C, int ldx, int xoff, int ldy, int yoff) {
    return C > 0 && C % 4 == 0 && ldx % 4 == 0 && xoff % 4 == 0 && ldy % 4 == 0 && yoff % 4 == 0 && xoff + C <= ldx && yoff + C <= ldy;
}

int r2n_avgpool(vp_ctx* ctx, int dt, const void* x, int ldx, int xoff, void* y, int ldy, int yoff, int B, int T, int F, int C, int stride,
                hipStream_t st) {
    if (stride != 1 && stride != 2) VP_FAIL(ctx, VP_EINVAL, "avgpool3x3: stride %d (1 or 2)", stride);
    if (!slices_ok(C, ldx, xoff, ldy, yoff) || B <= 0 || T <= 0 || F <= 0) VP_FAIL(ctx, VP_EINVAL, "avgpool3x3: bad shape / slice");
    const int To = down(T, stride), Fo = down(F, stride);
    const long long total = (long long)B * To * Fo * (C / 4);
    if (dt == VP_BF16) {
        PoolArgs<bf16_t> a{(const bf16_t*)x, (bf16_t*)y, nullptr, ldx, xoff, ldy, yoff, T, F, To, Fo, C / 4, stride, total};
        hipLaunchKernelGGL(r2n_avgpool_kernel<bf16_t>, dim3(pool_blocks(total)), dim3(256), 0, st, a);
    } else if (dt == VP_F32) {
        PoolArgs<float> a{(const float*)x, (float*)y, nullptr, ldx, xoff, ldy, yoff, T, F, To, Fo, C / 4, stride, total};
        hipLaunchKernelGGL(r2n_avgpool_kernel<float>, dim3(pool_blocks(total)), dim3(256), 0, st, a);
    } else {
        VP_FAIL(ctx, VP_EINVAL, "avgpool3x3: bad dtype");
    }
    VP_LAUNCH_CHECK(ctx, "avgpool3x3");
    return VP_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// launch graph
// ---------------------------------------------------------------------------------------------------------------------------------
struct R2nPlan {
    void *xa, *xb, *o1, *cat, *aux[2], *res;
    AspHeadBufs asp;
    size_t total;
    int Tp, Fp, T4, F4, C4;
};

void plan_r2n(const vp_res2net_weights* w, int B, int T, void* ws, R2nPlan& p) {
    const size_t es = vp_dtype_size(w->dtype);
    p.Tp = pool_out(stem_out(T)); p.Fp = pool_out(stem_out(w->feat_dim));
    int t = p.Tp, f = p.Fp;
    size_t big = (size_t)B * t * f * w->m_channels, o1 = 1, cat = 1, aux = 1, res = 1;
    for (int i = 0; i < w->n_blocks; ++i) {
        const vp_r2n_block& b = w->blk[i];
        const size_t pin = (size_t)B * t * f;
        const int to = down(t, b.stride), fo = down(f, b.stride);
        const size_t pout = (size_t)B * to * fo;
        if (pin * b.conv1.cin > big) big = pin * b.conv1.cin;
        if (pout * b.conv3.cout > big) big = pout * b.conv3.cout;
        if (pin * b.conv1.cout > o1) o1 = pin * b.conv1.cout;
        if (pout * b.conv1.cout > cat) cat = pout * b.conv1.cout;
        if (pin * b.width > aux) aux = pin * b.width;
        if (b.has_down && pout * b.down.cout > res) res = pout * b.down.cout;
        t = to; f = fo;
    }
    p.T4 = t; p.F4 = f; p.C4 = w->n_blocks > 0 ? w->blk[w->n_blocks - 1].conv3.cout : 0;
    const int Casp = p.F4 * p.C4;
    Carver c(ws);
    p.xa = c.take(big * es); p.xb = c.take(big * es);
    p.o1 = c.take(o1 * es); p.cat = c.take(cat * es);
    p.aux[0] = c.take(aux * es); p.aux[1] = c.take(aux * es);
    p.res = c.take(res * es);
    const AspHeadBytes ab = vp_asp_head_bytes(B, t, Casp, w->asp.att, es);
    p.asp.h = c.take(ab.h);
    p.asp.e = (float*)c.take(ab.e);
    p.asp.stats = (float*)c.take(ab.stats);
    p.asp.rowbias = (float*)c.take(ab.rowbias);
    p.asp.pooled = (float*)c.take(ab.pooled);
    p.total = c.off;
}

}  // namespace

extern "C" {

int vp_res2net_stem_fwd(vp_ctx* ctx, int dtype, const void* feats, void* out, const float* w, const float* bias, const float* scale,
                        const float* shift, int B, int T, int F, int C, vp_stream stream) {
    if (!ctx || !feats || !out || !w || B <= 0 || T <= 0 || F <= 0) VP_FAIL(ctx, VP_EINVAL, "res2net stem: bad arguments");
    return r2n_stem(ctx, dtype, feats, out, w, bias, scale, shift, B, T, F, C, (hipStream_t)stream);
}

int vp_avgpool3x3_fwd(vp_ctx* ctx, int dtype, const void* x, int ldx, int xoff, void* y, int ldy, int yoff, int B, int T, int F, int C,
                      int stride, vp_stream stream) {
    if (!ctx || !x || !y) VP_FAIL(ctx, VP_EINVAL, "avgpool3x3: null argument");
    return r2n_avgpool(ctx, dtype, x, ldx, xoff, y, ldy, yoff, B, T, F, C, stride, (hipStream_t)stream);
}

int vp_avgpool3x3_bwd_f32(vp_ctx* ctx, const float* dy, int lddy, int dyoff, float* dx, int lddx, int dxoff, int B, int T, int F, int C,
                          int stride, vp_stream stream) {
    if (!ctx || !dy || !dx) VP_FAIL(ctx, VP_EINVAL, "avgpool3x3_bwd: null argument");
    if (stride != 1 && stride != 2) VP_FAIL(ctx, VP_EINVAL, "avgpool3x3_bwd: stride %d (1 or 2)", stride);
    if (!slices_ok(C, lddy, dyoff, lddx, dxoff) || B <= 0 || T <= 0 || F <= 0) VP_FAIL(ctx, VP_EINVAL, "avgpool3x3_bwd: bad shape / slice");
    const long long total = (long long)B * T * F * (C / 4);
    PoolArgs<float> a{dy, dx, nullptr, lddy, dyoff, lddx, dxoff, T, F, down(T, stride), down(F, stride), C / 4, stride, total};
    hipLaunchKernelGGL(r2n_avgpool_bwd_kernel, dim3(pool_blocks(total)), dim3(256), 0, (hipStream_t)stream, a);
    VP_LAUNCH_CHECK(ctx, "avgpool3x3_bwd");
    return VP_OK;
}

int vp_maxpool3x3_fwd_f32(vp_ctx* ctx, const float* x, float* y, int B, int T, int F, int C, vp_stream stream) {
    if (!ctx || !x || !y || B <= 0 || T <= 0 || F <= 0 || C <= 0 || C % 4) VP_FAIL(ctx, VP_EINVAL, "maxpool3x3: bad arguments");
    const long long total = (long long)B * pool_out(T) * pool_out(F) * (C / 4);
    PoolArgs<float> a{x, y, nullptr, C, 0, C, 0, T, F, pool_out(T), pool_out(F), C / 4, 2, total};
    hipLaunchKernelGGL(r2n_maxpool_kernel, dim3(pool_blocks(total)), dim3(256), 0, (hipStream_t)stream, a);
    VP_LAUNCH_CHECK(ctx, "maxpool3x3");
    return VP_OK;
}

int vp_maxpool3x3_bwd_f32(vp_ctx* ctx, const float* x, const float* dy, float* dx, int B, int T, int F, int C, vp_stream stream) {
    if (!ctx || !x || !dy || !dx || B <= 0 || T <= 0 || F <= 0 || C <= 0 || C % 4) VP_FAIL(ctx, VP_EINVAL, "maxpool3x3_bwd: bad arguments");
    const long long total = (long long)B * T * F * (C / 4);
    PoolArgs<float> a{dy, dx, x, C, 0, C, 0, T, F, pool_out(T), pool_out(F), C / 4, 2, total};
    hipLaunchKernelGGL(r2n_maxpool_bwd_kernel, dim3(pool_blocks(total)), dim3(256), 0, (hipStream_t)stream, a);
    VP_LAUNCH_CHECK(ctx, "maxpool3x3_bwd");
    return VP_OK;
}

size_t vp_res2net_workspace_bytes(const vp_res2net_weights* w, int B, int T) {
    if (!w || B <= 0 || T <= 0 || w->n_blocks < 1 || w->n_blocks > VP_MAX_R2N_BLOCKS) return 0;
    R2nPlan p;
    plan_r2n(w, B, T, nullptr, p);
    return p.total;
}

int vp_res2net_fwd(vp_ctx* ctx, const vp_res2net_weights* w, const void* feats, int B, int T, float* emb, void* ws, size_t ws_bytes,
                   vp_stream stream) {
    if (!ctx || !w || !feats || !emb || B <= 0 || T <= 0) VP_FAIL(ctx, VP_EINVAL, "res2net: bad arguments");
    if (!vp_backbone_dtype_ok(w->dtype)) VP_FAIL(ctx, VP_EINVAL, "res2net: bad dtype");
    if (w->n_blocks < 1 || w->n_blocks > VP_MAX_R2N_BLOCKS || w->m_channels % 8 || w->m_channels > 256)
        VP_FAIL(ctx, VP_EUNSUP, "res2net: geometry not built (1..%d blocks, m_channels a multiple of 8 up to 256)", VP_MAX_R2N_BLOCKS);
    for (int i = 0; i < w->n_blocks; ++i) {
        const vp_r2n_block& b = w->blk[i];
        const int nums = b.scale > 1 ? b.scale - 1 : 1;
        if (b.scale < 1 || b.scale > VP_MAX_R2N_SCALE || (b.stride != 1 && b.stride != 2) || b.width < 8 || b.width % 8 ||
            b.conv1.cout != b.width * b.scale || b.conv3.cin != b.conv1.cout || (!b.has_down && b.conv3.cout != b.conv1.cin) ||
            (b.stride != 1 && !b.stage))
            VP_FAIL(ctx, VP_EINVAL, "res2net: block %d: inconsistent geometry", i);
        for (int j = 0; j < nums; ++j)
            if (b.convs[j].cin != b.width || b.convs[j].cout != b.width || b.convs[j].kw != 9)
                VP_FAIL(ctx, VP_EINVAL, "res2net: block %d: split conv %d is not 3x3 %d -> %d", i, j, b.width, b.width);
    }
    R2nPlan p;
    plan_r2n(w, B, T, ws, p);
    if (!ws || ws_bytes < p.total) VP_FAIL(ctx, VP_EWORKSPACE, "res2net: workspace %zu < %zu", ws_bytes, p.total);
    if (p.Tp < 1 || p.Fp < 1) VP_FAIL(ctx, VP_EINVAL, "res2net: %d frames x %d bins are too few for the stem", T, w->feat_dim);
    hipStream_t st = (hipStream_t)stream;
    const int dtc = w->dtype, dt = vp_storage_dtype(dtc);
    int rc;
    vp_conv1d_desc d;
    if ((rc = r2n_stem(ctx, dt, feats, p.xa, w->c1_w, w->c1_b, w->c1_scale, w->c1_shift, B, T, w->feat_dim, w->m_channels, st)))
        return rc;
    void* x = p.xa;
    void* xn = p.xb;
    int t = p.Tp, f = p.Fp;
    for (int i = 0; i < w->n_blocks; ++i) {
        const vp_r2n_block& b = w->blk[i];
        const int to = down(t, b.stride), fo = down(f, b.stride);
        const int W = b.width, S = b.scale, Cc = W * S, nums = S > 1 ? S - 1 : 1;
        auto off = [&](int j) { return (S > 1 ? j + 1 : j) * W; };    // column of chunk j (sp_j) in the conv1 output and the concat
        // o1 = relu(bn1(conv1x1(x))); a normal block's pass-through chunk (column 0) also lands in the concat buffer
        vp_layer_desc(d, b.conv1, dtc, VP_PAD_ZERO); vp_geom_rows(d, B, t * f, t * f);
        d.x = x; d.y = p.o1; d.act2 = VP_ACT_RELU;
        if (!b.stage && S > 1) { d.y2 = p.cat; d.ldy2 = Cc; d.y2off = 0; d.ysplit = W; }
        if ((rc = vp_conv1x1(ctx, d, st))) return rc;
        // sp_j = relu(bn(conv3x3 stride s (spx[j] | sp_{j-1} + spx[j]))) into the concat's column slice; a normal block's conv j also
        // writes the next conv's input sp_j + spx[j+1] (aux)
        for (int j = 0; j < nums; ++j) {
            const bool chained = !b.stage && j > 0;
            vp_layer_desc(d, b.convs[j], dtc, VP_PAD_ZERO); vp_geom2d(d, B, t, f, b.stride, true);
            d.act2 = VP_ACT_RELU;
            d.x = chained ? p.aux[(j - 1) & 1] : p.o1; d.ldx = chained ? W : Cc; d.xoff = chained ? 0 : off(j);
            d.y = p.cat; d.ldy = Cc; d.yoff = off(j);
            if (!b.stage && j + 1 < nums) {
                d.add_in = p.o1; d.ld_add = Cc; d.add_off = off(j + 1);
                d.aux = p.aux[j & 1]; d.ld_aux = W; d.aux_off = 0;
            }
            if ((rc = vp_conv1d_fwd(ctx, &d, st))) return rc;
        }
        // a stage block's last chunk: exclusive 3x3 average pool (stride s) straight into the concat's column 0
        if (b.stage && S > 1 && (rc = r2n_avgpool(ctx, dt, p.o1, Cc, 0, p.cat, Cc, 0, B, t, f, W, b.stride, st))) return rc;
        const void* res = x;
        int ldr = b.conv1.cin;
        if (b.has_down) {          // bn(conv1x1 stride (s, s)(x))
            vp_layer_desc(d, b.down, dtc, VP_PAD_ZERO);
            d.x = x; d.y = p.res;
            if ((rc = vp_conv1x1_strided(ctx, d, B, t, f, b.stride, st))) return rc;
            res = p.res; ldr = b.down.cout;
        }
        // x <- relu(bn3(conv1x1(concat)) + residual)
        vp_layer_desc(d, b.conv3, dtc, VP_PAD_ZERO); vp_geom_rows(d, B, to * fo, to * fo);
        d.x = p.cat; d.y = xn; d.res = res; d.ld_res = ldr; d.res_off = 0;
        d.act2 = VP_ACT_RELU;
        if ((rc = vp_conv1x1(ctx, d, st))) return rc;
        void* tmp = x; x = xn; xn = tmp;
        t = to; f = fo;
    }
    // ASP over time on (B, T4, F4*C4), then bn2 -> linear -> bn3 (folded + permuted at pack time)
    const int Casp = p.F4 * p.C4;
    if (w->asp.C != Casp) VP_FAIL(ctx, VP_EINVAL, "res2net: asp.C %d != %d (F' %d x C %d)", w->asp.C, Casp, p.F4, p.C4);
    return vp_asp_head(ctx, w->asp, dtc, x, B, t, Casp, p.asp, w->lin_w, w->lin_b, w->embd_dim, emb, st);
}

}  // extern "C"
