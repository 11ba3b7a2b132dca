// Host-side launch layer of the backbone forwards (ecapa.hip, campplus.hip, resnet_se.hip, eres2net.hip, res2net.hip): workspace carving,
// conv-descriptor construction, the 1x1 dispatch and the ASP head of the 2-D backbones.  Internal: nothing here is exported, and no
// other translation unit includes it.
#pragma once
#include "common.h"

// Bump allocator over the caller's workspace, 256-byte granules.  With a null base it only counts (the *_workspace_bytes entry points).
struct Carver {
    char* base; size_t off;
    explicit Carver(void* p) : base((char*)p), off(0) {}
    void* take(size_t bytes) {
        size_t o = off;
        off += vp_align_up(bytes ? bytes : 1, 256);
        return base ? (void*)(base + o) : nullptr;
    }
};

// output size of a stride-2 conv / pool whose padding is (kernel - 1) / 2: k1, k3 and CAM++'s k5
static inline int vp_down2(int v) { return (v - 1) / 2 + 1; }
static inline int vp_down(int v, int stride) { return stride == 2 ? vp_down2(v) : v; }

// dtype fields of a conv descriptor from a backbone's `dtype`
static inline void vp_desc_dtype(vp_conv1d_desc& d, int dt) {
    d.dtype_in = d.dtype_out = vp_storage_dtype(dt);
    d.mfma_bf16 = dt == VP_F32X3 ? 2 : 0;
}
// weights of a layer for a conv descriptor whose dtype fields are set: a split-precision backbone (VP_F32X3) hands over the layer's
// pre-split weights when it has them (only the activations are then split while staging)
static inline void vp_desc_weights(vp_conv1d_desc& d, const vp_tdnn_layer& L) {
    d.w = L.w;
    if (d.mfma_bf16 == 2 && d.dtype_in == VP_F32 && d.dtype_out == VP_F32 && L.w_hl) { d.w = L.w_hl; d.mfma_bf16 = 3; }
}

// A zeroed descriptor for layer L of a backbone of dtype `dtc`: dtype fields, the layer's channels / taps / weights / bias / folded BN,
// dense input and output rows (ldx = cin, ldy = cout), stride 1, dilation 1 (NOT L.dil: the dilated 1-D sites set it themselves).
// Geometry, activations, tensors and anything else are the call site's.
static inline void vp_layer_desc(vp_conv1d_desc& d, const vp_tdnn_layer& L, int dtc, int pad_mode) {
    memset(&d, 0, sizeof(d));
    vp_desc_dtype(d, dtc);
    d.Cin = L.cin; d.Cout = L.cout; d.KW = L.kw; d.dilation = 1; d.stride = 1;
    d.pad_mode = pad_mode; d.ldx = L.cin; d.ldy = L.cout;
    vp_desc_weights(d, L);
    d.bias = L.bias; d.bn_scale = L.bn_scale; d.bn_shift = L.bn_shift;
}

// 1-D geometry: B sequences of T_in rows in, T_out rows out (a position-major GEMM when the layer is 1x1)
static inline void vp_geom_rows(vp_conv1d_desc& d, int B, int T_in, int T_out) { d.B = B; d.T_in = T_in; d.T_out = T_out; }

// 2-D geometry of x (B, t, f, .): 3x3 pad 1 (k3) or 1x1, stride s on both axes
static inline void vp_geom2d(vp_conv1d_desc& d, int B, int t, int f, int s, bool k3) {
    d.B = B; d.T_in = t; d.F_in = f; d.T_out = vp_down(t, s); d.F_out = vp_down(f, s);
    d.KF = k3 ? 3 : 1; d.stride = s; d.stride_f = s; d.pad_left = k3 ? 1 : 0; d.pad_f = k3 ? 1 : 0;
}

// 1x1 convs over positions: the streaming kernel for the few-channel full-resolution stages (pointwise.hip), else the conv GEMM
static inline int vp_conv1x1(vp_ctx* ctx, const vp_conv1d_desc& d, hipStream_t st) {
    const int rc = vp_pointwise_bf16(ctx, &d, 1, st);
    return rc == VP_EUNSUP ? vp_conv1d_fwd(ctx, &d, st) : rc;
}

// a 1x1 conv with stride s on both axes of x (B, t, f, .) (downsample / shortcut): a plain pointwise conv over the B sequences of
// t * f positions when s == 1.  Sets the geometry of d.
static inline int vp_conv1x1_strided(vp_ctx* ctx, vp_conv1d_desc& d, int B, int t, int f, int s, hipStream_t st) {
    if (s == 1) {
        vp_geom_rows(d, B, t * f, t * f);
        return vp_conv1x1(ctx, d, st);
    }
    vp_geom2d(d, B, t, f, s, false);
    return vp_conv1d_fwd(ctx, &d, st);
}

// ASP head of the 2-D backbones (ResNetSE, Res2Net): attentive statistics pooling over time on the last map read as (B, T, C = F' C'),
// then bn2 -> linear -> bn3 (folded + permuted at pack time).
struct AspHeadBufs { void* h; float *e, *stats, *rowbias, *pooled; };
struct AspHeadBytes { size_t h, e, stats, rowbias, pooled; };
static inline AspHeadBytes vp_asp_head_bytes(int B, int T, int C, int att, size_t es) {
    return {(size_t)B * T * att * es, (size_t)B * T * C * 4, (size_t)B * 2 * C * 4, (size_t)B * att * 4, (size_t)B * 2 * C * 4};
}
static inline int vp_asp_head(vp_ctx* ctx, const vp_asp_weights& A, int dtc, const void* x, int B, int T, int C, const AspHeadBufs& w,
                              const float* lin_w, const float* lin_b, int embd_dim, float* emb, hipStream_t st) {
    int rc;
    if ((rc = vp_time_moments(ctx, vp_storage_dtype(dtc), x, C, B, T, C, 1e-12f, 0, w.stats, st))) return rc;
    VpAspBufs ab{w.h, w.e, nullptr, nullptr, w.stats, w.rowbias, w.pooled};
    if ((rc = vp_run_asp(ctx, A, dtc, x, C, nullptr, B, T, ab, st))) return rc;
    return vp_dense_f32_ex(ctx, w.pooled, 2 * C, lin_w, 0, lin_b, nullptr, nullptr, B, embd_dim, 2 * C, VP_ACT_NONE, emb, embd_dim, st);
}
