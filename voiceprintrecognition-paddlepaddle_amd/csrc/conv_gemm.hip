// conv1d / conv2d as an implicit GEMM on the gfx950 matrix cores, with the layer epilogue fused in.
//
// Replaces per launch: Conv1d.forward (ppvector/models/utils.py:65-93) / nn.Conv1D (tdnn.py:13-21,
// campplus.py:53-58,78-86,126) / nn.Conv2D (campplus.py:216-236,254-260) -> activation ->
// BatchNorm eval (utils.py:96-119, :147-148), the Res2Net hand-off x_{i+1} + y_i (ecapa_tdnn.py:36-47),
// the time sums SEBlock / ASP need (ecapa_tdnn.py:69-78, pooling.py:97-104), CAM++'s pre-activation
// BN-ReLU on the layer input (campplus.py:137-143,186-189), its context gate (campplus.py:92-94) and the
// ResBlock shortcut add (campplus.py:238-243).
//
// Layout: activations are position-major (B*T[*F], C) -- K (channels) contiguous for BOTH operands,
// so a conv tap is a row shift (reflect / zero padding handled in the row index), never an im2col.
//   M = B*T_out[*F_out] rows,  N = Cout,  K = taps*Cin  (k = tap*Cin + channel).
// Tile: 128 x {128, 64, 32} per 256-thread workgroup (4 waves), K staged 128 B per row per stage
// (64 bf16 / 32 f32), double-buffered LDS (XOR swizzle of the 16-B chunk index by row & 7: no bank
// conflicts -- SQ_LDS_BANK_CONFLICT = 0 measured) fed by a TWO-deep register prefetch of buffer
// loads (wave-uniform SRDs, out-of-range offsets for everything that must read as zero).
// MFMA: v_mfma_f32_16x16x32_bf16 (bf16 engine) or v_mfma_f32_16x16x4_f32 (exact-f32 engine), weights as
// the A operand and activations as the B operand so each lane ends up with 4 CONSECUTIVE output
// channels of one position: 8/16-byte epilogue loads and stores, float4 parameter reads.
// Roofline: MFMA-bound (dense contraction); algorithmic flops = 2*M*N*K per launch.
#include "common.h"

// ConvArgs, the mode ids, the kernel families and the launchers of the other translation units
#include "conv_gemm_impl.h"

namespace {

// The five environment switches, read once.  conv256 is the wide-tile selection of vpmi.h (vp_conv256_select() switches it at run time:
// A/B in one process).  VPMI_CONV256 is taken as written, also outside -1 .. 7, where it means what it always meant: below -1 the
// default, above 7 the two-stage kernel (conv_plan).  The others are A/B knobs:
//   VPMI_RING_MIN_COUT  narrowest layer the 256-column LDS-DMA tiles take (columns past Cout are zero-filled operands and masked
//                       stores: a 128-channel layer pays for 256), default 256
//   VPMI_HL_BN128       128-column K128 tiles for the narrow hl32 1x1 layers too (default: 64 columns up to Cout 128)
//   VPMI_BN64           64-column K128 tiles for bf16 input.  (Round 3 pinned that tile to 64 columns: kernels running beside it returned
//                       wrong lanes.  Round 4 found the cause in the VICTIMS, not here -- packed-f32 VALU instructions reading freshly
//                       loaded registers next to an MFMA-heavy wave, DESIGN.md section 8 -- and the library is now built without them.)
//   VPMI_GROUP_M        row tiles per group of the wide-tile kernels (not the bf16 K128X256_RING, which keeps its own rule)
struct ConvKnobs {
    int conv256, ring_min_cout, group_m;
    bool hl_bn128, bn64;
};
ConvKnobs& knobs() {
    static ConvKnobs k = [] {
        auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
        return ConvKnobs{num("VPMI_CONV256", -1), num("VPMI_RING_MIN_COUT", 256), num("VPMI_GROUP_M", 0),
                         getenv("VPMI_HL_BN128") != nullptr, getenv("VPMI_BN64") != nullptr};
    }();
    return k;
}

// what the validation derives from a descriptor
struct ConvShape {
    bool hl_in, hl_out, two_d;
    int epc, F_in, F_out;
    long long M;
    unsigned long long xbytes, wbytes, wrow;
};

struct ConvPlan {
    ConvKernel kernel;
    int mode;                               // MODE_* of conv_gemm_impl.h
    int tile_n;                             // tile columns: 32 / 64 / 128 (K128), 256
    int tiles_m, tiles_n, group_m;          // in units of the family's tile
};

constexpr int tile_rows(ConvKernel k) { return k == K256_TWO_STAGE || k == K256_RING ? 256 : 128; }

// Row tiles per group of the XCD-aware tile order (conv_gemm_impl.h): the workgroups of an XCD that run together share a group's
// operand panels in its L2.  K128X256_RING: two workgroups per CU, ~64 of an XCD share a group.
int group_size(ConvKernel k, int tiles_n) {
    const int budget = k == K128 ? 96 : k == K128X256_RING ? 64 : 32, most = k == K128X256_RING ? 32 : 16;
    const int g = budget / tiles_n;
    return g < 1 ? 1 : (g > most ? most : g);
}

int conv_validate(vp_ctx* ctx, const vp_conv1d_desc* d, ConvShape& s) {
    if (!d || !d->x || !d->w || !d->y) VP_FAIL(ctx, VP_EINVAL, "conv1d: null argument");
    if ((d->dtype_in != VP_F32 && d->dtype_in != VP_BF16 && d->dtype_in != VP_HL32) ||
        (d->dtype_out != VP_F32 && d->dtype_out != VP_BF16 && d->dtype_out != VP_HL32))
        VP_FAIL(ctx, VP_EINVAL, "conv1d: bad dtype");
    if (d->dtype_in == VP_F32 && d->dtype_out == VP_BF16) VP_FAIL(ctx, VP_EUNSUP, "conv1d: f32 -> bf16 not built");
    // (mode 3 = pre-split weights on the f32-tensor kernel; the hl32 kernels take split weights as they are, in mode 2)
    if (d->mfma_bf16 < 0 || d->mfma_bf16 > 3) VP_FAIL(ctx, VP_EINVAL, "conv1d: mfma_bf16 %d outside 0..3", d->mfma_bf16);
    if (d->mfma_bf16 == 3 && (d->dtype_in != VP_F32 || d->dtype_out != VP_F32)) VP_FAIL(ctx, VP_EINVAL, "conv1d: mfma_bf16 = 3 takes f32 tensors");
    const bool hl_in = d->dtype_in == VP_HL32, hl_out = d->dtype_out == VP_HL32;
    if (hl_in || hl_out) {
        // split bf16 planes (vpmi.h: VP_HL32): 32-channel groups; f32 x (split while staging, mfma_bf16 = 2) or hl32 x, hl32 w with hl32 x
        if ((hl_in && (d->Cin % 32 || d->ldx % 32 || d->xoff % 32)) ||
            (hl_out && (d->Cout % 32 || d->ldy % 32 || d->yoff % 32 || d->ysplit % 32 || d->ldy2 % 32 || d->y2off % 32 || d->ld_add % 32 ||
                        d->add_off % 32 || d->ld_aux % 32 || d->aux_off % 32 || d->ld_res % 32 || d->res_off % 32)))
            VP_FAIL(ctx, VP_EINVAL, "conv1d: hl32 tensors need channel counts, leading dimensions and offsets that are multiples of 32");
        if (d->dtype_in == VP_BF16 || d->dtype_out == VP_BF16 || (d->dtype_in == VP_F32 && d->mfma_bf16 != 2) || d->gate || d->pro_scale ||
            d->KF > 1 || d->F_in > 1 || d->F_out > 1)
            VP_FAIL(ctx, VP_EUNSUP, "conv1d: hl32 is built for 1-D layers of the split-precision engine (f32 / hl32 in with mfma_bf16 = 2 semantics)");
    }
    const int epc = d->dtype_in == VP_BF16 ? 8 : 4;
    if (d->B <= 0 || d->T_in <= 0 || d->T_out <= 0 || d->Cin <= 0 || d->Cout <= 0 || d->KW <= 0 || d->stride <= 0 ||
        d->dilation <= 0)
        VP_FAIL(ctx, VP_EINVAL, "conv1d: bad shape");
    if (d->Cin % epc || d->ldx % epc || d->xoff % epc) VP_FAIL(ctx, VP_EINVAL, "conv1d: Cin/ldx/xoff must be multiples of %d", epc);
    if (d->Cout % 4 || d->ldy % 4 || d->yoff % 4) VP_FAIL(ctx, VP_EINVAL, "conv1d: Cout/ldy/yoff must be multiples of 4");
    if (d->ysplit) {
        if (!d->y2 || d->ysplit % 4 || d->ldy2 % 4 || d->y2off % 4 || d->ysplit > d->Cout)
            VP_FAIL(ctx, VP_EINVAL, "conv1d: bad y2 split");
    }
    if (d->aux && (!d->add_in || d->ld_add % 4 || d->add_off % 4 || d->ld_aux % 4 || d->aux_off % 4))
        VP_FAIL(ctx, VP_EINVAL, "conv1d: bad aux/add_in");
    if (d->res && (d->ld_res % 4 || d->res_off % 4)) VP_FAIL(ctx, VP_EINVAL, "conv1d: bad residual");
    const bool two_d = d->KF > 1 || d->F_in > 1 || d->F_out > 1;
    const bool pro = d->pro_scale != nullptr;
    if (pro && (!d->pro_shift || d->KW != 1 || two_d)) VP_FAIL(ctx, VP_EINVAL, "conv1d: input prologue needs a 1x1 conv");
    const int span = d->dilation * ((two_d ? d->KW / (d->KF > 0 ? d->KF : 1) : d->KW) - 1);
    if (two_d) {
        if (d->KF < 1 || d->KW % d->KF || d->F_in < 1 || d->F_out < 1 || d->stride_f < 1 || d->pad_mode != VP_PAD_ZERO)
            VP_FAIL(ctx, VP_EINVAL, "conv2d: bad geometry (zero padding only)");
        if (d->rowbias || d->psum || d->gate) VP_FAIL(ctx, VP_EUNSUP, "conv2d: per-utterance epilogue terms are 1-D only");
    } else if (d->pad_mode == VP_PAD_NONE) {
        if ((d->T_out - 1) * d->stride + span > d->T_in - 1)
            VP_FAIL(ctx, VP_EINVAL, "conv1d: un-padded window leaves the input (T_in %d, T_out %d)", d->T_in, d->T_out);
        if (d->pad_left != 0) VP_FAIL(ctx, VP_EINVAL, "conv1d: pad_left with PAD_NONE");
    } else if (d->pad_mode == VP_PAD_REFLECT) {
        const int right = (d->T_out - 1) * d->stride - d->pad_left + span - (d->T_in - 1);
        if (d->pad_left >= d->T_in || right >= d->T_in) VP_FAIL(ctx, VP_EINVAL, "conv1d: reflect pad >= T_in");
    } else if (d->pad_mode != VP_PAD_ZERO) {
        VP_FAIL(ctx, VP_EINVAL, "conv1d: bad pad_mode");
    }
    if (d->gate && (d->gate_len < 1 || d->gate_nseg < 1)) VP_FAIL(ctx, VP_EINVAL, "conv1d: bad gate segmentation");
    const int F_in = two_d ? d->F_in : 1, F_out = two_d ? d->F_out : 1;
    const long long Mll = (long long)d->B * d->T_out * F_out;
    if (Mll > 0x7fffffffLL / 2) VP_FAIL(ctx, VP_EINVAL, "conv1d: too many output positions");
    const size_t es = d->dtype_in == VP_BF16 ? 2 : 4;
    const unsigned long long xbytes = ((unsigned long long)d->B * d->T_in * F_in - 1) * d->ldx * es + (d->xoff + d->Cin) * es;
    // (mfma_bf16 = 3: the weights are split bf16 planes whose rows are zero-padded to whole 32-element groups)
    const unsigned long long wrow = d->mfma_bf16 == 3 ? ((unsigned long long)d->KW * d->Cin + 31) / 32 * 32 : (unsigned long long)d->KW * d->Cin;
    const unsigned long long wbytes = (unsigned long long)d->Cout * wrow * es;
    if (wbytes >= 0xffffff00ull) VP_FAIL(ctx, VP_EUNSUP, "conv1d: weights larger than 4 GiB (32-bit buffer offsets)");
    s = ConvShape{hl_in, hl_out, two_d, epc, F_in, F_out, Mll, xbytes, wbytes, wrow};
    return VP_OK;
}

// The kernels address x through a 32-bit buffer offset.  Utterances are independent rows of the GEMM, so a larger activation
// tensor (ERes2Net-large at 128 utterances per GPU: BASELINE configs[4]) runs as consecutive launches over batch slices of bc
// utterances; a slice of the fused time sums must start on an M-tile boundary of the partial-sum arrays.  bc = 0: one launch.
int conv_slice(vp_ctx* ctx, const vp_conv1d_desc* d, const ConvShape& s, long long& bc) {
    bc = 0;
    if (s.xbytes < 0xffffff00ull) return VP_OK;
    const size_t es = d->dtype_in == VP_BF16 ? 2 : 4;
    const unsigned long long per_utt = (unsigned long long)d->T_in * s.F_in * d->ldx * es;
    bc = (long long)(0xe0000000ull / (per_utt ? per_utt : 1));
    if (d->psum) {
        int ga = d->T_out, gb = BM;                         // slices of bc utterances with bc * T_out a multiple of the M-tile
        while (gb) { const int t_ = ga % gb; ga = gb; gb = t_; }
        const long long q = BM / ga;
        bc = bc / q * q;
    }
    if (bc < 1 || d->B < 2) VP_FAIL(ctx, VP_EUNSUP, "conv1d: one utterance's activations exceed 4 GiB (32-bit buffer offsets)");
    return VP_OK;
}

// Kernel family, mode and tile geometry of one launch (a validated descriptor that needs no slicing).
// The wide bf16 layers go to the LDS-DMA tiles of conv_gemm256.hip; k.conv256 (vpmi.h: vp_conv256_select) says which.  Measured on
// MI355X, 1536 -> 1536 / 512 -> 512 launches at 256 x 298 rows (round 3, one session, with the fused time sums): K256_RING 322 / 70.6 us,
// K128X256_RING 332 / 64.4; without sums 313 / 62.0 and 320 / 55.2.  Inside the two-stream step (bench.py) K128X256_RING for every
// 1x1 layer beats "K128X256_RING for K <= 1024, else K256_RING" (7): 1.282 vs 1.301 ms (K256_RING everywhere: 1.313) -- a 4-wave
// workgroup with 80 KB of LDS leaves half a CU to the other launch sequence's memory-bound kernels.  Hence the default.
int conv_plan(vp_ctx* ctx, const vp_conv1d_desc* d, const ConvShape& s, const ConvKnobs& k, ConvPlan& p) {
    const int mode = s.two_d ? MODE_2D : (d->KW == 1 ? (d->pro_scale ? MODE_1X1_PRO : MODE_1X1) : MODE_TAPS);
    int bn = d->Cout <= 32 ? 32 : (d->Cout <= 64 ? 64 : 128);
    if (mode == MODE_1X1_PRO && bn > 64) bn = 64;
    if (d->dtype_in == VP_BF16 && d->dtype_out == VP_F32) bn = 128;
    if (s.hl_in || s.hl_out) bn = (s.hl_in && s.hl_out && mode == MODE_1X1 && d->Cout <= 128 && !k.hl_bn128) ? 64 : 128;
    if (k.bn64 && d->dtype_in == VP_BF16 && bn == 128) bn = 64;
    if (d->psum && vp_conv1d_nseg(d->T_out) > NSEG_MAX) VP_FAIL(ctx, VP_EUNSUP, "conv1d: T_out %d too short for fused time sums", d->T_out);
    const int M = (int)s.M, K = d->KW * d->Cin;
    auto take = [&](ConvKernel kernel, int pmode, int tile_n) {
        p.kernel = kernel; p.mode = pmode; p.tile_n = tile_n;
        p.tiles_m = (M + tile_rows(kernel) - 1) / tile_rows(kernel);
        p.tiles_n = (d->Cout + tile_n - 1) / tile_n;
        p.group_m = group_size(kernel, p.tiles_n);
    };
    // what every wide tile asks for: enough columns, no gate, and fused time sums in the layout of two utterance segments per 128 rows
    const bool wide = k.conv256 != 0 && d->Cout >= k.ring_min_cout && !d->gate && (!d->psum || d->T_out >= 128);
    // the ring kernels address a 1x1 layer as "source row m for output row m" with wave-uniform piece offsets and let the buffer
    // range check zero what lies past M / N / K: anything else (strided / padded 1x1, operands near 4 GiB) takes the two-stage
    // kernel with its per-row offsets
    const bool ring_ok = mode == MODE_1X1 && d->stride == 1 && d->pad_left == 0 && d->T_in == d->T_out && s.xbytes < 0xe0000000ull &&
                         s.wbytes < 0xe0000000ull;
    if (d->dtype_in == VP_BF16 && wide && (mode == MODE_TAPS || (mode == MODE_1X1 && d->Cin % 64 == 0))) {
        const int sel = k.conv256 < 0 ? 6 : k.conv256;       // 1, 2 (as 3) and 5 (as 4) name schedules that are no longer built
        ConvKernel want = sel == 6 || (sel == 7 && K <= 1024) ? K128X256_RING : (sel == 4 || sel == 5 || sel == 7 ? K256_RING : K256_TWO_STAGE);
        if (!ring_ok) want = K256_TWO_STAGE;                  // (tapped layers: the ring loop would spill, conv_gemm256.hip)
        // f32 output (the training engine's data-gradient GEMMs over bf16 dz) is built on K128X256_RING only
        const long long min_rows = want == K128X256_RING ? 128 * 32 : 256 * 64;      // enough tiles to be worth a wide-tile launch
        if ((d->dtype_out != VP_F32 || want == K128X256_RING) && M >= min_rows) {
            take(want, mode == MODE_TAPS && d->Cin % 64 ? MODE_TAPS_GEN : mode, 256);
            if (k.group_m > 0 && want != K128X256_RING) p.group_m = k.group_m;
            return VP_OK;
        }
    }
    if (s.hl_in && wide && ring_ok && M >= 128 * 32) {        // wide 1x1 layers in split precision
        take(K128X256_RING, mode, 256);
        if (k.group_m > 0) p.group_m = k.group_m;
        return VP_OK;
    }
    if (s.hl_in && !s.hl_out) VP_FAIL(ctx, VP_EUNSUP, "conv1d: hl32 -> f32 is built on the ring kernel only (wide 1x1 layers)");
    take(K128, mode, bn);
    return VP_OK;
}

}  // namespace

extern "C" {

int vp_conv256_select(int schedule) {
    const int prev = knobs().conv256;
    if (schedule >= -1 && schedule <= 7) knobs().conv256 = schedule;
    return prev;
}

int vp_conv1d_tiles_m(int B, int T_out) { return (int)(((long long)B * T_out + BM - 1) / BM); }
int vp_conv1d_nseg(int T_out) { return T_out > 0 ? (BM - 1) / T_out + 2 : 0; }

int vp_conv1d_plan(const vp_conv1d_desc* d, int* kernel, int* tile_n, int* tiles_m, int* tiles_n, int* group_m, int* launches) {
    ConvShape s;
    long long bc;
    int rc = conv_validate(nullptr, d, s);
    if (!rc) rc = conv_slice(nullptr, d, s, bc);
    if (rc) return rc;
    vp_conv1d_desc first = *d;
    if (bc && bc < d->B) {
        first.B = (int)bc;
        rc = conv_validate(nullptr, &first, s);
        if (rc) return rc;
    }
    ConvPlan p;
    rc = conv_plan(nullptr, &first, s, knobs(), p);
    if (rc) return rc;
    if (kernel) *kernel = p.kernel;
    if (tile_n) *tile_n = p.tile_n;
    if (tiles_m) *tiles_m = p.tiles_m;
    if (tiles_n) *tiles_n = p.tiles_n;
    if (group_m) *group_m = p.group_m;
    if (launches) *launches = bc ? (int)((d->B + bc - 1) / bc) : 1;
    return VP_OK;
}

int vp_conv1d_fwd(vp_ctx* ctx, const vp_conv1d_desc* d, vp_stream stream) {
    if (!ctx) return VP_EINVAL;
    ConvShape s;
    long long bc;
    int rc = conv_validate(ctx, d, s);
    if (!rc) rc = conv_slice(ctx, d, s, bc);
    if (rc) return rc;
    if (bc) {
        const size_t es = d->dtype_in == VP_BF16 ? 2 : 4, eo = d->dtype_out == VP_BF16 ? 2 : 4;
        for (long long b0 = 0; b0 < d->B; b0 += bc) {
            vp_conv1d_desc c = *d;
            c.B = (int)(d->B - b0 < bc ? d->B - b0 : bc);
            const size_t rin = (size_t)b0 * d->T_in * s.F_in, rout = (size_t)b0 * d->T_out * s.F_out;
            c.x = static_cast<const char*>(d->x) + rin * d->ldx * es;
            c.y = static_cast<char*>(d->y) + rout * d->ldy * eo;
            if (d->y2) c.y2 = static_cast<char*>(d->y2) + rout * d->ldy2 * eo;
            if (d->add_in) c.add_in = static_cast<const char*>(d->add_in) + rout * d->ld_add * eo;
            if (d->aux) c.aux = static_cast<char*>(d->aux) + rout * d->ld_aux * eo;
            if (d->res) c.res = static_cast<const char*>(d->res) + rout * d->ld_res * eo;
            if (d->rowbias) c.rowbias = d->rowbias + (size_t)b0 * d->Cout;
            if (d->gate) c.gate = d->gate + (size_t)b0 * d->gate_nseg * d->Cout;
            const size_t pso = rout / BM * (size_t)vp_conv1d_nseg(d->T_out) * d->Cout;
            if (d->psum) c.psum = d->psum + pso;
            if (d->psumsq) c.psumsq = d->psumsq + pso;
            rc = vp_conv1d_fwd(ctx, &c, stream);
            if (rc) return rc;
        }
        return VP_OK;
    }
    ConvPlan p;
    rc = conv_plan(ctx, d, s, knobs(), p);
    if (rc) return rc;
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x = d->x; a.w = d->w; a.bias = d->bias; a.rowbias = d->rowbias;
    a.x_bytes = (unsigned)s.xbytes; a.w_bytes = (unsigned)s.wbytes; a.y2 = d->y2;
    a.bn_scale = d->bn_scale; a.bn_shift = d->bn_shift; a.y = d->y; a.add_in = d->add_in; a.aux = d->aux;
    a.pro_scale = d->pro_scale; a.pro_shift = d->pro_shift; a.gate = d->gate; a.res = d->res;
    a.psum = d->psum; a.psumsq = d->psumsq;
    a.ldx = d->ldx; a.xoff = d->xoff; a.ldy2 = d->ldy2; a.y2off = d->y2off; a.ysplit = d->ysplit;
    a.ldy = d->ldy; a.yoff = d->yoff; a.ld_add = d->ld_add; a.add_off = d->add_off; a.ld_aux = d->ld_aux;
    a.aux_off = d->aux_off; a.ld_res = d->ld_res; a.res_off = d->res_off;
    a.M = (int)s.M; a.N = d->Cout; a.K = d->KW * d->Cin; a.cpt = d->Cin / s.epc; a.KC = a.K / s.epc; a.Cin = d->Cin;
    a.Kw = d->mfma_bf16 == 3 ? (int)s.wrow : a.K;   // (3: the weights are split planes, rows padded to 32-element groups)
    a.KT = (a.KC + 7) / 8;
    a.T_in = d->T_in; a.T_out = d->T_out; a.dilation = d->dilation; a.stride = d->stride; a.pad_left = d->pad_left;
    a.pad_mode = d->pad_mode; a.act = d->act; a.act2 = d->act2;
    a.F_in = s.F_in; a.F_out = s.F_out; a.KF = s.two_d ? d->KF : 1; a.stride_f = s.two_d ? d->stride_f : 1; a.pad_f = s.two_d ? d->pad_f : 0;
    a.gate_len = d->gate_len > 0 ? d->gate_len : 1; a.gate_nseg = d->gate_nseg;
    a.nseg = vp_conv1d_nseg(d->T_out);
    a.tiles_m = p.tiles_m; a.tiles_n = p.tiles_n; a.group_m = p.group_m;
    hipStream_t st = (hipStream_t)stream;
    const bool out_f32 = d->dtype_out == VP_F32;
    switch (p.kernel) {
    case K256_TWO_STAGE:
    case K256_RING:
        return vp_conv_launch256_bf16(ctx, a, p.kernel, p.mode, out_f32, st);
    case K128X256_RING:
        return s.hl_in ? vp_conv_launch_ring_x3(ctx, a, out_f32, st) : vp_conv_launch256_bf16(ctx, a, p.kernel, p.mode, out_f32, st);
    case K128:
        break;
    }
    if (s.hl_in) return vp_conv_launch_hl_hl(ctx, a, p.tile_n, p.mode, st);
    if (s.hl_out) return vp_conv_launch_x3_hl(ctx, a, p.tile_n, p.mode, st);
    if (d->dtype_in == VP_BF16) return (out_f32 ? vp_conv_launch_bf16_f32 : vp_conv_launch_bf16_bf16)(ctx, a, p.tile_n, p.mode, st);
    switch (d->mfma_bf16) {                   // f32 tensors
    case 3: return vp_conv_launch_x3w_f32(ctx, a, p.tile_n, p.mode, st);
    case 2: return vp_conv_launch_x3_f32(ctx, a, p.tile_n, p.mode, st);
    case 1: return vp_conv_launch_amp_f32(ctx, a, p.tile_n, p.mode, st);
    default: return vp_conv_launch_f32_f32(ctx, a, p.tile_n, p.mode, st);
    }
}

}  // extern "C"
