"""Float64 restatements of the training step's small kernels (csrc/train_ops.hip, csrc/se_train.hip), forward and backward, the
backwards as closed forms, and the inputs the tests plant (docs/train_ops.md).

Every operation takes `dt` (the dtype it computes in, float64 by default) and `rev` (walk every reduction backwards).  The exact
family's precondition is stated with them: evaluated in float32 in both orders the result is bit-identical to float64, so ANY
order of f32 accumulation -- the kernel's included -- must give exactly the float64 numbers
(tests/test_train_ops_oracle_cpu.py proves it for every planted case).

Two input families: 'exact' (small integers and dyadic rationals) and 'gauss' (standard normal, checked per element against
(n_terms + k) 2^-24 sum|terms|)."""
import numpy as np
import torch

U = 2.0 ** -24                       # half an ulp of 1.0f: the relative error of one float32 rounding
F32, F64 = np.float32, np.float64
GRID_CAP = 16384 * 256               # grid1d: at most 16 384 workgroups of 256 threads; beyond, the grid-stride loop runs again
DYADS = (0.25, 0.5, 0.75, 1.0, 2.0)

ACTS = {'relu': 1, 'sigmoid': 2, 'tanh': 3, 'hardtanh20': 4, 'silu': 5}      # VP_ACT_*


# ------------------------------------------------------------------------------------------------ helpers
def rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


def ints(g, shape, lo=-8, hi=8):
    return g.integers(lo, hi + 1, size=shape).astype(F32)


def dyads(g, shape, values=DYADS):
    return g.choice(np.asarray(values, F32), size=shape).astype(F32)


def gauss(g, shape):
    return g.standard_normal(size=shape).astype(F32)


def bf16(a):
    """Round to nearest even to bfloat16, returned in a's dtype (float64 values go through float32 first, as the kernels' do)."""
    a = np.asarray(a)
    r = torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(torch.bfloat16).to(torch.float32).numpy()
    return r.astype(a.dtype)


def seq_sum(a, axis, rev=False):
    """Sum along `axis` strictly in sequence (first to last, or last to first), in a's own dtype."""
    a = np.asarray(a)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis), a.dtype)
    if rev:
        a = np.flip(a, axis)
    return np.take(np.add.accumulate(a, axis=axis), -1, axis=axis)


def ulps(got, ref64):
    """|got - ref| in units of the float32 spacing at ref (got float32, ref float64)."""
    ref64 = np.asarray(ref64, F64)
    sp = np.spacing(np.abs(ref64).astype(F32)).astype(F64)
    return np.abs(np.asarray(got, F64) - ref64) / sp


# ------------------------------------------------------------------------------------------------ weight layouts
def weight_layouts(w):
    """w (Cout, Cin, KW) or (Cout, Cin, KF, KT) -> wp (Cout, KW*Cin), w2 (Cin, KW*Cout) by the kernel header's index formulas:
    tap j = kt*KF + kf (1-D: j = tap);  wp[o][j*Cin + c] = w[o][c][tap];  w2[c][(KW-1-j)*Cout + o] = w[o][c][tap]."""
    w = np.asarray(w)
    if w.ndim == 3:
        w = w[:, :, None, :]
    Cout, Cin, KF, KT = w.shape
    KW = KF * KT
    o, c, kf, kt = np.indices(w.shape)
    j = kt * KF + kf
    wp = np.full((Cout, KW * Cin), np.nan, w.dtype)
    w2 = np.full((Cin, KW * Cout), np.nan, w.dtype)
    wp[o, j * Cin + c] = w
    w2[c, (KW - 1 - j) * Cout + o] = w
    return wp, w2


LAYOUT_SHAPES = [(5, 3, 5), (64, 80, 5)]
LAYOUT_2D = [(3, 3), (1, 3), (3, 1), (1, 1)]


# ------------------------------------------------------------------------------------------------ bf16 weight panels
def prep_bf16(w, c0, nc):
    """w (rows, ld) f32, the column slice [c0, c0+nc) -> its bf16 copy (rows, nc) and bf16 transpose (nc, rows), as torch tensors."""
    t = torch.from_numpy(np.ascontiguousarray(w[:, c0:c0 + nc])).to(torch.bfloat16)
    return t.contiguous(), t.t().contiguous()


# (rows, ld, c0, nc, want_w16, want_wt16): edges first, then enough to reach 25 entries (two launches of at most 24)
PREP_ENTRIES = [(65, 1, 0, 1, True, True), (1, 65, 0, 65, True, True), (130, 70, 0, 70, True, True), (70, 200, 8, 100, True, True),
                (64, 64, 0, 64, True, False), (33, 130, 2, 128, False, True)] + \
               [(3 + 5 * i, 4 + 7 * i, i % 3, 4 + 7 * i - (i % 3) - (i % 2), True, True) for i in range(19)]


# ------------------------------------------------------------------------------------------------ optimisers
OPT_SIZES = [1, 255, GRID_CAP + 3 * 256 + 5]
OPT_STEPS = [1, 2, 1000]


def beta_pow32(beta, step):
    """1 - beta^t the way the entry point forms it: float32 powf, float32 subtraction."""
    return F32(1.0) - np.power(F32(beta), F32(step), dtype=F32)


def adam(p, g, m, v, lr, b1, b2, eps, wd, step, gscale, decoupled=False, dt=F64):
    """One Adam step (coupled L2: g += wd p) or AdamW step (decoupled: p *= 1 - lr wd first, the moments never see it).
    -> update p_new - p_old, m_new, v_new.  Scalars enter as their float32 values; 1 - beta^t and AdamW's keep factor are formed in
    float32 as the entry point's host code forms them."""
    f = lambda s: dt(F32(s))
    p, g, m, v = (np.asarray(a, dt) for a in (p, g, m, v))
    c1, c2 = dt(beta_pow32(b1, step)), dt(beta_pow32(b2, step))
    keep = dt(F32(1.0) - F32(lr) * F32(wd)) if decoupled else dt(1.0)
    wdc = dt(0.0) if decoupled else f(wd)
    om1, om2 = dt(F32(1.0) - F32(b1)), dt(F32(1.0) - F32(b2))
    gr = g * f(gscale) + wdc * p
    mn = f(b1) * m + om1 * gr
    vn = f(b2) * v + om2 * gr * gr
    pn = p * keep - f(lr) * (mn / c1) / (np.sqrt(vn / c2) + f(eps))
    return pn - p, mn, vn


def adam_bounds(p, g, m, v, lr, b1, b2, eps, wd, step, gscale, decoupled=False, exact_moments=False):
    """Per-element bounds (update, m, v) that hold for any float32 evaluation of adam(): (roundings) x 2^-24 x sum|terms|.
    m: g * gscale, wd * p, their sum, 1 - b1, two products, one sum = 7 roundings.  v: the same with gr * gr = 10.
    update: through m, plus 5 for sqrt(v / c2) (half of v's 10), plus m / c1, v / c2, sqrt, + eps, the quotient, lr *, an ulp of
    powf's beta^t and slack = 16 on the step's magnitude, plus the roundings of p * keep and of p_new on their own magnitude.
    exact_moments (the exact family: dyadic hyper-parameters, m and v exact, beta^t exact or underflowed, lr a power of two): the update
    has five inexact steps on the step itself (m / c1, v / c2, sqrt, + eps, the quotient) and one on p_new: 5 ulps of |step| plus
    1 ulp of |p_new|, an ulp taken at its largest, 2^-23 of the value."""
    _, mn, vn = adam(p, g, m, v, lr, b1, b2, eps, wd, step, gscale, decoupled)
    ap, ag, am, av = (np.abs(np.asarray(a, F64)) for a in (p, g, m, v))
    c1, c2 = F64(beta_pow32(b1, step)), F64(beta_pow32(b2, step))
    gr = ag * abs(gscale) + (0.0 if decoupled else abs(wd)) * ap
    em = 7 * U * (b1 * am + (1 - b1) * gr)
    ev = 10 * U * (b2 * av + (1 - b2) * gr * gr)
    den = np.sqrt(vn / c2) + F64(F32(eps))
    mag = lr * np.abs(mn) / c1 / den
    if exact_moments:
        upd = adam(p, g, m, v, lr, b1, b2, eps, wd, step, gscale, decoupled)[0]
        return 10 * U * mag + 2 * U * np.abs(np.asarray(p, F64) + upd), em * 0, ev * 0
    return lr * em / (c1 * den) + 16 * U * mag + 2 * U * (ap + mag), em, ev


# dyadic hyper-parameters: with integer p, g, m and v >= 0 the moments (and every momentum quantity) are exact in float32
EXACT_OPT = dict(lr=0.125, b1=0.5, b2=0.75, eps=2.0 ** -10, gscale=0.5)
GAUSS_OPT = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, gscale=0.37)


def opt_inputs(n, family):
    """p, g, m, v (v >= 0) of n elements; long buffers repeat a block of 4093."""
    g_ = rng(n, 12)
    k = min(n, 4093)
    if family == 'exact':
        blk = [ints(g_, k), ints(g_, k), ints(g_, k), ints(g_, k, 0, 8)]
    else:
        blk = [gauss(g_, k), gauss(g_, k), gauss(g_, k) * F32(0.1), gauss(g_, k) ** 2 * F32(0.01)]
    return [np.resize(b, n) for b in blk]


def momentum(p, g, vel, lr, mu, wd, nesterov, gscale, dt=F64):
    """paddle Momentum / SGD (mu = 0): g += wd p; vel = mu vel + g; p -= lr vel, or lr (g + mu vel) with Nesterov.  -> update, vel."""
    f = lambda s: dt(F32(s))
    p, g, vel = (np.asarray(a, dt) for a in (p, g, vel))
    gr = g * f(gscale) + f(wd) * p
    vn = f(mu) * vel + gr
    pn = p - f(lr) * (gr + f(mu) * vn if nesterov else vn)
    return pn - p, vn


def momentum_bounds(p, g, vel, lr, mu, wd, nesterov, gscale):
    """(update, velocity) bounds for any float32 evaluation of momentum(): vel costs 5 roundings on mu |vel| + |g gscale| + |wd p|;
    the update at most 9 on lr times its terms, plus p_new's own rounding."""
    ap, ag, av = (np.abs(np.asarray(a, F64)) for a in (p, g, vel))
    gr = ag * abs(gscale) + abs(wd) * ap
    a_v = mu * av + gr
    a_u = gr + mu * a_v if nesterov else a_v
    return 9 * U * lr * a_u + U * ap, 5 * U * a_v


# ------------------------------------------------------------------------------------------------ gradient packing
def pack_segments(dst, srcs, offs, sizes):
    """dst[off : off + n] = src[:n], zeros where src is None; everything else keeps its value."""
    out = np.array(dst, copy=True)
    for s, o, n in zip(srcs, offs, sizes):
        out[o:o + n] = 0.0 if s is None else s[:n]
    return out


# ------------------------------------------------------------------------------------------------ reflect fold, zero insertion
FOLD_TP = [(1, 0), (2, 1), (5, 4), (5, 2), (6, 3), (40, 4)]
FOLD_C = [4, 68]
FOLD_B = 3


def reflect_fold(dxp, T, pad, add=None, dt=F64, rev=False):
    """Adjoint of reflect padding along time: dxp (B, T + 2 pad, C) -> dx (B, T, C).  Padded frame j < pad is a copy of frame pad - j,
    padded frame T + pad + k (k < pad) of frame T - 2 - k: each frame's gradient is its own plus its mirror images' (a frame can have
    both when T <= 2 pad).  -> dx, and dx + add when add is given."""
    dxp = np.asarray(dxp, dt)
    B, Tp, C = dxp.shape
    assert Tp == T + 2 * pad and 0 <= pad < T
    terms = np.zeros((3, B, T, C), dt)
    terms[0] = dxp[:, pad:pad + T]
    for j in range(pad):
        terms[1, :, pad - j] = dxp[:, j]
        terms[2, :, T - 2 - j] = dxp[:, T + pad + j]
    dx = seq_sum(terms, 0, rev)
    if add is None:
        return dx
    return dx, dx + np.asarray(add, dt)


ZI_STRIDES = [(1, 1), (2, 2), (1, 2), (2, 1)]
ZI_IN_OUT = [(7, 4), (8, 4), (7, 3)]
ZI_C = [4, 36]


def zero_insert(dz, T_in, F_in, st, sf):
    """dz (B, T_out, F_out, C) -> up (B, T_in, F_in, C): up[b, t, f] = dz[b, t/st, f/sf] where st | t, sf | f and the quotient is in
    range, else 0 -- the adjoint of x[:, ::st, ::sf][:, :T_out, :F_out]."""
    dz = np.asarray(dz)
    B, T_out, F_out, C = dz.shape
    up = np.zeros((B, T_in, F_in, C), dz.dtype)
    nt = min(T_out, -(-T_in // st))
    nf = min(F_out, -(-F_in // sf))
    up[:, 0:nt * st:st, 0:nf * sf:sf] = dz[:, :nt, :nf]
    return up


# ------------------------------------------------------------------------------------------------ SE gate backward, utterance dots
SRB_SIMPLE_C, SRB_SIMPLE_T = [5, 64, 70], [1, 3, 4, 9]
SRB_CHUNK_C = [4, 12, 40, 1024]
SRB_B = 3


def srb_geometry(B, T, C):
    """(row groups RG, rows per chunk, chunks) of vp_scale_rows_bwd_ws_f32: CL = the power of two >= C/4 lanes across a row, RG = 256 / CL
    rows in flight, chunks of max(ceil(T / (2048 / B)), 8 RG) rows."""
    cl = 0
    while (1 << cl) < C // 4 and cl < 8:
        cl += 1
    RG = 256 >> cl
    ch = max(1, 2048 // B)
    rpc = max(-(-T // ch), 8 * RG)
    return RG, rpc, -(-T // rpc)


def srb_chunk_T(B, C):
    """T that reach: one row; exactly the four-row trip (twice); its tail; a last chunk with fewer rows than row groups."""
    RG, _, _ = srb_geometry(B, 1, C)
    T3 = 2 * 8 * RG + RG - 1                       # rpc = 8 RG while T <= 8 RG * (2048 / B)
    assert srb_geometry(B, T3, C)[1] == 8 * RG
    return [1, 8 * RG, 8 * RG + 1, T3]


def scale_rows_bwd(dy, x, s, dt=F64, rev=False):
    """out = x * s[b]: dx = dy * s[b], ds[b, c] = sum_t dy * x.  dy, x (B, T, C); s (B, C)."""
    dy, x, s = (np.asarray(a, dt) for a in (dy, x, s))
    return dy * s[:, None, :], seq_sum(dy * x, 1, rev)


UTT_T = [1, 7, 8, 9, 25, 32, 33, 57]
UTT_C = [4, 128, 132]
UTT_B = 2


def bn_apply_bf16(z, scale, shift):
    """bf16(fma(z, scale, shift)): the exact z * scale + shift (float64 holds it) rounded once to float32, then to bf16."""
    return bf16((np.asarray(z, F64) * np.asarray(scale, F64) + np.asarray(shift, F64)).astype(F32))


def utt_dot(dy, x, scale=None, shift=None, dt=F64, rev=False):
    """ds[b, c] = sum_t dy * x; with scale / shift, x is bf16(fma(z, scale, shift)) of the bf16 z handed in (the BatchNorm apply pass
    folded into the read: one float32 rounding of the exact z * scale + shift, then bf16)."""
    dy, x = np.asarray(dy, dt), np.asarray(x, dt)
    if scale is not None:
        x = bn_apply_bf16(x, scale, shift).astype(dt)
    return seq_sum(dy * x, 1, rev)


def scale_shift_rows(dy, s, dm, T, dt=F64):
    """dx[b, t, c] = dy * s[b, c] + dm[b, c] * (1/T), 1/T the float32 quotient the entry point passes to its kernel."""
    dy, s, dm = (np.asarray(a, dt) for a in (dy, s, dm))
    inv_t = dt(F32(1.0) / F32(T))
    return dy * s[:, None, :] + (dm * inv_t)[:, None, :]


# ------------------------------------------------------------------------------------------------ activations
PLANTED_X = np.asarray([0.0, 2.0 ** -126, -2.0 ** -126, 1.0, -1.0, 20.0 - 2.0 ** -19, 20.0, 20.0 + 2.0 ** -19, 30.0, -30.0, 100.0, -100.0],
                       F32)
ACT_BIG_N = 4 * GRID_CAP + 8


def act(kind, x, dt=F64):
    x = np.asarray(x, dt)
    one = dt(1.0)
    with np.errstate(over='ignore'):
        if kind == 'tanh':
            return np.tanh(x)
        if kind == 'sigmoid':
            return one / (one + np.exp(-x))
        if kind == 'relu':
            return np.maximum(x, dt(0.0))
        if kind == 'hardtanh20':
            return np.minimum(np.maximum(x, dt(0.0)), dt(20.0))
        if kind == 'silu':
            return x / (one + np.exp(-x))
    raise ValueError(kind)


def act_bwd(kind, dy, y, dt=F64):
    """dz from dy and the OUTPUT y (SiLU: the input).  ReLU'(0) = 0; hardtanh20' = 0 where the output is exactly 0 or 20."""
    dy, y = np.asarray(dy, dt), np.asarray(y, dt)
    one = dt(1.0)
    with np.errstate(over='ignore'):
        if kind == 'tanh':
            return dy * (one - y * y)
        if kind == 'sigmoid':
            return dy * (y * (one - y))
        if kind == 'relu':
            return np.where(y > 0, dy, dt(0.0))
        if kind == 'hardtanh20':
            return np.where((y > 0) & (y < 20), dy, dt(0.0))
        if kind == 'silu':
            sg = one / (one + np.exp(-y))
            return dy * (sg * (one + y * (one - sg)))
    raise ValueError(kind)


def act_f32(kind, x):
    """The same formulas restated in float32 on the CPU (torch.tanh; 1 / (1 + exp(-x)) in float32): what float32 itself costs."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=F32))
    if kind == 'tanh':
        return torch.tanh(t).numpy()
    if kind == 'sigmoid':
        return (1.0 / (1.0 + torch.exp(-t))).numpy()
    if kind == 'silu':
        return (t / (1.0 + torch.exp(-t))).numpy()
    return act(kind, x, F32)


def silu_bwd_f32(dy, x):
    dy, x = (torch.from_numpy(np.ascontiguousarray(a, dtype=F32)) for a in (dy, x))
    sg = 1.0 / (1.0 + torch.exp(-x))
    return (dy * (sg * (1.0 + x * (1.0 - sg)))).numpy()


REL_FLOOR = 2.0 ** -100


def silu_bwd_bound(x):
    """(measured, per-element bound per unit dy) for the SiLU derivative sg (1 + x (1 - sg)): its error scales with sg (1 + |x|), the size
    of its two terms, so the float32 CPU restatement's worst error is measured in that unit (plus the 2^-100 floor that keeps the
    subnormal sg of x = -100 out of a relative measure) and allowed four times over, element by element."""
    x64 = np.asarray(x, F64)
    with np.errstate(over='ignore'):
        scale = (1.0 + np.abs(x64)) / (1.0 + np.exp(-x64)) + REL_FLOOR
    one = np.ones_like(np.asarray(x, F32))
    m = float(np.max(np.abs(silu_bwd_f32(one, x) - act_bwd('silu', one, x)) / scale))
    return m, 4.0 * m * scale


def act_bwd_exact_inputs(kind):
    """(y or x, dy) of the exact family for the backward: integer dy; for tanh and sigmoid a dyadic y, so that dy (1 - y^2) and
    dy y (1 - y) are exact; for the others the values the forward block produces (SiLU: the inputs)."""
    g = rng(ord(kind[0]), 33)
    dy = ints(g, 4093)
    if kind == 'sigmoid':
        return dyads(g, 4093, (0.0, 0.25, 0.5, 0.75, 1.0)), dy
    if kind == 'tanh':
        return dyads(g, 4093, (-1.0, -0.5, 0.0, 0.25, 0.75, 1.0)), dy
    x = act_inputs(4093, 2)
    return (x if kind == 'silu' else act(kind, x).astype(F32)), dy


def rel_err(got, ref64):
    """|got - ref| / (|ref| + 2^-100): relative, with a floor that keeps results in the float32 subnormals (SiLU(-100)) out of it."""
    ref64 = np.asarray(ref64, F64)
    return np.abs(np.asarray(got, F64) - ref64) / (np.abs(ref64) + REL_FLOOR)


def act_bound(kind, x):
    """(measured, bound): the worst rel_err of the float32 CPU restatement over these inputs, and four times it -- the margin for the
    GPU's own expf / tanhf.  Never taken from a kernel's output."""
    m = float(np.max(rel_err(act_f32(kind, x), act(kind, x))))
    return m, 4.0 * m


def act_inputs(n, seed):
    """n values: the planted ones first, Gaussian (sigma 4, so the sigmoid's whole range is met) after; long inputs repeat a block of
    4093 (a prime: the block never lines up with the float4 lanes or the grid)."""
    block = np.concatenate([PLANTED_X, gauss(rng(seed), 4093 - len(PLANTED_X)) * F32(4.0)])
    return np.resize(block, n).astype(F32)


# ------------------------------------------------------------------------------------------------ AFF combine
AFF_SHAPES = [(1, 4), (37, 68)]


def aff_combine(t, x, y, dt=F64):
    t, x, y = (np.asarray(a, dt) for a in (t, x, y))
    return x * (dt(1.0) + t) + y * (dt(1.0) - t)


def aff_combine_bwd(g, t, x, y, dt=F64):
    g, t, x, y = (np.asarray(a, dt) for a in (g, t, x, y))
    return g * (dt(1.0) + t), g * (dt(1.0) - t), g * (x - y)


# ------------------------------------------------------------------------------------------------ CAM++ segment context / scale
SEG_LENS = [100, 4]
SEG_C = [4, 64, 68]
SEG_B = 2


def seg_T(seg):
    return sorted({1, 3, seg - 1, seg, seg + 1, 2 * seg, 2 * seg + 37})


def _segments(T, seg):
    return [(t0, min(T, t0 + seg)) for t0 in range(0, T, seg)]


def seg_ctx(x, seg, dt=F64, rev=False):
    """ctx[b, s, c] = mean_t x + mean_{t in segment s} x, the last segment over its valid frames only.  x (B, T, C)."""
    x = np.asarray(x, dt)
    T = x.shape[1]
    sums = np.stack([seq_sum(x[:, a:b], 1, rev) for a, b in _segments(T, seg)], 1)
    lens = np.asarray([b - a for a, b in _segments(T, seg)], dt)
    return sums / lens[None, :, None] + (seq_sum(sums, 1, rev) / dt(T))[:, None, :]


def seg_ctx_bwd(dctx, T, seg, dt=F64, rev=False):
    """dx[b, t, c] = sum_s dctx[b, s, c] / T + dctx[b, seg(t), c] / len(seg(t))."""
    dctx = np.asarray(dctx, dt)
    tot = seq_sum(dctx, 1, rev) / dt(T)
    dx = np.empty((dctx.shape[0], T, dctx.shape[2]), dt)
    for s, (a, b) in enumerate(_segments(T, seg)):
        dx[:, a:b] = (tot + dctx[:, s] / dt(b - a))[:, None, :]
    return dx


def seg_dctx(B, T, C, seg, family):
    """The gradient handed to seg_ctx_bwd: non-negative integers (its two terms then cannot cancel), or Gaussian."""
    r = rng(T, C, seg, 12)
    shape = (B, -(-T // seg), C)
    return ints(r, shape, 0, 8) if family == 'exact' else gauss(r, shape)


def seg_scale(y, m, seg, dt=F64):
    """out[b, t, c] = y[b, t, c] * m[b, seg(t), c]."""
    y, m = np.asarray(y, dt), np.asarray(m, dt)
    return y * np.repeat(m, seg, axis=1)[:, :y.shape[1]]


def seg_scale_bwd(g, y, m, seg, dt=F64, rev=False):
    """dy = g * m[b, seg(t)], dm[b, s, c] = sum_{t in s} g * y."""
    g, y, m = (np.asarray(a, dt) for a in (g, y, m))
    T = y.shape[1]
    dm = np.stack([seq_sum((g * y)[:, a:b], 1, rev) for a, b in _segments(T, seg)], 1)
    return g * np.repeat(m, seg, axis=1)[:, :T], dm


# ------------------------------------------------------------------------------------------------ SE dense layers
SE_SHAPES = [(4, 4), (64, 12), (516, 96), (1024, 1024), (80, 1000)]
SE_B = [1, 5]


def _rb(a, rnd):
    return bf16(a) if rnd else a


def se_dense_fwd(mean, w1, b1, w2, b2, rnd=0, dt=F64, rev=False):
    """a = ReLU(W1 mean + b1), s = sigmoid(W2 a + b2); rnd: mean, the weights and a are rounded to bf16 where they enter a product
    (the a that is RETURNED is not rounded).  mean (B, C), W1 (H, C), W2 (C, H).  -> a, z2 + b2 (the sigmoid's argument), s."""
    mean, w1, b1, w2, b2 = (np.asarray(v, dt) for v in (mean, w1, b1, w2, b2))
    z1 = seq_sum(_rb(w1, rnd)[None] * _rb(mean, rnd)[:, None, :], 2, rev)
    a = np.maximum(z1 + b1, dt(0.0))
    z2 = seq_sum(_rb(w2, rnd)[None] * _rb(a, rnd)[:, None, :], 2, rev) + b2
    return a, z2, dt(1.0) / (dt(1.0) + np.exp(-z2))


def se_dense_bwd(ds, mean, a, s, w1, w2, rnd=0, dt=F64, rev=False):
    """From d s and the saved a, s: dz2 = ds s (1 - s); da = W2^T dz2; dz1 = da [a > 0]; dmean = W1^T dz1;
    dW2 = dz2^T a, db2 = sum_b dz2, dW1 = dz1^T mean, db1 = sum_b dz1 (the biases from the unrounded dz).
    -> dmean, dW1, db1, dW2, db2."""
    ds, mean, a, s, w1, w2 = (np.asarray(v, dt) for v in (ds, mean, a, s, w1, w2))
    dz2 = ds * s * (dt(1.0) - s)
    da = seq_sum(_rb(w2, rnd)[None] * _rb(dz2, rnd)[:, :, None], 1, rev)            # (B, C, H) over C
    dz1 = np.where(a > 0, da, dt(0.0))
    dmean = seq_sum(_rb(w1, rnd)[None] * _rb(dz1, rnd)[:, :, None], 1, rev)         # (B, H, C) over H
    dw2 = seq_sum(_rb(dz2, rnd)[:, :, None] * _rb(a, rnd)[:, None, :], 0, rev)
    dw1 = seq_sum(_rb(dz1, rnd)[:, :, None] * _rb(mean, rnd)[:, None, :], 0, rev)
    return dmean, dw1, seq_sum(dz1, 0, rev), dw2, seq_sum(dz2, 0, rev)


def se_fwd_inputs(B, C, H, family):
    g = rng(B, C, H, 1)
    if family == 'exact':
        mean, w1, b1 = ints(g, (B, C), -4, 4), ints(g, (H, C), -2, 2), ints(g, H, -3, 3)
        a = se_dense_fwd(mean, w1, b1, np.zeros((C, H)), np.zeros(C))[0]
        # W2 in {-1, 0, 1} / 2^k, k chosen so that the sigmoid's argument is O(4): a power of two keeps every product exact
        k = int(np.ceil(np.log2(max(1.0, float(np.abs(a).max()) * np.sqrt(H) / 4))))
        return mean, w1, b1, ints(g, (C, H), -1, 1) * F32(2.0 ** -k), ints(g, C, -2, 2) * F32(0.5)
    return (gauss(g, (B, C)), gauss(g, (H, C)) / F32(np.sqrt(C)), gauss(g, H), gauss(g, (C, H)) / F32(np.sqrt(H)), gauss(g, C))


def se_bwd_inputs(B, C, H, family):
    g = rng(B, C, H, 2)
    if family == 'exact':
        return (ints(g, (B, C), -2, 2), ints(g, (B, C), -4, 4), ints(g, (B, H), 0, 4), dyads(g, (B, C), (0.25, 0.5, 0.75)),
                ints(g, (H, C), -1, 1), ints(g, (C, H), -1, 1))
    mean, w1, b1, w2, b2 = se_fwd_inputs(B, C, H, 'gauss')
    a, _, s = se_dense_fwd(mean, w1, b1, w2, b2)
    return gauss(g, (B, C)), mean, a.astype(F32), s.astype(F32), w1, w2


BF_FLIP = 2.0 ** -7                  # one bf16 ulp, relative: what a rounding that falls the other way on an inexact value moves


def se_fwd_bounds(mean, w1, b1, w2, b2, rnd=0):
    """Per-element bounds (a, the sigmoid's argument) for any float32 evaluation of se_dense_fwd: (C + 2) 2^-24 sum|terms| for a,
    (H + 2) 2^-24 sum|terms| plus a's inherited bound for the argument.  rnd: mean and the weights are rounded from the inputs (no
    freedom), but a is inexact when it is rounded: one bf16 ulp of |a| more."""
    am, aw1, ab1, aw2, ab2 = (np.abs(np.asarray(v, F64)) for v in (_rb(mean, rnd), _rb(w1, rnd), b1, _rb(w2, rnd), b2))
    aa = am @ aw1.T + ab1
    ea = (mean.shape[1] + 2) * U * aa
    return ea, (w1.shape[0] + 2) * U * (aa @ aw2.T + ab2) + (ea + (BF_FLIP * aa if rnd else 0.0)) @ aw2.T


def se_bwd_bounds(ds, mean, a, s, w1, w2, rnd=0):
    """Per-element bounds for any float32 evaluation of se_dense_bwd, (terms + roundings) 2^-24 sum|terms| propagated down
    the chain: dz2 costs 3 roundings, each matrix product its length + 1, and every later quantity inherits its operand's bound.
    rnd: dz2 and dz1 are inexact when they are rounded to bf16, so each rounding may fall the other way: one bf16 ulp (2^-7
    relative) of the rounded operand more, inherited likewise (the biases sum the unrounded dz: db2 has none, db1 inherits dz2's)."""
    ds, mean, a, s, w1, w2 = (np.abs(np.asarray(v, F64)) for v in (ds, _rb(mean, rnd), _rb(a, rnd), s, _rb(w1, rnd), _rb(w2, rnd)))
    B, C = ds.shape
    H = a.shape[1]
    f = BF_FLIP if rnd else 0.0
    adz2 = ds * s * (1.0 + s)
    ada = np.where(a > 0, adz2 @ w2, 0.0)                        # (B, H): sum_c |W2[c, h]| |dz2[c]|, masked like dz1
    return (((H + C + 5) * U + 2 * f) * (ada @ w1), ((B + C + 5) * U + 2 * f) * np.einsum('bh,bc->hc', ada, mean),
            ((B + C + 4) * U + f) * ada.sum(0), ((B + 4) * U + f) * np.einsum('bc,bh->ch', adz2, a), (B + 3) * U * adz2.sum(0))


# ------------------------------------------------------------------------------------------------ planted inputs per operation
def btc(B, T, C, family, key, n, nonneg=False):
    """n tensors (B, T, C) of the family."""
    g = rng(B, T, C, key)
    if family == 'exact':
        return [ints(g, (B, T, C), 0 if nonneg else -8, 8) for _ in range(n)]
    return [np.abs(gauss(g, (B, T, C))) if nonneg else gauss(g, (B, T, C)) for _ in range(n)]


def gates(B, C, family, key, nseg=None):
    g = rng(B, C, key, 77)
    shape = (B, C) if nseg is None else (B, nseg, C)
    return dyads(g, shape) if family == 'exact' else gauss(g, shape)


def bf16_operand(B, T, C, family, key):
    """A (B, T, C) tensor stored as bf16: integers <= 256 in magnitude (exact in bf16), or Gaussian rounded to bf16."""
    g = rng(B, T, C, key, 16)
    return ints(g, (B, T, C), -256, 256) if family == 'exact' else bf16(gauss(g, (B, T, C)))


def bn_affine(C, family, key):
    """scale, shift of the folded BatchNorm: dyadic scale and integer shift (fma(z, scale, shift) is then exact, its bf16 rounding plain
    round-to-nearest-even), or Gaussian."""
    g = rng(C, key, 5)
    if family == 'exact':
        return dyads(g, C), ints(g, C, -4, 4)
    return gauss(g, C), gauss(g, C)


def exact_cases():
    """Every planted exact-family case with a reduction or a product in it: (id, function of (dt, rev) -> tuple of arrays, rounded).
    The CPU test evaluates each in float32 forwards, float32 backwards and float64 and demands bit-identical results; `rounded` marks the
    one formula that ends in a single rounding of an exact value (dy * s + dm / T with dm a power of two and 1/T taken as float32): there
    float32 must equal the float64 result rounded to nearest even."""
    out = []

    def add(name, fn, rounded=False):
        out.append((name, fn, rounded))

    for (T, pad) in FOLD_TP:
        for C in FOLD_C:
            dxp, = btc(FOLD_B, T + 2 * pad, C, 'exact', 3, 1)
            ad, = btc(FOLD_B, T, C, 'exact', 4, 1)
            add(f'fold-T{T}-p{pad}-C{C}', lambda dt, rev, dxp=dxp, ad=ad, T=T, pad=pad: reflect_fold(dxp, T, pad, ad, dt=dt, rev=rev))
    srb = [(C, T) for C in SRB_SIMPLE_C for T in SRB_SIMPLE_T] + [(C, T) for C in SRB_CHUNK_C for T in srb_chunk_T(SRB_B, C)]
    for C, T in srb:
        dy, x = btc(SRB_B, T, C, 'exact', 5, 2)
        s = gates(SRB_B, C, 'exact', 5)
        add(f'scale_rows_bwd-C{C}-T{T}', lambda dt, rev, dy=dy, x=x, s=s: scale_rows_bwd(dy, x, s, dt=dt, rev=rev))
    for T in UTT_T:
        for C in UTT_C:
            dy, x = btc(UTT_B, T, C, 'exact', 6, 2)
            z = bf16_operand(UTT_B, T, C, 'exact', 6)
            sc, sh = bn_affine(C, 'exact', 6)
            s, dm = gates(UTT_B, C, 'exact', 7), dyads(rng(T, C, 8), (UTT_B, C), (1.0, 2.0, 4.0, 0.5))
            add(f'utt_dot-T{T}-C{C}', lambda dt, rev, dy=dy, x=x: (utt_dot(dy, x, dt=dt, rev=rev),))
            add(f'utt_dot_x16-T{T}-C{C}', lambda dt, rev, dy=dy, z=z: (utt_dot(dy, z, dt=dt, rev=rev),))
            add(f'utt_dot_z16-T{T}-C{C}', lambda dt, rev, dy=dy, z=z, sc=sc, sh=sh: (utt_dot(dy, z, sc, sh, dt=dt, rev=rev),))
            add(f'scale_shift_rows-T{T}-C{C}', lambda dt, rev, dy=dy, s=s, dm=dm, T=T: (scale_shift_rows(dy, s, dm, T, dt=dt),), rounded=True)
    for rows, C in AFF_SHAPES:
        g = rng(rows, C, 9)
        gg, x, y, t = ints(g, (rows, C)), ints(g, (rows, C)), ints(g, (rows, C)), dyads(g, (rows, C), (-0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75))
        add(f'aff-{rows}x{C}', lambda dt, rev, gg=gg, t=t, x=x, y=y: (aff_combine(t, x, y, dt),) + aff_combine_bwd(gg, t, x, y, dt))
    for seg in SEG_LENS:
        for T in seg_T(seg):
            for C in SEG_C + [5]:
                nseg = -(-T // seg)
                g, y = btc(SEG_B, T, C, 'exact', 10, 2)
                m = gates(SEG_B, C, 'exact', 10, nseg)
                add(f'seg_scale-s{seg}-T{T}-C{C}', lambda dt, rev, g=g, y=y, m=m, seg=seg:
                    (seg_scale(y, m, seg, dt),) + seg_scale_bwd(g, y, m, seg, dt=dt, rev=rev))
                x, = btc(SEG_B, T, C, 'exact', 11, 1, nonneg=True)
                add(f'seg_ctx_sums-s{seg}-T{T}-C{C}', lambda dt, rev, x=x, seg=seg: seg_ctx_sums(x, seg, dt, rev))
                dctx = seg_dctx(SEG_B, T, C, seg, 'exact')
                add(f'seg_ctx_bwd_sum-s{seg}-T{T}-C{C}', lambda dt, rev, dctx=dctx: (seq_sum(np.asarray(dctx, dt), 1, rev),))
    for kind in ('tanh', 'sigmoid'):
        v, dy = act_bwd_exact_inputs(kind)
        add(f'act_bwd-{kind}', lambda dt, rev, kind=kind, v=v, dy=dy: (act_bwd(kind, dy, v, dt),))
    for n in OPT_SIZES:
        p, g, m, v = (a[:4093] for a in opt_inputs(n, 'exact'))           # the long buffer repeats this block
        for wd in (0.0, 0.25):
            kw = dict(EXACT_OPT, wd=wd)
            add(f'adam-moments-n{n}-wd{wd}', lambda dt, rev, a=(p, g, m, v), kw=kw: adam(*a, step=2, dt=dt, **kw)[1:])
            add(f'adamw-moments-n{n}-wd{wd}', lambda dt, rev, a=(p, g, m, v), kw=kw: adam(*a, step=2, decoupled=True, dt=dt, **kw)[1:])
            for nest in (0, 1):
                add(f'momentum-n{n}-wd{wd}-nest{nest}', lambda dt, rev, a=(p, g, m), wd=wd, nest=nest:
                    momentum(*a, lr=0.125, mu=0.5, wd=wd, nesterov=nest, gscale=0.5, dt=dt))
    for C, H in SE_SHAPES:
        for B in SE_B:
            for rnd in (0, 1):
                fi, bi = se_fwd_inputs(B, C, H, 'exact'), se_bwd_inputs(B, C, H, 'exact')
                add(f'se_fwd-C{C}-H{H}-B{B}-r{rnd}', lambda dt, rev, fi=fi, rnd=rnd: se_dense_fwd(*fi, rnd=rnd, dt=dt, rev=rev)[:2])
                add(f'se_bwd-C{C}-H{H}-B{B}-r{rnd}', lambda dt, rev, bi=bi, rnd=rnd: se_dense_bwd(*bi, rnd=rnd, dt=dt, rev=rev))
    return out


def seg_ctx_sums(x, seg, dt, rev):
    """The exact part of seg_ctx (segment sums and their total) -- the two divisions and the sum after them are its three inexact steps."""
    x = np.asarray(x, dt)
    sums = np.stack([seq_sum(x[:, a:b], 1, rev) for a, b in _segments(x.shape[1], seg)], 1)
    return sums, seq_sum(sums, 1, rev)
