"""Oracle (CPU, float64 NumPy) of the BatchNorm training unit of csrc/bn_train.hip, and the inputs that put its kernels to work.
Test helper, not a test module; imports nothing of the engine.  docs/bn_train.md has the entry-point table and the bounds.

Forward (utils.py:96-119, batch statistics over the M rows of a (M, C) tensor):
    mean;  var = biased variance;  invstd = 1 / sqrt(var + eps);  scale = gamma invstd;  shift = beta - mean scale;
    y = z scale + shift, then nothing / max(., 0) / min(max(., 0), 20);  running = mom running + (1 - mom) batch, biased variance.
Backward, zhat = (z - mean) invstd:
    dz = [front] gamma invstd (g - sum g / M - zhat sum (g zhat) / M),  g = [behind] dy,  dbeta = sum g,  dgamma = sum g zhat,  dbias = sum dz
    front  = z > 0                       (a ReLU in FRONT of the BatchNorm: TDNNBlock's conv -> ReLU -> BN; it masks dz, not the sums)
    behind = 0 < z ms + mh [< mask_hi]   (a ReLU or Hardtanh(0, 20) BEHIND it; z ms + mh as the forward's one f32 fused multiply-add)
Every function takes float64 images of the f32 / bf16 numbers a kernel reads.

`stats_f32` is NOT a reference: float32 NumPy restatements of four ways to the variance -- (a) raw sums of x and x^2, (b) two passes,
(c) sums of x - x[0] and its square, (d) the same about the mean of the first eight rows -- that say how far ANY f32 implementation of each formula lies from float64.
"""
import functools
import types

import numpy as np

EPS = float(np.float32(1e-5))
MOM = float(np.float32(0.9))
ONE_MINUS_MOM = float(np.float32(1.0) - np.float32(0.9))       # what the kernel blends with: 1.f - momentum in f32
U24 = 2.0 ** -24

R_SWEEP = (0, 3, 10, 30, 100)
M_SWEEP = (2, 6, 19, 48, 777, 4097)
# bound 4 of the issue: what BNRows (centred input) holds at every r; the raw-sum paths are held to one_pass_bound
INVSTD_BOUND, MEAN_BOUND, VAR_REL, VAR_MEAN2, Y_BOUND = 2e-6, 2e-6, 4e-6, 1e-12, 2e-6
F32_L2, SUM_BOUND = 2e-6, 2e-6

# planted channels of `conditioned`
CH_CONST, CH_JITTER, CH_ZERO, CH_OUTLIER = 1, 2, 3, 4
CONST = -3.7
JITTER = 1.25


# ---------------------------------------------------------------------------------------------------- number formats
def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def bf16_round(a):
    """Round-to-nearest-even to bf16 of the f32 image of a (finite values); -> float32 array holding bf16 numbers."""
    u = f32(a).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def bf16_ulp(v):
    """Spacing of bf16 at |v| (8 significant bits; the smallest normal's below 2^-126)."""
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)


def fma32(a, b, c):
    """a * b + c rounded once to f32 (a, b, c f32 numbers: the product is exact in float64)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- forward
def clamp(y, act):
    return y if act == 0 else (np.maximum(y, 0.0) if act == 1 else np.minimum(np.maximum(y, 0.0), 20.0))


def finalize(mean, var, M, gamma=None, beta=None, eps=EPS, run_mean=None, run_var=None, mom=MOM, one_minus_mom=None):
    C = mean.shape[0]
    g = np.ones(C) if gamma is None else np.asarray(gamma, np.float64)
    b = np.zeros(C) if beta is None else np.asarray(beta, np.float64)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = g * invstd
    om = 1.0 - mom if one_minus_mom is None else one_minus_mom
    return types.SimpleNamespace(
        mean=mean, var=var, invstd=invstd, scale=scale, shift=b - mean * scale, beta=b, M=M,
        run_mean=None if run_mean is None else mom * np.asarray(run_mean, np.float64) + om * mean,
        run_var=None if run_var is None else mom * np.asarray(run_var, np.float64) + om * var)


def forward(z, gamma=None, beta=None, eps=EPS, act=0, run_mean=None, run_var=None, mom=MOM, one_minus_mom=None):
    z = np.asarray(z, np.float64)
    mean = z.mean(axis=0)
    var = ((z - mean) ** 2).mean(axis=0)
    o = finalize(mean, var, z.shape[0], gamma, beta, eps, run_mean, run_var, mom, one_minus_mom)
    o.y = clamp((z - mean) * o.scale + o.beta, act)        # (z scale + shift without its cancellation)
    return o


def from_partials(psum, psumsq, M, center=None, **kw):
    """What vp_bn_train_finalize must return for these partial rows (center: a finalize handed centred sums): sums of d and d^2 over the parts, d = x - center."""
    s1, s2 = np.asarray(psum, np.float64).sum(axis=0), np.asarray(psumsq, np.float64).sum(axis=0)
    d1 = s1 / M
    var = np.maximum(s2 / M - d1 * d1, 0.0)
    return finalize(d1 if center is None else np.asarray(center, np.float64) + d1, var, M, **kw)


# ---------------------------------------------------------------------------------------------------- backward
def mask_front(z):
    return np.asarray(z) > 0


def mask_behind(z, ms, mh, mask_hi=0.0):
    v = fma32(z, ms, mh)
    return (v > 0) & ((v < mask_hi) if mask_hi else True)


def dy_utt(dy, us, um, T):
    """dy * us[b] + um[b] / T, b = row // T (the SE block's input gradient, formed on the fly)."""
    dy = np.asarray(dy, np.float64)
    b = np.arange(dy.shape[0]) // T
    return dy * np.asarray(us, np.float64)[b] + np.asarray(um, np.float64)[b] / T


def dy_ctx(dy, alpha, beta, z16, xsc, xsh, T):
    """dy + alpha[b] + beta[b] * bf16(z * xsc + xsh): z16 the bf16-stored z, the affine one f32 fused multiply-add, then bf16."""
    dy = np.asarray(dy, np.float64)
    b = np.arange(dy.shape[0]) // T
    y16 = bf16_round(fma32(z16, xsc, xsh)).astype(np.float64)
    return dy + np.asarray(alpha, np.float64)[b] + np.asarray(beta, np.float64)[b] * y16


def col_sums(a, b=None, bmean=None, bscale=None, behind=None):
    """-> (2, C) sums, (2, C) sums of |terms|: sum a and sum a (b - bmean) bscale, a counted where `behind`."""
    a = np.asarray(a, np.float64)
    if behind is not None:
        a = a * behind
    t2 = a * (np.asarray(b, np.float64) - bmean) * bscale if b is not None else np.zeros_like(a)
    return np.stack([a.sum(0), t2.sum(0)]), np.stack([np.abs(a).sum(0), np.abs(t2).sum(0)])


def backward(dy, z, mean, invstd, gamma=None, front=None, behind=None, sums=None):
    """-> dz, dgamma, dbeta, dbias (float64).  sums: the (2, C) reductions the dz pass is handed (default: the exact ones)."""
    dy, z = np.asarray(dy, np.float64), np.asarray(z, np.float64)
    M, C = z.shape
    g = dy if behind is None else dy * behind
    zh = (z - mean) * invstd
    s = np.stack([g.sum(0), (g * zh).sum(0)]) if sums is None else np.asarray(sums, np.float64)
    gam = np.ones(C) if gamma is None else np.asarray(gamma, np.float64)
    dz = gam * invstd * (g - s[0] / M - zh * s[1] / M)
    if front is not None:
        dz = dz * front
    return dz, s[1], s[0], dz.sum(0)


# ---------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def conditioned(M, C, r, seed=0):
    """(M, C) float32, read-only: channel c has std s_c (log-uniform in [0.05, 2]) and mean +- r s_c; planted: CH_CONST exactly constant
    (-3.7), CH_JITTER 1.25 +- one f32 ulp, CH_ZERO all zero, and row 0 of CH_OUTLIER three s_c off its mean (row 0 is what formula (c)
    centres on)."""
    assert C > CH_OUTLIER
    g = np.random.default_rng(1000 * seed + 7 * M + 13 * C + r)
    s = 0.05 * 40.0 ** g.random(C)
    sign = np.where(g.random(C) < 0.5, -1.0, 1.0)
    x = (sign * r * s + s * g.standard_normal((M, C))).astype(np.float32)
    x[:, CH_CONST] = CONST
    x[:, CH_JITTER] = np.float32(JITTER) + np.spacing(np.float32(JITTER)) * g.integers(-1, 2, M).astype(np.float32)
    x[:, CH_ZERO] = 0.0
    x[0, CH_OUTLIER] = np.float32(sign[CH_OUTLIER] * (r + 3.0) * s[CH_OUTLIER])
    x.setflags(write=False)
    return x


def affine_params(C, seed):
    g = np.random.default_rng(seed)
    return (g.uniform(0.5, 1.5, C).astype(np.float32), (0.5 * g.standard_normal(C)).astype(np.float32),
            (0.1 * g.standard_normal(C)).astype(np.float32), g.uniform(0.5, 1.5, C).astype(np.float32))      # gamma, beta, run_mean, run_var


# ---------------------------------------------------------------------------------------------------- bounds
def stats_errors(mean, var, invstd, ref):
    """-> worst over channels of: invstd relative error; mean error / (|mean| + std); var error / (4e-6 var + 1e-12 mean^2) (<= 1 holds)."""
    inv = np.max(np.abs(invstd - ref.invstd) / ref.invstd)
    mu = np.max(np.abs(mean - ref.mean) / (np.abs(ref.mean) + np.sqrt(ref.var) + 1e-300))
    tol = VAR_REL * ref.var + VAR_MEAN2 * ref.mean ** 2
    va = np.max(np.where(np.abs(var - ref.var) <= tol, 0.0, np.abs(var - ref.var) / np.maximum(tol, 1e-300)))
    return float(inv), float(mu), float(va)


def y_error(y, z, ref, act=0):
    """worst |y - ref| / (|z scale| + |shift|), the two terms of the apply pass's one fused multiply-add"""
    z = np.asarray(z, np.float64)
    den = np.abs(z * ref.scale) + np.abs(ref.shift)
    return float(np.max(np.abs(np.asarray(y, np.float64) - clamp((z - ref.mean) * ref.scale + ref.beta, act)) / np.maximum(den, 1e-300)))


def rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-300))


# ---------------------------------------------------------------------------------------------------- float32 restatements
def colsum4_geometry(M, C4):
    """csrc/bn_train.hip colsum4_geometry restated -> cl_shift, colblocks, rows per chunk, chunks (RG = 256 >> cl_shift row groups)."""
    cl_shift = 6 if C4 >= 64 else (5 if C4 >= 32 else 4)
    CL, RG = 1 << cl_shift, 256 >> cl_shift
    colblocks = (C4 + CL - 1) // CL
    ch = max(1, min(512, 1024 // colblocks))
    rpc = max((M + ch - 1) // ch, 4 * RG)
    return cl_shift, colblocks, rpc, (M + rpc - 1) // rpc


def _dealt_sum(t, lanes):
    """float32 sum over axis 0 with row k dealt to accumulator k % lanes, each accumulator adding in row order, then the accumulators
    added in order: the shape of every reduction of the unit (row groups of a chunk, the 16 part-lanes of the partial-sum reduce)."""
    n = t.shape[0]
    pad = (-n) % lanes
    if pad:
        t = np.concatenate([t, np.zeros((pad,) + t.shape[1:], np.float32)])      # (adding +0 is exact)
    t = t.reshape(-1, lanes, *t.shape[1:])
    acc = np.zeros(t.shape[1:], np.float32)
    for row in t:
        acc = acc + row
    out = np.zeros(t.shape[2:], np.float32)
    for a in acc:
        out = out + a
    return out


def kernel_order_sum(t):
    """Column sums of the (M, C) float32 t in the order the four-channels-per-lane kernels add them: per chunk of rows, RG row groups
    each in row order, then the groups, then the chunks through the 16 part-lanes of sum_partials_kernel."""
    M, C = t.shape
    cl_shift, _, rpc, chunks = colsum4_geometry(M, max(C // 4, 1))
    parts = np.stack([_dealt_sum(t[k * rpc:(k + 1) * rpc], 256 >> cl_shift) for k in range(chunks)])
    return _dealt_sum(parts, 16)


def center(x):
    """The centre of formula (d): the f32 mean of the first eight rows, added as a tree; row 0 where there are fewer.  (BNRows centres on
    the mean of the first min(M, 8) rows, summed by vp_col_sums_f32: the same k^2 ~ 1 / 8, another order of additions.)"""
    x = np.asarray(x, np.float32)
    if x.shape[0] < 8:
        return x[0].copy()
    return (((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]))) * np.float32(0.125)


def stats_f32(x, formula, order='kernel'):
    """mean, var, invstd in float32 NumPy: 'a' raw sums, 'b' two passes, 'c' sums about row 0, 'd' sums about `center`.  order 'kernel': the sums added as the
    kernels add them (kernel_order_sum); 'sequential': one row after the other, the least favourable order there is."""
    x = np.asarray(x, np.float32)
    M = np.float32(x.shape[0])
    total = kernel_order_sum if order == 'kernel' else (lambda t: t.sum(0, dtype=np.float32))
    if formula == 'a':
        mu = total(x) / M
        var = total(x * x) / M - mu * mu
    elif formula == 'b':
        mu = total(x) / M
        d = x - mu
        var = total(d * d) / M
    else:
        c0 = x[0] if formula == 'c' else center(x)
        d = x - c0
        d1 = total(d) / M
        var = total(d * d) / M - d1 * d1
        mu = c0 + d1
    var = np.maximum(var, np.float32(0))
    return mu, var, (np.float32(1) / np.sqrt(var + np.float32(EPS))).astype(np.float32)


def invstd_error_f32(M, r, formula, C=64, seed=0, order='kernel'):
    x = conditioned(M, C, r, seed)
    ref = forward(x)
    _, _, inv = stats_f32(x, formula, order)
    return float(np.max(np.abs(inv - ref.invstd) / ref.invstd))


@functools.lru_cache(maxsize=None)
def one_pass_k(M, r, C=64):
    """k of the one-pass contract |invstd error| <= k (1 + r_c^2) 2^-24, r_c = |mean| / std of the channel: the worst channel of
    restatement (a) on conditioned(M, C, r), and at least 1 -- one
    rounding each of s2 / M and mean^2 already costs the variance (1 + r^2) 2^-24, so a smaller measured k is luck, not a property."""
    x = conditioned(M, C, r)
    ref = forward(x)
    live = ref.var > 0                              # (the exactly constant channels have no r_c; the fused-sum layers have none)
    rc2 = ref.mean[live] ** 2 / ref.var[live]
    err = (np.abs(stats_f32(x, 'a')[2] - ref.invstd) / ref.invstd)[live]
    return max(1.0, float(np.max(err / ((1 + rc2) * U24))))


def one_pass_bound(M, r_nominal, r_channel, C=64):
    """The fused-sum path's bound per channel: 4 k (1 + r_c^2) 2^-24 (4: the GPU's other summation order)."""
    return 4.0 * one_pass_k(M, r_nominal, C) * (1.0 + np.asarray(r_channel, np.float64) ** 2) * U24
