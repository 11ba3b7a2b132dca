"""Float64 restatements of the inference path's small kernels (csrc/small_ops.hip), the inputs the tests plant and the bounds
(docs/small_ops.md).  The helpers and the two input families are those of tests/train_ops_oracle.py (docs/train_ops.md):

'exact': small integers and dyadic rationals; every product and partial sum is representable in float32 in any order, so a kernel must
EQUAL float64 (tests/test_small_ops_oracle_cpu.py proves the precondition for every case of exact_cases()).  Where a formula still
rounds on such inputs, the roundings are counted.  'gauss': standard normal, |err| <= (n_terms + k) 2^-24 sum|terms| per element.

Every operation takes `dt` (the dtype it computes in) and `rev` (walk every reduction backwards)."""
import functools

import numpy as np
import torch

from tests.train_ops_oracle import F32, F64, REL_FLOOR, U, act, act_bound, bf16, dyads, gauss, ints, rng, seq_sum  # noqa: F401

BM = 128                             # rows of a conv M-tile (csrc/common.h: VP_CONV_BM)
SE_GRID_CAP = 4096 * 256             # the SE scale kernels and the cast: at most 4096 workgroups of 256 threads, then the loop runs again
SE_THREADS = 1024                    # threads of the one-workgroup-per-utterance SE gate kernel
VP_F32, VP_BF16, VP_HL32 = 0, 1, 3
ACT_IDS = {'none': 0, 'relu': 1, 'sigmoid': 2, 'tanh': 3}

# (B, T) of the kernels that read the convs' fused partial sums -- what each reaches: docs/small_ops.md
BT_CASES = [(130, 1), (5, 28), (3, 127), (3, 128), (3, 129), (3, 298)]
BT_LONG = [(1, 23808), (2, 300)]     # 186 tiles per utterance / fewer tiles than thread groups: with C = 64 (SE gate), C = 5 (moments)


def is_pow2(n):
    return n & (n - 1) == 0


# ------------------------------------------------------------------------------------------------ the convs' fused partial sums
def nseg(T):
    """Utterance segments per 128-row tile (vp_conv1d_nseg)."""
    return (BM - 1) // T + 2


def tiles_m(B, T):
    return (B * T + BM - 1) // BM


def conv_psum(v):
    """v (B, T, C) -> the partial time sums a conv leaves behind, (tiles, nseg, C) float32: tile tm holds rows [128 tm, 128 tm + 128) of
    the (B T, C) matrix, slot `seg` of it the rows of utterance (first utterance of the tile) + seg.  Slots no row touches are NaN: a
    kernel that reads one poisons its output."""
    B, T, C = v.shape
    r = np.arange(B * T)
    tm, b = r // BM, r // T
    key = tm * (B + 1) + b
    starts = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    ps = np.full((tiles_m(B, T), nseg(T), C), np.nan, F64)
    ps[tm[starts], b[starts] - (tm[starts] * BM) // T] = np.add.reduceat(np.asarray(v, F64).reshape(B * T, C), starts, axis=0)
    return ps.astype(F32)


def utt_slots(B, T):
    """Per utterance the (tile, segment) slots the kernels walk: tiles floor(b T / 128) .. floor(((b + 1) T - 1) / 128)."""
    out = []
    for b in range(B):
        tm = np.arange(b * T // BM, ((b + 1) * T - 1) // BM + 1)
        out.append((tm, b - tm * BM // T))
    return out


def utt_sums(ps, B, T, dt=F64, rev=False):
    ps = np.asarray(ps, dt)
    return np.stack([seq_sum(ps[tm, sg], 0, rev) for tm, sg in utt_slots(B, T)])


def n_tiles(B, T):
    return max(len(tm) for tm, _ in utt_slots(B, T))


# ------------------------------------------------------------------------------------------------ vp_moments_finalize(_affine)
MOM_C = [1, 5, 256, 257, 300]
MOM_EPS = 1e-5


def _moment_parts(ps, psq, B, T, dt, rev):
    inv = dt(1.0) / dt(T)                                        # float32: the quotient the kernel forms; float64: 1 / T itself
    md = utt_sums(ps, B, T, dt, rev) * inv
    return md, (None if psq is None else utt_sums(psq, B, T, dt, rev) * inv - md * md)


def moments(ps, psq, shift, scale, B, T, eps, want_std, dt=F64, rev=False):
    """stats (B, C or 2C) = [shift + scale mean_t | sqrt(max(scale^2 (E[z^2] - E[z]^2), eps))] from the partial sums of z and z^2;
    shift None = 0, scale None = 1 (vp_moments_finalize), eps taken as its float32 value."""
    md, var = _moment_parts(ps, psq if want_std else None, B, T, dt, rev)
    sh = dt(0.0) if shift is None else np.asarray(shift, dt)
    sc = dt(1.0) if scale is None else np.asarray(scale, dt)
    mean = sh + sc * md
    if not want_std:
        return mean
    return np.concatenate([mean, np.sqrt(np.maximum(var * sc * sc, dt(F32(eps))))], 1)


def moments_bounds(ps, psq, shift, scale, B, T, eps, want_std, n_terms):
    """Per-element bound for any float32 evaluation.  mean: n_terms additions (0 on the exact family: integer sums are exact), 1/T, the
    product with it, scale *, + shift = (n_terms + 4) 2^-24 (|shift| + |scale| sum|psum| / T).  Variance: twice that on md^2 plus the
    product, n_terms + 2 on E[z^2], the difference, scale^2 twice -- (n_terms + 8) 2^-24 scale^2 (E|z^2| + E|z|^2) covers them; the std
    moves by at most that over the reference std (max(., eps) is 1-Lipschitz and sqrt a - sqrt b = (a - b) / (sqrt a + sqrt b)), plus
    the rounding of sqrt."""
    a1 = utt_sums(np.abs(ps), B, T) / T
    sh = 0.0 if shift is None else np.abs(np.asarray(shift, F64))
    sc = 1.0 if scale is None else np.abs(np.asarray(scale, F64))
    em = (n_terms + 4) * U * (sh + sc * a1)
    if not want_std:
        return em
    std = moments(ps, psq, shift, scale, B, T, eps, 1)[:, ps.shape[-1]:]
    ev = (n_terms + 8) * U * sc * sc * (utt_sums(np.abs(psq), B, T) / T + a1 * a1)
    return np.concatenate([em + 0 * a1, ev / std + 2 * U * std], 1)


def planted_std_bound(psq, scale, std, B, T):
    """The bound of the mean-8, std-1/4 channel (E[x^2] - E[x]^2 is a difference of nearby numbers): (T + 4) 2^-24 E[x^2] / (2 std), x the
    quantity whose std is returned (scale z); psq (.., C), scale (C) or None, std (B, C) -> (B, C)."""
    sc = 1.0 if scale is None else np.asarray(scale, F64)
    return (T + 4) * U * sc * sc * (utt_sums(psq, B, T) / T) / (2 * std)


def var32_min(z, B, T):
    """The smallest float32 E[x^2] - E[x]^2 over the utterances of one channel z (B, T), the larger of the two summation orders."""
    z = np.asarray(z, F64).reshape(B, T, 1)
    return float(max(_moment_parts(conv_psum(z), conv_psum(z * z), B, T, F32, rev)[1].min() for rev in (False, True)))


@functools.lru_cache(None)
def negvar_channel(B, T):
    """(B, T) values 1 <= v < 2, all within one float32 ulp of a constant: the true variance is ~1e-15 while float32's E[x^2] - E[x]^2 is
    rounding noise of size 1e-7 -- the first candidate of a fixed sequence for which that noise comes out NEGATIVE for an utterance, in
    both summation orders (T = 1: E[x^2] - E[x]^2 is 0 in float32, a constant)."""
    if T == 1:
        return np.full((B, T), F32(1.1), F64)
    for seed in range(256):
        g = rng(B, T, seed, 99)
        c = F32(1.0 + g.random())
        z = (c + np.spacing(c) * g.integers(0, 2, (B, T)).astype(F32)).astype(F32).astype(F64)
        if var32_min(z, B, T) < 0:
            return z
    raise AssertionError(f'no negative float32 variance found for B={B} T={T}')


PLANTED = {'const': 0, 'negvar': 1, 'near': 2, 'scale0': 3}      # channels, when C >= 5


def moments_inputs(B, T, C, family):
    """z (B, T, C) float64 (float32 values), scale, shift.  With C >= 5: channel 0 constant (variance 0 -> sqrt(eps)), channel 1
    negvar_channel, channel 2 = 8 +- 1/4 alternating (mean 8, std 1/4), channel 3 has scale 0; scales of both signs."""
    g = rng(B, T, C, 41)
    z = (ints(g, (B, T, C)) if family == 'exact' else gauss(g, (B, T, C))).astype(F64)
    if family == 'exact':
        scale, shift = dyads(g, C) * g.choice(np.asarray([-1.0, 1.0], F32), C), ints(g, C, -4, 4)
    else:
        scale, shift = gauss(g, C), gauss(g, C)
    if C >= 5:
        z[:, :, PLANTED['const']] = 3.0
        z[:, :, PLANTED['negvar']] = negvar_channel(B, T)
        z[:, :, PLANTED['near']] = 8.0 + 0.25 * (1 - 2 * (np.arange(T) % 2))[None, :]
        scale[PLANTED['scale0']] = 0.0
        scale[PLANTED['negvar']] = 1.0 if family == 'exact' else scale[PLANTED['negvar']]
    return z, scale.astype(F32), shift.astype(F32)


def moments_n_terms(B, T, C, family):
    """n_terms of moments_bounds per channel: the additions that can round -- none on the exact family's integer channels (every partial
    sum is exact), the tiles of an utterance on Gaussian channels and on the two planted non-integer channels."""
    n = np.full(C, n_tiles(B, T) if family == 'gauss' else 0, F64)
    if C >= 5:
        n[[PLANTED['negvar'], PLANTED['near']]] = n_tiles(B, T)
    return n


# ------------------------------------------------------------------------------------------------ vp_se_gate_fwd
SE_GATE_CASES = [                     # (C, H, [(B, T), ...]): what each reaches is in docs/small_ops.md
    (4, 4, [(130, 1), (3, 128), (5, 28)]),
    (64, 8, [(1, 23808), (2, 300), (3, 127)]),
    (192, 24, [(5, 28), (3, 129), (3, 298)]),
    (512, 128, [(3, 298), (130, 1), (3, 128)]),
    (516, 64, [(3, 298), (5, 28), (3, 127)]),
    (768, 96, [(3, 298), (130, 1), (3, 129)]),
    (1020, 128, [(3, 298), (5, 28), (3, 128)]),
    (1024, 128, [(3, 298), (3, 127)]),
    (1024, 1024, [(3, 298), (5, 28)]),
]
SE_GATE_FLAT = [(C, H, B, T) for C, H, bts in SE_GATE_CASES for B, T in bts]


def _mv(x, w, dt, rev):
    """x (B, K) @ w (K, N): strictly sequential in float32; float64 may take any order (it is the reference)."""
    if dt is F64:
        return np.asarray(x, F64) @ np.asarray(w, F64)
    return seq_sum(np.asarray(x, dt)[:, :, None] * np.asarray(w, dt)[None], 1, rev)


def se_gate(ps, shift, w1, b1, w2, b2, B, T, dt=F64, rev=False):
    """mean = shift + (sum of the utterance's partial sums) / T; a = ReLU(mean W1 + b1); z = a W2 + b2; s = sigmoid(z).
    W1 (C, H), W2 (H, C): input-major.  -> mean, a, z, s."""
    mean = utt_sums(ps, B, T, dt, rev) / dt(T)
    if shift is not None:
        mean = np.asarray(shift, dt) + mean
    a = np.maximum(_mv(mean, w1, dt, rev) + np.asarray(b1, dt), dt(0.0))
    z = _mv(a, w2, dt, rev) + np.asarray(b2, dt)
    return mean, a, z, dt(1.0) / (dt(1.0) + np.exp(-z))


def se_gate_inputs(B, T, C, H, family):
    """-> psum (tiles, nseg, C) float32, shift, W1 (C, H), b1, W2 (H, C), b2.  exact: the conv output minus shift is an integer m[b, c] in
    -4..4 plus a zero-sum pattern over time (+j, -j on frame pairs), so every partial sum is an integer, the time sum is T m and the
    quotient by T is m exactly for ANY T; W1 small integers; W2 in {-1, 0, 1} / 2^k with k such that the sigmoid's argument is O(4)."""
    g = rng(B, T, C, H, 43)
    if family == 'gauss':
        return (conv_psum(gauss(g, (B, T, C))), gauss(g, C) * F32(0.3), gauss(g, (C, H)) / F32(np.sqrt(C)), gauss(g, H) * F32(0.1),
                gauss(g, (H, C)) / F32(np.sqrt(H)), gauss(g, C) * F32(0.1))
    m = ints(g, (B, 1, C), -4, 4).astype(F64)
    j = np.repeat(ints(g, (B, (T + 1) // 2, C), -4, 4), 2, axis=1)[:, :T].astype(F64)
    j *= (1 - 2 * (np.arange(T) % 2))[None, :, None]
    if T % 2:
        j[:, -1] = 0
    shift, w1, b1 = ints(g, C, -2, 2), ints(g, (C, H), -2, 2), ints(g, H, -3, 3)
    a = np.maximum((shift + m[:, 0]) @ w1.astype(F64) + b1, 0.0)
    k = int(np.ceil(np.log2(max(1.0, float(np.abs(a).max()) * np.sqrt(H) / 4))))
    return conv_psum(m + j), shift, w1, b1, ints(g, (H, C), -1, 1) * F32(2.0 ** -k), ints(g, C, -2, 2) * F32(0.5)


@functools.lru_cache(None)
def expf_model():
    """(c1, c2): the relative error of a float32 restatement of the fast exponential, exp2(x log2 e) with the product rounded to float32,
    is at most (c1 |x| + c2) 2^-24 -- the product's rounding moves the result by |x| 2^-24 relative, exp2 itself by a constant.
    Measured on the CPU against float64 over 65 536 arguments in [-12, 12] and the quarters in [-12, 12]: c2 = the worst error at
    |x| <= 1, c1 = the worst remaining slope.  Never taken from a kernel's output; the tests allow four times it (docs/small_ops.md)."""
    x = np.concatenate([np.linspace(-12.0, 12.0, 1 << 16), np.arange(-48, 49) / 4.0]).astype(F32)
    e32 = torch.exp2(torch.from_numpy(x) * F32(1.4426950408889634)).numpy()
    ref = np.exp(x.astype(F64))
    rel = np.abs(e32.astype(F64) - ref) / ref / U
    small = np.abs(x) <= 1
    c2 = float(rel[small].max())
    c1 = float(max(0.0, ((rel[~small] - c2) / np.abs(x[~small])).max()))
    return c1, c2


def sigmoid_bound(z, s):
    """|err| of s = 1 / (1 + exp(-z)) formed with the fast exponential from an argument z: exp's relative error times ds / d(ln e) =
    s (1 - s), plus the roundings of 1 + e and of the quotient, 2 x 2^-24 s."""
    c1, c2 = expf_model()
    return 4.0 * (c1 * np.abs(z) + c2) * U * s * (1.0 - s) + 2.0 * U * s


def se_gate_bounds(ps, shift, w1, b1, w2, b2, B, T):
    """Bound on the sigmoid's ARGUMENT for any float32 evaluation: the mean costs (tiles + 2) 2^-24 (|shift| + sum|psum| / T), a matvec
    of K terms (K + 2) 2^-24 sum|terms|, and every stage inherits its operand's bound through |W|."""
    aw1, aw2 = np.abs(np.asarray(w1, F64)), np.abs(np.asarray(w2, F64))
    am = (0.0 if shift is None else np.abs(np.asarray(shift, F64))) + utt_sums(np.abs(ps), B, T) / T
    em = (n_tiles(B, T) + 2) * U * am
    aa = am @ aw1 + np.abs(b1)
    ea = (w1.shape[0] + 2) * U * aa + em @ aw1
    return (w2.shape[0] + 2) * U * (aa @ aw2 + np.abs(b2)) + ea @ aw2


# ------------------------------------------------------------------------------------------------ SE scale + residual
def fma32(x, s, r):
    """round_f32(x s + r) with ONE rounding, for float32-valued operands: the product is exact in float64, TwoSum gives the sum's
    rounding error, and where the float64 sum sits exactly on a float32 tie that error decides the direction."""
    x, s, r = (np.asarray(v, F64) for v in np.broadcast_arrays(x, s, r))
    p = x * s
    h = p + r
    bb = h - p
    e = (p - (h - bb)) + (r - bb)                                # h + e = p + r exactly
    f = h.astype(F32)
    d = h - f.astype(F64)                                        # exact
    other = np.nextafter(f, np.where(d > 0, F32(np.inf), F32(-np.inf)).astype(F32))
    tie = (d != 0) & (np.abs(d) * 2 == np.abs(other.astype(F64) - f.astype(F64))) & (e != 0)
    return np.where(tie & (np.sign(e) == np.sign(d)), other, f).astype(F32)


def se_scale(x, s, res):
    """out[b, t, c] = fma(x, s[b, c], res) rounded once to float32 (x, res (B, T, C); s (B, C))."""
    return fma32(x, np.asarray(s)[:, None, :], res)


def se_scale_z16(z, bsc, bsh, s, res):
    """The bf16 SE variant that forms BatchNorm on the fly, with the kernel's two roundings: h = bf16(fma(z, sc, sh)), out = bf16(fma(h, s, res))."""
    h = bf16(fma32(z, np.asarray(bsc)[None, None, :], np.asarray(bsh)[None, None, :]))
    return bf16(fma32(h, np.asarray(s)[:, None, :], res))


def bf16_tie_near(v64):
    """True where the float64 value lies within 2^-24 (relative) of the midpoint of two neighbouring bf16 numbers."""
    v64 = np.abs(np.asarray(v64, F64))
    lo = (v64.astype(F32).view(np.uint32) & np.uint32(0xffff0000)).view(F32).astype(F64)       # truncation: the bf16 at or below |v|
    hi = ((lo.astype(F32).view(np.uint32) + np.uint32(0x10000))).view(F32).astype(F64)
    return np.abs(v64 - 0.5 * (lo + hi)) <= U * v64


def bf16_neighbours(v32):
    """The bf16 numbers just below and just above (in magnitude) each float32 value, as float32."""
    bits = np.asarray(v32, F32).view(np.uint32) & np.uint32(0xffff0000)
    return bits.view(F32), (bits + np.uint32(0x10000)).view(F32)


def se_inputs(B, T, C, family, stored_bf16, key=0):
    """x, res (B, T, C) and the gate s (B, C): exact = integers (|v| <= 256 when stored as bf16, else <= 8) and dyadic gates."""
    g = rng(B, T, C, key, 47)
    if family == 'exact':
        hi = 256 if stored_bf16 else 8
        return ints(g, (B, T, C), -hi, hi), ints(g, (B, T, C), -hi, hi), dyads(g, (B, C))
    x, r, s = gauss(g, (B, T, C)), gauss(g, (B, T, C)), gauss(g, (B, C))
    return (bf16(x), bf16(r), s) if stored_bf16 else (x, r, s)


Z16_TIES = np.asarray([257.0, -259.0, 261.0, -263.0], F32)        # odd integers past 256 lie on bf16 ties: 257 -> 256, -259 -> -260


def z16_inputs(B, T, C, family):
    """z, res (B, T, C) bf16-valued, BatchNorm scale / shift (C), gate s (B, C).  exact: integers <= 256, dyadic scale, integer shift
    (both fmas exact, both bf16 roundings plain round-to-nearest-even) with ties planted at BOTH roundings: channel 0 has scale 1,
    shift 1 and z = Z16_TIES - 1, so z sc + sh walks the ties; channel 1 has h = 256, s = 1, res = +-1 or +-3: h s + res is a tie."""
    g = rng(B, T, C, 49)
    if family == 'gauss':
        return bf16(gauss(g, (B, T, C))), gauss(g, C), gauss(g, C), gauss(g, (B, C)), bf16(gauss(g, (B, T, C)))
    z, res = ints(g, (B, T, C), -256, 256), ints(g, (B, T, C), -256, 256)
    sc, sh, s = dyads(g, C), ints(g, C, -4, 4), dyads(g, (B, C))
    sc[:2], sh[:2], s[:, 1] = 1.0, (1.0, 0.0), 1.0
    z[:, :, 0] = np.resize(Z16_TIES - 1, (B, T))
    z[:, :, 1] = 256.0
    res[:, :, 1] = np.resize(np.asarray([1.0, -1.0, 3.0, 5.0], F32), (B, T))
    return z, sc, sh, s, res


# ------------------------------------------------------------------------------------------------ vp_dense_f32
DENSE_CASES = [(1, 1, 1, 0)] + [(m, n, k, kn) for m, n, k in [(16, 16, 64), (17, 33, 68), (5, 17, 19), (7, 20, 1020), (7, 20, 1024),
                                                                (7, 20, 1028)] for kn in (0, 1)] + [(3, 192, 3072, 0)]


def dense(a, w, bias, kind='none', dt=F64, rev=False):
    """act(a (M, K) @ w (K, N) + bias) -> the pre-activation and the output."""
    z = _mv(a, w, dt, rev)
    if bias is not None:
        z = z + np.asarray(bias, dt)
    return z, (z if kind == 'none' else act(kind, z, dt))


def dense_bound(a, w, bias):
    """(K + 2) 2^-24 (|a| @ |w| + |bias|): K products and additions in any order and grouping, the bias."""
    K = a.shape[1]
    return (K + 2) * U * (np.abs(np.asarray(a, F64)) @ np.abs(np.asarray(w, F64)) + (0.0 if bias is None else np.abs(np.asarray(bias, F64))))


@functools.lru_cache(None)
def act_rel_bound(kind):
    """The relative bound of docs/train_ops.md for tanh / sigmoid: 4 x the worst error of the float32 CPU restatement against float64 over
    that document's 4093 planted and Gaussian arguments (2.45e-07 and 4.41e-07), applied as bound * (|ref| + 2^-100)."""
    from tests.train_ops_oracle import act_inputs
    return act_bound(kind, act_inputs(4093, 1))[1]


def dense_inputs(M, N, K, family):
    """a (M, K), w (K, N), bias (N).  exact: a in -4..4, w in {-1, 0, 1} / 2^k (k such that the activations' argument is O(4)), bias halves."""
    g = rng(M, N, K, 53)
    if family == 'exact':
        k = int(np.ceil(np.log2(max(1.0, np.sqrt(K) / 2))))
        return ints(g, (M, K), -4, 4), ints(g, (K, N), -1, 1) * F32(2.0 ** -k), ints(g, N, -4, 4) * F32(0.5)
    return gauss(g, (M, K)), gauss(g, (K, N)) / F32(np.sqrt(K)), gauss(g, N)


# ------------------------------------------------------------------------------------------------ vp_cast_f32_bf16
CAST_N = [1, 3, 4, 5, 1001, SE_GRID_CAP * 4 + 7]                 # 4096 * 1024 + 7: a second grid-stride trip and the scalar tail
CAST_PLANTED = np.asarray(
    [0.0, -0.0, 1.0, -1.0, 257.0, -259.0, 1.00390625, 1.01171875, 1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -24,   # ties, near ties
     2.0 ** -126, -2.0 ** -126, 2.0 ** -127, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, 2.0 ** -149, -2.0 ** -149, 2.0 ** -126 - 2.0 ** -149,
     3.3895313892515355e38, 3.4028234663852886e38, -3.4028234663852886e38,          # the largest bf16; FLT_MAX rounds to Inf
     np.inf, -np.inf, np.nan], F32)


def cast_inputs(n):
    """n float32: NaN, +-Inf, +-0, ties, subnormals first where n allows, Gaussian after; long inputs repeat a block of 4093."""
    block = np.concatenate([CAST_PLANTED[::-1] if n < 8 else CAST_PLANTED, gauss(rng(61), 4093 - len(CAST_PLANTED))])
    return np.resize(block, n).astype(F32)


def cast_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ the exactness precondition
def exact_cases():
    """Every planted exact-family case with a product or a reduction in it: (id, function of (dt, rev) -> tuple of arrays).  The CPU test
    evaluates each in float32 first-to-last, float32 last-to-first and float64 and demands three bit-identical results."""
    out = []
    for C, H, B, T in SE_GATE_FLAT:
        inp = se_gate_inputs(B, T, C, H, 'exact')
        out.append((f'se_gate-C{C}-H{H}-B{B}-T{T}', lambda dt, rev, inp=inp, B=B, T=T: se_gate(*inp, B, T, dt=dt, rev=rev)[:3]))
    for B, T in BT_CASES + BT_LONG:
        if not is_pow2(T):
            continue                                              # 1 / T rounds: counted roundings instead (moments_bounds)
        for C in MOM_C:
            z, scale, shift = moments_inputs(B, T, C, 'exact')
            keep = [c for c in range(C) if C < 5 or c != PLANTED['negvar']]
            ps, psq = conv_psum(z)[..., keep], conv_psum(z * z)[..., keep]
            out.append((f'moments-B{B}-T{T}-C{C}', lambda dt, rev, ps=ps, psq=psq, sc=scale[keep], sh=shift[keep], B=B, T=T:
                        (moments(ps, None, sh, sc, B, T, MOM_EPS, 0, dt, rev), _moment_parts(ps, psq, B, T, dt, rev)[1])))
    for M, N, K, kn in DENSE_CASES:
        if kn == 0:
            a, w, bias = dense_inputs(M, N, K, 'exact')
            out.append((f'dense-{M}x{N}x{K}', lambda dt, rev, a=a, w=w, bias=bias: dense(a, w, bias, 'relu', dt, rev)))
    for bf in (False, True):
        x, r, s = se_inputs(3, 37, 40, 'exact', bf)
        out.append((f'se_scale-bf{int(bf)}', lambda dt, rev, x=x, r=r, s=s: (np.asarray(x, dt) * np.asarray(s, dt)[:, None, :] + np.asarray(r, dt),)))
    z, sc, sh, s, r = z16_inputs(3, 37, 40, 'exact')
    h = bf16(np.asarray(z, F64) * sc + sh)
    out.append(('se_scale-z16', lambda dt, rev: (np.asarray(z, dt) * np.asarray(sc, dt) + np.asarray(sh, dt),
                                                 np.asarray(h, dt) * np.asarray(s, dt)[:, None, :] + np.asarray(r, dt))))
    return out
