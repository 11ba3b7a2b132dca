"""The BatchNorm training unit of csrc/bn_train.hip -- vp_bn_train_finalize, the vp_col_sums_* reductions, the vp_affine_rows_* apply
passes, the vp_bn_relu_bwd_* backward passes and their callers BNRows / ConvBlock / Conv2dBlock -- against the float64 oracle of
tests/bn_oracle.py, entry point by entry point (docs/bn_train.md).  Run with -m gpu on an MI355X.

Statistics   BNRows centres its input (d = x - mean of the first rows, ppvector.train.functions.bn_centred_stats): over conditioned(M, C, r),
             r = |mean| / std up to 100, invstd 2e-6 relative; |var - ref| <= 4e-6 ref + 1e-12 mean^2 (a constant channel comes out near 0,
             not as noise); mean 2e-6 of |mean| + std; the running statistics the same through a real blend; y against the oracle.
             ConvBlock (fused sums and separate pass) and Conv2dBlock take var = s2 / M - mean^2 from raw sums of x and x^2: over convs
             whose bias sets r, invstd within 4 k (1 + r_c^2) 2^-24 per channel, k from the CPU calibration's restatement (a)
             (tests/test_bn_oracle_cpu.py), asserted for r <= 10, measured and printed at r = 30 and 100; mean 2e-6 of |mean| + std at
             every r; y, the apply pass, per element 2e-6 of (|z scale| + |shift|) with the scale and shift the kernels produced.
Reductions   |sum - ref| <= 2e-6 sum |terms| per channel (a gradient formed on the fly counts by its pieces);
backward     f32 dz 2e-6 relative L2;  bf16 dz within one bf16 ulp of the rounded float64 value plus what f32 costs the value before
             it is rounded (2e-6 of |g| + |s1 / M| + |zhat s2 / M|, times |gamma invstd|: near a cancellation the bf16 ulp of the result
             is smaller than the f32 rounding of its terms);  dbias from the unrounded values.
Geometry     C on both sides of every cl_shift step of colsum4_geometry with a last column block that is not full, M below one row
             group, around the four-row trip's tail and into a second chunk; one contiguous pitch and one wider (ld = C + 8, the slice
             at column 4, NaN in the padding columns, outputs framed by a sentinel).

Every case's operands are built once on the CPU in the stored dtype, and the float64 reference sees those numbers."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from tests import bn_oracle as bo

pytestmark = pytest.mark.gpu

C_EDGES = (60, 64, 68, 124, 128, 132, 252, 256, 260, 1536)
M_EDGES = (1, 15, 16, 17, 63, 64, 65, 129, 257, 4097)
UTT_BT = ((1, 1), (17, 1), (257, 1), (1, 7), (9, 7), (37, 7), (586, 7), (1, 64), (2, 64), (65, 64))      # M = B * T
SENTINEL = -768.0                      # (a bf16 number)
NAN = float('nan')


@pytest.fixture(scope='module')
def N():
    from ppvector import _native as N
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: these tests must run on an MI355X (no CPU fallback exists)')
    N.ctx(0)
    return N


@pytest.fixture(autouse=True)
def default_dispatch():
    exported = [v for v in ('VPMI_BN_RELU_UNFOLDED', 'VPMI_BN_BIAS_GRAD_SUMS') if os.environ.get(v) is not None]
    assert not exported, f'unset {", ".join(exported)}: the paths pinned here are those of the default dispatch'


@pytest.fixture(scope='module')
def worst():
    """entry point -> worst figures over the module, printed at the end (docs/bn_train.md quotes them)."""
    w = {}
    yield w
    for k in sorted(w):
        print(f'[bn worst] {k}: ' + '  '.join(f'{n} {v:.2e}' for n, v in sorted(w[k].items())))


def note(worst, key, **figs):
    d = worst.setdefault(key, {})
    for n, v in figs.items():
        d[n] = max(d.get(n, 0.0), float(v))


def hctx(N):
    return N.ctx(torch.device('cuda', 0))


# ------------------------------------------------------------------------------------------------------------ device buffers
def geom(C, wide):
    return (C + 8, 4) if wide else (C, 0)


class In:
    """(M, C) numbers as columns [off, off + C) of a (M, ld) device buffer whose other columns are NaN."""

    def __init__(self, a, wide=False, bf16=False):
        M, C = a.shape
        ld, off = geom(C, wide)
        buf = torch.full((M, ld), NAN, dtype=torch.float32)
        buf[:, off:off + C] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        self.buf = (buf.to(torch.bfloat16) if bf16 else buf).cuda()
        self.ld, self.ptr = ld, self.buf.data_ptr() + off * self.buf.element_size()


class Out:
    """A (M, C) output as rows [1, M + 1), columns [off, off + C) of a (M + 2, ld) buffer filled with a sentinel (or with `init`)."""

    def __init__(self, M, C, wide=False, bf16=False, init=None):
        self.M, self.C = M, C
        self.ld, self.off = geom(C, wide)
        buf = torch.full((M + 2, self.ld), SENTINEL, dtype=torch.float32)
        if init is not None:
            buf[1:M + 1, self.off:self.off + C] = torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32))
        self.buf = (buf.to(torch.bfloat16) if bf16 else buf).cuda()
        self.ptr = self.buf.data_ptr() + (self.ld + self.off) * self.buf.element_size()

    def get(self):
        """-> the (M, C) result as float64; asserts that nothing outside it was written."""
        torch.cuda.synchronize()
        b = self.buf.float().cpu().numpy().astype(np.float64)
        inner = b[1:self.M + 1, self.off:self.off + self.C].copy()
        b[1:self.M + 1, self.off:self.off + self.C] = SENTINEL
        assert (b == SENTINEL).all(), 'a kernel wrote outside its output slice'
        return inner


def vec(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def framed(n):
    """n floats inside a sentinel frame of 4 on either side -> tensor, pointer, checker"""
    t = torch.full((n + 8,), SENTINEL, device='cuda')
    return t, t.data_ptr() + 16


def unframe(t):
    torch.cuda.synchronize()
    a = t.cpu().numpy().astype(np.float64)
    assert (a[:4] == SENTINEL).all() and (a[-4:] == SENTINEL).all(), 'a kernel wrote outside its output vector'
    return a[4:-4]


def workspace(nbytes):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device='cuda')


# ------------------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=3)
def case(M, C, T=1):
    """Seeded operands of one (M, C[, T]) shape, float32 arrays holding what the kernels read."""
    g = np.random.default_rng(100003 * M + 17 * C + T)
    B = M // T
    c = types.SimpleNamespace(M=M, C=C, T=T, B=B)
    c.dy = g.standard_normal((M, C)).astype(np.float32)
    c.z = (0.5 + 2.0 * g.standard_normal((M, C))).astype(np.float32)
    c.z[:, 1] = np.abs(c.z[:, 1])                          # a channel the front ReLU never masks ...
    c.z[::2, 2] = 0.0                                      # ... and one that sits ON the mask's edge in half its rows (z > 0 is false at 0)
    c.z16 = bo.bf16_round(c.z)
    c.mean = (0.5 + 0.1 * g.standard_normal(C)).astype(np.float32)
    c.invstd = g.uniform(0.3, 0.8, C).astype(np.float32)
    c.gamma = (g.uniform(0.5, 1.5, C) * np.where(g.random(C) < 0.2, -1, 1)).astype(np.float32)
    # the affine of an activation BEHIND the BatchNorm: z ms + mh ~ N(3 + mh, 6): some of it below 0, some above 20
    c.ms = (3.0 * g.uniform(0.5, 1.5, C) * np.where(g.random(C) < 0.3, -1, 1)).astype(np.float32)
    c.mh = g.uniform(-3.0, 12.0, C).astype(np.float32)
    c.us, c.um = g.uniform(0.2, 1.0, (B, C)).astype(np.float32), g.standard_normal((B, C)).astype(np.float32)
    c.alpha, c.beta = (0.3 * g.standard_normal((B, C))).astype(np.float32), (0.3 * g.standard_normal((B, C))).astype(np.float32)
    c.xsc, c.xsh = g.uniform(0.3, 0.8, C).astype(np.float32), (0.2 * g.standard_normal(C)).astype(np.float32)
    c.old = g.standard_normal((M, C)).astype(np.float32)   # what an accumulating dz pass finds in its output
    return c


def abs_pieces(c, form, z):
    """sum-of-|pieces| image of the gradient a reduction sums: what its f32 rounding is relative to."""
    dy = np.abs(c.dy.astype(np.float64))
    b = np.arange(c.M) // c.T
    if form == 'utt':
        return dy * np.abs(c.us.astype(np.float64))[b] + np.abs(c.um.astype(np.float64))[b] / c.T
    if form == 'ctx':
        y16 = np.abs(bo.bf16_round(bo.fma32(z, c.xsc, c.xsh)).astype(np.float64))
        return dy + np.abs(c.alpha.astype(np.float64))[b] + np.abs(c.beta.astype(np.float64))[b] * y16
    return dy


def gradient(c, form, z):
    if form == 'utt':
        return bo.dy_utt(c.dy, c.us, c.um, c.T)
    if form == 'ctx':
        return bo.dy_ctx(c.dy, c.alpha, c.beta, z, c.xsc, c.xsh, c.T)
    return c.dy.astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ reductions
def run_col_sums(N, c, entry, wide, two=True, mask_hi=0.0):
    """-> sums (2, C) float64 from the named entry point"""
    lib, ctx = N.lib(), hctx(N)
    M, C = c.M, c.C
    b16 = entry in ('b16', 'utt', 'ctx')
    a, b = In(c.dy, wide), In(c.z16 if b16 else c.z, wide, bf16=b16)
    mu, sc = vec(c.mean), vec(c.invstd)
    st, sp = framed(2 * C)
    ws = workspace(lib.vp_col_sums_workspace_bytes(M, C))
    tail = (M, C, sp, ws.data_ptr(), ws.numel(), N.stream_ptr())
    keep = [vec(c.ms), vec(c.mh), vec(c.us), vec(c.um), vec(c.alpha), vec(c.beta), vec(c.xsc), vec(c.xsh)]
    if entry == 'f32':
        rc = lib.vp_col_sums_f32(ctx, a.ptr, a.ld, b.ptr if two else None, b.ld, mu.data_ptr() if two else None, sc.data_ptr() if two else None, *tail)
    elif entry == 'masked':
        rc = lib.vp_col_sums_masked_f32(ctx, a.ptr, a.ld, b.ptr, b.ld, mu.data_ptr(), sc.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), mask_hi, *tail)
    elif entry == 'b16':
        rc = lib.vp_col_sums_f32_b16(ctx, a.ptr, a.ld, b.ptr, b.ld, mu.data_ptr(), sc.data_ptr(), *tail)
    elif entry == 'utt':
        rc = lib.vp_col_sums_f32_b16_utt(ctx, a.ptr, a.ld, keep[2].data_ptr(), keep[3].data_ptr(), c.T, b.ptr, b.ld, mu.data_ptr(), sc.data_ptr(), *tail)
    else:
        rc = lib.vp_col_sums_f32_b16_ctx(ctx, a.ptr, a.ld, keep[4].data_ptr(), keep[5].data_ptr(), c.T, keep[6].data_ptr(), keep[7].data_ptr(),
                                         b.ptr, b.ld, mu.data_ptr(), sc.data_ptr(), *tail)
    N.check(rc, ctx)
    return unframe(st).reshape(2, C)


def check_col_sums(N, worst, c, entry, wide, two=True, mask_hi=0.0):
    got = run_col_sums(N, c, entry, wide, two, mask_hi)
    z = c.z16 if entry in ('b16', 'utt', 'ctx') else c.z
    form = entry if entry in ('utt', 'ctx') else 'plain'
    behind = bo.mask_behind(z, c.ms, c.mh, mask_hi) if entry == 'masked' else None
    g = gradient(c, form, z)
    ref, _ = bo.col_sums(g, z if two else None, c.mean.astype(np.float64), c.invstd.astype(np.float64), behind)
    pieces = abs_pieces(c, form, z) * (1.0 if behind is None else behind)
    tol = np.stack([pieces.sum(0), (pieces * np.abs((z.astype(np.float64) - c.mean) * c.invstd)).sum(0) if two else np.zeros(c.C)])
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    figure = float(np.max(err / np.maximum(tol, 1e-30)))
    note(worst, f'vp_col_sums {entry}', of_sum_abs=figure)
    assert (err <= bo.SUM_BOUND * tol).all(), (entry, c.M, c.C, c.T, wide, mask_hi, figure)


@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('C', C_EDGES)
def test_col_sums_vs_float64(N, worst, C, wide):
    """vp_col_sums_f32 (one sum and two), vp_col_sums_masked_f32 (mask_hi 0 and 20), vp_col_sums_f32_b16."""
    for M in M_EDGES:
        c = case(M, C)
        check_col_sums(N, worst, c, 'f32', wide)
        check_col_sums(N, worst, c, 'f32', wide, two=False)
        check_col_sums(N, worst, c, 'masked', wide, mask_hi=0.0)
        check_col_sums(N, worst, c, 'masked', wide, mask_hi=20.0)
        check_col_sums(N, worst, c, 'b16', wide)


@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('C', C_EDGES)
def test_col_sums_per_utterance_vs_float64(N, worst, C, wide):
    """vp_col_sums_f32_b16_utt (dy us[b] + um[b] / T) and vp_col_sums_f32_b16_ctx (dy + alpha[b] + beta[b] bf16(z xsc + xsh)), M = B T."""
    for B, T in UTT_BT:
        c = case(B * T, C, T)
        check_col_sums(N, worst, c, 'utt', wide)
        check_col_sums(N, worst, c, 'ctx', wide)


def test_col_sums_scalar_kernel_vs_float64(N, worst):
    """C % 4 != 0, or a base that is not 16-byte aligned: the one-channel-per-lane kernel, the same sums."""
    lib, ctx = N.lib(), hctx(N)
    for M, C in ((1, 6), (17, 6), (513, 6), (1025, 70), (4097, 6)):
        c = case(M, C)
        got = run_col_sums(N, c, 'f32', False)
        ref, tol = bo.col_sums(c.dy, c.z, c.mean.astype(np.float64), c.invstd.astype(np.float64))
        assert (np.abs(got - ref) <= bo.SUM_BOUND * tol).all(), (M, C)
    c = case(257, 64)                      # C % 4 == 0 on a view that starts one float into its rows: not 16-byte aligned
    a, b = In(c.dy, True), In(c.z, True)
    st, sp = framed(2 * 60)
    ws = workspace(lib.vp_col_sums_workspace_bytes(257, 60))
    mu, sc = vec(c.mean[1:61]), vec(c.invstd[1:61])
    N.check(lib.vp_col_sums_f32(ctx, a.ptr + 4, a.ld, b.ptr + 4, b.ld, mu.data_ptr(), sc.data_ptr(), 257, 60, sp, ws.data_ptr(), ws.numel(),
                                N.stream_ptr()), ctx)
    ref, tol = bo.col_sums(c.dy[:, 1:61], c.z[:, 1:61], c.mean[1:61].astype(np.float64), c.invstd[1:61].astype(np.float64))
    assert (np.abs(unframe(st).reshape(2, 60) - ref) <= bo.SUM_BOUND * tol).all()


# ------------------------------------------------------------------------------------------------------------ backward passes
def exact_sums(c, g, z, behind=None):
    """the (2, C) reductions a dz pass is handed, as the f32 numbers it reads"""
    s, _ = bo.col_sums(g, z, c.mean.astype(np.float64), c.invstd.astype(np.float64), behind)
    return s.astype(np.float32)


def term_scale(c, pieces, z, sums, gamma):
    """|gamma invstd| (|g| + |s1 / M| + |zhat s2 / M|), |g| by its pieces: what the f32 rounding of a dz element is relative to.  (dz itself
    is a difference: with M = 1 it is g - s1 = 0 up to the zhat term, and an error measured against |dz| would measure nothing.)"""
    zh = (z.astype(np.float64) - c.mean) * c.invstd
    gi = np.abs((1.0 if gamma is None else gamma.astype(np.float64)) * c.invstd)
    return gi * (pieces + np.abs(sums[0].astype(np.float64)) / c.M + np.abs(zh * sums[1].astype(np.float64)) / c.M)


def check_dz(worst, key, got, ref, bf16, scale, where):
    assert np.isfinite(got).all(), where
    if bf16:
        tol = bo.bf16_ulp(ref) + bo.F32_L2 * scale
        err = np.abs(got - bo.bf16_round(ref).astype(np.float64))
        note(worst, key, dz_bf16_of_tol=np.max(err / tol), beyond_one_ulp=float((err > bo.bf16_ulp(ref)).sum()))
        assert (err <= tol).all(), (where, float(np.max(err / tol)))
        assert ((ref == 0) <= (got == 0)).all(), where               # a masked element is an exact zero
    else:
        e = bo.rel_l2(got, ref)
        note(worst, key, dz_rel_l2=e)
        assert e <= bo.F32_L2, (where, e)
        assert ((ref == 0) <= (got == 0)).all(), where


def check_dbias(worst, key, got, dz_ref, scale, where):
    """dbias = sum_m dz: 2e-6 of the sum of |terms|, a term counted by the pieces it is the difference of (term_scale)"""
    err, tol = np.abs(got - dz_ref.sum(0)), scale.sum(0)
    note(worst, key, dbias_of_sum_abs=np.max(err / np.maximum(tol, 1e-30)))
    assert (err <= bo.SUM_BOUND * tol).all(), where


def run_dbias(N, c, entry, wide, relu_mask, use_gamma):
    """vp_bn_relu_bwd_dbias_{f32, bf16out, b16, b16_utt, b16_ctx} -> dz (M, C), dbias (C), and the reference's ingredients"""
    lib, ctx = N.lib(), hctx(N)
    M, C = c.M, c.C
    z16 = entry in ('b16', 'utt', 'ctx')
    out16 = entry != 'f32'
    z = c.z16 if z16 else c.z
    form = entry if entry in ('utt', 'ctx') else 'plain'
    g = gradient(c, form, z)
    gamma = c.gamma if use_gamma else None
    sums = exact_sums(c, g, z)
    dy, zd = In(c.dy, wide), In(z, wide, bf16=z16)
    dz = Out(M, C, wide, bf16=out16)
    mu, sc, gm, sm = vec(c.mean), vec(c.invstd), vec(c.gamma), vec(sums)
    keep = [vec(c.us), vec(c.um), vec(c.alpha), vec(c.beta), vec(c.xsc), vec(c.xsh)]
    dbt, dbp = framed(C)
    ws = workspace(lib.vp_bn_relu_bwd_dbias_workspace_bytes(M, C))
    mid = (zd.ptr, zd.ld, mu.data_ptr(), sc.data_ptr(), gm.data_ptr() if use_gamma else None, sm.data_ptr(), M, C, relu_mask, dz.ptr, dz.ld, dbp,
           ws.data_ptr(), ws.numel(), N.stream_ptr())
    if entry == 'utt':
        rc = lib.vp_bn_relu_bwd_dbias_b16_utt(ctx, dy.ptr, dy.ld, keep[0].data_ptr(), keep[1].data_ptr(), c.T, *mid)
    elif entry == 'ctx':
        rc = lib.vp_bn_relu_bwd_dbias_b16_ctx(ctx, dy.ptr, dy.ld, keep[2].data_ptr(), keep[3].data_ptr(), c.T, keep[4].data_ptr(), keep[5].data_ptr(), *mid)
    else:
        fn = {'f32': lib.vp_bn_relu_bwd_dbias_f32, 'bf16out': lib.vp_bn_relu_bwd_dbias_bf16out, 'b16': lib.vp_bn_relu_bwd_dbias_b16}[entry]
        rc = fn(ctx, dy.ptr, dy.ld, *mid)
    N.check(rc, ctx)
    front = bo.mask_front(z) if relu_mask else None
    ref = bo.backward(g, z, c.mean.astype(np.float64), c.invstd.astype(np.float64), gamma, front=front, sums=sums)[0]
    return dz.get(), unframe(dbt), ref, term_scale(c, abs_pieces(c, form, z), z, sums, gamma) * (1.0 if front is None else front), out16


def check_dbias_entry(N, worst, c, entry, wide, relu_mask, use_gamma):
    got, db, ref, scale, out16 = run_dbias(N, c, entry, wide, relu_mask, use_gamma)
    where = (entry, c.M, c.C, c.T, wide, relu_mask, use_gamma)
    key = f'vp_bn_relu_bwd_dbias {entry}'
    check_dz(worst, key, got, ref, out16, scale, where)
    check_dbias(worst, key, db, ref, scale, where)


@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('C', C_EDGES)
def test_bn_relu_bwd_dbias_vs_float64(N, worst, C, wide):
    """vp_bn_relu_bwd_dbias_f32 / _bf16out / _b16: dz and its column sums, with and without the front ReLU's mask and gamma."""
    for i, M in enumerate(M_EDGES):
        c = case(M, C)
        for entry in ('f32', 'bf16out', 'b16'):
            check_dbias_entry(N, worst, c, entry, wide, relu_mask=1, use_gamma=True)
        check_dbias_entry(N, worst, c, ('f32', 'bf16out', 'b16')[i % 3], wide, relu_mask=0, use_gamma=False)


@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('C', C_EDGES)
def test_bn_relu_bwd_dbias_per_utterance_vs_float64(N, worst, C, wide):
    """vp_bn_relu_bwd_dbias_b16_utt / _b16_ctx: the gradient formed on the fly, M = B T."""
    for i, (B, T) in enumerate(UTT_BT):
        c = case(B * T, C, T)
        check_dbias_entry(N, worst, c, 'utt', wide, relu_mask=1, use_gamma=True)
        check_dbias_entry(N, worst, c, 'ctx', wide, relu_mask=i % 2, use_gamma=bool(i % 3))


def run_bwd(N, c, wide, masked, relu_mask=0, mask_hi=0.0, accumulate=0, use_gamma=True):
    """vp_bn_relu_bwd_f32 / vp_bn_relu_bwd_masked_f32 -> dz, reference"""
    lib, ctx = N.lib(), hctx(N)
    M, C = c.M, c.C
    behind = bo.mask_behind(c.z, c.ms, c.mh, mask_hi) if masked else None
    sums = exact_sums(c, c.dy.astype(np.float64), c.z, behind)
    dy, zd = In(c.dy, wide), In(c.z, wide)
    dz = Out(M, C, wide, init=c.old if accumulate else None)
    mu, sc, gm, sm, ms, mh = vec(c.mean), vec(c.invstd), vec(c.gamma), vec(sums), vec(c.ms), vec(c.mh)
    gp = gm.data_ptr() if use_gamma else None
    if masked:
        rc = lib.vp_bn_relu_bwd_masked_f32(ctx, dy.ptr, dy.ld, zd.ptr, zd.ld, mu.data_ptr(), sc.data_ptr(), gp, sm.data_ptr(), ms.data_ptr(), mh.data_ptr(),
                                           mask_hi, M, C, dz.ptr, dz.ld, accumulate, N.stream_ptr())
    else:
        rc = lib.vp_bn_relu_bwd_f32(ctx, dy.ptr, dy.ld, zd.ptr, zd.ld, mu.data_ptr(), sc.data_ptr(), gp, sm.data_ptr(), M, C, relu_mask, dz.ptr, dz.ld,
                                    N.stream_ptr())
    N.check(rc, ctx)
    ref = bo.backward(c.dy, c.z, c.mean.astype(np.float64), c.invstd.astype(np.float64), c.gamma if use_gamma else None,
                      front=bo.mask_front(c.z) if relu_mask else None, behind=behind, sums=sums)[0]
    return dz.get(), ref


@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('C', C_EDGES)
def test_bn_relu_bwd_vs_float64(N, worst, C, wide):
    """vp_bn_relu_bwd_f32 (front mask on and off) and vp_bn_relu_bwd_masked_f32 (mask_hi 0 and 20, accumulate 0 and 1)."""
    for i, M in enumerate(M_EDGES):
        c = case(M, C)
        for relu_mask in (0, 1):
            got, ref = run_bwd(N, c, wide, False, relu_mask=relu_mask, use_gamma=bool(relu_mask))
            check_dz(worst, 'vp_bn_relu_bwd_f32', got, ref, False, None, ('plain', M, C, wide, relu_mask))
        for mask_hi, accumulate in ((0.0, 0), (20.0, 1), (20.0, 0), (0.0, 1)):
            got, ref = run_bwd(N, c, wide, True, mask_hi=mask_hi, accumulate=accumulate)
            where = ('masked', M, C, wide, mask_hi, accumulate)
            if accumulate:
                # dz += : the sum is one more f32 rounding of |old| + |new|; judged as a whole tensor like the plain pass
                want = ref + c.old.astype(np.float64)
                e = bo.rel_l2(got, want)
                note(worst, 'vp_bn_relu_bwd_masked_f32 (accumulate)', dz_rel_l2=e)
                assert e <= bo.F32_L2, (where, e)
                assert bo.rel_l2(got, ref) > 0.1, where           # ... and it did add
            else:
                check_dz(worst, 'vp_bn_relu_bwd_masked_f32', got, ref, False, None, where)


# ------------------------------------------------------------------------------------------------------------ apply passes
def run_affine(N, c, entry, wide, relu):
    lib, ctx = N.lib(), hctx(N)
    z16, y16 = entry in ('b16_f32', 'b16_b16'), entry in ('b16_b16', 'f32_b16')
    z = c.z16 if z16 else c.z
    zd, y = In(z, wide, bf16=z16), Out(c.M, c.C, wide, bf16=y16)
    sc, sh = vec(c.ms), vec(c.mh)
    fn = getattr(lib, 'vp_affine_rows_' + entry)
    N.check(fn(ctx, zd.ptr, zd.ld, sc.data_ptr(), sh.data_ptr(), c.M, c.C, y.ptr, y.ld, relu, N.stream_ptr()), ctx)
    return y.get(), z, y16


@pytest.mark.parametrize('M,C', [(1, 4), (4097, 4), (1, 260), (4097, 260)])
def test_affine_rows_vs_float64(N, worst, M, C):
    """vp_affine_rows_f32 / _b16_f32 / _b16_b16 / _f32_b16, every relu flag, contiguous and wider pitches: one fused multiply-add per
    element, 2e-6 of (|z scale| + |shift|); a bf16 output within one bf16 ulp of the rounded float64 value besides."""
    c = case(M, C)
    for entry in ('f32', 'b16_f32', 'b16_b16', 'f32_b16'):
        for relu in (0, 1, 2):
            for wide in (False, True):
                got, z, y16 = run_affine(N, c, entry, wide, relu)
                z64 = z.astype(np.float64)
                ref = bo.clamp(z64 * c.ms + c.mh, relu)
                den = np.abs(z64 * c.ms) + np.abs(c.mh)
                if y16:
                    err = np.abs(got - bo.bf16_round(ref).astype(np.float64))
                    tol = bo.bf16_ulp(ref) + bo.Y_BOUND * den
                else:
                    err, tol = np.abs(got - ref), bo.Y_BOUND * den
                note(worst, f'vp_affine_rows_{entry}', of_tol=np.max(err / np.maximum(tol, 1e-30)))
                assert np.isfinite(got).all() and (err <= tol).all(), (entry, relu, wide, M, C)
                if relu:
                    assert got.min() >= 0 and (relu == 1 or got.max() <= 20)
                    assert M == 1 or ((got == 0).any() and (relu == 1 or (got == 20).any()))        # (the clamps were exercised)


@pytest.mark.parametrize('M,C', [(1, 4), (4097, 4), (1, 260), (4097, 260)])
def test_affine_rows_aux_vs_float64(N, worst, M, C):
    """vp_affine_rows_aux_f32: y into a column slice of a wider tensor; with `add`, aux = y + add from the same pass."""
    lib, ctx = N.lib(), hctx(N)
    c = case(M, C)
    sc, sh = vec(c.ms), vec(c.mh)
    z64 = c.z.astype(np.float64)
    ref = z64 * c.ms + c.mh
    den = np.abs(z64 * c.ms) + np.abs(c.mh)
    for with_add in (False, True):
        zd, y, add, aux = In(c.z, True), Out(M, C, True), In(c.old, True), Out(M, C, False)
        N.check(lib.vp_affine_rows_aux_f32(ctx, zd.ptr, zd.ld, sc.data_ptr(), sh.data_ptr(), M, C, y.ptr, y.ld, add.ptr if with_add else None,
                                           add.ld if with_add else 0, aux.ptr if with_add else None, aux.ld if with_add else 0, N.stream_ptr()), ctx)
        got = y.get()
        assert (np.abs(got - ref) <= bo.Y_BOUND * den).all(), (M, C, with_add)
        if with_add:
            a = aux.get()
            assert (np.abs(a - (ref + c.old)) <= bo.Y_BOUND * (den + np.abs(c.old))).all(), (M, C)
        else:
            torch.cuda.synchronize()
            assert (aux.buf == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------ finalize
def run_finalize(N, ps, pq, M, C, gamma, beta, rm, rv, mom, eps):
    lib, ctx = N.lib(), hctx(N)
    psd, pqd = vec(ps), vec(pq)
    outs = [framed(C) for _ in range(4)]
    gd, bd = (vec(gamma) if gamma is not None else None), (vec(beta) if beta is not None else None)
    rmt, rvt = (framed(C) if rm is not None else (None, None)), (framed(C) if rv is not None else (None, None))
    if rm is not None:
        rmt[0][4:-4] = vec(rm)
    if rv is not None:
        rvt[0][4:-4] = vec(rv)
    args = (gd.data_ptr() if gd is not None else None, bd.data_ptr() if bd is not None else None, rmt[1], rvt[1], mom, eps,
            outs[0][1], outs[1][1], outs[2][1], outs[3][1], N.stream_ptr())
    rc = lib.vp_bn_train_finalize(ctx, psd.data_ptr(), pqd.data_ptr(), ps.shape[0], M, C, *args)
    N.check(rc, ctx)
    mean, invstd, scale, shift = (unframe(t) for t, _ in outs)
    return mean, invstd, scale, shift, (unframe(rmt[0]) if rm is not None else None), (unframe(rvt[0]) if rv is not None else None)


@pytest.mark.parametrize('C', [1, 6, 15, 16, 17, 64, 3072])
def test_bn_train_finalize_vs_float64(N, worst, C):
    """vp_bn_train_finalize alone, on random partial rows: around the four-row trip (k + 48 < nparts) and the 16 part-lanes.
    The partial sums are given, so the float64 formula on the same partials is the reference: the part sums to 2e-6 of sum |parts|, the
    statistics to what that leaves them (var = s2 / M - mu^2 is judged by its terms), the folded affine and the blend to f32 rounding."""
    M, eps, mom = 1000, bo.EPS, bo.MOM
    for i, nparts in enumerate((1, 15, 16, 17, 48, 49, 63, 64, 65, 113, 1200)):
        g = np.random.default_rng(31 * nparts + C)
        ps = (g.standard_normal((nparts, C)) * 30 + 40).astype(np.float32)
        pq = (g.uniform(0.5, 1.5, (nparts, C)) * (M / nparts) * 40 + (ps.astype(np.float64).sum(0) / M) ** 2 * M / nparts).astype(np.float32)
        gamma, beta, rm, rv = bo.affine_params(C, nparts)
        if i % 3 == 1:
            gamma = beta = None
        if i % 4 == 2:
            rm = rv = None
        ref = bo.from_partials(ps, pq, M, gamma=gamma, beta=beta, eps=eps, run_mean=rm, run_var=rv, mom=mom, one_minus_mom=bo.ONE_MINUS_MOM)
        mean, invstd, scale, shift, rmn, rvn = run_finalize(N, ps, pq, M, C, gamma, beta, rm, rv, mom, eps)
        a1, a2 = np.abs(ps.astype(np.float64)).sum(0) / M, np.abs(pq.astype(np.float64)).sum(0) / M
        d1 = ps.astype(np.float64).sum(0) / M
        mean_tol = bo.SUM_BOUND * a1
        var_tol = bo.SUM_BOUND * (a2 + 2 * np.abs(d1) * a1)
        assert (np.abs(mean - ref.mean) <= mean_tol).all(), (C, nparts)
        inv_tol = 0.5 * ref.invstd * var_tol / (ref.var + eps) + 2e-7 * ref.invstd
        assert (np.abs(invstd - ref.invstd) <= inv_tol).all(), (C, nparts)
        g64 = np.ones(C) if gamma is None else gamma.astype(np.float64)
        b64 = np.zeros(C) if beta is None else beta.astype(np.float64)
        # scale and shift from the kernel's OWN mean and invstd: two and three f32 roundings
        assert (np.abs(scale - g64 * invstd) <= 2e-7 * np.abs(g64 * invstd)).all(), (C, nparts)
        assert (np.abs(shift - (b64 - mean * g64 * invstd)) <= 2e-7 * (np.abs(b64) + np.abs(mean * g64 * invstd))).all(), (C, nparts)
        if gamma is None:
            assert (scale == invstd).all() and (np.abs(shift + mean * invstd) <= 2e-7 * np.abs(mean * invstd)).all()
        if rm is not None:
            assert (np.abs(rmn - ref.run_mean) <= bo.ONE_MINUS_MOM * mean_tol + 2e-7 * (np.abs(mom * rm) + np.abs(bo.ONE_MINUS_MOM * ref.mean))).all(), (C, nparts)
            assert (np.abs(rvn - ref.run_var) <= bo.ONE_MINUS_MOM * var_tol + 2e-7 * (np.abs(mom * rv) + bo.ONE_MINUS_MOM * ref.var)).all(), (C, nparts)
        note(worst, 'vp_bn_train_finalize', mean_of_tol=np.max(np.abs(mean - ref.mean) / mean_tol), invstd_of_tol=np.max(np.abs(invstd - ref.invstd) / inv_tol))


def test_bn_train_finalize_running_variance_is_the_biased_one(N):
    """One part holding exact sums of M = 2 rows: the running variance blends var = 1 (biased), not 2 (unbiased); shift carries beta."""
    x = np.array([[1.0, -3.0, 5.0, 0.0], [3.0, -1.0, 5.0, 2.0]])
    ps, pq = x.sum(0, keepdims=True).astype(np.float32), (x * x).sum(0, keepdims=True).astype(np.float32)
    gamma, beta = np.full(4, 2.0, np.float32), np.array([0.5, -0.25, 8.0, 0.0], np.float32)
    mean, invstd, scale, shift, rm, rv = run_finalize(N, ps, pq, 2, 4, gamma, beta, np.zeros(4, np.float32), np.zeros(4, np.float32), 0.5, 0.0 + bo.EPS)
    var = np.array([1.0, 1.0, 0.0, 1.0])
    assert (mean == [2.0, -2.0, 5.0, 1.0]).all() and np.allclose(rv, 0.5 * var, rtol=1e-6, atol=0) and np.allclose(rm, 0.5 * mean, rtol=1e-6)
    ref = bo.finalize(mean, var, 2, gamma, beta, bo.EPS)
    assert np.allclose(invstd, ref.invstd, rtol=1e-6) and np.allclose(scale, ref.scale, rtol=1e-6)
    assert np.allclose(shift, ref.shift, rtol=1e-6, atol=1e-6) and abs(shift[2] - (8.0 - 5.0 * ref.scale[2])) < 1e-3 * abs(ref.shift[2])


# ------------------------------------------------------------------------------------------------------------ statistics conditioning
COND_SHAPES = ((2, 64), (6, 3072), (48, 3072), (777, 128), (4097, 64))


def one_pass_figure(invstd, ref, M, r, C=64):
    """worst channel of the invstd error over the one-pass bound 4 k (1 + r_c^2) 2^-24, the largest r_c, the worst error; channels whose
    float64 variance is exactly 0 have no r_c and are reported apart (their raw-sum variance is rounding noise of mean^2)."""
    live = ref.var > 0
    rc = np.abs(ref.mean[live]) / np.sqrt(ref.var[live])
    e = np.abs(invstd - ref.invstd) / ref.invstd
    const = float(e[~live].max()) if (~live).any() else 0.0
    return float(np.max(e[live] / bo.one_pass_bound(M, r, rc, C))), float(rc[rc < 1e4].max()), float(e[live].max()), const


def saved_statistics(out, z_index):
    """An autograd Function output's saved tensors -> the tensor the statistics were taken of (float64), the kernel's mean and invstd"""
    saved = out.grad_fn.saved_tensors
    torch.cuda.synchronize()
    return tuple(t.detach().double().cpu().numpy() for t in (saved[z_index], saved[z_index + 1], saved[z_index + 2]))


def check_one_pass(worst, key, invstd, mean, ref, M, r, where, C=64):
    """All statistics of the unit are raw sums of x and x^2, var = s2 / M - mean^2: invstd within 4 k (1 + r_c^2) 2^-24, asserted for
    r <= 10 and printed above (docs/bn_train.md: what a path that meets 2e-6 at every r takes)."""
    figure, rmax, e, const = one_pass_figure(invstd, ref, M, r, C)
    e_mu = float(np.max(np.abs(mean - ref.mean) / (np.abs(ref.mean) + np.sqrt(ref.var) + 1e-300)))
    print(f'[{key}] {where}: |mean|/std max {rmax:.1f}  invstd error {e:.2e} = {figure:.2f} of 4 k (1 + r_c^2) 2^-24 (k {bo.one_pass_k(M, r, C):.2f}); '
          f'constant channels {const:.2e}; mean {e_mu:.2e} of |mean| + std')
    note(worst, f'{key} r={r}', invstd=e, of_one_pass_bound=figure, invstd_constant_channels=const, mean=e_mu)
    assert e_mu <= bo.MEAN_BOUND, (key, where, e_mu)
    if r <= 10:
        assert figure <= 1.0, (key, where, figure)


def blend_tol(ref, run0, what):
    """the running statistics 'through the blend': (1 - mom) of the statistic's own bound plus the blend's f32 roundings (the running
    mean is blended from sum d + M center: five roundings of |run| + |mean| cover it)"""
    own = bo.MEAN_BOUND * (np.abs(ref.mean) + np.sqrt(ref.var)) if what == 'mean' else bo.VAR_REL * ref.var + bo.VAR_MEAN2 * ref.mean ** 2
    stat = ref.mean if what == 'mean' else ref.var
    return bo.ONE_MINUS_MOM * own + 5 * bo.U24 * (np.abs(run0) + np.abs(stat))


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('r', bo.R_SWEEP)
@pytest.mark.parametrize('M,C', COND_SHAPES)
def test_bnrows_statistics_conditioning(N, worst, M, C, r, relu):
    """BNRows forward and backward over conditioned(M, C, r), at every r up to 100 (the issue's bound 4): invstd 2e-6 relative;
    |var - ref| <= 4e-6 ref + 1e-12 mean^2 (the constant channels come out near zero, not as noise); mean 2e-6 of |mean| + std; the running
    statistics the same through a real blend (momentum 0.9 on seeded buffers).
    y, per element: the apply pass 2e-6 (|z scale| + |shift|) of the kernel's own operands (z = x - center), and against the float64
    oracle 2e-6 (|x - mean| scale + (|mean| + std) scale + |beta|) -- a tolerance that carries the statistics' own error (the issue's
    expression with the reference's shift cannot hold where shift cancels, docs/bn_train.md).
    Backward: dx per channel in L2 and dgamma per channel to 2e-6 of their terms, dbeta to 2e-6 sum |dy|."""
    from ppvector.train.functions import BNRows
    x = bo.conditioned(M, C, r)
    gamma, beta, rm0, rv0 = bo.affine_params(C, M + r)
    act = 1 if relu else 0
    ref = bo.forward(x, gamma, beta, act=act, run_mean=rm0, run_var=rv0, one_minus_mom=bo.ONE_MINUS_MOM)
    where = f'M={M} C={C} r={r} relu={relu}'
    # the batch statistics themselves: momentum 0 on zeroed buffers hands them back
    zm, zv = torch.zeros(C, device='cuda'), torch.zeros(C, device='cuda')
    y0 = BNRows.apply(vec(x).requires_grad_(), vec(gamma), vec(beta), zm, zv, 0.0, 1e-5, relu)
    d, mean_d, invstd = saved_statistics(y0, 0)
    center = -y0.grad_fn.neg_center.double().cpu().numpy()
    mean, var = zm.double().cpu().numpy(), zv.double().cpu().numpy()
    e_inv, e_mu, e_var = bo.stats_errors(mean, var, invstd, ref)
    note(worst, 'BNRows', invstd=e_inv, mean=e_mu, var_of_bound=e_var)
    print(f'[BNRows] {where}: invstd {e_inv:.2e}  mean {e_mu:.2e} of |mean| + std  var beyond its bound x{e_var:.2f}')
    assert e_inv <= bo.INVSTD_BOUND and e_mu <= bo.MEAN_BOUND and e_var == 0.0, (where, e_inv, e_mu, e_var)
    assert (np.abs(d - (x.astype(np.float64) - center)) <= bo.U24 * (np.abs(x) + np.abs(center))).all(), where      # d = x - center, one rounding
    assert (np.abs(mean - (center + mean_d)) <= 4 * bo.U24 * (np.abs(center) + np.abs(mean_d))).all(), where      # (sum x = sum d + M center)
    # the step as the models run it
    xd, gd, bd = (torch.from_numpy(np.array(t)).cuda().requires_grad_() for t in (x, gamma, beta))
    rm, rv = vec(rm0), vec(rv0)
    y = BNRows.apply(xd, gd, bd, rm, rv, 0.9, 1e-5, relu)
    scale, shift = (y.grad_fn.fold if relu else (None, None))
    dy = np.random.default_rng(M + C + r).standard_normal((M, C)).astype(np.float32)
    y.backward(torch.from_numpy(dy).cuda())
    torch.cuda.synchronize()
    assert (np.abs(rm.double().cpu().numpy() - ref.run_mean) <= blend_tol(ref, rm0, 'mean')).all(), where
    assert (np.abs(rv.double().cpu().numpy() - ref.run_var) <= blend_tol(ref, rv0, 'var')).all(), where
    got = y.detach().double().cpu().numpy()
    assert (got == y0.detach().double().cpu().numpy()).all(), where                   # the running buffers do not enter y
    x64 = x.astype(np.float64)
    tol = bo.Y_BOUND * (np.abs(x64 - ref.mean) * np.abs(ref.scale) + (np.abs(ref.mean) + np.sqrt(ref.var)) * np.abs(ref.scale) + np.abs(ref.beta))
    e_y = float(np.max(np.abs(got - ref.y) / tol))
    note(worst, 'BNRows', y_vs_oracle_of_tol=e_y)
    assert e_y <= 1.0, (where, e_y)
    if relu:                                            # the apply pass alone, on the operands the folded backward keeps
        sc, sh = scale.double().cpu().numpy(), shift.double().cpu().numpy()
        e_apply = float(np.max(np.abs(got - bo.clamp(d * sc + sh, 1)) / np.maximum(np.abs(d * sc) + np.abs(sh), 1e-300)))
        note(worst, 'BNRows', y_apply=e_apply)
        assert e_apply <= bo.Y_BOUND, (where, e_apply)
    behind = (got > 0) if relu else None                                                # the mask the forward applied
    dz, dgamma, dbeta, _ = bo.backward(dy, x, ref.mean, ref.invstd, gamma, behind=behind)
    # per channel, against the pieces the results are sums and differences of.  zhat is formed from the centred d: good to
    # 2^-24 (|d| + |E d|) invstd plus what the statistics leave; dz is itself a difference (with M = 2, zhat = +-1 and dz = 0 but for eps).
    g = dy.astype(np.float64) * (1.0 if behind is None else behind)
    zp = (np.abs(x64 - ref.mean) + np.abs(center - ref.mean) + np.sqrt(ref.var)) * ref.invstd
    s2p = (np.abs(g) * zp).sum(0)
    terms = np.abs(gamma * ref.invstd) * (np.abs(g) + np.abs(dbeta) / M + zp * s2p / M)
    e_dx = float(np.max(np.linalg.norm(xd.grad.double().cpu().numpy() - dz, axis=0) / np.maximum(np.linalg.norm(terms, axis=0), 1e-300)))
    e_dg = float(np.max(np.abs(gd.grad.double().cpu().numpy() - dgamma) / np.maximum(s2p, 1e-300)))
    note(worst, 'BNRows', dx_of_terms=e_dx, dgamma_of_terms=e_dg)
    print(f'[BNRows backward] {where}: dx {e_dx:.2e}  dgamma {e_dg:.2e} of their terms')
    assert e_dx <= bo.F32_L2 and e_dg <= bo.F32_L2, (where, e_dx, e_dg)
    assert (np.abs(bd.grad.double().cpu().numpy() - dbeta) <= bo.SUM_BOUND * np.abs(g).sum(0)).all(), where


def test_bnrows_refuses_six_channels(N):
    """BNRows is four channels wide (its apply and backward passes are): it says so for C = 6, before anything is launched."""
    from ppvector import _native
    from ppvector.train.functions import BNRows
    x = bo.conditioned(48, 6, 3)
    gamma, beta, _, _ = bo.affine_params(6, 1)
    with pytest.raises(_native.VpmiError):
        BNRows.apply(vec(x), vec(gamma), vec(beta), None, None, 0.9, 1e-5, True)


@pytest.mark.parametrize('r', bo.R_SWEEP)
@pytest.mark.parametrize('T_out', [18, 19, 200])
def test_conv_block_statistics(N, worst, T_out, r):
    """ConvBlock (conv -> ReLU -> BatchNorm), the bias r std of the conv's output so that |mean| / std ~ r behind the ReLU.
    T_out = 18: vp_conv1d_nseg > 8, a separate column-sum pass; T_out = 19, 200: the conv epilogue's fused sums.  Both are raw sums,
    held to the one-pass bound for r <= 10 and printed above (docs/bn_train.md: their layers have |mean| / std below 3.2).  The
    reference statistics are float64 statistics of the z the conv stored."""
    from ppvector.train.functions import ConvBlock
    lib = N.lib()
    B, Cin, Cout, kw = 4, 64, 64, 3
    T = T_out + kw - 1
    fused = lib.vp_conv1d_nseg(T_out) <= 8
    assert fused == (T_out >= 19)
    g = np.random.default_rng(T_out)
    x = g.standard_normal((B * T, Cin)).astype(np.float32)
    w = (g.standard_normal((Cout, Cin, kw)) / np.sqrt(Cin * kw) * (0.05 * 40.0 ** g.random((Cout, 1, 1)))).astype(np.float32)
    xt = torch.from_numpy(x).double().reshape(B, T, Cin).transpose(1, 2)
    std = torch.nn.functional.conv1d(xt, torch.from_numpy(w).double()).std(dim=(0, 2)).numpy()
    bias = (r * std).astype(np.float32)
    gamma, beta, _, _ = bo.affine_params(Cout, T_out)
    rm, rv = torch.zeros(Cout, device='cuda'), torch.zeros(Cout, device='cuda')
    out = ConvBlock.apply(vec(x).requires_grad_(), vec(w), vec(bias), None, vec(gamma), vec(beta), rm, rv,
                          dict(B=B, T=T, relu=True, momentum=0.0))
    z64, mean, invstd = saved_statistics(out, 2)
    ref = bo.forward(z64, gamma, beta)
    check_one_pass(worst, 'ConvBlock fused sums' if fused else 'ConvBlock separate pass', invstd, mean, ref, B * T_out, r, f'T_out={T_out} r={r}')


@pytest.mark.parametrize('act', ['relu', 'hardtanh'])
@pytest.mark.parametrize('r', bo.R_SWEEP)
def test_conv2d_block_statistics(N, worst, r, act):
    """Conv2dBlock (conv -> BatchNorm -> ReLU / Hardtanh), bias +- r std: raw sums as well, the one-pass bound for r <= 10; y is the
    apply pass of the scale and shift the folded backward keeps."""
    from ppvector.train.functions import Conv2dBlock
    B, T, Fq, Cin, Cout = 2, 9, 10, 8, 32
    g = np.random.default_rng(r + 5)
    x = g.standard_normal((B * T * Fq, Cin)).astype(np.float32)
    w = (g.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(Cin * 9) * (0.05 * 40.0 ** g.random((Cout, 1, 1, 1)))).astype(np.float32)
    xt = torch.from_numpy(x).double().reshape(B, T, Fq, Cin).permute(0, 3, 2, 1)           # (B, C, F, T), weight (Cout, Cin, kF, kT)
    std = torch.nn.functional.conv2d(xt, torch.from_numpy(w).double(), padding=1).std(dim=(0, 2, 3)).numpy()
    bias = (r * std * np.where(g.random(Cout) < 0.5, -1, 1)).astype(np.float32)
    gamma, beta, _, _ = bo.affine_params(Cout, r)
    rm, rv = torch.zeros(Cout, device='cuda'), torch.zeros(Cout, device='cuda')
    out = Conv2dBlock.apply(vec(x).requires_grad_(), vec(w), vec(bias), vec(gamma), vec(beta), rm, rv, dict(B=B, T=T, F=Fq, act=act, momentum=0.0))
    z64, mean, invstd = saved_statistics(out, 2)
    a = {'relu': 1, 'hardtanh': 2}[act]
    ref = bo.forward(z64, gamma, beta, act=a)
    rc = np.abs(ref.mean) / np.sqrt(ref.var)
    assert r == 0 or rc.max() > 0.8 * r
    check_one_pass(worst, 'Conv2dBlock', invstd, mean, ref, B * T * Fq, r, f'r={r} act={act}')
    scale, shift, hi = out.grad_fn.fold                 # what the folded backward re-evaluates the mask from: the apply pass's operands
    assert hi == (20.0 if act == 'hardtanh' else 0.0)
    scale, shift = scale.double().cpu().numpy(), shift.double().cpu().numpy()
    got = out.detach().double().cpu().numpy()
    e_y = float(np.max(np.abs(got - bo.clamp(z64 * scale + shift, a)) / np.maximum(np.abs(z64 * scale) + np.abs(shift), 1e-300)))
    note(worst, 'Conv2dBlock', y_apply=e_y)
    assert e_y <= bo.Y_BOUND, (r, act, e_y)


# ------------------------------------------------------------------------------------------------------------ mask agreement
@pytest.mark.parametrize('mask_hi,relu', [(0.0, 1), (20.0, 2)])
def test_forward_and_backward_masks_agree_exactly(N, mask_hi, relu):
    """The folded backward re-evaluates 0 < z ms + mh [< 20] instead of reading the forward's output.  On 2^20 elements, with elements
    planted exactly ON 0 and ON 20: vp_col_sums_masked_f32 with a = 1 returns per-channel counts, and they equal the counts of
    0 < y [< 20] in what vp_affine_rows_f32 stored; vp_bn_relu_bwd_masked_f32 zeroes exactly the same elements."""
    lib, ctx = N.lib(), hctx(N)
    M, C = 4096, 256
    g = np.random.default_rng(int(mask_hi) + 3)
    ms = (g.uniform(0.3, 3.0, C) * np.where(g.random(C) < 0.3, -1, 1)).astype(np.float32)
    mh = g.uniform(-2.0, 12.0, C).astype(np.float32)
    z = (4.0 * g.standard_normal((M, C))).astype(np.float32)
    # planted: powers of two in ms and small integers in z and mh make z ms + mh exactly 0 / exactly 20 whatever the contraction
    ms[:8] = [1.0, 2.0, -0.5, 4.0, 1.0, -2.0, 0.25, 8.0]
    mh[:8] = [-3.0, 6.0, 1.0, 20.0, 17.0, 26.0, 19.0, 4.0]
    z[::3, :8] = np.array([3.0, -3.0, 2.0, 0.0, 3.0, 3.0, 4.0, 2.0], np.float32)          # -> 0, 0, 0, 20, 20, 20, 20, 20
    # and near misses: one ulp either side of the edge in z
    z[1::3, :8] = np.nextafter(z[::3, :8][:z[1::3].shape[0]], np.float32(np.inf))
    z[2::3, :8] = np.nextafter(z[::3, :8][:z[2::3].shape[0]], np.float32(-np.inf))
    zd, ones = vec(z), torch.ones(M, C, device='cuda')
    msd, mhd, mu, sc = vec(ms), vec(mh), vec(np.zeros(C)), vec(np.ones(C))
    y = torch.empty(M, C, device='cuda')
    N.check(lib.vp_affine_rows_f32(ctx, zd.data_ptr(), C, msd.data_ptr(), mhd.data_ptr(), M, C, y.data_ptr(), C, relu, N.stream_ptr()), ctx)
    sums = torch.empty(2, C, device='cuda')
    ws = workspace(lib.vp_col_sums_workspace_bytes(M, C))
    N.check(lib.vp_col_sums_masked_f32(ctx, ones.data_ptr(), C, zd.data_ptr(), C, mu.data_ptr(), sc.data_ptr(), msd.data_ptr(), mhd.data_ptr(), mask_hi,
                                       M, C, sums.data_ptr(), ws.data_ptr(), ws.numel(), N.stream_ptr()), ctx)
    dz = torch.empty(M, C, device='cuda')
    zero2 = torch.zeros(2, C, device='cuda')
    N.check(lib.vp_bn_relu_bwd_masked_f32(ctx, ones.data_ptr(), C, zd.data_ptr(), C, mu.data_ptr(), sc.data_ptr(), None, zero2.data_ptr(), msd.data_ptr(),
                                          mhd.data_ptr(), mask_hi, M, C, dz.data_ptr(), C, 0, N.stream_ptr()), ctx)
    torch.cuda.synchronize()
    passed = (y > 0) & ((y < 20) if relu == 2 else torch.ones_like(y, dtype=torch.bool))
    want = bo.mask_behind(z, ms, mh, mask_hi)
    assert (passed.cpu().numpy() == want).all()                                      # the forward is the one fused multiply-add
    on_edge = (bo.fma32(z, ms, mh) == 0) | ((bo.fma32(z, ms, mh) == 20) if relu == 2 else False)
    assert on_edge[:, :8].sum() >= (8 if relu == 2 else 3) * (M // 3) and not want[on_edge].any()          # the planted elements sit on the edges and do not pass
    assert torch.equal(sums[0], passed.sum(0).float()), (sums[0] - passed.sum(0).float()).abs().max().item()
    assert torch.equal(dz != 0, passed)                                              # (sums handed in are 0: dz = [mask] * 1)


# ------------------------------------------------------------------------------------------------------------ argument contracts
def test_argument_contracts(N):
    """The guards as the entry points state them: nothing is launched, a code comes back and the outputs keep their sentinel."""
    lib, ctx = N.lib(), hctx(N)
    M, C, T = 64, 64, 8
    f = torch.zeros(M + 2, C + 8, device='cuda')
    h = torch.zeros(M + 2, C + 8, dtype=torch.bfloat16, device='cuda')
    v = torch.zeros(M * C + 8, device='cuda')
    out = torch.full((M + 2, C + 8), SENTINEL, device='cuda')
    out16 = torch.full((M + 2, C + 8), SENTINEL, dtype=torch.bfloat16, device='cuda')
    sums = torch.full((2 * C,), SENTINEL, device='cuda')
    need = lib.vp_col_sums_workspace_bytes(M, C)
    ws = workspace(need)
    need_db = lib.vp_bn_relu_bwd_dbias_workspace_bytes(M, C)
    F, H, V, O, O16, S, W, st = f.data_ptr(), h.data_ptr(), v.data_ptr(), out.data_ptr(), out16.data_ptr(), sums.data_ptr(), ws.data_ptr(), N.stream_ptr()
    EINVAL, EWS, EUNSUP = N.VP_EINVAL, N.VP_EWORKSPACE, N.VP_EUNSUP

    def col_b16(a=F, lda=C, b=H, ldb=C, m=M, c=C, wsb=need, mu=V):
        return lib.vp_col_sums_f32_b16(ctx, a, lda, b, ldb, mu, V, m, c, S, W, wsb, st)

    def col_utt(a=F, us=V, t=T, b=H, m=M, c=C, wsb=need):
        return lib.vp_col_sums_f32_b16_utt(ctx, a, C, us, V, t, b, C, V, V, m, c, S, W, wsb, st)

    def col_ctx(a=F, al=V, t=T, b=H, m=M, c=C, wsb=need, xs=V):
        return lib.vp_col_sums_f32_b16_ctx(ctx, a, C, al, V, t, xs, V, b, C, V, V, m, c, S, W, wsb, st)

    def dbias(fn, dy=F, z=F, dz=O, c=C, lddz=C, wsb=need_db, db=S, m=M):
        return fn(ctx, dy, C, z, C, V, V, V, V, m, c, 1, dz, lddz, db, W, wsb, st)

    def dbias_utt(dy=F, us=V, t=T, z=H, dz=O16, m=M, wsb=need_db):
        return lib.vp_bn_relu_bwd_dbias_b16_utt(ctx, dy, C, us, V, t, z, C, V, V, V, V, m, C, 1, dz, C, S, W, wsb, st)

    def dbias_ctx(dy=F, al=V, t=T, z=H, dz=O16, m=M, wsb=need_db, xs=V):
        return lib.vp_bn_relu_bwd_dbias_b16_ctx(ctx, dy, C, al, V, t, xs, V, z, C, V, V, V, V, m, C, 1, dz, C, S, W, wsb, st)

    calls = {
        # C % 4
        'col_b16 C%4': (col_b16(c=62), EINVAL), 'col_utt C%4': (col_utt(c=62), EINVAL), 'col_ctx C%4': (col_ctx(c=62), EINVAL),
        'dbias_f32 C%4': (dbias(lib.vp_bn_relu_bwd_dbias_f32, c=62), EINVAL), 'dbias pitch%4': (dbias(lib.vp_bn_relu_bwd_dbias_f32, lddz=C + 2), EINVAL),
        'affine C%4': (lib.vp_affine_rows_f32(ctx, F, C, V, V, M, 62, O, C, 0, st), EINVAL),
        'affine pitch%4': (lib.vp_affine_rows_f32(ctx, F, C + 2, V, V, M, C, O, C, 0, st), EINVAL),
        'affine_b16_b16 C%4': (lib.vp_affine_rows_b16_b16(ctx, H, C, V, V, M, 62, O16, C, 0, st), EINVAL),
        'bwd C%4': (lib.vp_bn_relu_bwd_f32(ctx, F, C, F, C, V, V, V, V, M, 62, 1, O, C, st), EINVAL),
        'bwd_masked C%4': (lib.vp_bn_relu_bwd_masked_f32(ctx, F, C, F, C, V, V, V, V, V, V, 0.0, M, 62, O, C, 0, st), EINVAL),
        # misaligned pointers
        'col_b16 a+4': (col_b16(a=F + 4), EINVAL), 'col_b16 b+2': (col_b16(b=H + 2), EINVAL),
        'col_utt us+4': (col_utt(us=V + 4), EINVAL), 'col_ctx alpha+4': (col_ctx(al=V + 4), EINVAL),
        'dbias_f32 dy+4': (dbias(lib.vp_bn_relu_bwd_dbias_f32, dy=F + 4), EINVAL), 'dbias_f32 z+8': (dbias(lib.vp_bn_relu_bwd_dbias_f32, z=F + 8), EINVAL),
        'dbias_bf16out dz+4': (dbias(lib.vp_bn_relu_bwd_dbias_bf16out, dz=O16 + 4), EINVAL), 'dbias_b16 z+4': (dbias(lib.vp_bn_relu_bwd_dbias_b16, z=H + 4, dz=O16), EINVAL),
        'dbias_utt dz+2': (dbias_utt(dz=O16 + 2), EINVAL), 'dbias_ctx dy+8': (dbias_ctx(dy=F + 8), EINVAL),
        'affine_aux y+4': (lib.vp_affine_rows_aux_f32(ctx, F, C, V, V, M, C, O + 4, C, None, 0, None, 0, st), EINVAL),
        # M % T
        'col_utt M%T': (col_utt(t=7), EINVAL), 'col_ctx M%T': (col_ctx(t=7), EINVAL), 'dbias_utt M%T': (dbias_utt(t=7), EINVAL),
        'dbias_ctx M%T': (dbias_ctx(t=7), EINVAL), 'col_utt T=0': (col_utt(t=0), EINVAL),
        # null operands
        'col_f32 a': (lib.vp_col_sums_f32(ctx, None, C, None, C, None, None, M, C, S, W, need, st), EINVAL),
        'col_f32 b without bmean': (lib.vp_col_sums_f32(ctx, F, C, F, C, None, V, M, C, S, W, need, st), EINVAL),
        'col_f32 sums': (lib.vp_col_sums_f32(ctx, F, C, None, C, None, None, M, C, None, W, need, st), EINVAL),
        'col_masked b': (lib.vp_col_sums_masked_f32(ctx, F, C, None, C, V, V, V, V, 0.0, M, C, S, W, need, st), EINVAL),
        'col_masked ms': (lib.vp_col_sums_masked_f32(ctx, F, C, F, C, V, V, None, V, 0.0, M, C, S, W, need, st), EINVAL),
        'col_masked mask_hi<0': (lib.vp_col_sums_masked_f32(ctx, F, C, F, C, V, V, V, V, -1.0, M, C, S, W, need, st), EINVAL),
        'col_b16 bmean': (col_b16(mu=None), EINVAL), 'col_ctx bn_scale': (col_ctx(xs=None), EINVAL), 'dbias_ctx bn_scale': (dbias_ctx(xs=None), EINVAL),
        'finalize psum': (lib.vp_bn_train_finalize(ctx, None, V, 1, M, C, V, V, None, None, 0.9, 1e-5, O, O, O, O, st), EINVAL),
        'finalize mean': (lib.vp_bn_train_finalize(ctx, V, V, 1, M, C, V, V, None, None, 0.9, 1e-5, None, O, O, O, st), EINVAL),
        'finalize nparts': (lib.vp_bn_train_finalize(ctx, V, V, 0, M, C, V, V, None, None, 0.9, 1e-5, O, O, O, O, st), EINVAL),
        'affine z': (lib.vp_affine_rows_f32(ctx, None, C, V, V, M, C, O, C, 0, st), EINVAL),
        'affine_aux aux without add': (lib.vp_affine_rows_aux_f32(ctx, F, C, V, V, M, C, O, C, None, 0, O, C, st), EINVAL),
        'bwd sums': (lib.vp_bn_relu_bwd_f32(ctx, F, C, F, C, V, V, V, None, M, C, 1, O, C, st), EINVAL),
        'bwd_masked mh': (lib.vp_bn_relu_bwd_masked_f32(ctx, F, C, F, C, V, V, V, V, V, None, 0.0, M, C, O, C, 0, st), EINVAL),
        'dbias dbias': (dbias(lib.vp_bn_relu_bwd_dbias_f32, db=None), EINVAL), 'dbias M=0': (dbias(lib.vp_bn_relu_bwd_dbias_f32, m=0), EINVAL),
        # a workspace one byte short
        'col_f32 ws': (lib.vp_col_sums_f32(ctx, F, C, None, C, None, None, M, C, S, W, need - 1, st), EWS),
        'col_masked ws': (lib.vp_col_sums_masked_f32(ctx, F, C, F, C, V, V, V, V, 0.0, M, C, S, W, need - 1, st), EWS),
        'col_b16 ws': (col_b16(wsb=need - 1), EWS), 'col_utt ws': (col_utt(wsb=need - 1), EWS), 'col_ctx ws': (col_ctx(wsb=need - 1), EWS),
        'dbias_f32 ws': (dbias(lib.vp_bn_relu_bwd_dbias_f32, wsb=need_db - 1), EWS), 'dbias_utt ws': (dbias_utt(wsb=need_db - 1), EWS),
        'dbias_ctx ws': (dbias_ctx(wsb=need_db - 1), EWS),
        'col_f32 null ws': (lib.vp_col_sums_f32(ctx, F, C, None, C, None, None, M, C, S, None, need, st), EWS),
        # the masked reduction on a view the four-channel kernel cannot read: the caller falls back to the materialised mask
        'col_masked a+4': (lib.vp_col_sums_masked_f32(ctx, F + 4, C, F, C, V, V, V, V, 0.0, M, C, S, W, need, st), EUNSUP),
        'col_masked C%4': (lib.vp_col_sums_masked_f32(ctx, F, C, F, C, V, V, V, V, 0.0, M, 62, S, W, need, st), EUNSUP),
        'col_masked pitch%4': (lib.vp_col_sums_masked_f32(ctx, F, C + 2, F, C, V, V, V, V, 0.0, M, C, S, W, need, st), EUNSUP),
    }
    torch.cuda.synchronize()
    wrong = {k: (rc, want) for k, (rc, want) in calls.items() if rc != want}
    assert not wrong, wrong
    assert (out == SENTINEL).all() and (out16 == SENTINEL).all() and (sums == SENTINEL).all()
    assert lib.vp_col_sums_workspace_bytes(M, C) == 1024 * 2 * C * 4 + 256 and need_db == 1024 * C * 4 + 256
