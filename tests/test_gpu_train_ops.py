"""The training step's small kernels (csrc/train_ops.hip, csrc/se_train.hip), entry point by entry point through ppvector._native,
against the float64 oracle of tests/train_ops_oracle.py at the shapes where each takes another branch (docs/train_ops.md has the map
from case to branch).  Run with -m gpu on an MI355X.

Two input families per test.  'exact': small integers and dyadic rationals, every product and partial sum representable in float32
in any order (tests/test_train_ops_oracle_cpu.py proves that for every case planted here), so the kernel must EQUAL float64 element for
element -- or differ by at most as many ulps as the formula has inexact steps, a count each test states.  'gauss': standard normal,
per element |err| <= (n_terms + k) 2^-24 sum|terms|, a bound on any float32 evaluation; it only guards the scale.  Kernels that move
or select data are bit-equal on both.  Every output lies between sentinel margins that must come back untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import train_ops_oracle as O

pytestmark = pytest.mark.gpu

F32, F64, U = np.float32, np.float64, O.U
SENT = -768.0                   # exact in bf16 too
MARGIN = 64                     # elements on either side of every output (256 bytes of f32, 128 of bf16): the payload stays 16-byte aligned
VP_EINVAL, VP_EUNSUP, VP_EWORKSPACE = -1, -4, -5
FAMILIES = ('exact', 'gauss')
TINY = 3 * 2.0 ** -149           # three roundings into the float32 subnormals (sigmoid(-100) is one): the relative model ends there


@pytest.fixture(scope='module')
def N():
    from ppvector import _native as N
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: these tests must run on an MI355X (no CPU fallback exists)')
    N.ctx(0)
    return N


class Buf:
    """n elements on the GPU between two sentinel margins (`shift` more elements in front: a deliberately odd address)."""

    def __init__(self, n, init=None, dtype=torch.float32, shift=0):
        self.n, self.lo = int(n), MARGIN + shift
        self.full = torch.full((self.n + self.lo + MARGIN,), SENT, dtype=dtype, device='cuda')
        self.t = self.full[self.lo:self.lo + self.n]
        if init is not None:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(init)).reshape(-1).to(dtype))

    @property
    def p(self):
        return self.t.data_ptr()

    def get(self, shape=None):
        """The payload as a CPU array, after asserting that both margins still hold the sentinel."""
        torch.cuda.synchronize()
        assert bool((self.full[:self.lo] == SENT).all()) and bool((self.full[self.lo + self.n:] == SENT).all()), 'a margin was written'
        a = self.t.cpu()
        a = a.numpy() if a.dtype != torch.bfloat16 else a
        return a if shape is None else a.reshape(shape)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.full == SENT).all())


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


def devs(*arrays):
    """The arrays on the GPU and their addresses; the caller holds the tensors for as long as a kernel may read them."""
    ts = [dev(a) for a in arrays]
    return ts, [t.data_ptr() for t in ts]


def env(N):
    return N.lib(), N.ctx(0), N.stream_ptr()


def same(got, ref, what=''):
    """Bit-equal to the float64 reference (which must itself be a float32 number)."""
    got, ref = np.asarray(got), np.asarray(ref, F64)
    assert got.dtype in (F32, F64) and got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = got.astype(F64) != ref
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        pytest.fail(f'{what}: {int(bad.sum())} of {bad.size} elements differ from float64, first at {i}: {got[i]!r} != {ref[i]!r}')


def rounded(got, ref, what=''):
    """Equal to the float64 reference rounded to nearest even: the formula ends in one rounding of an exact value."""
    same(got, np.asarray(ref, F64).astype(F32).astype(F64), what)


def within(got, ref, bound, what=''):
    got, ref, bound = np.asarray(got), np.asarray(ref, F64), np.asarray(bound, F64)
    assert got.dtype in (F32, F64) and got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bound)                                        # NaN fails
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        pytest.fail(f'{what}: {int(bad.sum())} of {bad.size} elements out of bound, first at {i}: {got[i]!r} vs {ref[i]!r}, '
                    f'err {err[i]:.3e} > {np.broadcast_to(bound, err.shape)[i]:.3e}; worst err/bound {np.nanmax(err / np.maximum(bound, 1e-300)):.2f}')


def ulps_within(got, ref, k, what=''):
    """At most k float32 ulps from the float64 reference: k = the formula's count of inexact operations."""
    u = O.ulps(got, ref)
    assert np.all(u <= k), f'{what}: worst {float(np.max(u)):.2f} ulps > {k}'


def check(fam, got, ref, bound, what=''):
    same(got, ref, what) if fam == 'exact' else within(got, ref, bound, what)


# ------------------------------------------------------------------------------------------------ weight layouts
def _layouts(N, w, which, KF=None, KT=None):
    lib, ctx, st = env(N)
    Cout, Cin = w.shape[:2]
    n = w.size
    wd = dev(w)
    wp, w2 = Buf(n), Buf(n)
    a = wp.p if which in ('wp', 'both') else None
    b = w2.p if which in ('w2', 'both') else None
    if KF is None:
        N.check(lib.vp_conv_weight_layouts_f32(ctx, wd.data_ptr(), Cout, Cin, w.shape[2], a, b, st), ctx)
    else:
        N.check(lib.vp_conv2d_weight_layouts_f32(ctx, wd.data_ptr(), Cout, Cin, KF, KT, a, b, st), ctx)
    rp, r2 = O.weight_layouts(w)
    if a:
        assert np.array_equal(wp.get(rp.shape), rp)
    else:
        assert wp.untouched()
    if b:
        assert np.array_equal(w2.get(r2.shape), r2)
    else:
        assert w2.untouched()


@pytest.mark.parametrize('which', ['wp', 'w2', 'both'])
@pytest.mark.parametrize('Cout,Cin,KW', O.LAYOUT_SHAPES)
def test_conv_weight_layouts(N, Cout, Cin, KW, which):
    """wp[o][tap Cin + c] and w2[c][(KW-1-tap) Cout + o] from (Cout, Cin, KW), either output alone or both: bit-equal; a NULL output's
    buffer is not written."""
    for fam in FAMILIES:
        g = O.rng(Cout, Cin, KW)
        _layouts(N, O.ints(g, (Cout, Cin, KW)) if fam == 'exact' else O.gauss(g, (Cout, Cin, KW)), which)


@pytest.mark.parametrize('which', ['wp', 'w2', 'both'])
@pytest.mark.parametrize('KF,KT', O.LAYOUT_2D)
def test_conv2d_weight_layouts(N, KF, KT, which):
    """The 2-D panels: tap order kt KF + kf from the model's (Cout, Cin, KF, KT), incl. the degenerate 1 x 3, 3 x 1 and 1 x 1."""
    for Cout, Cin, _ in O.LAYOUT_SHAPES:
        for fam in FAMILIES:
            g = O.rng(Cout, Cin, KF, KT)
            shape = (Cout, Cin, KF, KT)
            _layouts(N, O.ints(g, shape) if fam == 'exact' else O.gauss(g, shape), which, KF, KT)
    lib, ctx, st = env(N)
    w = dev(np.zeros(16, F32))
    assert lib.vp_conv2d_weight_layouts_f32(ctx, w.data_ptr(), 2, 2, 2, 2, None, None, st) == VP_EINVAL


# ------------------------------------------------------------------------------------------------ bf16 weight panels
@pytest.mark.parametrize('fam', FAMILIES)
def test_prep_weights_bf16_edges_and_two_launches(N, fam):
    """25 matrices in one call (24 per launch: two launches): rows / cols off the 64 x 64 tile (65 x 1, 1 x 65, 130 x 70), column slices
    (ld > cols, c0 > 0), w16 only, wt16 only.  Bit-equal to torch's .to(bfloat16) and its transpose; nothing outside is written."""
    lib, ctx, st = env(N)
    E = O.PREP_ENTRIES
    n = len(E)
    ws, a16, t16, refs = [], [], [], []
    for i, (rows, ld, c0, nc, want_a, want_t) in enumerate(E):
        g = O.rng(i, rows, ld)
        w = O.ints(g, (rows, ld), -256, 256) if fam == 'exact' else O.gauss(g, (rows, ld))
        ws.append(dev(w))
        a16.append(Buf(rows * nc, dtype=torch.bfloat16))
        t16.append(Buf(rows * nc, dtype=torch.bfloat16))
        refs.append(O.prep_bf16(w, c0, nc))
    arr = lambda t, v: (t * n)(*v)
    rc = lib.vp_prep_weights_bf16(ctx, arr(C.c_void_p, [w.data_ptr() + 4 * e[2] for w, e in zip(ws, E)]),
                                  arr(C.c_void_p, [b.p if e[4] else None for b, e in zip(a16, E)]),
                                  arr(C.c_void_p, [b.p if e[5] else None for b, e in zip(t16, E)]),
                                  arr(C.c_int, [e[0] for e in E]), arr(C.c_int, [e[3] for e in E]), arr(C.c_int, [e[1] for e in E]), n, st)
    N.check(rc, ctx)
    for i, (rows, ld, c0, nc, want_a, want_t) in enumerate(E):
        if want_a:
            assert torch.equal(a16[i].get((rows, nc)), refs[i][0]), (i, E[i])
        else:
            assert a16[i].untouched(), i
        if want_t:
            assert torch.equal(t16[i].get((nc, rows)), refs[i][1]), (i, E[i])
        else:
            assert t16[i].untouched(), i


# ------------------------------------------------------------------------------------------------ optimisers
def _opt_state(n, fam):
    host = O.opt_inputs(n, fam)
    return host, [Buf(n, a) for a in host]


@pytest.mark.parametrize('step', O.OPT_STEPS)
@pytest.mark.parametrize('n', O.OPT_SIZES)
def test_adam_and_adamw_per_element(N, n, step):
    """vp_adam_step_f32 / vp_adamw_step_f32 on flat buffers of 1, 255 and 16 384 * 256 + 3 * 256 + 5 elements (the grid-stride loop's
    second trip, ragged), steps 1, 2, 1000, grad_scale != 1, weight decay 0 and not.  Compared per element: m, v and the UPDATE
    p_new - p_old (p itself would hide it behind |p|).  exact family (dyadic hyper-parameters): m and v equal float64; the update has
    6 inexact steps -- m / c1, v / c2, sqrt, + eps and the quotient on the step (lr is a power of two, beta^t exact or underflowed),
    then p_new -- and must lie within 5 ulps of |step| plus 1 ulp of |p_new| (10 x 2^-24 |step| + 2 x 2^-24 |p_new|).
    gauss: the bounds of train_ops_oracle.adam_bounds."""
    lib, ctx, st = env(N)
    k = min(n, 4093)                                             # the buffers repeat a block: the oracle sees one block
    for fam in FAMILIES:
        for wd in (0.0, 0.25 if fam == 'exact' else 1e-2):
            for name, decoupled in (('adam', False), ('adamw', True)):
                kw = dict(O.EXACT_OPT if fam == 'exact' else O.GAUSS_OPT, wd=wd, step=step)
                host, (p, g, m, v) = _opt_state(n, fam)
                fn = lib.vp_adamw_step_f32 if decoupled else lib.vp_adam_step_f32
                N.check(fn(ctx, p.p, g.p, m.p, v.p, n, kw['lr'], kw['b1'], kw['b2'], kw['eps'], wd, step, kw['gscale'], st), ctx)
                blk = [a[:k] for a in host]
                ru, rm, rv = (np.resize(a, n) for a in O.adam(*blk, decoupled=decoupled, **kw))
                eu, em, ev = (np.resize(a, n) for a in O.adam_bounds(*blk, decoupled=decoupled, exact_moments=(fam == 'exact'), **kw))
                what = f'{name} {fam} wd={wd}'
                assert np.array_equal(g.get(), host[1])
                check(fam, m.get(), rm, em, what + ' m')
                check(fam, v.get(), rv, ev, what + ' v')
                within(p.get().astype(F64) - host[0], ru, eu, what + ' update')        # the difference of two float32 is exact here


@pytest.mark.parametrize('n', O.OPT_SIZES)
def test_momentum_nesterov_sgd_per_element(N, n):
    """vp_momentum_step_f32: momentum 0.9 / 0.5, Nesterov, and SGD (momentum 0), weight decay 0 and not, grad_scale != 1.  exact family:
    velocity and update equal float64 (nothing in the formula is inexact on dyadic inputs); gauss: train_ops_oracle.momentum_bounds."""
    lib, ctx, st = env(N)
    k = min(n, 4093)
    for fam in FAMILIES:
        lr, gs = (0.125, 0.5) if fam == 'exact' else (0.05, 0.37)
        for mu, nest in ((0.5 if fam == 'exact' else 0.9, 0), (0.5 if fam == 'exact' else 0.9, 1), (0.0, 0)):
            for wd in (0.0, 0.25 if fam == 'exact' else 1e-2):
                host, (p, g, vel, _) = _opt_state(n, fam)
                N.check(lib.vp_momentum_step_f32(ctx, p.p, g.p, vel.p, n, lr, mu, wd, nest, gs, st), ctx)
                blk = [a[:k] for a in host[:3]]
                ru, rv = (np.resize(a, n) for a in O.momentum(*blk, lr, mu, wd, nest, gs))
                eu, ev = (np.resize(a, n) for a in O.momentum_bounds(*blk, lr, mu, wd, nest, gs))
                what = f'momentum {fam} mu={mu} nesterov={nest} wd={wd}'
                check(fam, vel.get(), rv, ev, what + ' velocity')
                check(fam, p.get().astype(F64) - host[0], ru, eu, what + ' update')


def test_optimisers_reject_bad_arguments(N):
    lib, ctx, st = env(N)
    b = [Buf(8, np.ones(8, F32)) for _ in range(4)]
    assert lib.vp_adam_step_f32(ctx, b[0].p, b[1].p, b[2].p, b[3].p, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1.0, st) == VP_EINVAL     # step 0
    assert lib.vp_adamw_step_f32(ctx, b[0].p, b[1].p, b[2].p, b[3].p, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, st) == VP_EINVAL    # n 0
    assert lib.vp_momentum_step_f32(ctx, b[0].p, None, b[2].p, 8, 1e-3, 0.9, 0.0, 0, 1.0, st) == VP_EINVAL
    for x in b:
        assert np.all(x.get() == 1.0)


# ------------------------------------------------------------------------------------------------ gradient packing
def test_pack_segments_130_segments_every_path(N):
    """130 segments in one call (128 per launch: two launches) into a sentinel-filled flat buffer with gaps: a NULL source (zeros), a
    size-0 segment, an odd destination offset and a misaligned source (scalar path), a 16-byte-aligned segment with n % 4 == 3 (float4
    body + scalar tail) and one of 512 * 1024 + 1027 floats (past the 512-workgroup cap: the strided loops run again).  Integer and Gaussian
    values; bit-equal; the gaps and margins keep their sentinel."""
    lib, ctx, st = env(N)
    g = O.rng(130)
    sizes = [int(v) for v in g.integers(1, 300, size=130)]
    sizes[3], sizes[5], sizes[7], sizes[9], sizes[129] = 0, 4 * 9 + 3, 512 * 1024 + 1027, 1031, 4 * 5 + 3
    gaps = [int(v) * 4 for v in g.integers(0, 3, size=130)]       # offsets stay multiples of 4 (16-byte aligned) unless made odd below
    sizes = [s + (-s) % 4 if i not in (3, 5, 7, 129) else s for i, s in enumerate(sizes)]
    offs, cur = [], 0
    for i, s in enumerate(sizes):
        if i in (9, 64):
            cur += 1                                               # an odd offset: the scalar path
        elif cur % 4:
            cur += 4 - cur % 4
        offs.append(cur)
        cur += s + gaps[i]
    total = cur + 8
    assert offs[5] % 4 == 0 and sizes[5] % 4 == 3 and offs[7] % 4 == 0 and offs[9] % 2 == 1 and offs[11] % 4 == 0
    assert offs[2] % 4 == 0 and offs[128] % 4 == 0 and sizes[3] == 0 and sizes[7] == 512 * 1024 + 1027
    n = len(sizes)
    for fam in FAMILIES:
        host = [O.ints(g, s + 1, 1, 8) if fam == 'exact' else O.gauss(g, s + 1) for s in sizes]
        held = [dev(h) for h in host]
        srcs, ptrs = [], []
        for i, (h, d) in enumerate(zip(host, held)):
            if i in (2, 128):
                srcs.append(None); ptrs.append(None)                   # no gradient arrived: zeros
            elif i == 11:
                srcs.append(h[1:]); ptrs.append(d.data_ptr() + 4)      # source off the 16-byte grid, destination on it
            else:
                srcs.append(h); ptrs.append(d.data_ptr())
        dst = Buf(total)
        rc = lib.vp_pack_segments_f32(ctx, (C.c_void_p * n)(*ptrs), (C.c_longlong * n)(*offs), (C.c_longlong * n)(*sizes), n, dst.p, st)
        N.check(rc, ctx)
        ref = O.pack_segments(np.full(total, SENT, F32), srcs, offs, sizes)
        got = dst.get()
        bad = np.nonzero(got != ref)[0]
        assert bad.size == 0, f'{fam}: {bad.size} elements differ, first at {int(bad[0])}: segment starts {offs[:12]}'
    assert lib.vp_pack_segments_f32(ctx, (C.c_void_p * 1)(None), (C.c_longlong * 1)(-1), (C.c_longlong * 1)(4), 1, dst.p, st) == VP_EINVAL
    assert np.array_equal(dst.get(), ref)


# ------------------------------------------------------------------------------------------------ reflect fold
@pytest.mark.parametrize('Cc', O.FOLD_C)
@pytest.mark.parametrize('T,pad', O.FOLD_TP)
def test_reflect_fold_and_fold_into(N, T, pad, Cc):
    """vp_reflect_fold_f32 and vp_reflect_fold_into_f32 at pad = 0, pad = T - 1 ((2, 1), (5, 4)) and T <= 2 pad ((5, 4), (6, 3): a frame
    receives both mirror images), B = 3; _into writes a channel slice (lddx = C + 8, 4 channels in) of a sentinel-filled tensor, with
    and without add (ld_add = C + 4) / sum.  exact: equal float64; gauss: three terms (four in sum), (n + 1) 2^-24 sum|terms|."""
    lib, ctx, st = env(N)
    B = O.FOLD_B
    for fam in FAMILIES:
        dxp, = O.btc(B, T + 2 * pad, Cc, fam, 3, 1)
        add, = O.btc(B, T, Cc, fam, 4, 1)
        ref, rsum = O.reflect_fold(dxp, T, pad, add)
        ab, absum = O.reflect_fold(np.abs(dxp), T, pad, np.abs(add))
        dxpd = dev(dxp)
        dx = Buf(B * T * Cc)
        N.check(lib.vp_reflect_fold_f32(ctx, dxpd.data_ptr(), B, T, pad, Cc, dx.p, st), ctx)
        check(fam, dx.get((B, T, Cc)), ref, 4 * U * ab, f'fold {fam}')
        ldx, lda = Cc + 8, Cc + 4
        addw = np.full((B * T, lda), 99.0, F32)
        addw[:, :Cc] = add.reshape(B * T, Cc)
        addd = dev(addw)
        for with_add in (False, True):
            wide, sm = Buf(B * T * ldx), Buf(B * T * Cc)
            rc = lib.vp_reflect_fold_into_f32(ctx, dxpd.data_ptr(), B, T, pad, Cc, wide.p + 16, ldx, addd.data_ptr() if with_add else None,
                                              lda if with_add else 0, sm.p if with_add else None, st)
            N.check(rc, ctx)
            w = wide.get((B * T, ldx))
            check(fam, np.ascontiguousarray(w[:, 4:4 + Cc]).reshape(B, T, Cc), ref, 4 * U * ab, f'fold_into {fam}')
            assert np.all(w[:, :4] == SENT) and np.all(w[:, 4 + Cc:] == SENT), 'fold_into wrote outside its channel slice'
            if with_add:
                check(fam, sm.get((B, T, Cc)), rsum, 5 * U * absum, f'fold_into sum {fam}')
            else:
                assert sm.untouched()


def test_reflect_fold_rejects_what_it_cannot_do(N):
    """pad >= T, C % 4 != 0 and a misaligned dx: VP_EINVAL, nothing written."""
    lib, ctx, st = env(N)
    src = dev(np.ones(3 * 20 * 8, F32))
    dx, sm = Buf(3 * 8 * 8 + 8), Buf(3 * 8 * 8)
    p = src.data_ptr()
    assert lib.vp_reflect_fold_f32(ctx, p, 3, 4, 4, 8, dx.p, st) == VP_EINVAL
    assert lib.vp_reflect_fold_f32(ctx, p, 3, 4, 5, 8, dx.p, st) == VP_EINVAL
    assert lib.vp_reflect_fold_f32(ctx, p, 3, 4, 1, 6, dx.p, st) == VP_EINVAL
    assert lib.vp_reflect_fold_into_f32(ctx, p, 3, 4, 4, 8, dx.p, 8, None, 0, None, st) == VP_EINVAL
    assert lib.vp_reflect_fold_into_f32(ctx, p, 3, 4, 1, 6, dx.p, 8, None, 0, None, st) == VP_EINVAL
    assert lib.vp_reflect_fold_into_f32(ctx, p, 3, 4, 1, 8, dx.p + 4, 8, None, 0, None, st) == VP_EINVAL       # dx off the 16-byte grid
    assert lib.vp_reflect_fold_into_f32(ctx, p, 3, 4, 1, 8, dx.p, 10, None, 0, None, st) == VP_EINVAL          # lddx % 4
    assert lib.vp_reflect_fold_into_f32(ctx, p, 3, 4, 1, 8, dx.p, 8, p, 8, None, st) == VP_EINVAL              # add without sum
    assert dx.untouched() and sm.untouched()


# ------------------------------------------------------------------------------------------------ zero insertion
@pytest.mark.parametrize('Cc', O.ZI_C)
@pytest.mark.parametrize('n_in,n_out', O.ZI_IN_OUT)
@pytest.mark.parametrize('st_,sf', O.ZI_STRIDES)
def test_zero_insert_2d(N, st_, sf, n_in, n_out, Cc):
    """up[b, t, f] = dz[b, t / st, f / sf] on the stride grid, zeros elsewhere -- (7, 3) at stride 2: row 6 has quotient 3 = T_out and must
    be ZERO, not a read past dz.  The same three (in, out) pairs on the F axis.  Bit-equal on both families."""
    lib, ctx, st = env(N)
    B = 2
    for T_in, T_out, F_in, F_out in ((n_in, n_out, 5, 3), (5, 3, n_in, n_out)):
        for fam in FAMILIES:
            g = O.rng(st_, sf, n_in, n_out, Cc)
            shape = (B, T_out, F_out, Cc)
            dz = O.ints(g, shape, 1, 8) if fam == 'exact' else O.gauss(g, shape)
            dzd = Buf(dz.size, dz)                                 # dz between sentinels: a read past it would show as -768
            up = Buf(B * T_in * F_in * Cc)
            N.check(lib.vp_zero_insert_2d_f32(ctx, dzd.p, B, T_out, F_out, Cc, T_in, F_in, st_, sf, up.p, st), ctx)
            assert np.array_equal(up.get((B, T_in, F_in, Cc)), O.zero_insert(dz, T_in, F_in, st_, sf)), (fam, T_in, F_in)
    assert lib.vp_zero_insert_2d_f32(ctx, dzd.p, B, T_out, F_out, 6, T_in, F_in, st_, sf, up.p, st) == VP_EINVAL


# ------------------------------------------------------------------------------------------------ SE gate backward
def _srb_inputs(B, T, Cc, fam):
    dy, x = O.btc(B, T, Cc, fam, 5, 2)
    s = O.gates(B, Cc, fam, 5)
    rdx, rds = O.scale_rows_bwd(dy, x, s)
    return dy, x, s, rdx, rds, O.scale_rows_bwd(np.abs(dy), np.abs(x), np.abs(s))[1]


@pytest.mark.parametrize('T', O.SRB_SIMPLE_T)
@pytest.mark.parametrize('Cc', O.SRB_SIMPLE_C)
def test_scale_rows_bwd_simple_kernel(N, Cc, T):
    """vp_scale_rows_bwd_f32 (a workgroup per 64 channels of an utterance, four row groups): C = 5, 64, 70 (a second workgroup with six live
    lanes), T = 1, 3 (idle row groups), 4, 9.  dx = dy * s is one rounding of an exact product: equal to float64 rounded, both families;
    ds: exact / (T + 1) 2^-24 sum|dy x|."""
    lib, ctx, st = env(N)
    B = O.SRB_B
    for fam in FAMILIES:
        dy, x, s, rdx, rds, ab = _srb_inputs(B, T, Cc, fam)
        dx, ds = Buf(B * T * Cc), Buf(B * Cc)
        hold, ins = devs(dy, x, s)
        N.check(lib.vp_scale_rows_bwd_f32(ctx, *ins, B, T, Cc, dx.p, ds.p, st), ctx)
        rounded(dx.get((B, T, Cc)), rdx, f'dx {fam}')
        check(fam, ds.get((B, Cc)), rds, (T + 1) * U * ab, f'ds {fam}')


@pytest.mark.parametrize('Cc', O.SRB_CHUNK_C)
def test_scale_rows_bwd_chunked_kernel(N, Cc):
    """vp_scale_rows_bwd_ws_f32 at C = 4 (one lane per row, 256 row groups), 12 (an idle lane in every row), 40, 1024 (one row group) and
    T = 1, 8 RG (two four-row trips, no tail), 8 RG + 1 (one row of tail), 2 rpc + RG - 1 (three chunks, the last with
    fewer rows than row groups).  The workspace is exactly vp_scale_rows_bwd_workspace_bytes with a sentinel after it; one byte less is
    VP_EWORKSPACE and writes nothing."""
    lib, ctx, st = env(N)
    B = O.SRB_B
    for T in O.srb_chunk_T(B, Cc):
        for fam in FAMILIES:
            dy, x, s, rdx, rds, ab = _srb_inputs(B, T, Cc, fam)
            need = int(lib.vp_scale_rows_bwd_workspace_bytes(B, T, Cc))
            _, rpc, chunks = O.srb_geometry(B, T, Cc)
            assert need == B * chunks * Cc * 4 + 256
            dx, ds, ws = Buf(B * T * Cc), Buf(B * Cc), Buf(need // 4)
            hold, ins = devs(dy, x, s)
            args = (ctx, *ins, B, T, Cc, dx.p, ds.p, ws.p)
            assert lib.vp_scale_rows_bwd_ws_f32(*args, need - 1, st) == VP_EWORKSPACE
            assert dx.untouched() and ds.untouched() and ws.untouched()
            N.check(lib.vp_scale_rows_bwd_ws_f32(*args, need, st), ctx)
            ws.get()                                               # margins after the workspace
            rounded(dx.get((B, T, Cc)), rdx, f'dx {fam} T={T}')
            check(fam, ds.get((B, Cc)), rds, (T + 2) * U * ab, f'ds {fam} T={T}')


def test_scale_rows_bwd_ws_unsupported_shapes(N):
    """C = 1028 and C % 4 != 0: VP_EUNSUP (the caller keeps the simple kernel), nothing written; the workspace query answers 0."""
    lib, ctx, st = env(N)
    src = dev(np.ones(2 * 3 * 1028, F32))
    dx, ds, ws = Buf(2 * 3 * 1028), Buf(2 * 1028), Buf(4096)
    for Cc in (1028, 6, 70):
        assert lib.vp_scale_rows_bwd_workspace_bytes(2, 3, Cc) == 0
        assert lib.vp_scale_rows_bwd_ws_f32(ctx, src.data_ptr(), src.data_ptr(), src.data_ptr(), 2, 3, Cc, dx.p, ds.p, ws.p, 4096 * 4, st) == VP_EUNSUP
    assert dx.untouched() and ds.untouched() and ws.untouched()


# ------------------------------------------------------------------------------------------------ utterance dots, scale + shift
@pytest.mark.parametrize('Cc', O.UTT_C)
@pytest.mark.parametrize('T', O.UTT_T)
def test_utt_dot_and_scale_shift_rows(N, T, Cc):
    """vp_utt_dot_f32 / _x16 / _z16 around the 32-frame unrolled trip (t + 24 < T) and the 8-frame tail: T = 1, 7, 8, 9 (tail only), 25, 32
    (one trip, no tail), 33, 57 (trips + ragged tail); C/4 = 1, 32, 33 (a second workgroup with one live lane); B = 2.  exact: equal
    float64 (the bf16 operands are integers <= 256; bf16(fma(z, scale, shift)) is a plain round-to-nearest-even of an exact float32);
    gauss: (T + 1) 2^-24 sum|dy x|.  vp_scale_shift_rows_f32 on the same grid: with dm a power of two and 1/T taken as the float32 the
    entry point passes, the fma is ONE rounding of an exact value: equal to float64 rounded; gauss: 3 roundings."""
    lib, ctx, st = env(N)
    B = O.UTT_B
    for fam in FAMILIES:
        dy, x = O.btc(B, T, Cc, fam, 6, 2)
        z = O.bf16_operand(B, T, Cc, fam, 6)
        sc, sh = O.bn_affine(Cc, fam, 6)
        dyd, zd, xd, scd, shd = dev(dy), dev(z, torch.bfloat16), dev(x), dev(sc), dev(sh)
        for name, ref, ab, call in (
                ('f32', O.utt_dot(dy, x), O.utt_dot(np.abs(dy), np.abs(x)),
                 lambda o: lib.vp_utt_dot_f32(ctx, dyd.data_ptr(), xd.data_ptr(), B, T, Cc, o, st)),
                ('x16', O.utt_dot(dy, z), O.utt_dot(np.abs(dy), np.abs(z)),
                 lambda o: lib.vp_utt_dot_x16(ctx, dyd.data_ptr(), zd.data_ptr(), B, T, Cc, o, st)),
                ('z16', O.utt_dot(dy, z, sc, sh), O.utt_dot(np.abs(dy), np.abs(O.bn_apply_bf16(z, sc, sh))),
                 lambda o: lib.vp_utt_dot_z16(ctx, dyd.data_ptr(), zd.data_ptr(), scd.data_ptr(), shd.data_ptr(), B, T, Cc, o, st))):
            ds = Buf(B * Cc)
            N.check(call(ds.p), ctx)
            check(fam, ds.get((B, Cc)), ref, (T + 1) * U * ab, f'utt_dot_{name} {fam}')
        s = O.gates(B, Cc, fam, 7)
        dm = O.dyads(O.rng(T, Cc, 8), (B, Cc), (1.0, 2.0, 4.0, 0.5)) if fam == 'exact' else O.gates(B, Cc, fam, 8)
        dx = Buf(B * T * Cc)
        hold, (sp, dmp) = devs(s, dm)
        N.check(lib.vp_scale_shift_rows_f32(ctx, dyd.data_ptr(), sp, dmp, B, T, Cc, dx.p, st), ctx)
        ref = O.scale_shift_rows(dy, s, dm, T)
        if fam == 'exact':
            rounded(dx.get((B, T, Cc)), ref, 'scale_shift_rows exact')
        else:
            within(dx.get((B, T, Cc)), ref, 3 * U * O.scale_shift_rows(np.abs(dy), np.abs(s), np.abs(dm), T), 'scale_shift_rows gauss')


def test_utt_dot_rejects_bad_arguments(N):
    lib, ctx, st = env(N)
    src = dev(np.ones(64, F32))
    ds = Buf(16)
    p = src.data_ptr()
    assert lib.vp_utt_dot_f32(ctx, p, p, 1, 2, 6, ds.p, st) == VP_EINVAL
    assert lib.vp_utt_dot_f32(ctx, p + 4, p, 1, 2, 4, ds.p, st) == VP_EINVAL
    assert lib.vp_utt_dot_x16(ctx, p, p + 2, 1, 2, 4, ds.p, st) == VP_EINVAL
    assert lib.vp_scale_shift_rows_f32(ctx, p, p, p, 1, 2, 6, ds.p, st) == VP_EINVAL
    assert ds.untouched()


# ------------------------------------------------------------------------------------------------ activations
def _act_block(kind, seed):
    """inputs, float64 outputs, and the forward bound of one 4093-block (long buffers repeat it)."""
    x = O.act_inputs(4093, seed)
    return x, O.act(kind, x), O.act_bound(kind, x)


@pytest.mark.parametrize('n', [4, O.ACT_BIG_N])
@pytest.mark.parametrize('kind', list(O.ACTS))
def test_activation_forward(N, kind, n):
    """vp_act_f32, all five kinds, over the planted values (0, +-2^-126, +-1, 20 - 2^-19, 20, 20 + 2^-19, +-30, +-100) and Gaussian ones;
    n = 4 (one float4) and 4 (16 384 * 256) + 8 (the grid-stride loop's second trip: two float4).  ReLU and hardtanh20 select: bit-equal.
    tanh, sigmoid, SiLU: |err| <= bound (|ref| + 2^-100), bound = 4 x the worst relative error of the float32 CPU restatement of the
    same formula on the same inputs (docs/train_ops.md quotes it) -- never the kernel's own output.  No NaN or Inf at +-100."""
    lib, ctx, st = env(N)
    xb, rb, (measured, bound) = _act_block(kind, 1)
    if n == 4:                                                     # the twelve planted values, four at a time
        chunks = [xb[i:i + 4] for i in (0, 4, 8)]
    else:
        chunks = [np.resize(xb, n)]
    for x in chunks:
        ref = O.act(kind, x) if n == 4 else np.resize(rb, n)
        y, xd = Buf(len(x)), dev(x)
        N.check(lib.vp_act_f32(ctx, O.ACTS[kind], xd.data_ptr(), len(x), y.p, st), ctx)
        got = y.get()
        assert np.all(np.isfinite(got)), kind
        if kind in ('relu', 'hardtanh20'):
            same(got, ref, kind)
        else:
            within(got, ref, bound * (np.abs(ref) + O.REL_FLOOR), f'{kind} (float32 itself: {measured:.3e}, bound {bound:.3e})')


@pytest.mark.parametrize('n', [4, O.ACT_BIG_N])
@pytest.mark.parametrize('kind', list(O.ACTS))
def test_activation_backward(N, kind, n):
    """vp_act_bwd_f32 (and vp_relu_bwd_f32) from the OUTPUT y (SiLU: the input).  Conventions pinned: ReLU'(0) = 0, hardtanh20' = 0 at an
    output of exactly 0 or 20 and 1 one ulp inside.  The masks are bit-equal.  tanh / sigmoid: exact family (y dyadic, dy integer) equals
    float64; gauss 3 roundings: 3 2^-24 |dy| (1 + y^2) resp. |dy| |y| (1 + |y|), plus 3 x 2^-149 where the result is subnormal.  
    SiLU: |err| <= |dy| x 4 m sg (1 + |x|), m the float32 CPU restatement's worst error of the derivative in units of sg (1 + |x|), the
    size of its terms (train_ops_oracle.silu_bwd_bound): relative where the derivative is tiny."""
    lib, ctx, st = env(N)
    xb, yb, _ = _act_block(kind, 2)
    src = xb if kind == 'silu' else yb.astype(F32)                 # what the entry point is handed
    cases = [('gauss', src, O.gauss(O.rng(ord(kind[0]), 3), 4093)), ('exact',) + O.act_bwd_exact_inputs(kind)]
    for fam, v, dy in cases:
        ref = O.act_bwd(kind, dy, v)
        if kind == 'tanh':
            bound = 3 * U * np.abs(dy) * (1 + v.astype(F64) ** 2) + TINY * (1 + np.abs(dy))
        elif kind == 'sigmoid':
            bound = 3 * U * np.abs(dy) * np.abs(v) * (1 + np.abs(v.astype(F64))) + TINY * (1 + np.abs(dy))
        elif kind == 'silu':
            bound = O.silu_bwd_bound(v)[1] * np.abs(dy)
        else:
            bound = None
        if n == 4:
            idx = [slice(0, 4), slice(4, 8), slice(8, 12)]
            runs = [(v[i], dy[i], ref[i], None if bound is None else bound[i]) for i in idx]
        else:
            runs = [tuple(None if a is None else np.resize(a, n) for a in (v, dy, ref, bound))]
        for vv, dd, rr, bb in runs:
            hold, (ddp, vvp) = devs(dd, vv)
            fns = [lambda o: lib.vp_act_bwd_f32(ctx, O.ACTS[kind], ddp, vvp, len(vv), o, st)]
            if kind == 'relu':
                fns.append(lambda o: lib.vp_relu_bwd_f32(ctx, ddp, vvp, len(vv), o, st))
            for fn in fns:
                dz = Buf(len(vv))
                N.check(fn(dz.p), ctx)
                got = dz.get()
                assert np.all(np.isfinite(got))
                if bb is None or (fam == 'exact' and kind != 'silu'):
                    same(got, rr, f'{kind} backward {fam}')
                else:
                    within(got, rr, bb, f'{kind} backward {fam}')


def test_activation_conventions_and_bad_arguments(N):
    """The derivative conventions at the kinks, spelled out, and n % 4 != 0 -> VP_EINVAL with nothing written."""
    lib, ctx, st = env(N)
    y = np.asarray([0.0, 2.0 ** -126, 20.0 - 2.0 ** -19, 20.0, -0.0, 1.0, 19.0, 20.0], F32)
    dy, yd = dev(np.full(8, 3.0, F32)), dev(y)
    for act, fn, expect in (('relu', 'act', [0, 3, 3, 3, 0, 3, 3, 3]), ('relu', 'relu', [0, 3, 3, 3, 0, 3, 3, 3]),
                            ('hardtanh20', 'act', [0, 3, 3, 0, 0, 3, 3, 0])):
        dz = Buf(8)
        if fn == 'act':
            N.check(lib.vp_act_bwd_f32(ctx, O.ACTS[act], dy.data_ptr(), yd.data_ptr(), 8, dz.p, st), ctx)
        else:
            N.check(lib.vp_relu_bwd_f32(ctx, dy.data_ptr(), yd.data_ptr(), 8, dz.p, st), ctx)
        assert dz.get().tolist() == expect, (act, fn)
    x = dev(np.asarray([20.0 + 2.0 ** -19, -2.0 ** -126, 100.0, -100.0], F32))
    out = Buf(4)
    N.check(lib.vp_act_f32(ctx, O.ACTS['hardtanh20'], x.data_ptr(), 4, out.p, st), ctx)
    assert out.get().tolist() == [20.0, 0.0, 20.0, 0.0]
    out = Buf(8)
    for n in (6, 7, 0):
        assert lib.vp_act_f32(ctx, O.ACTS['tanh'], dy.data_ptr(), n, out.p, st) == VP_EINVAL
        assert lib.vp_act_bwd_f32(ctx, O.ACTS['tanh'], dy.data_ptr(), dy.data_ptr(), n, out.p, st) == VP_EINVAL
        assert lib.vp_relu_bwd_f32(ctx, dy.data_ptr(), dy.data_ptr(), n, out.p, st) == VP_EINVAL
    assert lib.vp_act_f32(ctx, 0, dy.data_ptr(), 8, out.p, st) == VP_EINVAL and lib.vp_act_f32(ctx, 6, dy.data_ptr(), 8, out.p, st) == VP_EINVAL
    assert out.untouched()


# ------------------------------------------------------------------------------------------------ AFF combine
@pytest.mark.parametrize('rows,Cc', O.AFF_SHAPES)
def test_aff_combine_and_backward(N, rows, Cc):
    """o = x (1 + t) + y (1 - t); dx = g (1 + t), dy = g (1 - t), dt = g (x - y) at 1 x 4 and 37 x 68.  exact (t dyadic in (-1, 1)): equal
    float64; gauss: 5 roundings forward, 2 per backward output, on sum|terms|."""
    lib, ctx, st = env(N)
    for fam in FAMILIES:
        r = O.rng(rows, Cc, 9)
        if fam == 'exact':
            g, x, y = (O.ints(r, (rows, Cc)) for _ in range(3))
            t = O.dyads(r, (rows, Cc), (-0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75))
        else:
            g, x, y = (O.gauss(r, (rows, Cc)) for _ in range(3))
            t = np.tanh(O.gauss(r, (rows, Cc))).astype(F32)
        gd, td, xd, yd = dev(g), dev(t), dev(x), dev(y)
        o = Buf(rows * Cc)
        N.check(lib.vp_aff_combine_f32(ctx, td.data_ptr(), xd.data_ptr(), yd.data_ptr(), rows, Cc, o.p, st), ctx)
        ag, at, ax, ay = (np.abs(a.astype(F64)) for a in (g, t, x, y))
        check(fam, o.get((rows, Cc)), O.aff_combine(t, x, y), 5 * U * (ax + ay) * (1 + at), f'aff {fam}')
        outs = [Buf(rows * Cc) for _ in range(3)]
        N.check(lib.vp_aff_combine_bwd_f32(ctx, gd.data_ptr(), td.data_ptr(), xd.data_ptr(), yd.data_ptr(), rows * Cc, *(b.p for b in outs), st), ctx)
        bounds = (2 * U * ag * (1 + at), 2 * U * ag * (1 + at), 2 * U * ag * (ax + ay))
        for b, ref, bd, nm in zip(outs, O.aff_combine_bwd(g, t, x, y), bounds, ('dx', 'dy', 'dt')):
            check(fam, b.get((rows, Cc)), ref, bd, f'aff bwd {nm} {fam}')
    assert lib.vp_aff_combine_f32(ctx, td.data_ptr(), xd.data_ptr(), yd.data_ptr(), rows, 6, o.p, st) == VP_EINVAL
    assert lib.vp_aff_combine_bwd_f32(ctx, gd.data_ptr(), td.data_ptr(), xd.data_ptr(), yd.data_ptr(), 6, *(b.p for b in outs), st) == VP_EINVAL


# ------------------------------------------------------------------------------------------------ CAM++ segment ops
@pytest.mark.parametrize('Cc', O.SEG_C + [5])
@pytest.mark.parametrize('seg', O.SEG_LENS)
def test_segment_context_forward_and_backward(N, seg, Cc):
    """vp_seg_ctx_f32 / vp_seg_ctx_bwd_f32, seg_len 100 and 4, T = 1, 3, seg - 1, seg, seg + 1, 2 seg, 2 seg + 37 (the last segment's mean
    over its valid frames only), C = 4, 64, 68 and 5 (no C % 4 requirement), B = 2.  exact family, NON-NEGATIVE integers (no cancellation
    between the two means): the sums are exact, then two quotients and one sum are inexact: <= 3 ulps.  gauss: (T + 3) resp.
    (nseg + 3) 2^-24 sum|terms|."""
    lib, ctx, st = env(N)
    B = O.SEG_B
    for T in O.seg_T(seg):
        nseg = -(-T // seg)
        for fam in FAMILIES:
            x, = O.btc(B, T, Cc, fam, 11, 1, nonneg=(fam == 'exact'))
            out, xd = Buf(B * nseg * Cc), dev(x)
            N.check(lib.vp_seg_ctx_f32(ctx, xd.data_ptr(), B, T, Cc, seg, out.p, st), ctx)
            ref = O.seg_ctx(x, seg)
            if fam == 'exact':
                ulps_within(out.get((B, nseg, Cc)), ref, 3, f'seg_ctx T={T}')
            else:
                within(out.get((B, nseg, Cc)), ref, (T + 3) * U * O.seg_ctx(np.abs(x), seg), f'seg_ctx gauss T={T}')
            dctx = O.seg_dctx(B, T, Cc, seg, fam)
            dx, dcd = Buf(B * T * Cc), dev(dctx)
            N.check(lib.vp_seg_ctx_bwd_f32(ctx, dcd.data_ptr(), B, T, Cc, seg, dx.p, st), ctx)
            ref = O.seg_ctx_bwd(dctx, T, seg)
            if fam == 'exact':
                ulps_within(dx.get((B, T, Cc)), ref, 3, f'seg_ctx_bwd T={T}')
            else:
                within(dx.get((B, T, Cc)), ref, (nseg + 3) * U * O.seg_ctx_bwd(np.abs(dctx), T, seg), f'seg_ctx_bwd gauss T={T}')


@pytest.mark.parametrize('Cc', O.SEG_C)
@pytest.mark.parametrize('seg', O.SEG_LENS)
def test_segment_scale_forward_and_backward(N, seg, Cc):
    """vp_seg_scale_f32 / vp_seg_scale_bwd_f32 on the same (seg_len, T, C) grid.  out = y * m and dy = g * m are one rounding of an exact
    product: equal to float64 rounded on both families.  dm: exact / (len + 1) 2^-24 sum|g y|.  (The backward takes C = 5 as well.)"""
    lib, ctx, st = env(N)
    B = O.SEG_B
    for T in O.seg_T(seg):
        nseg = -(-T // seg)
        for fam in FAMILIES:
            for C2 in ((Cc, 5) if Cc == 4 else (Cc,)):
                g, y = O.btc(B, T, C2, fam, 10, 2)
                m = O.gates(B, C2, fam, 10, nseg)
                gd, yd, md = dev(g), dev(y), dev(m)
                if C2 % 4 == 0:
                    out = Buf(B * T * C2)
                    N.check(lib.vp_seg_scale_f32(ctx, yd.data_ptr(), md.data_ptr(), B, T, C2, seg, out.p, st), ctx)
                    rounded(out.get((B, T, C2)), O.seg_scale(y, m, seg), f'seg_scale {fam} T={T}')
                dy, dm = Buf(B * T * C2), Buf(B * nseg * C2)
                N.check(lib.vp_seg_scale_bwd_f32(ctx, gd.data_ptr(), yd.data_ptr(), md.data_ptr(), B, T, C2, seg, dy.p, dm.p, st), ctx)
                rdy, rdm = O.seg_scale_bwd(g, y, m, seg)
                rounded(dy.get((B, T, C2)), rdy, f'seg_scale_bwd dy {fam} T={T}')
                check(fam, dm.get((B, nseg, C2)), rdm, (min(seg, T) + 1) * U * O.seg_scale_bwd(np.abs(g), np.abs(y), np.abs(m), seg)[1],
                      f'seg_scale_bwd dm {fam} T={T} C={C2}')
    assert lib.vp_seg_scale_f32(ctx, yd.data_ptr(), md.data_ptr(), B, 1, 6, seg, out.p, st) == VP_EINVAL


# ------------------------------------------------------------------------------------------------ SE dense layers
@pytest.mark.parametrize('rnd', [0, 1])
@pytest.mark.parametrize('B', O.SE_B)
@pytest.mark.parametrize('Cc,H', O.SE_SHAPES)
def test_se_dense_forward(N, Cc, H, B, rnd):
    """vp_se_dense_train_fwd at (C, H) = (4, 4), (64, 12), (516, 96: C/4 = 129, a second trip of st_matvec<16> with one live column),
    (1024, 1024), (80, 1000).  exact family: a equals float64 (with round_bf16 the operands are rounded to bf16 exactly where the
    oracle rounds them); s = sigmoid of an exact argument: the sigmoid bound (4 x float32's own error on these arguments).
    gauss: a within (C + 2) 2^-24 sum|terms|, s within a quarter of its argument's bound plus the sigmoid bound; with round_bf16 the
    argument's bound holds one bf16 ulp of |a| more (a is inexact when it is rounded: train_ops_oracle.se_fwd_bounds)."""
    lib, ctx, st = env(N)
    for fam in FAMILIES:
        mean, w1, b1, w2, b2 = O.se_fwd_inputs(B, Cc, H, fam)
        ra, rz, rs = O.se_dense_fwd(mean, w1, b1, w2, b2, rnd=rnd)
        a, s = Buf(B * H), Buf(B * Cc)
        hold, ins = devs(mean, w1, b1, w2, b2)
        N.check(lib.vp_se_dense_train_fwd(ctx, *ins, B, Cc, H, rnd, a.p, s.p, st), ctx)
        _, sb = O.act_bound('sigmoid', rz.astype(F32))
        if fam == 'exact':
            same(a.get((B, H)), ra, f'a rnd={rnd}')
            assert np.array_equal(rz.astype(F32).astype(F64), rz)
            within(s.get((B, Cc)), rs, sb * (rs + O.REL_FLOOR), f's rnd={rnd}')
        else:
            ea, ez = O.se_fwd_bounds(mean, w1, b1, w2, b2, rnd)
            within(a.get((B, H)), ra, ea, f'a gauss rnd={rnd}')
            within(s.get((B, Cc)), rs, 0.25 * ez + sb * rs, f's gauss rnd={rnd}')


@pytest.mark.parametrize('rnd', [0, 1])
@pytest.mark.parametrize('B', O.SE_B)
@pytest.mark.parametrize('Cc,H', O.SE_SHAPES)
def test_se_dense_backward(N, Cc, H, B, rnd):
    """vp_se_dense_train_bwd takes a and s as inputs: planted dyadic s in {1/4, 1/2, 3/4} and integer ds, a (with zeros: the ReLU mask),
    mean, W1, W2 -> dmean, dW1, db1, dW2, db2 all EQUAL float64, for H that do not divide 1024 (12, 96, 1000: 1024 / H groups and
    tid % H) and C that do not (516, 80).  gauss: train_ops_oracle.se_bwd_bounds (with round_bf16: one bf16 ulp more per rounded inexact operand).  The workspace is exactly
    vp_se_dense_train_bwd_workspace_bytes with a sentinel after it."""
    lib, ctx, st = env(N)
    need = int(lib.vp_se_dense_train_bwd_workspace_bytes(B, Cc, H))
    assert need == B * (Cc + H) * 4 + 256
    for fam in FAMILIES:
        ins = O.se_bwd_inputs(B, Cc, H, fam)
        refs = O.se_dense_bwd(*ins, rnd=rnd)
        bounds = O.se_bwd_bounds(*ins, rnd=rnd) if fam == 'gauss' else (None,) * 5
        outs = [Buf(n) for n in (B * Cc, H * Cc, H, Cc * H, Cc)]
        ws = Buf(need // 4)
        hold, ptrs = devs(*ins)
        N.check(lib.vp_se_dense_train_bwd(ctx, *ptrs, B, Cc, H, rnd, *(o.p for o in outs), ws.p, need, st), ctx)
        ws.get()
        for o, ref, bd, nm in zip(outs, refs, bounds, ('dmean', 'dW1', 'db1', 'dW2', 'db2')):
            check(fam, o.get(ref.shape), ref, bd, f'{nm} {fam} rnd={rnd}')


def test_se_dense_unsupported_shapes_and_short_workspace(N):
    """C = 6 (forward: C % 4), C = 1028, H = 1028: VP_EUNSUP; a workspace one byte short: VP_EWORKSPACE; nothing written either way."""
    lib, ctx, st = env(N)
    src = dev(np.ones(1028 * 1028, F32))
    p = src.data_ptr()
    outs = [Buf(1028 * 8) for _ in range(5)]
    ws = Buf(4096)
    for Cc, H in ((6, 8), (1028, 8), (8, 1028), (8, 6)):
        assert lib.vp_se_dense_train_fwd(ctx, p, p, p, p, p, 2, Cc, H, 0, outs[0].p, outs[1].p, st) == VP_EUNSUP, (Cc, H)
    for Cc, H in ((1028, 8), (8, 1028)):
        assert lib.vp_se_dense_train_bwd(ctx, p, p, p, p, p, p, 2, Cc, H, 0, *(o.p for o in outs), ws.p, 4096 * 4, st) == VP_EUNSUP, (Cc, H)
    need = int(lib.vp_se_dense_train_bwd_workspace_bytes(2, 8, 8))
    assert lib.vp_se_dense_train_bwd(ctx, p, p, p, p, p, p, 2, 8, 8, 0, *(o.p for o in outs), ws.p, need - 1, st) == VP_EWORKSPACE
    assert lib.vp_se_dense_train_bwd(ctx, p, p, p, p, p, p, 2, 8, 8, 0, *(o.p for o in outs), None, need, st) == VP_EWORKSPACE
    assert all(o.untouched() for o in outs) and ws.untouched()
