"""The inference path's small kernels (csrc/small_ops.hip), one public entry point at a time through ppvector._native, against the
float64 oracle of tests/small_ops_oracle.py at the shapes where each takes another branch (docs/small_ops.md has the map from case to
branch).  Run with -m gpu on an MI355X.

The machinery is that of tests/test_gpu_train_ops.py: two input families per test ('exact' must EQUAL float64, or differ by a counted
number of roundings; 'gauss' is bounded per element by (n_terms + k) 2^-24 sum|terms|), every output between sentinel margins that must
come back untouched, a rejected call leaves its outputs all sentinel.  Nothing here is judged by a norm."""
import numpy as np
import pytest
import torch

from tests import small_ops_oracle as S
from tests.test_gpu_train_ops import FAMILIES, SENT, VP_EINVAL, Buf, N, dev, devs, env, same, ulps_within, within  # noqa: F401

pytestmark = pytest.mark.gpu

F32, F64, U = np.float32, np.float64, S.U
BF = torch.bfloat16


def bits(t):
    """The raw 16-bit patterns of a bf16 tensor / 32-bit patterns of a float32 array."""
    return t.view(torch.int16).numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t).view(np.int32)


# ------------------------------------------------------------------------------------------------ vp_se_gate_fwd
@pytest.mark.parametrize('Cc,H,B,T', S.SE_GATE_FLAT)
def test_se_gate(N, Cc, H, B, T):
    """vp_se_gate_fwd from partial sums laid out as the convs leave them (NaN in every slot no tile row touches).  The time mean is split
    over max(1, 1024 / C) thread groups: 256 (C = 4), 16, 5 with 64 idle threads (192), 2 (512), and ONE group with idle threads at
    C = 516, 768, 1020 -- where the threads past C used to overwrite the mean of channels 0 .. 1023 - C with the bare shift.
    exact: integer means for any T, integer W1, W2 in {-1, 0, 1} / 2^k: the sigmoid's argument is exact, s within the sigmoid bound
    (4 x the measured float32 model of the fast exponential).  gauss: a quarter of the argument's accumulation bound more."""
    lib, ctx, st = env(N)
    for fam in FAMILIES:
        inp = S.se_gate_inputs(B, T, Cc, H, fam)
        for shift in ((inp[1], None) if fam == 'exact' else (inp[1],)):
            args = (inp[0], shift) + inp[2:]
            _, _, rz, rs = S.se_gate(*args, B, T)
            out = Buf(B * Cc)
            hold = [dev(a) for a in args if a is not None]
            p = [t.data_ptr() for t in hold]
            if shift is None:
                p.insert(1, None)
            N.check(lib.vp_se_gate_fwd(ctx, p[0], p[1], B, T, Cc, H, p[2], p[3], p[4], p[5], out.p, st), ctx)
            bound = S.sigmoid_bound(rz, rs)
            if fam == 'gauss':
                bound = bound + 0.25 * S.se_gate_bounds(*args, B, T)
            within(out.get((B, Cc)), rs, bound, f'se_gate {fam} shift={shift is not None}')


def test_se_gate_rejects(N):
    lib, ctx, st = env(N)
    src = dev(np.ones(1028 * 1028, F32))
    p = src.data_ptr()
    out = Buf(4 * 1028)
    for Cc, H in ((6, 8), (8, 6), (1028, 8), (8, 1028)):
        assert lib.vp_se_gate_fwd(ctx, p, p, 2, 3, Cc, H, p, p, p, p, out.p, st) != 0, (Cc, H)
    assert lib.vp_se_gate_fwd(ctx, None, p, 2, 3, 8, 8, p, p, p, p, out.p, st) == VP_EINVAL
    assert lib.vp_se_gate_fwd(ctx, p, p, 0, 3, 8, 8, p, p, p, p, out.p, st) == VP_EINVAL
    assert out.untouched()


# ------------------------------------------------------------------------------------------------ vp_moments_finalize(_affine)
_MOM = [(B, T, C) for B, T in S.BT_CASES for C in S.MOM_C] + [(B, T, 5) for B, T in S.BT_LONG]


@pytest.mark.parametrize('B,T,Cc', _MOM)
def test_moments_finalize(N, B, T, Cc):
    """vp_moments_finalize (shift NULL and given) and vp_moments_finalize_affine (scales of both signs and zero), want_std 0 and 1
    (ld = C vs 2C), C = 1, 5, 256, 257 (a second workgroup with one live lane), 300.  Planted with C >= 5: a constant channel and a
    channel of scale 0 (variance 0 -> sqrt(eps)), a channel whose float32 variance is negative (clamped: sqrt(eps), finite), and
    8 +- 1/4 (std within (T + 4) 2^-24 E[x^2] / (2 std)).
    exact with T a power of two: 1/T, the mean and the variance are exact -- the mean EQUALS float64, the std is within 3 ulps
    (scale^2 twice, sqrt).  Otherwise the roundings are counted: small_ops_oracle.moments_bounds."""
    lib, ctx, st = env(N)
    eps = S.MOM_EPS
    P = S.PLANTED
    for fam in FAMILIES:
        z, scale, shift = S.moments_inputs(B, T, Cc, fam)
        ps, psq = S.conv_psum(z), S.conv_psum(z * z)
        hold, (pps, ppsq, psc, psh) = devs(ps, psq, scale, shift)
        nt = S.moments_n_terms(B, T, Cc, fam)
        for want in (0, 1):
            ld = (1 + want) * Cc
            for sc, sh in ((None, None), (None, shift), (scale, shift)):
                stats = Buf(B * ld)
                if sc is None:
                    rc = lib.vp_moments_finalize(ctx, pps, ppsq if want else None, None if sh is None else psh, B, T, Cc, eps, want, stats.p, st)
                else:
                    rc = lib.vp_moments_finalize_affine(ctx, pps, ppsq if want else None, psc, psh, B, T, Cc, eps, want, stats.p, st)
                N.check(rc, ctx)
                got = stats.get((B, ld))
                ref = S.moments(ps, psq, sh, sc, B, T, eps, want)
                what = f'moments {fam} want_std={want} scale={sc is not None} shift={sh is not None}'
                assert np.all(np.isfinite(got)), what
                within(got, ref, S.moments_bounds(ps, psq, sh, sc, B, T, eps, want, nt), what)
                sharp = fam == 'exact' and S.is_pow2(T)
                keep = [c for c in range(Cc) if Cc < 5 or c != P['negvar']]
                if sharp:
                    same(got[:, keep], ref[:, keep], what + ' mean')
                if want and sharp:
                    ulps_within(got[:, [Cc + c for c in keep]], ref[:, [Cc + c for c in keep]], 3, what + ' std')
                if want and Cc >= 5:
                    root = np.full(B, np.sqrt(F64(F32(eps))))
                    for name in ('const', 'negvar') + (('scale0',) if sc is not None else ()):
                        ulps_within(got[:, Cc + P[name]], root, 1, f'{what}: {name} channel is sqrt(eps)')
                    if T > 1:
                        c = Cc + P['near']
                        within(got[:, c], ref[:, c], S.planted_std_bound(psq, sc, ref[:, Cc:], B, T)[:, P['near']], what + ' mean 8, std 1/4')


def test_moments_finalize_rejects(N):
    """NULL psumsq with want_std, B = 65536 (past the grid's y limit: no launch), NULL scale for the affine entry: VP_EINVAL, nothing written."""
    lib, ctx, st = env(N)
    src = dev(np.ones(4096, F32))
    p = src.data_ptr()
    stats = Buf(64)
    assert lib.vp_moments_finalize(ctx, p, None, p, 2, 3, 8, 1e-5, 1, stats.p, st) == VP_EINVAL
    assert lib.vp_moments_finalize_affine(ctx, p, None, p, p, 2, 3, 8, 1e-5, 1, stats.p, st) == VP_EINVAL
    assert lib.vp_moments_finalize(ctx, p, p, p, 65536, 3, 8, 1e-5, 1, stats.p, st) == VP_EINVAL
    assert lib.vp_moments_finalize_affine(ctx, p, p, p, p, 65536, 3, 8, 1e-5, 0, stats.p, st) == VP_EINVAL
    assert lib.vp_moments_finalize_affine(ctx, p, p, None, p, 2, 3, 8, 1e-5, 1, stats.p, st) == VP_EINVAL
    assert lib.vp_moments_finalize_affine(ctx, p, p, p, None, 2, 3, 8, 1e-5, 1, stats.p, st) == VP_EINVAL
    assert lib.vp_moments_finalize(ctx, p, p, p, 2, 0, 8, 1e-5, 1, stats.p, st) == VP_EINVAL
    assert stats.untouched()


# ------------------------------------------------------------------------------------------------ SE scale + residual
SE_BT = (3, 37)
SE_BIG_BT = (2, 4097)            # with C = 129 (f32, bf16) or 132 (HL32) vectors per row: past 4096 * 256 vectors, a ragged second trip
_V = {'f32': 4, 'bf16': 8, 'hl32': 32}
_DT = {'f32': S.VP_F32, 'bf16': S.VP_BF16, 'hl32': S.VP_HL32}


def _se_layouts(flavour):
    """(B, T, C, ldx, xoff, ldr, roff, ldo, ooff): C one vector wide and five (HL32: three) -- B T C / V is no multiple of 256 -- as
    slices of wider rows with columns on both sides, then the case past the grid cap, contiguous."""
    V = _V[flavour]
    out = [(*SE_BT, C, C + 2 * V, V, C + V, V, C + 3 * V, V) for C in ((32, 96) if flavour == 'hl32' else (V, 5 * V))]
    Cb = {'f32': 516, 'bf16': 1032, 'hl32': 1056}[flavour]
    return out + [(*SE_BIG_BT, Cb, Cb, 0, Cb, 0, Cb, 0)]


def _frame(vals, ld, off, fill=np.nan):
    """(B, T, C) values as the column slice [off, off + C) of a (B T, ld) matrix; `fill` everywhere else."""
    B, T, C = vals.shape
    f = np.full((B * T, ld), fill, F32)
    f[:, off:off + C] = vals.reshape(B * T, C)
    return f


def _slice_ok(full, C, off, what):
    """The payload's written slice, after asserting that the columns on both sides still hold the sentinel."""
    side = np.ones(full.shape[1], bool)
    side[off:off + C] = False
    assert bool((full[:, side] == SENT).all()), f'{what}: a column beside the slice was written'
    return full[:, off:off + C]


def _bf16_check(got, v32, v64, fam, what):
    """got (bf16 tensor) against the float32 fma value rounded to bf16.  exact: equal.  gauss: the other neighbour is allowed only
    where the float64 value lies within 2^-24 relative of a bf16 tie; the share of such elements stays below 1e-3."""
    g = got.float().numpy()
    ref = S.bf16(v32)
    diff = g != ref
    if fam == 'exact':
        assert not diff.any(), f'{what}: {int(diff.sum())} of {diff.size} differ, first at {tuple(int(i[0]) for i in np.nonzero(diff))}'
        return
    lo, hi = S.bf16_neighbours(v32)
    ok = ~diff | (S.bf16_tie_near(v64) & ((g == lo) | (g == hi)))
    assert ok.all(), f'{what}: {int((~ok).sum())} elements are neither the rounded value nor a tie neighbour'
    assert diff.mean() < 1e-3, f'{what}: {diff.mean():.2e} of the elements took the other tie neighbour'


@pytest.mark.parametrize('case', [0, 1, 2])
@pytest.mark.parametrize('flavour', ['f32', 'bf16', 'hl32'])
def test_se_scale_residual(N, flavour, case):
    """vp_se_scale_residual: out = fma(x, s[b], res), ONE float32 rounding, then the storage rounding.
    f32: equal to the float64 fma rounded once (both families).  bf16: that value rounded to bf16 (exact: equal; gauss: see _bf16_check).
    HL32: inputs through pack_hl32, the output planes bit-equal to pack_hl32 of the float32 result."""
    from ppvector.models.utils import pack_hl32, unpack_hl32
    lib, ctx, st = env(N)
    B, T, Cc, ldx, xoff, ldr, roff, ldo, ooff = _se_layouts(flavour)[case]
    tdt = BF if flavour == 'bf16' else torch.float32
    for fam in FAMILIES:
        x, r, s = S.se_inputs(B, T, Cc, fam, flavour == 'bf16')
        fx, fr = _frame(x, ldx, xoff), _frame(r, ldr, roff)
        if flavour == 'hl32':
            hx, hr = pack_hl32(torch.from_numpy(fx)), pack_hl32(torch.from_numpy(fr))
            x = unpack_hl32(hx).numpy()[:, xoff:xoff + Cc].reshape(B, T, Cc)         # hi + lo: what the kernel works on
            r = unpack_hl32(hr).numpy()[:, roff:roff + Cc].reshape(B, T, Cc)
            dx, dr = hx.cuda(), hr.cuda()
        else:
            dx, dr = dev(fx, tdt), dev(fr, tdt)
        ds = dev(s)
        out = Buf(B * T * ldo, dtype=tdt)
        N.check(lib.vp_se_scale_residual(ctx, _DT[flavour], dx.data_ptr(), ldx, xoff, ds.data_ptr(), dr.data_ptr(), ldr, roff,
                                         out.p, ldo, ooff, B, T, Cc, st), ctx)
        v32 = S.se_scale(x, s, r).reshape(B * T, Cc)
        what = f'se_scale {flavour} {fam} C={Cc}'
        if flavour == 'bf16':
            got = _slice_ok(out.get((B * T, ldo)).float().numpy(), Cc, ooff, what)
            v64 = (x.astype(F64) * s.astype(F64)[:, None, :] + r.astype(F64)).reshape(B * T, Cc)
            _bf16_check(torch.from_numpy(np.ascontiguousarray(got)).to(BF), v32, v64, fam, what)
        else:
            got = np.ascontiguousarray(_slice_ok(out.get((B * T, ldo)), Cc, ooff, what))
            ref = v32 if flavour == 'f32' else pack_hl32(torch.from_numpy(v32)).numpy()
            bad = bits(got) != bits(ref)
            assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.size} words differ, first at {tuple(int(i[0]) for i in np.nonzero(bad))}'
            if flavour == 'f32':
                same(got, v32.astype(F64), what)


@pytest.mark.parametrize('case', [0, 1, 2])
def test_se_scale_residual_shadow(N, case):
    """vp_se_scale_residual_shadow: `out` as the f32 flavour; the shadow bit-equal to out.to(bfloat16) in its own slice (ld_shadow,
    shadow_off multiples of 4), sentinel around it."""
    lib, ctx, st = env(N)
    B, T, Cc, ldx, xoff, ldr, roff, ldo, ooff = _se_layouts('f32')[case]
    lds, soff = (Cc, 0) if case == 2 else (Cc + 8, 4)
    for fam in FAMILIES:
        x, r, s = S.se_inputs(B, T, Cc, fam, False, key=1)
        hold, (px, pr, pg) = devs(_frame(x, ldx, xoff), _frame(r, ldr, roff), s)
        out, sh = Buf(B * T * ldo), Buf(B * T * lds, dtype=BF)
        N.check(lib.vp_se_scale_residual_shadow(ctx, px, ldx, xoff, pg, pr, ldr, roff, out.p, ldo, ooff, sh.p, lds, soff, B, T, Cc, st), ctx)
        v32 = S.se_scale(x, s, r).reshape(B * T, Cc)
        what = f'se_scale shadow {fam} C={Cc}'
        same(_slice_ok(out.get((B * T, ldo)), Cc, ooff, what), v32.astype(F64), what)
        got = _slice_ok(sh.get((B * T, lds)).float().numpy(), Cc, soff, what + ' shadow')
        assert np.array_equal(bits(torch.from_numpy(np.ascontiguousarray(got)).to(BF)), bits(S.cast_bf16(v32))), what + ' shadow'


@pytest.mark.parametrize('case', [0, 1, 2])
def test_se_scale_residual_z16(N, case):
    """vp_se_scale_residual_z16 with the kernel's two roundings, h = bf16(fma(z, sc, sh)) then bf16(fma(h, s, res)), ties planted at both
    (257 -> 256, -259 -> -260): bit-equal on both families (each fma is one float32 rounding, each bf16 rounding ties-to-even)."""
    lib, ctx, st = env(N)
    B, T, Cc, ldz, _, ldr, roff, ldo, ooff = _se_layouts('bf16')[case]
    for fam in FAMILIES:
        z, sc, sh, s, r = S.z16_inputs(B, T, Cc, fam)
        dz, dr = dev(_frame(z, ldz, 0), BF), dev(_frame(r, ldr, roff), BF)
        hold, (psc, psh, pg) = devs(sc, sh, s)
        out = Buf(B * T * ldo, dtype=BF)
        N.check(lib.vp_se_scale_residual_z16(ctx, dz.data_ptr(), ldz, psc, psh, pg, dr.data_ptr(), ldr, roff, out.p, ldo, ooff, B, T, Cc, st), ctx)
        what = f'se_scale z16 {fam} C={Cc}'
        got = _slice_ok(out.get((B * T, ldo)).float().numpy(), Cc, ooff, what)
        ref = S.se_scale_z16(z, sc, sh, s, r).reshape(B * T, Cc)
        bad = got != ref
        assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.size} differ, first at {tuple(int(i[0]) for i in np.nonzero(bad))}'
        if fam == 'exact':
            assert got[0, 1] == 256.0 and got[2, 1] == 260.0               # the planted ties of the second rounding: 257 -> 256, 259 -> 260


def test_se_scale_residual_rejects(N):
    """Widths and offsets off the vector width, and -- every flavour moves 16-byte vectors -- a base pointer (x, s, res or out) 4 or 8
    bytes off: VP_EINVAL before any launch.  Shadow: 4 bytes off, shadow_off = 2, a shadow with bf16 tensors.  z16: C = 12, a
    misaligned gate.  Every output stays sentinel."""
    lib, ctx, st = env(N)
    B, T = 2, 3
    src = dev(np.ones(4096, F32))
    p = src.data_ptr()
    out, sh = Buf(1024), Buf(1024, dtype=BF)
    for flavour, V in _V.items():
        dt, Cc = _DT[flavour], 2 * V
        call = lambda x=p, s=p, r=p, o=out.p, C_=Cc, ld=Cc, off=0: lib.vp_se_scale_residual(
            ctx, dt, x, ld, off, s, r, ld, off, o, ld, off, B, T, C_, st)
        for off in (4, 8):
            assert call(x=p + off) == VP_EINVAL and call(s=p + off) == VP_EINVAL and call(r=p + off) == VP_EINVAL, (flavour, off)
            assert call(o=out.p + off) == VP_EINVAL, (flavour, off)
        assert call(C_=Cc + V // 2) == VP_EINVAL and call(ld=Cc + V // 2) == VP_EINVAL and call(ld=2 * Cc, off=V // 2) == VP_EINVAL, flavour
    shadow = lambda o=out.p, q=sh.p, ld=16, off=0: lib.vp_se_scale_residual_shadow(ctx, p, 8, 0, p, p, 8, 0, o, 8, 0, q, ld, off, B, T, 8, st)
    assert shadow(q=sh.p + 4) == VP_EINVAL and shadow(off=2) == VP_EINVAL and shadow(ld=10) == VP_EINVAL and shadow(o=out.p + 4) == VP_EINVAL
    z16 = lambda C_=16, s=p, o=out.p: lib.vp_se_scale_residual_z16(ctx, p, 16, p, p, s, p, 16, 0, o, 16, 0, B, T, C_, st)
    assert z16(C_=12) == VP_EINVAL and z16(s=p + 4) == VP_EINVAL and z16(o=out.p + 8) == VP_EINVAL
    assert lib.vp_se_scale_residual(ctx, 7, p, 8, 0, p, p, 8, 0, out.p, 8, 0, B, T, 8, st) == VP_EINVAL
    assert out.untouched() and sh.untouched()


# ------------------------------------------------------------------------------------------------ vp_dense_f32
_DENSE_VARIANTS = [dict(), dict(kind='relu'), dict(kind='sigmoid'), dict(kind='tanh'), dict(lda=4), dict(lda=1), dict(ldo=3), dict(woff=1),
                   dict(bias=False), dict(kind='tanh', lda=1, ldo=3, woff=1)]


def _dense_run(N, a, w, bias, kn, kind='none', lda=0, ldo=0, woff=0):
    lib, ctx, st = env(N)
    (M, K), Nn = a.shape, w.shape[1]
    fa = np.full((M, K + lda), np.nan, F32)
    fa[:, :K] = a
    wl = np.concatenate([np.full(woff, np.nan, F32), (w if kn else w.T).reshape(-1)])
    hold, (pa, pw) = devs(fa, wl)
    db = None if bias is None else dev(bias)
    out = Buf(M * (Nn + ldo))
    N.check(lib.vp_dense_f32(ctx, pa, K + lda, pw + 4 * woff, kn, None if db is None else db.data_ptr(), M, Nn, K, S.ACT_IDS[kind],
                             out.p, Nn + ldo, st), ctx)
    return _slice_ok(out.get((M, Nn + ldo)), Nn, 0, f'dense {M}x{Nn}x{K}')


@pytest.mark.parametrize('M,Nn,K,kn', S.DENSE_CASES)
def test_dense_f32(N, M, Nn, K, kn):
    """vp_dense_f32 on the f32 matrix cores, W as [N][K] (kn = 0) and [K][N] (kn = 1): the 64-wide fast loop (it walks a wave's whole
    share), the 16-wide loop that takes over when the fast path is off and its scalar fallbacks (lda = K + 1: `a` off the float4
    path; W 4 bytes off; K % 4 != 0), 4 vs 16 waves at K = 1020 / 1024, waves that
    start past K (1028), partial 16 x 16 tiles, ldo = N + 3 with sentinel columns, no bias, all four activations.
    exact: NONE and RELU EQUAL float64; sigmoid and tanh of an exact argument within the activation bounds of docs/train_ops.md (4 x
    float32's own error: 4.41e-07 and 2.45e-07 relative).  gauss: (K + 2) 2^-24 (|a| |W| + |bias|) through the activation's slope, plus that bound."""
    for fam in FAMILIES:
        a, w, bias = S.dense_inputs(M, Nn, K, fam)
        for v in _DENSE_VARIANTS:
            v = dict(v)
            b = bias if v.pop('bias', True) else None
            kind = v.get('kind', 'none')
            got = _dense_run(N, a, w, b, kn, **v)
            rz, ry = S.dense(a, w, b, kind)
            what = f'dense {fam} kn={kn} {v} bias={b is not None}'
            if kind in ('sigmoid', 'tanh'):
                bound = S.act_rel_bound(kind) * (np.abs(ry) + S.REL_FLOOR)
                if fam == 'exact':
                    assert np.array_equal(rz.astype(F32).astype(F64), rz)
                else:
                    bound = bound + (0.25 if kind == 'sigmoid' else 1.0) * S.dense_bound(a, w, b)
                within(got, ry, bound, what)
            elif fam == 'exact':
                same(got, ry, what)
            else:
                within(got, ry, S.dense_bound(a, w, b), what)


def test_dense_f32_rejects(N):
    lib, ctx, st = env(N)
    src = dev(np.ones(256, F32))
    p = src.data_ptr()
    out = Buf(256)
    assert lib.vp_dense_f32(ctx, None, 4, p, 0, p, 2, 2, 4, 0, out.p, 2, st) == VP_EINVAL
    assert lib.vp_dense_f32(ctx, p, 4, None, 0, p, 2, 2, 4, 0, out.p, 2, st) == VP_EINVAL
    assert lib.vp_dense_f32(ctx, p, 4, p, 0, p, 0, 2, 4, 0, out.p, 2, st) == VP_EINVAL
    assert lib.vp_dense_f32(ctx, p, 4, p, 0, p, 2, 2, 0, 0, out.p, 2, st) == VP_EINVAL
    assert out.untouched()


# ------------------------------------------------------------------------------------------------ vp_cast_f32_bf16
@pytest.mark.parametrize('n', S.CAST_N)
def test_cast_f32_bf16(N, n):
    """n = 1, 3 (scalar tail only), 4 (one float4), 5, 1001, 4096 * 1024 + 7 (a second grid-stride trip and a tail): bit-equal to
    .to(torch.bfloat16) -- ties to even, +-0, float32 subnormals onto the bf16 subnormals, FLT_MAX to Inf, +-Inf; NaN stays NaN."""
    lib, ctx, st = env(N)
    x = S.cast_inputs(n)
    dx = dev(x)
    y = Buf(n, dtype=BF)
    N.check(lib.vp_cast_f32_bf16(ctx, dx.data_ptr(), y.p, n, st), ctx)
    got, ref = y.get(), S.cast_bf16(x)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan)
    bad = (bits(got) != bits(ref)) & ~nan.numpy()
    assert not bad.any(), f'{int(bad.sum())} of {n} differ, first at {int(np.nonzero(bad)[0][0])}: {x[np.nonzero(bad)[0][0]]!r}'


def test_cast_f32_bf16_rejects(N):
    lib, ctx, st = env(N)
    dx = dev(np.ones(16, F32))
    y = Buf(16, dtype=BF)
    assert lib.vp_cast_f32_bf16(ctx, dx.data_ptr() + 4, y.p, 8, st) == VP_EINVAL
    assert lib.vp_cast_f32_bf16(ctx, dx.data_ptr(), y.p + 2, 8, st) == VP_EINVAL
    assert lib.vp_cast_f32_bf16(ctx, dx.data_ptr(), y.p, 0, st) == VP_EINVAL
    assert lib.vp_cast_f32_bf16(ctx, None, y.p, 8, st) == VP_EINVAL
    assert y.untouched()
