"""The float64 oracle of the inference path's small kernels (tests/small_ops_oracle.py) checked on the CPU, so that it cannot be
wrong unnoticed: each restatement against plain float64 torch, the partial-sum layout against a row-by-row walk, the single-rounding
fma against exact rational arithmetic, every stated bound against the oracle's own float32 evaluations -- and the exact family's
precondition for every planted case: float32 in two summation orders is bit-identical to float64."""
from fractions import Fraction
import math

import numpy as np
import pytest
import torch

from tests import small_ops_oracle as S

F32, F64, U = np.float32, np.float64, S.U
ALL_BT = S.BT_CASES + S.BT_LONG


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    assert a.shape == b.shape
    assert np.max(np.abs(a - b)) <= tol * max(1.0, float(np.max(np.abs(b)))), float(np.max(np.abs(a - b)))


# ------------------------------------------------------------------------------------------------ the exactness precondition
_CASES = S.exact_cases()


@pytest.mark.parametrize('name,fn', _CASES, ids=[c[0] for c in _CASES])
def test_exact_family_is_order_independent_in_float32(name, fn):
    """float32 first-to-last == float32 last-to-first == float64, bit for bit, for every output of every planted exact case."""
    fwd, bwd, ref = fn(F32, False), fn(F32, True), fn(F64, False)
    for a, b, r in zip(fwd, bwd, ref):
        assert a.dtype == F32 and r.dtype == F64
        assert np.array_equal(a, b), name
        assert np.array_equal(a.astype(F64), r), name
        assert np.all(np.isfinite(r))


def test_exact_cases_cover_the_case_lists():
    names = [c[0] for c in _CASES]
    assert len(set(names)) == len(names)
    assert sum(n.startswith('se_gate-') for n in names) == len(S.SE_GATE_FLAT) == 25
    assert sum(n.startswith('moments-') for n in names) == 2 * len(S.MOM_C)          # T = 1 and 128
    assert sum(n.startswith('dense-') for n in names) == 8


def test_case_lists_reach_their_branches():
    """The geometry the case tables of docs/small_ops.md claim."""
    groups = lambda C: max(1, S.SE_THREADS // C)
    assert [groups(C) for C, _, _ in S.SE_GATE_CASES] == [256, 16, 5, 2, 1, 1, 1, 1, 1]
    assert S.SE_THREADS - 5 * 192 == 64 and (192 // 4) * (1024 // (192 // 4)) != 1024            # idle threads; nv = 6 at H = 24
    assert 1024 % (24 // 4) != 0
    assert S.nseg(1) == 129 and S.nseg(298) == 2 and S.nseg(128) == 2 and S.nseg(127) == 3
    assert S.n_tiles(1, 23808) == 186 > groups(64) and S.n_tiles(2, 300) < groups(64)
    for (M, N, K, kn) in S.DENSE_CASES:
        nw = 16 if K >= 1024 else 4
        kper = ((K + nw - 1) // nw + 15) // 16 * 16
        if K == 1028:
            assert (nw - 1) * kper >= K                                               # the last wave starts past K
        if K == 1020:
            assert nw == 4
    assert S.SE_GRID_CAP * 4 + 7 == 4096 * 1024 + 7


# ------------------------------------------------------------------------------------------------ the partial-sum layout
@pytest.mark.parametrize('B,T', ALL_BT)
def test_conv_psum_layout(B, T):
    """conv_psum against a row-by-row walk of the 128-row tiles (the construction of test_se_gate_kernel_vs_float64); utt_sums reads
    exactly the touched slots (no NaN) and returns the plain time sums."""
    C = 3
    v = S.ints(S.rng(B, T), (B, T, C)).astype(F64)
    ps = S.conv_psum(v)
    assert ps.shape == (S.tiles_m(B, T), S.nseg(T), C) and ps.dtype == F32
    ref = np.full(ps.shape, np.nan)
    rows = v.reshape(B * T, C)
    for r in range(B * T):
        tm = r // 128
        seg = r // T - (tm * 128) // T
        ref[tm, seg] = np.where(np.isnan(ref[tm, seg]), 0.0, ref[tm, seg]) + rows[r]
    assert np.array_equal(ps, ref.astype(F32), equal_nan=True)
    assert np.isnan(ps).any() or B * T % 128 == 0 and 128 % T == 0
    assert np.array_equal(S.utt_sums(ps, B, T), v.sum(1))
    touched = np.zeros(ps.shape[:2], bool)
    for tm, sg in S.utt_slots(B, T):
        assert not touched[tm, sg].any()
        touched[tm, sg] = True
    assert np.array_equal(touched, ~np.isnan(ps[..., 0]))


# ------------------------------------------------------------------------------------------------ SE gate
@pytest.mark.parametrize('C,H,B,T', [(64, 8, 2, 300), (192, 24, 5, 28), (768, 96, 3, 129)])
def test_se_gate_oracle_vs_torch(C, H, B, T):
    """Against float64 torch on the activations themselves: mean over time + shift, two Linear layers, sigmoid."""
    g = S.rng(C, H, B, T)
    y = S.ints(g, (B, T, C)).astype(F64)
    shift, w1, b1, w2, b2 = S.gauss(g, C), S.gauss(g, (C, H)), S.gauss(g, H), S.gauss(g, (H, C)) / F32(8), S.gauss(g, C)
    mean, a, z, s = S.se_gate(S.conv_psum(y), shift, w1, b1, w2, b2, B, T)
    t = lambda v: torch.from_numpy(np.asarray(v, F64))
    tm = t(y).mean(1) + t(shift)
    ta = torch.relu(tm @ t(w1) + t(b1))
    close(mean, tm.numpy())
    close(a, ta.numpy())
    close(s, torch.sigmoid(ta @ t(w2) + t(b2)).numpy())


@pytest.mark.parametrize('C,H,B,T', [(4, 4, 130, 1), (64, 8, 1, 23808), (516, 64, 3, 298)])
def test_se_gate_exact_inputs_give_integer_means(C, H, B, T):
    """The exact family's mean is an integer for ANY T (the time sum is T m), its argument a multiple of 2^-k of modest size."""
    inp = S.se_gate_inputs(B, T, C, H, 'exact')
    mean, a, z, s = S.se_gate(*inp, B, T)
    assert np.array_equal(mean, np.round(mean)) and np.abs(mean).max() <= 6 and np.abs(mean).max() >= 3
    assert np.abs(z).max() < 64 and np.array_equal(z.astype(F32).astype(F64), z)
    assert np.mean((s > 0.02) & (s < 0.98)) > 0.5                      # most gates are away from saturation: a wrong mean shows


@pytest.mark.parametrize('C,H,B,T', [(64, 8, 1, 23808), (192, 24, 3, 298), (1024, 128, 3, 127)])
def test_se_gate_bound_holds_for_float32(C, H, B, T):
    inp = S.se_gate_inputs(B, T, C, H, 'gauss')
    ref = S.se_gate(*inp, B, T)[2]
    bound = S.se_gate_bounds(*inp, B, T)
    for rev in (False, True):
        assert np.all(np.abs(S.se_gate(*inp, B, T, dt=F32, rev=rev)[2] - ref) <= bound)


def test_sigmoid_bound_from_the_measured_exponential():
    """c1, c2 are measured on the CPU; a float32 sigmoid built on the restated fast exponential, and torch's own, stay inside a QUARTER
    of the bound the GPU tests allow (they allow 4 x the measured model)."""
    c1, c2 = S.expf_model()
    print(f'expf model: c1 = {c1:.3f}, c2 = {c2:.3f} (units of 2^-24)')
    assert 0 <= c1 <= 1.5 and 0.5 <= c2 <= 3.0
    z = np.concatenate([np.linspace(-12, 12, 50001), np.arange(-48, 49) / 4.0]).astype(F32)
    s = 1.0 / (1.0 + np.exp(-z.astype(F64)))
    quarter = (c1 * np.abs(z) + c2) * U * s * (1 - s) + 2 * U * s
    t = torch.from_numpy(z)
    fast = (1.0 / (1.0 + torch.exp2(-t * F32(1.4426950408889634)))).numpy()
    assert np.all(np.abs(fast - s) <= quarter)
    assert np.all(np.abs((1.0 / (1.0 + torch.exp(-t))).numpy() - s) <= quarter)
    assert np.all(S.sigmoid_bound(z, s) >= quarter)


# ------------------------------------------------------------------------------------------------ moments
@pytest.mark.parametrize('B,T', ALL_BT)
def test_moments_oracle_vs_torch(B, T):
    C = 7
    for fam in ('exact', 'gauss'):
        z, scale, shift = S.moments_inputs(B, T, C, fam)
        got = S.moments(_exact_psum(z), _exact_psum(z * z), shift, scale, B, T, S.MOM_EPS, 1)
        y = torch.from_numpy(z * scale.astype(F64) + shift.astype(F64))
        close(got[:, :C], y.mean(1).numpy(), 1e-11)
        var = (torch.from_numpy(z).var(1, unbiased=False) * torch.from_numpy(scale.astype(F64)) ** 2).numpy()
        keep = np.abs(var - F32(S.MOM_EPS)) > 1e-9                    # away from the clamp's corner
        ref = np.sqrt(np.maximum(var, F64(F32(S.MOM_EPS))))
        assert np.max(np.abs(got[:, C:] - ref)[keep] * ref[keep]) < 1e-10           # E[z^2] - E[z]^2 in float64: 1e-13 absolute on the variance


def _exact_psum(v):
    """The partial sums kept in float64 (no rounding to float32): for comparisons against torch on the unrounded data."""
    B, T, C = v.shape
    ps = np.full((S.tiles_m(B, T), S.nseg(T), C), np.nan)
    for b, (tm, sg) in enumerate(S.utt_slots(B, T)):
        for t_, s_ in zip(tm, sg):
            lo, hi = max(b * T, t_ * 128), min((b + 1) * T, (t_ + 1) * 128)
            ps[t_, s_] = v.reshape(B * T, C)[lo:hi].sum(0)
    return ps


@pytest.mark.parametrize('B,T', ALL_BT)
def test_negative_float32_variance_is_clamped(B, T):
    """The planted near-constant channel: float32's E[x^2] - E[x]^2 is NEGATIVE for some utterance in both summation orders (T > 1),
    float64's is tiny; sqrt(max(., eps)) returns sqrt(eps), finite, in both -- without the clamp float32 would return NaN."""
    z = S.negvar_channel(B, T)
    if T > 1:
        assert S.var32_min(z, B, T) < 0
        assert np.ptp(z) <= np.spacing(F32(z.min())) and 1 <= z.min()
    z3 = z.reshape(B, T, 1)
    ps, psq = S.conv_psum(z3), S.conv_psum(z3 * z3)
    for dt in (F32, F64):
        for rev in (False, True):
            std = S.moments(ps, psq, None, None, B, T, S.MOM_EPS, 1, dt, rev)[:, 1]
            assert np.array_equal(std, np.full(B, np.sqrt(dt(F32(S.MOM_EPS))), dt))
    with np.errstate(invalid='ignore'):
        naive = np.sqrt(S._moment_parts(ps, psq, B, T, F32, False)[1])
    assert T == 1 or np.isnan(naive).any()


@pytest.mark.parametrize('C', [5, 257])
@pytest.mark.parametrize('B,T', ALL_BT)
def test_moments_bounds_hold_for_float32(B, T, C):
    """Both families, both entry points' forms (scale given or not), both summation orders: the oracle's float32 evaluation lies inside
    moments_bounds; the mean-8 / std-1/4 channel inside (T + 4) 2^-24 E[x^2] / (2 std) on the std; the constant channel gives sqrt(eps)."""
    if C == 257 and (B, T) in S.BT_LONG:
        return
    for fam in ('exact', 'gauss'):
        z, scale, shift = S.moments_inputs(B, T, C, fam)
        ps, psq = S.conv_psum(z), S.conv_psum(z * z)
        for sc, sh in ((None, None), (None, shift), (scale, shift)):
            ref = S.moments(ps, psq, sh, sc, B, T, S.MOM_EPS, 1)
            bound = S.moments_bounds(ps, psq, sh, sc, B, T, S.MOM_EPS, 1, S.moments_n_terms(B, T, C, fam))
            near = S.planted_std_bound(psq, sc, ref[:, C:], B, T)[:, S.PLANTED['near']]
            for rev in (False, True):
                got = S.moments(ps, psq, sh, sc, B, T, S.MOM_EPS, 1, F32, rev)
                assert np.all(np.isfinite(got))
                assert np.all(np.abs(got - ref) <= bound), (fam, float(np.max(np.abs(got - ref) / bound)))
                if T > 1:
                    assert np.all(np.abs(got[:, C + S.PLANTED['near']] - ref[:, C + S.PLANTED['near']]) <= near)
                assert np.all(got[:, C + S.PLANTED['const']] == np.sqrt(F32(S.MOM_EPS)))
            if T % 2 == 0 and sc is None:
                assert np.allclose(ref[:, C + S.PLANTED['near']], 0.25, rtol=1e-6)
                assert np.allclose(ref[:, S.PLANTED['near']] - (0 if sh is None else sh[S.PLANTED['near']]), 8)


# ------------------------------------------------------------------------------------------------ SE scale + residual
def _round_f32(q):
    """A Fraction rounded once to float32 (nearest, ties to even; normal range)."""
    if q == 0:
        return 0.0
    e = math.frexp(float(q))[1]
    while abs(q) >= Fraction(2) ** e:
        e += 1
    while abs(q) < Fraction(2) ** (e - 1):
        e -= 1
    return float(round(q / Fraction(2) ** (e - 24)) * Fraction(2) ** (e - 24))


def test_fma32_is_one_rounding():
    """fma32 against exact rational arithmetic: Gaussian triples, and sums built to sit on or next to a float32 tie, where rounding the
    float64 sum again (a double rounding) would go wrong."""
    g = S.rng(71)
    x, s, r = (S.gauss(g, 4000) for _ in range(3))
    x[:6] = [1 + 2.0 ** -23, 1 + 2.0 ** -23, 3.0, 1 + 2.0 ** -12, 1 + 2.0 ** -12, 1.0]
    s[:6] = [1 + 2.0 ** -23, 1 - 2.0 ** -23, 0.5, 1 + 2.0 ** -12, 1 - 2.0 ** -12, 1.0]
    r[:6] = [2.0 ** -24 - 2.0 ** -22, 2.0 ** -24, 2.0 ** -24, 2.0 ** 30, -2.0 ** 30 + 64, 2.0 ** -24]
    got = S.fma32(x, s, r)
    ref = np.asarray([_round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))) for a, b, c in zip(x, s, r)], F64)
    assert got.dtype == F32 and np.array_equal(got.astype(F64), ref)
    twice = (x.astype(F64) * s.astype(F64) + r.astype(F64)).astype(F32)
    print('double rounding differs on', int(np.sum(twice != got)), 'of', got.size)


def test_bf16_tie_helpers_and_z16_oracle():
    lo, hi = S.bf16_neighbours(np.asarray([257.0, -259.0, 1.0], F32))
    assert list(lo) == [256.0, -258.0, 1.0] and list(hi) == [258.0, -260.0, 1.0078125]
    assert list(S.bf16_tie_near([257.0, -259.0, 257.0 * (1 + 2.0 ** -25), 257.01, 256.0])) == [True, True, True, False, False]
    assert list(S.bf16(S.Z16_TIES)) == [256.0, -260.0, 260.0, -264.0]
    # z16: rounding h first matters -- z = 257, s = 1, res = 1: h = bf16(257) = 256, out = bf16(257) = 256; unrounded it would be 258
    out = S.se_scale_z16(np.full((1, 1, 1), 257.0, F32), [1.0], [0.0], np.ones((1, 1), F32), np.ones((1, 1, 1), F32))
    assert out.item() == 256.0


def test_hl32_pack_is_what_the_oracle_assumes():
    """pack_hl32 / unpack_hl32: hi = bf16(v), lo = bf16(v - hi), hi + lo exact in float32 and within 2^-16 relative of v; integers and
    dyadics of the exact family survive unchanged."""
    from ppvector.models.utils import pack_hl32, unpack_hl32
    v = torch.from_numpy(S.gauss(S.rng(73), (5, 96)))
    p = pack_hl32(v)
    assert p.dtype == torch.float32 and p.shape == v.shape
    raw = p.view(torch.bfloat16).reshape(5, 3, 64).float()
    assert torch.equal(raw[..., :32].reshape(5, 96), v.to(torch.bfloat16).float())
    u = unpack_hl32(p)
    assert torch.equal(u.double(), raw[..., :32].double().reshape(5, 96) + raw[..., 32:].double().reshape(5, 96))
    assert float(((u - v).abs() / v.abs()).max()) <= 2.0 ** -16
    w = torch.from_numpy(S.ints(S.rng(74), (4, 32)) * F32(0.75))
    assert torch.equal(unpack_hl32(pack_hl32(w)), w)


# ------------------------------------------------------------------------------------------------ dense, cast
def test_dense_oracle_and_bound():
    for M, N, K in ((17, 33, 68), (3, 192, 3072)):
        a, w, bias = S.dense_inputs(M, N, K, 'gauss')
        t = lambda v: torch.from_numpy(np.asarray(v, F64))
        for kind, fn in (('none', lambda v: v), ('relu', torch.relu), ('sigmoid', torch.sigmoid), ('tanh', torch.tanh)):
            close(S.dense(a, w, bias, kind)[1], fn(t(a) @ t(w) + t(bias)).numpy())
        ref, bound = S.dense(a, w, bias)[0], S.dense_bound(a, w, bias)
        for rev in (False, True):
            assert np.all(np.abs(S.dense(a, w, bias, dt=F32, rev=rev)[0] - ref) <= bound)
        ea, ew, eb = S.dense_inputs(M, N, K, 'exact')
        assert np.abs(S.dense(ea, ew, eb)[0]).max() < 32


def test_cast_planted_values():
    """What round-to-nearest-even does to the planted values: ties to even, the bf16 subnormals, FLT_MAX to Inf, NaN stays NaN."""
    f = lambda v: S.cast_bf16(np.asarray([v], F32)).float().item()
    assert f(257.0) == 256.0 and f(-259.0) == -260.0 and f(1.00390625) == 1.0 and f(1.01171875) == 1.015625
    assert f(1.0 + 2.0 ** -8 + 2.0 ** -23) == 1.0078125 and f(1.0 + 2.0 ** -8 - 2.0 ** -24) == 1.0
    assert f(2.0 ** -133) == 2.0 ** -133 and f(2.0 ** -134) == 0.0 and f(3 * 2.0 ** -134) == 2.0 ** -132 and f(2.0 ** -149) == 0.0
    assert f(3.4028234663852886e38) == math.inf and f(3.3895313892515355e38) == 3.3895313892515355e38
    assert math.copysign(1.0, f(-0.0)) == -1.0 and math.isnan(f(math.nan))
    for n in S.CAST_N[:5]:
        x = S.cast_inputs(n)
        assert x.size == n and (n >= 8 or np.isnan(x[0]))
    assert np.isnan(S.cast_inputs(1001)).sum() == 1
