"""The pooling statistics kernels of the training step against the float64 oracle of tests/pooling_oracle.py, entry point by entry
point, at the T where their dispatch changes and at the clamp's edges (docs/pooling_stats.md).  Run with -m gpu on an MI355X.

Forward  vp_asp_softmax_stats (f32 x: reg<20> T <= 160, reg<40> T <= 320, streaming above; bf16 x: streaming) and
         vp_asp_softmax_stats_l16 (bf16 logits, f32 or bf16 x, T <= 320), per element:
             |mu - ref| <= 4e-6 sum_t al |x|,   |sd - ref| <= 2e-5 ref
         -- four times what float32 costs the kernels' formula restated in NumPy (tests/test_pooling_oracle_cpu.py), so the
         bound comes from the reference side.
Backward vp_attn_stats_bwd_f32 / _de16 (the same three-way choice) and _e16, handed the REFERENCE's pooled (rounded to f32) so that
         the backward kernel is judged alone: rel-L2 of dx < 2e-5, of de < 2e-5 (f32) / 4e-3 (bf16: 2^-9 per element), over the whole
         tensor and again over the last min(8, T) frames alone (the register kernels' clamped tail).
Clamp    planted channels whose weighted variance is below eps although (in three of five) not every x - mu is 0.
Time     TimeStats, vp_time_stats_bwd_coeffs, vp_time_stats_bwd_add_x16 on constant channels and at T around their unroll of 32.

Every case's operands are built once on the CPU, rounded to the stored dtype, and the float64 reference sees those numbers."""
import os

import numpy as np
import pytest
import torch

from tests import pooling_oracle as po

pytestmark = pytest.mark.gpu

DE_F32, DE_BF16, DX = 2e-5, 4e-3, 2e-5
SWITCHES = ('VPMI_ASP_STATS_PLAIN', 'VPMI_ASB_PLAIN')


@pytest.fixture(scope='module')
def N():
    from ppvector import _native as N
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: these tests must run on an MI355X (no CPU fallback exists)')
    N.ctx(0)
    return N


@pytest.fixture(autouse=True)
def default_dispatch():
    """The A/B switches are read once per process into a static: with one exported, the register kernels never run and these
    tests would say nothing about them.  They fail, naming the variable."""
    exported = [v for v in SWITCHES if os.environ.get(v) is not None]
    assert not exported, f'unset {", ".join(exported)}: the kernels pinned here are those of the default dispatch'


@pytest.fixture(scope='module')
def worst():
    """entry point -> worst figures over the module, printed at the end (docs/pooling_stats.md quotes them)."""
    w = {}
    yield w
    for k in sorted(w):
        print(f'[pooling worst] {k}: ' + '  '.join(f'{n} {v:.2e}' for n, v in sorted(w[k].items())))


def note(worst, key, **figs):
    d = worst.setdefault(key, {})
    for n, v in figs.items():
        d[n] = max(d.get(n, 0.0), v)


def rows(t, bf16=False):
    """(B, T, C) CPU float32 -> (B*T, C) on the GPU in the stored dtype (the values are already representable in it)."""
    t = t.reshape(-1, t.shape[-1])
    return (t.to(torch.bfloat16) if bf16 else t).contiguous().cuda()


def hctx(N):
    return N.ctx(torch.device('cuda', 0))


def forward(N, c, entry, x_bf16, xd=None, ldx=None, xoff=0):
    """pooled (B, 2C) of one forward entry point; entry: 'asp' (f32 logits) or 'l16' (bf16 logits).  -> rc, pooled (sentinel-filled)"""
    lib, ctx = N.lib(), hctx(N)
    xd = rows(c.x, x_bf16) if xd is None else xd
    ed = rows(c.e, entry == 'l16')
    pooled = torch.full((c.B, 2 * c.C), -768.0, device='cuda')
    dt = N.VP_BF16 if x_bf16 else N.VP_F32
    ldx = c.C if ldx is None else ldx
    if entry == 'l16':
        rc = lib.vp_asp_softmax_stats_l16(ctx, ed.data_ptr(), xd.data_ptr(), dt, ldx, xoff, c.B, c.T, c.C, 1e-12, pooled.data_ptr(), N.stream_ptr())
    else:
        rc = lib.vp_asp_softmax_stats(ctx, dt, ed.data_ptr(), xd.data_ptr(), ldx, xoff, c.B, c.T, c.C, 1e-12, pooled.data_ptr(), N.stream_ptr())
    torch.cuda.synchronize()
    return rc, pooled.cpu()


def check_forward(N, worst, key, c, entry, x_bf16, **kw):
    rc, pooled = forward(N, c, entry, x_bf16, **kw)
    N.check(rc, hctx(N))
    assert torch.isfinite(pooled).all()
    mu_err, sd_err = po.forward_errors(pooled.numpy(), c.pooled, c.e, c.x)
    print(f'[{key}] T={c.T} C={c.C} r={c.r}: mu {mu_err:.2e} of sum al|x|, std {sd_err:.2e}')
    note(worst, key, mu=mu_err, std=sd_err)
    assert mu_err <= po.MU_BOUND and sd_err <= po.SD_BOUND, (key, c.T, c.C, c.r, mu_err, sd_err)


# (entry, x bf16, the channel counts: 100 = a half-empty second 64-channel block and no 4-alignment)
FWD_ENTRIES = (('asp', False, (64, 100)), ('asp', True, (64, 96)), ('l16', False, (64, 96)), ('l16', True, (64, 96)))


def fwd_key(entry, x_bf16):
    return ('vp_asp_softmax_stats_l16' if entry == 'l16' else 'vp_asp_softmax_stats') + (' x bf16' if x_bf16 else ' x f32')


# ------------------------------------------------------------------------------------------------------------ (a) forward, T sweep
@pytest.mark.parametrize('T', po.T_SWEEP)
def test_forward_T_sweep(N, worst, T):
    for entry, x_bf16, Cs in FWD_ENTRIES:
        for C in Cs:
            c = po.asp_case(T, C, po.R_SWEEP, x_bf16, entry == 'l16')
            if entry == 'l16' and T > 320:
                rc, pooled = forward(N, c, entry, x_bf16)
                assert rc == N.VP_EUNSUP and (pooled == -768.0).all()          # refused, and nothing written
                continue
            check_forward(N, worst, fwd_key(entry, x_bf16), c, entry, x_bf16)


# ------------------------------------------------------------------------------------------------------------ (b) forward, conditioning
@pytest.mark.parametrize('r', po.R_COND)
@pytest.mark.parametrize('T', po.T_COND)
def test_forward_conditioning(N, worst, T, r):
    """x = r s + s N(0,1): raw E[x^2] - E[x]^2 in f32 costs the std (r^2) 6e-8 -- 2e-4 ... 1e-3 at r = 30 in the CPU restatement."""
    check_forward(N, worst, fwd_key('asp', False) + ' (conditioning)', po.asp_case(T, 64, r), 'asp', False)
    if T <= 320:
        for x_bf16 in (False, True):
            check_forward(N, worst, fwd_key('l16', x_bf16) + ' (conditioning)', po.asp_case(T, 64, r, x_bf16, True), 'l16', x_bf16)


# ------------------------------------------------------------------------------------------------------------ (c) forward, column slice
@pytest.mark.parametrize('T', [160, 321])
def test_forward_on_a_column_slice_between_nan_columns(N, worst, T):
    """x as columns [C, 2C) of a (B*T, 3C) buffer whose other columns are NaN (also the first frame's, which the kernels centre on)."""
    for entry, x_bf16, Cs in FWD_ENTRIES:
        if entry == 'l16' and T > 320:
            continue
        C = Cs[0]
        c = po.asp_case(T, C, po.R_SWEEP, x_bf16, entry == 'l16')
        wide = torch.full((c.B * T, 3 * C), float('nan'))
        wide[:, C:2 * C] = c.x.reshape(-1, C)
        xd = (wide.to(torch.bfloat16) if x_bf16 else wide).cuda()
        check_forward(N, worst, fwd_key(entry, x_bf16) + ' (slice)', c, entry, x_bf16, xd=xd, ldx=3 * C, xoff=C)


# ------------------------------------------------------------------------------------------------------------ (d) backward, T sweep
def backward(N, c, entry, x_bf16, pooled, lddx):
    """entry: 'f32' | 'de16' | 'e16'.  -> rc, de (B, T, C) float32 CPU, dx buffer (B*T, lddx) CPU (sentinel-filled before the call)"""
    lib, ctx = N.lib(), hctx(N)
    xd, ed = rows(c.x, x_bf16), rows(c.e, entry == 'e16')
    pd, dpd = pooled.float().contiguous().cuda(), c.dp.cuda()
    de = torch.full((c.B * c.T, c.C), -768.0, dtype=torch.float32 if entry == 'f32' else torch.bfloat16, device='cuda')
    dx = torch.full((c.B * c.T, lddx), -768.0, device='cuda')
    if entry == 'e16':
        rc = lib.vp_attn_stats_bwd_e16(ctx, ed.data_ptr(), xd.data_ptr(), N.VP_BF16 if x_bf16 else N.VP_F32, c.C, pd.data_ptr(), dpd.data_ptr(),
                                       c.B, c.T, c.C, 1e-12, de.data_ptr(), dx.data_ptr(), lddx, N.stream_ptr())
    else:
        fn = lib.vp_attn_stats_bwd_f32 if entry == 'f32' else lib.vp_attn_stats_bwd_de16
        rc = fn(ctx, ed.data_ptr(), xd.data_ptr(), c.C, pd.data_ptr(), dpd.data_ptr(), c.B, c.T, c.C, 1e-12, de.data_ptr(), dx.data_ptr(), lddx,
                N.stream_ptr())
    torch.cuda.synchronize()
    return rc, de.float().cpu().view(c.B, c.T, c.C), dx.cpu()


def grad_errors(c, de, dx, channels=None):
    """rel-L2 of (de, dx) over the whole tensor and over the last min(8, T) frames alone."""
    ch = slice(None) if channels is None else channels
    k = min(8, c.T)
    return (po.rel(de[:, :, ch], c.de[:, :, ch]), po.rel(dx[:, :, ch], c.dx[:, :, ch]),
            po.rel(de[:, -k:, ch], c.de[:, -k:, ch]), po.rel(dx[:, -k:, ch], c.dx[:, -k:, ch]))


BWD_ENTRIES = (('f32', False, (64, 100)), ('de16', False, (64, 100)), ('e16', False, (64, 96)), ('e16', True, (64, 96)))


def bwd_key(entry, x_bf16):
    return {'f32': 'vp_attn_stats_bwd_f32', 'de16': 'vp_attn_stats_bwd_de16', 'e16': 'vp_attn_stats_bwd_e16'}[entry] + (' x bf16' if x_bf16 else ' x f32')


@pytest.mark.parametrize('T', po.T_SWEEP)
def test_backward_T_sweep(N, worst, T):
    for entry, x_bf16, Cs in BWD_ENTRIES:
        for C in Cs:
            c = po.asp_case(T, C, po.R_SWEEP, x_bf16, entry == 'e16', backward=True)
            if entry == 'e16' and T > 320:
                rc, de, dx = backward(N, c, entry, x_bf16, c.pooled, C)
                assert rc == N.VP_EUNSUP and (de == -768.0).all() and (dx == -768.0).all()
                continue
            for lddx in (C, 2 * C):                 # dx dense, and into the left half of a sentinel-filled buffer twice as wide
                rc, de, dxb = backward(N, c, entry, x_bf16, c.pooled, lddx)
                N.check(rc, hctx(N))
                assert (dxb[:, C:] == -768.0).all(), 'dx written outside its C columns'
                dx = dxb[:, :C].reshape(c.B, T, C)
                assert torch.isfinite(de).all() and torch.isfinite(dx).all()
                e_de, e_dx, t_de, t_dx = grad_errors(c, de, dx)
                key = bwd_key(entry, x_bf16)
                print(f'[{key}] T={T} C={C} lddx={lddx}: de {e_de:.2e} dx {e_dx:.2e}; last {min(8, T)} frames: de {t_de:.2e} dx {t_dx:.2e}')
                note(worst, key, de=max(e_de, t_de), dx=max(e_dx, t_dx))
                tol = DE_F32 if entry == 'f32' else DE_BF16
                assert e_de < tol and t_de < tol and e_dx < DX and t_dx < DX, (key, T, C, lddx, e_de, e_dx, t_de, t_dx)


# ------------------------------------------------------------------------------------------------------------ (e) backward, clamp and spike
def check_planted(worst, key, c, de, dx, de_tol):
    """Clamped channels get dx = al dmu and (constant ones) no de; everything is finite; the rest keeps the bounds of (d).

    dx = al dmu "to 1e-6 relative" is taken per (utterance, channel) in rel-L2: an f32 al = expf(e - max) / z carries the rounding
    of e - max, up to 2^-21 |e - max| ~ 5e-7 where al is small, so a per-element 1e-6 would test expf's argument, while any
    contribution of the std (2 dv (x - mu) with dv = dsd / 2e-6: 0.1 dsd on the jitter channel) is five orders above either."""
    C = c.C
    assert torch.isfinite(de).all() and torch.isfinite(dx).all()
    dmu = c.dp.double()[:, None, :C]
    ref_dx = c.al * dmu
    worst_dx = worst_de = 0.0
    for ch in po.CLAMPED:
        for b in range(c.B):
            worst_dx = max(worst_dx, po.rel(dx[b, :, ch], ref_dx[b, :, ch]))
        scale = (dmu * c.x.double() * c.al)[:, :, ch].abs()
        err = (de[:, :, ch].double() - (c.de[:, :, ch] if ch == po.CH_JITTER else 0.0)).abs()
        if ch == po.CH_ZERO:
            assert (err == 0).all()
        else:
            worst_de = max(worst_de, (err / scale).max().item())
    rest = [ch for ch in range(C) if ch not in po.CLAMPED]
    e_de, e_dx, t_de, t_dx = grad_errors(c, de, dx, rest)
    print(f'[{key}] T={c.T}: clamped channels dx {worst_dx:.2e}, de {worst_de:.2e} of |dmu x| al; the rest: de {e_de:.2e} dx {e_dx:.2e}, '
          f'last frames de {t_de:.2e} dx {t_dx:.2e}')
    note(worst, key, clamped_dx=worst_dx, clamped_de=worst_de, de=max(e_de, t_de), dx=max(e_dx, t_dx))
    assert worst_dx <= 1e-6 and worst_de <= 1e-6, (key, c.T, worst_dx, worst_de)
    assert e_de < de_tol and t_de < de_tol and e_dx < DX and t_dx < DX, (key, c.T, e_de, e_dx, t_de, t_dx)


@pytest.mark.parametrize('T', po.T_PLANTED)
def test_clamped_and_spiked_channels_end_to_end_f32(N, worst, T):
    """AttnStats.apply: the forward's own sd = sqrtf(max(var, eps)) decides the backward's mask."""
    from ppvector.train.functions import AttnStats
    c = po.asp_case(T, 64, planted=True, backward=True)
    xd, ed = rows(c.x).requires_grad_(), rows(c.e).requires_grad_()
    pooled = AttnStats.apply(ed, xd, c.B, T)
    pooled.backward(c.dp.cuda())
    mu_err, sd_err = po.forward_errors(pooled.detach().cpu().numpy(), c.pooled, c.e, c.x)
    print(f'[AttnStats planted] T={T}: mu {mu_err:.2e}, std {sd_err:.2e}')
    assert mu_err <= po.MU_BOUND and sd_err <= po.SD_BOUND
    check_planted(worst, 'AttnStats (planted)', c, ed.grad.cpu().view(c.B, T, 64), xd.grad.cpu().view(c.B, T, 64), DE_F32)


@pytest.mark.parametrize('x_bf16', [False, True])
@pytest.mark.parametrize('T', [t for t in po.T_PLANTED if t <= 320])
def test_clamped_and_spiked_channels_end_to_end_bf16_logits(N, worst, T, x_bf16):
    """vp_asp_softmax_stats_l16, then vp_attn_stats_bwd_e16 on its pooled."""
    c = po.asp_case(T, 64, po.R_SWEEP, x_bf16, True, planted=True, backward=True)
    rc, pooled = forward(N, c, 'l16', x_bf16)
    N.check(rc, hctx(N))
    mu_err, sd_err = po.forward_errors(pooled.numpy(), c.pooled, c.e, c.x)
    assert mu_err <= po.MU_BOUND and sd_err <= po.SD_BOUND, (mu_err, sd_err)
    rc, de, dx = backward(N, c, 'e16', x_bf16, pooled, 64)
    N.check(rc, hctx(N))
    check_planted(worst, 'l16 + e16 (planted)' + (' x bf16' if x_bf16 else ' x f32'), c, de, dx.view(c.B, T, 64), DE_BF16)


# ------------------------------------------------------------------------------------------------------------ (f) time statistics
ULP2 = 2.0 ** -22              # dmean * (1.f / T) against dmean / T: two f32 roundings


def assert_constant_channels(c, dx, plus=None):
    for ch in (po.CH_ZERO, po.CH_CONST):
        want = (c.ds.double()[:, ch] / c.T)[:, None].expand(c.B, c.T)
        got = dx[:, :, ch].double() - (0.0 if plus is None else plus[:, :, ch].double())
        tol = ULP2 * want.abs() if plus is None else ULP2 * (want.abs() + 2 * plus[:, :, ch].double().abs())
        assert ((got - want).abs() <= tol).all(), ('constant channel', ch, (got - want).abs().max().item())


@pytest.mark.parametrize('tstp', [False, True])
@pytest.mark.parametrize('C', [64, 98])
@pytest.mark.parametrize('T', po.T_TIME)
def test_time_stats_vs_oracle(N, worst, T, C, tstp):
    """TimeStats.apply: biased, eps = 1e-12 and tstp (unbiased, + 1e-8).  C = 98 takes the scalar time_moments_kernel<float>; the
    backward kernel is four channels wide and refuses C % 4 != 0."""
    from ppvector.train.functions import TimeStats
    c = po.time_case(T, C, tstp)
    xd = rows(c.x).requires_grad_(C % 4 == 0)
    st = TimeStats.apply(xd, c.B, T, tstp)
    e_m, e_s = po.rel(st[:, :C], c.stats[:, :C]), po.rel(st[:, C:], c.stats[:, C:])
    assert e_m < 2e-6 and e_s < 2e-6, (e_m, e_s)
    stc = st.detach().cpu()
    for ch in (po.CH_ZERO, po.CH_CONST):
        assert (stc[:, ch] == (0.0 if ch == po.CH_ZERO else po.CONST)).all()
        assert (stc[:, C + ch] == float(np.sqrt(np.float32(c.eps)))).all()
    key = f'TimeStats tstp={tstp}'
    if C % 4:
        lib, ctx = N.lib(), hctx(N)
        dx, dsd = torch.full_like(xd, -768.0), c.ds.cuda()
        rc = lib.vp_time_stats_bwd_f32(ctx, xd.data_ptr(), C, st.data_ptr(), dsd.data_ptr(), c.B, T, C, c.eps, int(tstp), dx.data_ptr(), C, N.stream_ptr())
        torch.cuda.synchronize()
        assert rc == N.VP_EINVAL and lib.vp_last_error(ctx) and (dx == -768.0).all()
        note(worst, key, mean=e_m, std=e_s)
        return
    st.backward(c.ds.cuda())
    dx = xd.grad.cpu().view(c.B, T, C)
    e_dx = po.rel(dx, c.dx)
    print(f'[{key}] T={T} C={C}: mean {e_m:.2e} std {e_s:.2e} dx {e_dx:.2e}')
    note(worst, key, mean=e_m, std=e_s, dx=e_dx)
    assert torch.isfinite(dx).all() and e_dx < 2e-5, e_dx
    assert_constant_channels(c, dx)


@pytest.mark.parametrize('T', po.T_TIME)
def test_time_stats_coefficients_and_bf16_x_on_clamped_channels(N, worst, T):
    """vp_time_stats_bwd_coeffs on the forward kernel's own stats: beta == 0 and alpha == dmean / T where the clamp held; and
    vp_time_stats_bwd_add_x16 (x stored as bf16, the gradient added to another) on the same channels."""
    lib, ctx = N.lib(), hctx(N)
    C = 64
    c = po.time_case(T, C, False)
    xd, dsd = rows(c.x), c.ds.cuda()
    stats = torch.empty(c.B, 2 * C, device='cuda')
    N.check(lib.vp_time_stats_f32(ctx, xd.data_ptr(), C, c.B, T, C, 1e-12, 0, stats.data_ptr(), N.stream_ptr()), ctx)
    ab = torch.full((2, c.B, C), -768.0, device='cuda')
    N.check(lib.vp_time_stats_bwd_coeffs(ctx, stats.data_ptr(), dsd.data_ptr(), c.B, T, C, 1e-12, ab.data_ptr(), N.stream_ptr()), ctx)
    alpha, beta = ab[0].cpu(), ab[1].cpu()
    for ch in (po.CH_ZERO, po.CH_CONST):
        want = c.ds.double()[:, ch] / T
        assert (beta[:, ch] == 0).all()
        assert ((alpha[:, ch].double() - want).abs() <= ULP2 * want.abs()).all()
    dx = alpha[:, None].double() + beta[:, None].double() * c.x.double()
    e_ab = po.rel(dx, c.dx)
    e_beta = po.rel(beta, c.beta)
    # x stored as bf16, stats as the float64 reference rounded to f32 (on the clamped channels: exactly the forward kernels' sqrtf(eps))
    c16 = po.time_case(T, C, False, x_bf16=True)
    st16 = c16.stats.float()
    assert (st16[:, [C + po.CH_ZERO, C + po.CH_CONST]] == float(np.sqrt(np.float32(1e-12)))).all()
    g = torch.Generator().manual_seed(T)
    add = torch.randn(c.B * T, C, generator=g)
    out, x16d, st16d, ds16d = add.clone().cuda(), rows(c16.x, True), st16.cuda(), c16.ds.cuda()
    N.check(lib.vp_time_stats_bwd_add_x16(ctx, x16d.data_ptr(), C, st16d.data_ptr(), ds16d.data_ptr(), c.B, T, C, 1e-12, 0,
                                          out.data_ptr(), C, out.data_ptr(), C, N.stream_ptr()), ctx)
    got = out.cpu().view(c.B, T, C)
    e_x16 = po.rel(got.double() - add.view(c.B, T, C).double(), c16.dx)
    print(f'[time stats coeffs / x16] T={T}: alpha + beta x {e_ab:.2e}, beta {e_beta:.2e}, add_x16 {e_x16:.2e}')
    note(worst, 'vp_time_stats_bwd_coeffs', dx=e_ab, beta=e_beta)
    note(worst, 'vp_time_stats_bwd_add_x16', dx=e_x16)
    assert e_ab < 2e-5 and e_beta < 2e-5 and e_x16 < 2e-5
    assert_constant_channels(c16, got, plus=add.view(c.B, T, C))


@pytest.mark.parametrize('T', [7, 161])
def test_time_stats_bwd_add_f32_in_place(N, worst, T):
    """vp_time_stats_bwd_add_f32 (the f32 ASP backward with global context; no other test names it): the gradient through the
    biased statistics added in place to another gradient of x, handed the float64 reference's stats rounded to f32.  The f32 sum
    add + g rounds at half an ulp of add (~1): 6e-8 against g ~ 2 / T, 5e-6 at T = 161 -- inside the family's 2e-5."""
    lib, ctx = N.lib(), hctx(N)
    C = 64
    c = po.time_case(T, C, False)
    add = torch.randn(c.B * T, C, generator=torch.Generator().manual_seed(T))
    out, xd, st, dsd = add.clone().cuda(), rows(c.x), c.stats.float().cuda(), c.ds.cuda()
    N.check(lib.vp_time_stats_bwd_add_f32(ctx, xd.data_ptr(), C, st.data_ptr(), dsd.data_ptr(), c.B, T, C, 1e-12, 0, out.data_ptr(), C,
                                          out.data_ptr(), C, N.stream_ptr()), ctx)
    got = out.cpu().view(c.B, T, C)
    e_dx = po.rel(got.double() - add.view(c.B, T, C).double(), c.dx)
    print(f'[time stats add_f32] T={T}: dx {e_dx:.2e}')
    note(worst, 'vp_time_stats_bwd_add_f32', dx=e_dx)
    assert torch.isfinite(got).all() and e_dx < 2e-5, e_dx
    assert_constant_channels(c, got, plus=add.view(c.B, T, C))


# ------------------------------------------------------------------------------------------------------------ (g) argument checks
@pytest.mark.parametrize('bad', ['B = 65536', 'T = 0', 'null pooled'])
def test_argument_checks(N, bad):
    lib, ctx = N.lib(), hctx(N)
    B, T, C = 2, 8, 64
    f32 = torch.zeros(B * T, C, device='cuda')
    b16 = torch.zeros(B * T, C, dtype=torch.bfloat16, device='cuda')
    pooled = torch.zeros(B, 2 * C, device='cuda')
    Bb, Tb = (65536 if bad == 'B = 65536' else B), (0 if bad == 'T = 0' else T)
    pp = None if bad == 'null pooled' else pooled.data_ptr()
    st = N.stream_ptr()
    calls = {
        'vp_asp_softmax_stats': lambda: lib.vp_asp_softmax_stats(ctx, N.VP_F32, f32.data_ptr(), f32.data_ptr(), C, 0, Bb, Tb, C, 1e-12, pp, st),
        'vp_asp_softmax_stats_l16': lambda: lib.vp_asp_softmax_stats_l16(ctx, b16.data_ptr(), f32.data_ptr(), N.VP_F32, C, 0, Bb, Tb, C, 1e-12, pp, st),
        'vp_attn_stats_bwd_f32': lambda: lib.vp_attn_stats_bwd_f32(ctx, f32.data_ptr(), f32.data_ptr(), C, pp, pooled.data_ptr(), Bb, Tb, C, 1e-12,
                                                                   f32.data_ptr(), f32.data_ptr(), C, st),
        'vp_attn_stats_bwd_e16': lambda: lib.vp_attn_stats_bwd_e16(ctx, b16.data_ptr(), f32.data_ptr(), N.VP_F32, C, pp, pooled.data_ptr(), Bb, Tb, C,
                                                                   1e-12, b16.data_ptr(), f32.data_ptr(), C, st),
    }
    # (the context keeps the last message: each call must leave its own, told apart by the entry point's tag)
    tags = {'vp_asp_softmax_stats': 'asp:', 'vp_asp_softmax_stats_l16': 'asp_l16:', 'vp_attn_stats_bwd_f32': 'attn_stats_bwd:',
            'vp_attn_stats_bwd_e16': 'attn_stats_bwd_e16:'}
    for name, call in calls.items():
        rc = call()
        msg = lib.vp_last_error(ctx).decode()
        assert rc == N.VP_EINVAL, (name, bad, rc)
        assert msg.startswith(tags[name]) and len(msg) > len(tags[name]) + 1, (name, bad, msg)
    torch.cuda.synchronize()
