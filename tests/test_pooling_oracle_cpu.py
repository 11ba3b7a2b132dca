"""Pins tests/pooling_oracle.py -- the float64 reference, the planted inputs and the forward bound of tests/test_gpu_pooling_stats.py --
on the CPU: the closed forms written in the kernels' comments are float64 autograd; constant channels get what the kernels are
held to; the float32 restatement of the forward says where the GPU bound comes from; the float32 facts the clamp mask rests on."""
import numpy as np
import pytest
import torch

from tests import pooling_oracle as po


def _close(got, ref, tol=1e-12):
    """max-abs against the reference's own scale (float64 closed form against float64 autograd)."""
    return (got - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


# -------------------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize('T,C,r,planted', [(1, 8, 3, False), (2, 8, 3, False), (9, 8, 0, False), (47, 16, 3, False), (37, 16, 3, True),
                                           (333, 8, 10, True)])
def test_asp_closed_forms_are_float64_autograd(T, C, r, planted):
    """dv, dalpha, S, de, dx of csrc/pooling_stats.hip against autograd of the defining graph, intermediate by intermediate."""
    x, e, dp = po.inputs(2, T, C, r, 11 * T + C, planted)
    cf = po.asp_stats_bwd_closed(e, x, dp)
    de, dx = po.asp_stats_bwd(e, x, dp)
    assert _close(cf.de, de) and _close(cf.dx, dx)
    # the intermediates: gradients of the same loss with respect to alpha and the variance, as autograd sees them
    ed, xd = e.double(), x.double()
    al = torch.softmax(ed, dim=1).requires_grad_()
    mu = (al * xd).sum(1)
    var = (al * (xd - mu[:, None]) ** 2).sum(1)
    var.retain_grad()
    sd = torch.sqrt(torch.where(var > po.EPS, var, torch.full_like(var, po.EPS)))
    (torch.cat([mu, sd], 1) * dp.double()).sum().backward()
    assert _close(cf.dv, var.grad)
    # d loss / d alpha_t = dmu x_t + dv ((x_t - mu)^2 - 2 sum_s alpha_s (x_s - mu) x_t); the last sum is 0 at the softmax's alpha
    assert _close(cf.dalpha, al.grad)
    assert _close(cf.S, (al.detach() * al.grad).sum(1))


@pytest.mark.parametrize('T', [1, 2, 9, 57])
def test_time_stats_coefficient_form_is_float64_autograd(T):
    """alpha + beta x of vp_time_stats_bwd_coeffs against autograd of [mean | sqrt(clamp(var_biased, eps))]."""
    c = po.time_case(T, 16, False)
    assert _close(c.alpha[:, None] + c.beta[:, None] * c.x.double(), c.dx)
    for ch in (po.CH_ZERO, po.CH_CONST):
        assert (c.beta[:, ch] == 0).all() and torch.equal(c.alpha[:, ch], c.ds.double()[:, ch] / T)


def test_unbiased_std_of_one_frame_and_of_a_constant_channel_with_eps_0():
    """The 0 / 0 -> 0 limit: what torch.std's backward gives at var = 0, and a finite value for T = 1 (torch.std: NaN)."""
    x, _, ds = po.inputs(2, 6, 8, 3, 5)
    x[:, :, po.CH_CONST] = po.CONST
    st, dx = po.time_stats(x, 0.0, True), po.time_stats_bwd(x, ds, 0.0, True)
    ref = x.double().std(1, unbiased=True)
    assert _close(st[:, 8:], ref) and torch.isfinite(dx).all()
    assert torch.equal(dx[:, :, po.CH_CONST], (ds.double()[:, po.CH_CONST] / 6)[:, None].expand(2, 6))
    xr = x.double().clone().requires_grad_()
    (torch.cat([xr.mean(1), xr.std(1, unbiased=True)], 1) * ds.double()).sum().backward()
    keep = [ch for ch in range(8) if ch != po.CH_CONST]
    assert _close(dx[:, :, keep], xr.grad[:, :, keep])
    one = po.time_stats(x[:, :1], po.EPS_TSTP, True)
    assert torch.equal(one[:, 8:], torch.full((2, 8), po.EPS_TSTP, dtype=torch.float64).sqrt())


# -------------------------------------------------------------------------------------------------------- planted channels
@pytest.mark.parametrize('T', po.T_PLANTED)
def test_planted_channels_in_float64(T):
    """Clamped channels: dx = al dmu and de = 0 (to 1e-12); the spikes are one-hot, clamped, and mu sits on the spiked frame."""
    c = po.asp_case(T, 64, planted=True, backward=True)
    C = c.C
    dmu = c.dp.double()[:, None, :C]
    for ch in po.CLAMPED:
        assert (c.pooled[:, C + ch] == po.EPS ** 0.5).all()
        assert _close(c.dx[:, :, ch], (c.al * dmu)[:, :, ch])
    for ch in (po.CH_ZERO, po.CH_CONST):
        assert c.de[:, :, ch].abs().max().item() <= 1e-12
    assert c.de[:, :, po.CH_JITTER].abs().max().item() <= 1e-6              # (x moves by an ulp: de = al dmu (x_t - mu), ~1e-7)
    for ch, t in ((po.CH_SPIKE_FIRST, 0), (po.CH_SPIKE_LAST, T - 1)):
        assert (c.al[:, t, ch] >= 1 - 1e-15).all() and (c.pooled[:, C + ch] == po.EPS ** 0.5).all()
        assert torch.equal(c.pooled[:, ch].float(), c.x[:, t, ch])
    ulp = float(np.spacing(np.float32(po.CONST)))
    jit = c.x[:, :, po.CH_JITTER].double() - po.CONST
    assert set(np.unique(jit.numpy() / ulp)) == {-1.0, 0.0, 1.0}


@pytest.mark.parametrize('T', po.T_TIME)
@pytest.mark.parametrize('tstp', [False, True])
def test_time_stats_constant_channels_in_float64(T, tstp):
    c = po.time_case(T, 64, tstp)
    for ch in (po.CH_ZERO, po.CH_CONST):
        assert torch.equal(c.dx[:, :, ch], (c.ds.double()[:, ch] / T)[:, None].expand(c.B, T))
        assert (c.stats[:, c.C + ch] == c.eps ** 0.5).all()


# -------------------------------------------------------------------------------------------------------- the forward bound
def forward_table():
    """Every (T, C, r, x_bf16, e_bf16) of the GPU forward tests (a), (b) and (c)."""
    cases = []
    for T in po.T_SWEEP:
        cases += [(T, C, po.R_SWEEP, False, False) for C in (64, 100)] + [(T, C, po.R_SWEEP, True, False) for C in (64, 96)]
        if T <= 320:
            cases += [(T, C, po.R_SWEEP, xb, True) for C in (64, 96) for xb in (False, True)]
    for T in po.T_COND:
        for r in po.R_COND:
            cases += [(T, 64, r, False, False)] + ([(T, 64, r, xb, True) for xb in (False, True)] if T <= 320 else [])
    return sorted(set(cases))


@pytest.fixture(scope='module')
def restated():
    """case -> {centre: (mu error, std error)} of the float32 restatement against float64, over the whole forward table."""
    out = {}
    for case in forward_table():
        c = po.asp_case(*case)
        out[case] = {centre: po.forward_errors(po.asp_stats_f32_restatement(c.e.numpy(), c.x.numpy(), po.EPS, centre), c.pooled, c.e, c.x)
                     for centre in (None, 'first_frame', 'two_pass')}
    return out


def test_f32_restatement_of_the_kernels_formula_is_within_a_quarter_of_the_gpu_bound(restated):
    """The GPU forward bound (std 2e-5 relative per element) is four times what float32 arithmetic itself costs the formula the
    kernels compute (first-frame centre, variance from a second pass): <= 5e-6 on every case of the table.  Measured: std 2.5e-7,
    mu 1.1e-6 of sum al |x| (the first frame can be several std from a mean near 0 at r = 0)."""
    worst_mu = max(v['two_pass'][0] for v in restated.values())
    worst_sd = max(v['two_pass'][1] for v in restated.values())
    print(f'two_pass restatement over {len(restated)} cases: mu {worst_mu:.2e} of sum al|x|, std {worst_sd:.2e} relative')
    assert worst_sd <= po.SD_BOUND / 4
    assert worst_mu <= po.MU_BOUND / 2


def test_one_pass_first_frame_centring_holds_at_long_utterances_only(restated):
    """s2 / s0 - md^2 about the first frame: within a quarter of the bound on the conditioning table's register-kernel sizes
    (T = 47, 200: 4.7e-6 at every r), where var ~ (mu - x_0)^2.  It does NOT hold the bound over the T sweep: a softmax over few
    frames is peaked, mu sits on one frame and var << (mu - x_0)^2 -- 6e-4 at T = 2, 4e-5 at T = 9, single elements above 5e-6 up to
    T = 333.  Hence the second pass in the kernels; this test documents that the bound tells the two apart."""
    cond = [v['first_frame'][1] for k, v in restated.items() if k[0] in (47, 200) and k[1] == 64 and k[2] in po.R_COND]
    print(f'first_frame one-pass, T = 47 / 200 conditioning cases: std {max(cond):.2e}')
    assert max(cond) <= po.SD_BOUND / 4
    short = max(v['first_frame'][1] for k, v in restated.items() if k[0] == 2)
    print(f'first_frame one-pass, T = 2: std {short:.2e}')
    assert short > po.SD_BOUND


def test_uncentred_restatement_exceeds_the_gpu_bound_at_r_30(restated):
    """Raw E[x^2] - E[x]^2 loses (mean / std)^2 of the precision: the bound separates it from the centred formulas."""
    for T in po.T_COND:
        raw, two = restated[(T, 64, 30, False, False)][None][1], restated[(T, 64, 30, False, False)]['two_pass'][1]
        print(f'T = {T}, r = 30: uncentred std error {raw:.2e}, two-pass {two:.2e}')
        assert raw > po.SD_BOUND > 4 * two


# -------------------------------------------------------------------------------------------------------- the clamp mask
@pytest.mark.parametrize('eps', [1e-12, 1e-8])
def test_f32_sqrt_of_the_clamp_squares_back_to_no_more_than_the_clamp(eps):
    """The backward kernels infer "the forward clamped" from sd * sd > eps on the stored sd = sqrtf(max(var, eps)): a clamped
    channel must square back to <= eps in float32.  True at the two eps the engine uses (a correctly rounded sqrtf; 1e-6 does not)."""
    e32 = np.float32(eps)
    sd = np.sqrt(e32)
    assert sd.dtype == np.float32 and not sd * sd > e32
    assert np.nextafter(sd, np.float32(1)) ** 2 > e32               # and the very next sd counts as unclamped
    e6 = np.float32(1e-6)
    assert np.sqrt(e6) * np.sqrt(e6) > e6                           # (why the inference must not be reused at another eps)
