"""Oracle (CPU, float64) of the pooling statistics the training step runs through, and the inputs that put their kernels to work.
Test helper, not a test module; imports nothing of the engine.

Attentive statistics (pooling.py:114-123), exactly as the kernels define them:
    al = softmax_t(e);  mu = sum_t al x;  sd = sqrt(clamp(sum_t al (x - mu)^2, min=eps))
with the clamp's subgradient ZERO when it clamps (var <= eps).  Time statistics: [mean | sqrt(clamp(var_biased, eps))] (the ASP
context) or [mean | sqrt(var_unbiased + eps)] (TemporalStatsPool), the variance of a single frame taken as 0 and d sqrt(0) as 0
(what torch.std returns).  Every function takes the float64 images of the f32 / bf16 numbers a kernel reads, shaped (B, T, C).

`asp_stats_bwd` / `time_stats_bwd` are float64 autograd; `asp_stats_bwd_closed` / `time_stats_bwd_coeffs` are the closed forms
written in the comments of csrc/pooling_stats.hip (tests/test_pooling_oracle_cpu.py holds them to autograd at 1e-12).

`asp_stats_f32_restatement` is NOT a reference: it restates the forward in float32 NumPy in the kernels' order of operations and
exists to say how far ANY f32 one-pass implementation of that formula lies from float64 -- the forward bound of
tests/test_gpu_pooling_stats.py is four times its worst error over the same table, so the bound comes from the reference side.

`inputs` builds the seeded operands: x = r s_c + s_c N(0,1) with a per-channel scale s_c in [0.2, 2] and r = mean / std the
conditioning ratio (0: centred data; 3 ... 10: what a BatchNorm with |beta| / gamma of 3 ... 10 hands on); e = 2 N(0,1).
"""
import functools
import types

import numpy as np
import torch

EPS = float(np.float32(1e-12))             # the clamp of the ASP statistics as the kernels receive it (a C float)
EPS_TSTP = float(np.float32(1e-8))

# the T at which the statistics kernels change: one frame; fewer frames than the 8 frame groups of the register kernels; one more
# than 8; no multiple of 8; both sides of reg<20> / reg<40> (160) and of reg<40> / streaming (320); deep in the streaming kernel
T_SWEEP = (1, 2, 7, 8, 9, 47, 159, 160, 161, 319, 320, 321, 333)
T_COND = (47, 200, 333)                    # one per kernel
R_COND = (0, 3, 10, 30)
R_SWEEP = 3                                # the T sweeps run at an ordinary BatchNorm output
T_PLANTED = (37, 200, 333)
T_TIME = (1, 8, 9, 32, 33, 57)
B = 2

# planted channels (`inputs(..., planted=True)`), the same in every utterance
CH_ZERO, CH_CONST, CH_SPIKE_FIRST, CH_SPIKE_LAST, CH_JITTER = 1, 2, 3, 4, 5
CONST = 1.25
SPIKE = 60.0
# CH_ZERO, CH_CONST: exactly constant over time -- the weighted variance is 0, the clamp holds, sd = sqrt(eps).
# CH_SPIKE_*: one logit 60 above the rest, on frame 0 / frame T - 1: softmax is one-hot to 1e-26, the variance ~1e-26 clamps although
#   x varies, mu sits on one frame's x (frame 0 is also what the forward kernels centre on; frame T - 1 is not).
# CH_JITTER: 1.25 +- one f32 ulp: variance ~1e-14 < eps clamps, yet x - mu != 0 in f32 -- the channel on which a backward that
#   takes the clamped sd = 1e-6 for a real one (dv = dsd / 2e-6) adds a spurious 0.1 dsd to dx.  (On the exactly constant channels
#   x - mu is 0 in f32 once the forward centres on a frame, and such a backward would go unnoticed.)
CLAMPED = (CH_ZERO, CH_CONST, CH_JITTER)


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def inputs(Bn, T, C, r, seed, planted=False, x_bf16=False, e_bf16=False):
    """-> x, e (Bn, T, C) float32 holding the numbers as stored (rounded to bf16 where asked), dpooled (Bn, 2C) float32."""
    g = torch.Generator().manual_seed(seed)
    s = 0.2 + 1.8 * torch.rand(C, generator=g, dtype=torch.float64)
    x = (r * s + s * torch.randn(Bn, T, C, generator=g, dtype=torch.float64)).float()
    e = (2 * torch.randn(Bn, T, C, generator=g, dtype=torch.float64)).float()
    dp = torch.randn(Bn, 2 * C, generator=g, dtype=torch.float64).float()
    if planted:
        assert C > CH_JITTER
        x[:, :, CH_ZERO] = 0.0
        x[:, :, CH_CONST] = CONST
        e[:, 0, CH_SPIKE_FIRST] += SPIKE
        e[:, T - 1, CH_SPIKE_LAST] += SPIKE
        ulp = float(np.spacing(np.float32(CONST)))
        x[:, :, CH_JITTER] = (CONST + ulp * torch.randint(-1, 2, (Bn, T), generator=g).double()).float()
    if x_bf16:
        x = bf16_round(x)               # (0, 1.25 and the spikes survive; the jitter channel becomes exactly constant)
    if e_bf16:
        e = bf16_round(e)
    return x, e, dp


# ---------------------------------------------------------------------------------------------------- attentive statistics
def _asp_graph(e, x, eps):
    al = torch.softmax(e, dim=1)
    mu = (al * x).sum(1)
    var = (al * (x - mu[:, None]) ** 2).sum(1)
    sd = torch.sqrt(torch.where(var > eps, var, torch.full_like(var, eps)))         # (the constant branch carries no gradient)
    return al, mu, var, sd


def asp_stats(e, x, eps=EPS):
    """[mu | sd] (B, 2C), float64."""
    _, mu, _, sd = _asp_graph(e.double(), x.double(), eps)
    return torch.cat([mu, sd], 1)


def asp_stats_bwd(e, x, dpooled, eps=EPS):
    """(de, dx) of sum(pooled * dpooled) by float64 autograd."""
    e, x = e.double().clone().requires_grad_(), x.double().clone().requires_grad_()
    _, mu, _, sd = _asp_graph(e, x, eps)
    (torch.cat([mu, sd], 1) * dpooled.double()).sum().backward()
    return e.grad, x.grad


def asp_stats_bwd_closed(e, x, dpooled, eps=EPS):
    """The closed forms of csrc/pooling_stats.hip (attn_stats_bwd_kernel's comment), float64:
        dv = [var > eps] dsd / (2 sd);  dalpha_t = dmu x_t + dv (x_t - mu)^2;  S = sum_t alpha_t dalpha_t
        de_t = alpha_t (dalpha_t - S);  dx_t = alpha_t (dmu + 2 dv (x_t - mu))"""
    e, x, dp = e.double(), x.double(), dpooled.double()
    C = x.shape[2]
    al, mu, var, sd = _asp_graph(e, x, eps)
    dmu, dsd = dp[:, None, :C], dp[:, None, C:]
    dv = torch.where(var > eps, dp[:, C:] / (2 * sd), torch.zeros_like(sd))[:, None]
    d = x - mu[:, None]
    dalpha = dmu * x + dv * d * d
    S = (al * dalpha).sum(1, keepdim=True)
    return types.SimpleNamespace(al=al, dv=dv[:, 0], dalpha=dalpha, S=S[:, 0], de=al * (dalpha - S), dx=al * (dmu + 2 * dv * d))


def asp_stats_f32_restatement(e, x, eps=EPS, centre=None):
    """The forward in float32 NumPy, in the register kernels' order: subtract the per-channel max of the logits; p = exp(e - max);
    frame t goes to group t % 8, each group accumulates its sums sequentially over its frames, the 8 groups are then summed in order.
    centre:
      None           one pass, d = x:  md = sum p d / sum p, var = sum p d^2 / sum p - md^2  (raw E[x^2] - E[x]^2)
      'first_frame'  the same with d = x - (the utterance's frame 0 of the channel), mu = centre + md
      'two_pass'     d and mu as 'first_frame'; the variance from a second pass, var = sum p (d - md)^2 / sum p -- what the kernels
                     compute when no centre is handed to them
    sd = sqrt(max(var, eps)).  -> [mu | sd] float32"""
    assert centre in (None, 'first_frame', 'two_pass')
    f = np.float32
    e, x = np.asarray(e, dtype=f), np.asarray(x, dtype=f)
    Bn, T, C = x.shape
    c0 = np.zeros((Bn, C), f) if centre is None else x[:, 0, :].copy()
    mx = e.max(axis=1)

    def grouped(term):
        acc = np.zeros((8, Bn, C), f)
        for t in range(T):
            acc[t % 8] += term(t)
        tot = np.zeros((Bn, C), f)
        for g in range(8):
            tot += acc[g]
        return tot

    p = lambda t: np.exp(e[:, t] - mx, dtype=f)
    d = lambda t: x[:, t] - c0
    t0, t1 = grouped(p), grouped(lambda t: p(t) * d(t))
    md = t1 / t0
    if centre == 'two_pass':
        var = grouped(lambda t: p(t) * (d(t) - md) * (d(t) - md)) / t0
    else:
        var = grouped(lambda t: p(t) * d(t) * d(t)) / t0 - md * md
    return np.concatenate([c0 + md, np.sqrt(np.maximum(var, f(eps)))], axis=1)


def forward_errors(got, ref, e, x):
    """The two per-element figures the forward is held to: max |mu - ref| / sum_t al |x|  and  max |sd - ref| / ref.
    got: (B, 2C) array-like in any precision; ref = asp_stats(e, x)."""
    got = torch.as_tensor(np.asarray(got)).double()
    C = x.shape[2]
    scale = (torch.softmax(e.double(), dim=1) * x.double().abs()).sum(1)
    num = (got[:, :C] - ref[:, :C]).abs()
    # (an all-zero channel has scale 0: its mu must be exactly 0)
    mu_err = torch.where(scale > 0, num / scale.clamp(min=1e-300), torch.where(num == 0, 0.0, float('inf'))).max().item()
    sd_err = ((got[:, C:] - ref[:, C:]).abs() / ref[:, C:]).max().item()
    return mu_err, sd_err


MU_BOUND, SD_BOUND = 4e-6, 2e-5            # the GPU forward bounds; the f32 restatement stays within SD_BOUND / 4 (test_pooling_oracle_cpu.py)


# ---------------------------------------------------------------------------------------------------- time statistics
def _time_graph(x, eps, unbiased):
    T = x.shape[1]
    m = x.mean(1)
    ss = ((x - m[:, None]) ** 2).sum(1)
    if unbiased:
        v = ss / max(T - 1, 1) + eps
        pos = v > 0                                                 # eps = 0 on a constant channel: sqrt(0) with derivative 0
        sd = torch.where(pos, torch.sqrt(torch.where(pos, v, torch.ones_like(v))), torch.zeros_like(v))
    else:
        v = ss / T
        sd = torch.sqrt(torch.where(v > eps, v, torch.full_like(v, eps)))
    return m, v, sd


def time_stats(x, eps=EPS, unbiased=False):
    """[mean | std] (B, 2C), float64."""
    m, _, sd = _time_graph(x.double(), eps, unbiased)
    return torch.cat([m, sd], 1)


def time_stats_bwd(x, dstats, eps=EPS, unbiased=False):
    """dx of sum(stats * dstats) by float64 autograd."""
    x = x.double().clone().requires_grad_()
    m, _, sd = _time_graph(x, eps, unbiased)
    (torch.cat([m, sd], 1) * dstats.double()).sum().backward()
    return x.grad


def time_stats_bwd_coeffs(x, dstats, eps=EPS):
    """The biased branch's gradient as per-utterance coefficients, dx[b, t, c] = alpha[b, c] + beta[b, c] x[b, t, c]
    (vp_time_stats_bwd_coeffs): beta = [var > eps] dstd / (std T), alpha = dmean / T - beta mean.  -> alpha, beta (B, C) float64"""
    x, ds = x.double(), dstats.double()
    T, C = x.shape[1], x.shape[2]
    m, v, sd = _time_graph(x, eps, False)
    beta = torch.where(v > eps, ds[:, C:] / (sd * T), torch.zeros_like(sd))
    return ds[:, :C] / T - beta * m, beta


# ---------------------------------------------------------------------------------------------------- cases, built once
@functools.lru_cache(maxsize=None)
def asp_case(T, C, r=R_SWEEP, x_bf16=False, e_bf16=False, planted=False, backward=False, Bn=B):
    """One case of the tables above: the stored operands, the float64 reference of the forward and (backward=True) of the gradients.
    Cached and shared between tests: treat every tensor as read-only."""
    seed = 1000 * T + C + 7 * int(r) + (1 << 20) * (2 * int(x_bf16) + int(e_bf16)) + (1 << 22) * int(planted)
    x, e, dp = inputs(Bn, T, C, r, seed, planted, x_bf16, e_bf16)
    c = types.SimpleNamespace(B=Bn, T=T, C=C, r=r, x=x, e=e, dp=dp, pooled=asp_stats(e, x))
    if backward:
        c.de, c.dx = asp_stats_bwd(e, x, dp)
        c.al = torch.softmax(e.double(), dim=1)
    return c


@functools.lru_cache(maxsize=None)
def time_case(T, C, tstp, x_bf16=False, Bn=B):
    """x with the two constant channels planted, d stats, the float64 [mean | std], dx and (biased) alpha / beta."""
    x, _, ds = inputs(Bn, T, C, R_SWEEP, 77000 + 100 * T + C + int(tstp), False, x_bf16)
    x[:, :, CH_ZERO] = 0.0
    x[:, :, CH_CONST] = CONST
    eps = EPS_TSTP if tstp else EPS
    c = types.SimpleNamespace(B=Bn, T=T, C=C, x=x, ds=ds, eps=eps, stats=time_stats(x, eps, tstp), dx=time_stats_bwd(x, ds, eps, tstp))
    if not tstp:
        c.alpha, c.beta = time_stats_bwd_coeffs(x, ds, eps)
    return c


def rel(a, b):
    """rel-L2 as the suite's GPU tests take it."""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-30)).item()
