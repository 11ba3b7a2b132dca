"""tests/bn_oracle.py pinned against float64 torch (batch_norm + autograd) and the Paddle shim's BatchNorm, and the float32 calibration of
the four variance formulas behind the bounds of tests/test_gpu_bn_train.py (docs/bn_train.md quotes the printed tables).  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bn_oracle as bo


def _case(M, C, r, seed):
    g = np.random.default_rng(seed)
    z = bo.conditioned(M, C, r, seed)
    gamma, beta, rm, rv = bo.affine_params(C, seed)
    dy = g.standard_normal((M, C)).astype(np.float32)
    return z, gamma, beta, rm, rv, dy


@pytest.mark.parametrize('M,C,r', [(2, 8, 0), (19, 6, 3), (48, 64, 10), (257, 12, 30)])
@pytest.mark.parametrize('act', [0, 1, 2])
def test_oracle_vs_torch_float64(M, C, r, act):
    z, gamma, beta, rm, rv, dy = _case(M, C, r, 3)
    o = bo.forward(z, gamma, beta, act=act, run_mean=rm, run_var=rv)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    gt, bt = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (gamma, beta))
    rmt, rvt = torch.tensor(rm, dtype=torch.float64), torch.tensor(rv, dtype=torch.float64)
    y = F.batch_norm(zt, None, None, gt, bt, True, 0.0, bo.EPS)
    ya = y if act == 0 else (y.clamp(min=0) if act == 1 else y.clamp(0, 20))
    np.testing.assert_allclose(o.y, ya.detach().numpy(), rtol=1e-12, atol=1e-12)
    dyt = torch.tensor(dy, dtype=torch.float64)
    ya.backward(dyt)
    # the activation behind the BatchNorm, as a mask on dy re-evaluated from z (what the folded backward does)
    behind = None if act == 0 else bo.mask_behind(z, bo.f32(o.scale), bo.f32(o.shift), 20.0 if act == 2 else 0.0)
    if behind is not None:                      # (f32 scale / shift move no element of this data across 0 or 20)
        assert (behind == ((y.detach().numpy() > 0) & ((y.detach().numpy() < 20) if act == 2 else True))).all()
    dz, dgamma, dbeta, dbias = bo.backward(dy, z, o.mean, o.invstd, gamma, behind=behind)
    scale = np.abs(zt.grad.numpy()).max()
    np.testing.assert_allclose(dz, zt.grad.numpy(), rtol=0, atol=1e-9 * max(scale, 1.0) * (1 + r * r))
    np.testing.assert_allclose(dgamma, gt.grad.numpy(), rtol=1e-9 * (1 + r * r), atol=1e-9 * (1 + r * r))
    np.testing.assert_allclose(dbeta, bt.grad.numpy(), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(dbias, dz.sum(0), rtol=0, atol=1e-12)
    # the planted channels: exactly constant ones have variance 0 (invstd = eps^-1/2), the jitter channel ~1e-14
    assert o.var[bo.CH_CONST] == 0 and o.var[bo.CH_ZERO] == 0 and 0 <= o.var[bo.CH_JITTER] < 1e-13
    # a ReLU in FRONT of the BatchNorm (TDNNBlock): z = relu(u), d u = [u > 0] d z
    ut = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    zr = torch.relu(ut)                         # (subgradient 0 at 0, as the kernels' z > 0; the all-zero channel sits there)
    F.batch_norm(zr, None, None, gt.detach(), bt.detach(), True, 0.0, bo.EPS).backward(dyt)
    zr = zr.detach().numpy()
    of = bo.forward(zr)
    dzf = bo.backward(dy, zr, of.mean, of.invstd, gamma, front=bo.mask_front(zr))[0]
    np.testing.assert_allclose(dzf, ut.grad.numpy(), rtol=0, atol=1e-9 * max(np.abs(ut.grad.numpy()).max(), 1.0) * (1 + r * r))


def test_running_statistics_follow_the_paddle_convention():
    """run = mom * run + (1 - mom) * batch with the BIASED variance (oracle/paddle_shim.py; torch blends the unbiased one, the other way round)."""
    from oracle import paddle_shim as ps
    z, gamma, beta, rm, rv, _ = _case(19, 8, 3, 5)
    bn = ps.BatchNorm1D(8, momentum=0.9, epsilon=bo.EPS).double()          # (eps as the kernels receive it: a C float)
    with torch.no_grad():
        bn.weight.copy_(torch.tensor(gamma)), bn.bias.copy_(torch.tensor(beta))
        bn._mean.copy_(torch.tensor(rm)), bn._variance.copy_(torch.tensor(rv))
    bn.train()
    y = bn(torch.tensor(z, dtype=torch.float64))
    o = bo.forward(z, gamma, beta, run_mean=rm, run_var=rv, mom=0.9)
    np.testing.assert_allclose(o.y, y.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(o.y, bo.clamp(z * o.scale + o.shift, 0), rtol=0, atol=1e-11)      # (the folded form the kernels apply)
    np.testing.assert_allclose(o.run_mean, bn._mean.numpy(), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(o.run_var, bn._variance.numpy(), rtol=1e-13, atol=1e-15)
    unbiased = 0.9 * rv.astype(np.float64) + 0.1 * o.var * 19 / 18
    assert np.abs(unbiased - o.run_var)[0] > 1e-4 * o.run_var[0]           # the two conventions are far apart at M = 19
    # from_partials on exact partial sums is the same statistics, raw or about a centre
    zz = z.astype(np.float64)
    for center in (None, zz[0]):
        d = zz - (0 if center is None else center)
        p = bo.from_partials(np.stack([d[:7].sum(0), d[7:].sum(0)]), np.stack([(d[:7] ** 2).sum(0), (d[7:] ** 2).sum(0)]), 19, center)
        np.testing.assert_allclose(p.mean, o.mean, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(p.var, o.var, rtol=1e-9, atol=1e-13)


def test_bf16_helpers():
    v = np.array([1.0, 1.00390625, 1.01171875, -3.7, 0.0, 1e-3, 65280.0, 2.0 ** -120], dtype=np.float32)
    want = torch.tensor(v).to(torch.bfloat16).float().numpy()
    assert (bo.bf16_round(v) == want).all()
    assert bo.bf16_round(np.float32(1.00390625)) == 1.0 and bo.bf16_round(np.float32(1.01171875)) == np.float32(1.015625)    # ties to even
    g = np.random.default_rng(0)
    w = (g.standard_normal(4096) * 10.0 ** g.uniform(-6, 6, 4096)).astype(np.float32)
    assert (bo.bf16_round(w) == torch.tensor(w).to(torch.bfloat16).float().numpy()).all()
    assert bo.bf16_ulp(1.0) == 2.0 ** -7 and bo.bf16_ulp(-1.99) == 2.0 ** -7 and bo.bf16_ulp(2.0) == 2.0 ** -6
    assert bo.fma32(np.float32(3), np.float32(1 + 2 ** -23), np.float32(-3)) == np.float32(3 * 2 ** -23)


def test_calibration_of_the_variance_formulas():
    """float32 restatements over conditioned(M, 64, r), the sums added in the kernels' order: (b) two-pass, (c) sums about row 0 and
    (d) sums about the mean of the first eight rows hold the invstd bound 2e-6 at every r; (a) raw sums -- what the conv paths run, and BNRows ran --
    leaves it at r >= 30.
    (c) holds it with little to spare, and added strictly row after row (printed, not asserted) it does not: where row 0 lies k std from
    the mean, (c) costs (1 + k^2) roundings (k^2 <= M - 1), so at k = 3.3 (M = 48, r = 0, channel 21) it reaches 2.3e-6 -- and on centred
    data it is worse than the raw sums it replaces.  (d) has k^2 ~ 1/8: it keeps 4x of margin: what BNRows runs (docs/bn_train.md)."""
    rows = {}
    for r in bo.R_SWEEP:
        for M in bo.M_SWEEP:
            rows[M, r] = tuple(bo.invstd_error_f32(M, r, f) for f in 'abcd')
            print(f'[bn calibration, rows in sequence] M={M:5d} r={r:3d}: ' +
                  '  '.join(f'({f}) {bo.invstd_error_f32(M, r, f, order="sequential"):.2e}' for f in 'abcd'))
    print('\n[bn calibration] invstd relative error of float32 restatements (a) raw sums, (b) two-pass, (c) about row 0, (d) about the mean of '
          'rows 0..7; k = worst channel of (a) / ((1 + r_c^2) 2^-24)')
    for (M, r), (a, b, c, d) in rows.items():
        print(f'[bn calibration] M={M:5d} r={r:3d}: (a) {a:.2e}  (b) {b:.2e}  (c) {c:.2e}  (d) {d:.2e}  k {bo.one_pass_k(M, r):.2f}')
    worst = {f: max(v[i] for v in rows.values()) for i, f in enumerate('abcd')}
    print('[bn calibration] worst ' + '  '.join(f'({f}) {v:.2e}' for f, v in worst.items()))
    for (M, r), (a, b, c, d) in rows.items():
        assert b <= bo.INVSTD_BOUND and c <= bo.INVSTD_BOUND and d <= bo.INVSTD_BOUND, (M, r, b, c, d)
    # the bound is meant to sit well above what the chosen formula costs: 4x at least
    assert worst['b'] <= bo.INVSTD_BOUND / 4 and worst['d'] <= bo.INVSTD_BOUND / 4
    for r in (30, 100):
        assert max(rows[M, r][0] for M in bo.M_SWEEP) > bo.INVSTD_BOUND, r
    # the one-pass contract k (1 + r^2) 2^-24 stays a rounding-level statement: k does not grow with r
    assert max(bo.one_pass_k(M, r) for M in bo.M_SWEEP for r in bo.R_SWEEP) < 64


def test_calibration_var_and_mean_bounds_hold_for_the_centred_formula():
    for r in bo.R_SWEEP:
        for M in bo.M_SWEEP:
            x = bo.conditioned(M, 64, r)
            ref = bo.forward(x)
            for f in 'bcd':
                mu, var, inv = bo.stats_f32(x, f)
                e_inv, e_mu, e_var = bo.stats_errors(mu, var, inv, ref)
                assert e_inv <= bo.INVSTD_BOUND and e_mu <= bo.MEAN_BOUND and e_var == 0.0, (M, r, f, e_inv, e_mu, e_var)
            if r >= 30 and M >= 19:         # raw sums: the constant channel comes out as noise, the variance bound is missed
                mu, var, inv = bo.stats_f32(x, 'a')
                assert bo.stats_errors(mu, var, inv, ref)[2] > 1.0, (M, r)


def test_survey_of_batchnorm_input_conditioning():
    """Largest |mean| / std per BatchNorm layer of the backbones whose oracle forward reports batch statistics (ECAPA, TDNN), seeded
    init, 6 x 1 s.  Prints the table of docs/bn_train.md; asserts only what the table is quoted for: the pooled BatchNorm is the ill-conditioned one."""
    from oracle import fbank as ofb
    from oracle import models as om
    w = ofb.synth_waves(6, 16000, seed=21, lowpass=0.9)
    feats = torch.from_numpy(ofb.featurize(w, method_args=dict(sr=16000, n_mels=80))).double()
    table = {}
    for name, params, fwd in (('ecapa', om.ecapa_params, om.ecapa_forward), ('tdnn', om.tdnn_params, om.tdnn_forward)):
        p = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in params(80, seed=21).items()}
        stats = {}
        with torch.no_grad():
            fwd(p, feats, training=True, stats_out=stats)
        for k, (m, v) in stats.items():
            ratio = (m.abs() / v.clamp(min=1e-30).sqrt()).flatten()
            table[name, k] = (float(ratio.max()), float(ratio.median()), int((ratio > 30).sum()), ratio.numel())
    for (name, k), (mx, med, n30, n) in table.items():
        print(f'[bn survey] {name:5s} {k:45s} max |mean|/std {mx:8.2f}  median {med:6.2f}  above 30: {n30} of {n}')
    pooled = max(v[0] for (n, k), v in table.items() if n == 'ecapa' and 'asp_bn' in k)
    convs = max(v[0] for (n, k), v in table.items() if n == 'ecapa' and 'asp_bn' not in k)
    assert pooled > 10 and convs < 10, (pooled, convs)


C_EDGES = (60, 64, 68, 124, 128, 132, 252, 256, 260, 1536)       # the sweeps of tests/test_gpu_bn_train.py
M_EDGES = (1, 15, 16, 17, 63, 64, 65, 129, 257, 4097)


def test_shape_sets_reach_the_geometry_edges():
    """The C and M of the sweeps, read against colsum4_geometry (restated in tests/bn_oracle.py): every cl_shift, a last column block that
    is not full, fewer rows than row groups, a four-row trip with a tail, and more than one chunk."""
    shifts = {bo.colsum4_geometry(4097, C // 4)[0] for C in C_EDGES}
    assert shifts == {4, 5, 6}
    assert {(C // 4 < 32, C // 4 < 64) for C in C_EDGES} == {(True, True), (False, True), (False, False)}
    assert any((C // 4) % (1 << bo.colsum4_geometry(1, C // 4)[0]) for C in C_EDGES)
    for C in (64, 128, 256):
        cl_shift, _, rpc, chunks = bo.colsum4_geometry(4097, C // 4)
        RG = 256 >> cl_shift
        assert chunks > 1 and rpc >= 4 * RG and min(M_EDGES) < RG
        assert any(M % (4 * RG) not in (0,) and M > 4 * RG for M in M_EDGES)
