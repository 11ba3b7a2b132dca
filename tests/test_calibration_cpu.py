"""The host half of the score calibration (ppvector/metric/calibration.py; docs/calibration.md): the oracle's gradient and Hessian
against finite differences of its own objective, the package's Newton fit against the oracle's restatement, min_cllr_from_ranks
against a pool-adjacent-violators over every single pair, the Calibration object, and the refusals that need no device."""
import json
import math
import warnings

import numpy as np
import pytest

from tests import calibration_oracle as oc
from tests import trial_ranks_oracle as ot


def _score_list(seed, grid=None):
    """40 .. 400 scores in (-1, 1), two overlapping classes (targets higher on average) with at least two members each; ``grid``:
    rounded to multiples of 1 / grid, which ties scores within and across the classes."""
    rs = np.random.RandomState(seed)
    n = rs.randint(40, 401)
    target = rs.uniform(size=n) < rs.uniform(0.1, 0.5)
    target[:2], target[2:4] = True, False
    scores = np.clip(rs.standard_normal(n) * 0.15 + np.where(target, rs.uniform(0.15, 0.5), 0.0), -0.99, 0.99)
    if grid:
        scores = np.round(scores * grid) / grid
    p = rs.permutation(n)
    return scores[p], target[p]


# ------------------------------------------------------------------------------------------------ the oracle's own derivatives
@pytest.mark.parametrize('prior', [0.5, 0.2])
@pytest.mark.parametrize('a,b', [(1.0, 0.0), (9.3, -3.5), (-4.0, 2.0), (20.0, -4.0)])
def test_oracle_gradient_and_hessian_against_central_differences(a, b, prior):
    """Central differences with step h: (f(x + h) - f(x - h)) / 2h = f'(x) + h^2 f'''(xi) / 6.  J is a convex combination (the class
    weights P / NT and (1 - P) / NN add up to 1 over the pairs) of softplus(+-(a s + b)) with |s| <= 1, so every third and fourth
    partial derivative of J is bounded by max |softplus'''| = max |sigma''| = 1 / (6 sqrt 3) < 1/8 and max |sigma'''| = 1/8: the
    truncation is at most h^2 / 48.  Each J, and each gradient entry, is an exactly rounded sum of terms good to a few ulps, below
    64 ulps of max(1, J) in all: the quotient adds 64 * 2^-53 max(1, J) / h.  h = 1e-4 balances the two: 2.1e-10 + 0.7e-10 max(1, J)."""
    h = 1e-4
    scores, target = _score_list(3)
    NT, NN = int(target.sum()), int((~target).sum())
    tau = oc.logit(prior)

    def at(x, y):
        return oc.objective(oc.sums(scores, target, x, y + tau)[0], NT, NN, prior)

    J, g, H = at(a, b)
    tol = h * h / 48 + 64 * oc.U * max(1.0, J) / h
    fd_g = np.array([(at(a + h, b)[0] - at(a - h, b)[0]) / (2 * h), (at(a, b + h)[0] - at(a, b - h)[0]) / (2 * h)])
    fd_H = np.array([(at(a + h, b)[1] - at(a - h, b)[1]) / (2 * h), (at(a, b + h)[1] - at(a, b - h)[1]) / (2 * h)])
    print(f'[calibration fd a={a} b={b} P={prior}] J {J:.6f} |g - fd| {np.abs(g - fd_g).max():.2e} |H - fd| {np.abs(H - fd_H).max():.2e} '
          f'(bound {tol:.2e})')
    assert np.abs(g - fd_g).max() <= tol and np.abs(H - fd_H).max() <= tol
    assert H[0, 1] == H[1, 0] and H[0, 0] > 0 and np.linalg.det(H) > 0


def test_package_objective_and_fit_equal_the_oracle():
    """ppvector's objective and Newton loop, fed the oracle's sums: the restatement in tests/calibration_oracle.py takes the same
    steps, so the iterates agree bit for bit; Cllr of the fit is below the raw scores' and above minCllr."""
    from ppvector.metric import calibration as C
    for seed, prior in ((1, 0.5), (2, 0.5), (5, 0.1), (8, 0.5)):
        scores, target = _score_list(seed, grid=50 if seed % 2 else None)
        NT, NN = int(target.sum()), int((~target).sum())
        S = oc.sums(scores, target, 2.5, -0.75)[0]
        J, g, H = C.objective(S, NT, NN, prior)
        rJ, rg, rH = oc.objective(S, NT, NN, prior)
        assert J == rJ and (g == rg).all() and (H == rH).all()
        a, b, S_fit, iterations, evaluations, converged = C.newton_fit(lambda x, y: oc.sums(scores, target, x, y)[0], NT, NN, prior)
        assert (a, b, iterations, evaluations, converged) == oc.fit(scores, target, prior)
        assert converged and 1 <= iterations <= 50 and evaluations >= iterations + 1
        assert np.abs(C.objective(S_fit, NT, NN, prior)[1]).max() < 1e-5         # a stationary point
        t, hist = ot.ranks_from_scores(scores, target)
        fitted, raw, floor = oc.cllr(scores, target, a, b), oc.cllr(scores, target), C.min_cllr_from_ranks(t, hist)
        assert C.cllr_from_sums(oc.sums(scores, target, a, b)[0], NT, NN) == fitted
        print(f'[calibration fit seed {seed} P={prior}] a {a:.4f} b {b:.4f} in {iterations} steps, {evaluations} evaluations; '
              f'Cllr raw {raw:.4f} fitted {fitted:.4f} min {floor:.4f}')
        assert floor <= fitted and (prior != 0.5 or fitted <= raw)


def test_fit_ends_on_separable_classes_and_reports_the_cap():
    from ppvector.metric import calibration as C
    # separable: J has no minimiser (a grows, J falls towards 0); the loop still ends, at a finite iterate, as the oracle's does
    scores = np.array([-0.5, -0.25, 0.0, 0.5, 0.75])
    target = np.array([False, False, False, True, True])
    with warnings.catch_warnings():
        warnings.simplefilter('error')                      # newton_fit itself does not warn: fit_calibration does
        a, b, S, iterations, evaluations, converged = C.newton_fit(lambda x, y: oc.sums(scores, target, x, y)[0], 2, 3)
    assert iterations <= 50 and math.isfinite(a) and math.isfinite(b) and a > 10
    assert (a, b, iterations, evaluations, converged) == oc.fit(scores, target)
    assert C.objective(S, 2, 3)[0] < 1e-6
    # the cap: two steps are not enough on overlapping classes
    scores, target = _score_list(1)
    NT, NN = int(target.sum()), int((~target).sum())
    a, b, _, iterations, _, converged = C.newton_fit(lambda x, y: oc.sums(scores, target, x, y)[0], NT, NN, max_iter=2)
    assert not converged and iterations == 2 and (a, b) != (1.0, 0.0)
    assert oc.fit(scores, target, max_iter=2)[:3] == (a, b, 2) and oc.fit(scores, target, max_iter=2)[4] is False


# ------------------------------------------------------------------------------------------------ minCllr
@pytest.mark.parametrize('grid', [None, 50, 10, 4])
def test_min_cllr_from_ranks_equals_the_expanded_pav(grid):
    """grid = None: no ties; 50, 10, 4: dozens of ties, between a target and a non-target among them."""
    from ppvector.metric.calibration import min_cllr_from_ranks
    tied = empty = 0
    for seed in range(30):
        scores, target = _score_list(seed, grid)
        t, hist = ot.ranks_from_scores(scores, target)
        got, want = min_cllr_from_ranks(t, hist), oc.min_cllr_expanded(scores, target)
        assert abs(got - want) <= 1e-12 * want, (seed, got, want)
        assert 0.0 <= got < 1.0                     # 0: a coarse grid can leave nothing but ties, which the rule separates
        tied += int(np.isin(scores[~target], t).sum())
        empty += int((hist == 0).sum())
    assert empty > 0 and (grid is None) == (tied == 0), (tied, empty)


def test_min_cllr_edge_cases():
    from ppvector.metric.calibration import min_cllr_from_ranks
    # every non-target in bin 0: separable, the floor is exactly 0 -- also with a non-target EQUAL to the lowest target (the ranks'
    # tie rule puts it before the target)
    for scores, target in (([0.1, 0.2, 0.3, 0.5, 0.6], [0, 0, 0, 1, 1]), ([0.1, 0.5, 0.5, 0.6], [0, 0, 1, 1])):
        t, hist = ot.ranks_from_scores(np.asarray(scores), np.asarray(target, bool))
        assert hist[0] == hist.sum() and min_cllr_from_ranks(t, hist) == 0.0 == oc.min_cllr_expanded(scores, np.asarray(target, bool))
    # NT = 1, inside, below and above the non-targets
    for s_t in (0.35, -1.0, 1.0):
        scores, target = np.array([0.1, 0.2, 0.3, 0.4, 0.5, s_t]), np.array([0, 0, 0, 0, 0, 1], bool)
        t, hist = ot.ranks_from_scores(scores, target)
        got, want = min_cllr_from_ranks(t, hist), oc.min_cllr_expanded(scores, target)
        assert len(t) == 1 and abs(got - want) <= 1e-12 * want, (s_t, got, want)
    # every target below every non-target: one block, p = the prior, llr = 0: exactly one bit
    t, hist = ot.ranks_from_scores(np.array([0.1, 0.2, 0.7, 0.8, 0.9]), np.array([1, 1, 0, 0, 0], bool))
    assert min_cllr_from_ranks(t, hist) == pytest.approx(1.0, abs=1e-15)
    # counts no array could hold: the runs are never expanded
    big = min_cllr_from_ranks(np.array([0.5, 0.6], np.float32), np.array([3 * 10 ** 12, 10 ** 12, 0]))
    small = min_cllr_from_ranks(np.array([0.5, 0.6], np.float32), np.array([3, 1, 0]))
    assert 0.0 < big < 1.0 and 0.0 < small < 1.0
    with pytest.raises(ValueError):
        min_cllr_from_ranks(np.zeros(0, np.float32), np.array([5]))
    with pytest.raises(ValueError):
        min_cllr_from_ranks(np.array([0.5], np.float32), np.array([0, 0]))
    with pytest.raises(ValueError):
        min_cllr_from_ranks(np.array([0.5, 0.6], np.float32), np.array([1, 2]))


# ------------------------------------------------------------------------------------------------ Calibration
def test_calibration_threshold_inverts_posterior_at_the_bayes_point(tmp_path):
    from ppvector.metric.calibration import Calibration
    for a, b in ((9.3, -3.5), (0.37, 0.0125), (-4.0, 2.0)):
        cal = Calibration(a, b)
        for p, cm, cf in ((0.5, 1, 1), (0.01, 1, 1), (0.001, 10, 1), (0.3, 1, 5)):
            thr = cal.threshold(p, cm, cf)
            # at the Bayes point the two expected costs are equal: c_miss P(tar | s) = c_fa (1 - P(tar | s))
            assert cal.posterior(thr, p) == pytest.approx(cf / (cf + cm), rel=1e-12)
            assert cal.llr(thr) == pytest.approx(math.log(cf * (1 - p) / (cm * p)), rel=1e-12, abs=1e-12)
        s = np.array([-0.5, 0.0, 0.25, 1.0])
        assert (cal.llr(s) == a * s + b).all() and cal.llr(0.25) == a * 0.25 + b and isinstance(cal.llr(0.25), float)
        post = cal.posterior(s, 0.1)
        assert ((post > 0) & (post < 1)).all() and (np.diff(post) * a > 0).all()
        assert cal.posterior(1e6 if a > 0 else -1e6) == 1.0 and cal.posterior(-1e6 if a > 0 else 1e6) == 0.0    # no overflow
    with pytest.raises(ValueError):
        Calibration(float('nan'), 0.0)
    with pytest.raises(ValueError):
        Calibration(1.0, 0.0, prior=1.0)


def test_calibration_save_load_round_trips_the_bits(tmp_path):
    from ppvector.metric.calibration import Calibration
    cal = Calibration(146.0 / 3.0, -59.0 / 7.0, prior=0.1 + 0.2, normalised=True)
    path = str(tmp_path / 'cal.json')
    cal.save(path)
    back = Calibration.load(path)
    assert (back.a, back.b, back.prior, back.normalised) == (cal.a, cal.b, cal.prior, True) and back == cal
    assert np.float64(back.a).tobytes() == np.float64(cal.a).tobytes() and np.float64(back.b).tobytes() == np.float64(cal.b).tobytes()
    assert sorted(json.load(open(path))) == ['a', 'b', 'normalised', 'prior']            # these numbers and nothing else


# ------------------------------------------------------------------------------------------------ no device needed
def test_entry_points_refuse_on_the_host():
    from ppvector import _native as N
    lib = N.load_library()
    need = lib.vp_trial_calib_partials_bytes
    for Nt, Ne, D in ((10, 20, 190), (10, 20, 1028), (0, 20, 192), (10, 0, 192), (10, 20, 0)):     # D % 4, D > 1024, no rows
        assert need(Nt, Ne, D) == 0, (Nt, Ne, D)
        assert lib.vp_trial_ranks_workspace_bytes(Nt, Ne, D, 1) == 0
        # before anything touches a device: no context, no pointers
        assert lib.vp_trial_calib_sums_f32(None, None, Nt, None, Ne, D, None, None, None, 0, None, 0, None) == N.VP_EUNSUP
        assert lib.vp_trial_calib_sums_norm_f32(None, None, Nt, None, Ne, D, None, None, None, 0, None, None, None, None, None, 0,
                                                None) == N.VP_EUNSUP
    # 96 bytes per workgroup: one for (1, 2); three trial tiles times two row ranges for (65, 257)
    assert need(1, 2, 16) == 96 and need(65, 257, 192) == 6 * 96 and need(65, 257, 1024) == 6 * 96
    assert need(16384, 16384, 192) <= 96 * 2048
    # a supported shape with nothing behind it is refused as well, and still without a device
    assert lib.vp_trial_calib_sums_f32(None, None, 10, None, 20, 192, None, None, None, 0, None, 0, None) == N.VP_EINVAL


def test_fit_calibration_error_paths():
    from ppvector import _native as N
    from ppvector.metric.calibration import fit_calibration
    x = np.ones((3, 8), np.float32)
    with pytest.raises(ValueError):                         # NT = 0: no trial speaker is enrolled
        fit_calibration(x, [0, 1, 2], x, [3, 4, 5])
    with pytest.raises(ValueError):                         # NN = 0: one speaker
        fit_calibration(x, [7, 7, 7], x, [7, 7, 7])
    with pytest.raises(ValueError):
        fit_calibration(x, [0, 1, 2], x, [0, 1, 2], prior=0.0)
    with pytest.raises(N.VpmiError):                        # host tensors: the engine has no CPU fallback
        fit_calibration(x, [0, 1, 2], x, [0, 1, 2])
