"""Score calibration (docs/calibration.md; the reference has none): the affine map llr = a s + b that turns a cosine, or the z of a
score normalisation, into a log-likelihood ratio, fitted by logistic regression over ALL (trial, enrol) pairs without the (Nt, Ne)
matrix -- the objective, its gradient and its Hessian are twelve float64 sums over the pairs, one pass of csrc/calibrate.hip per
evaluation (TrialRanks.calib_sums) -- with the cost of the LLR (Cllr) and the ranking's own floor (minCllr, a host function of the
(targets, hist) the fused trial scorer returns).  Opt-in: nothing else in the package calls it.
"""
import json
import math
import warnings

import numpy as np

LN2 = math.log(2.0)


def _logit(p):
    return math.log(p / (1.0 - p))


class Calibration:
    """llr = a s + b.  ``prior`` is the target prior the fit weighted the classes with; ``normalised`` says whether s is the z of a
    score normalisation (True) or the raw cosine: a calibration fitted on one must not be applied to the other."""

    def __init__(self, a, b, prior=0.5, normalised=False):
        self.a, self.b, self.prior, self.normalised = float(a), float(b), float(prior), bool(normalised)
        if not (math.isfinite(self.a) and math.isfinite(self.b)):
            raise ValueError(f'Calibration: a = {a}, b = {b} are not finite')
        if not 0.0 < self.prior < 1.0:
            raise ValueError(f'Calibration: prior = {prior} outside (0, 1)')

    def __repr__(self):
        return f'Calibration(a={self.a!r}, b={self.b!r}, prior={self.prior!r}, normalised={self.normalised!r})'

    def __eq__(self, other):
        return isinstance(other, Calibration) and (self.a, self.b, self.prior, self.normalised) == (other.a, other.b, other.prior,
                                                                                                 other.normalised)

    def llr(self, scores):
        """The log-likelihood ratio (natural log) of scores: float64, a float for a scalar."""
        s = np.asarray(scores, dtype=np.float64)
        out = self.a * s + self.b
        return float(out) if out.ndim == 0 else out

    def posterior(self, scores, p_target=0.5):
        """P(same speaker | score) for a target prior p_target."""
        x = np.asarray(self.llr(scores), dtype=np.float64) + _logit(p_target)
        e = np.exp(-np.abs(x))
        out = np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        return float(out) if out.ndim == 0 else out

    def threshold(self, p_target, c_miss=1, c_fa=1):
        """The Bayes threshold IN THE SCORE DOMAIN: accepting s >= threshold minimises the expected cost c_miss p_target P(miss) +
        c_fa (1 - p_target) P(false accept) when the LLRs are calibrated.  It can be handed as ``threshold=`` to the existing calls.
        (For a < 0 a larger score is weaker evidence and the comparison turns round; a fit on useful scores has a > 0.)"""
        return (math.log(c_fa * (1.0 - p_target) / (c_miss * p_target)) - self.b) / self.a

    def save(self, path):
        with open(path, 'w', encoding='utf-8') as f:
            json.dump(dict(a=self.a, b=self.b, prior=self.prior, normalised=self.normalised), f)

    @classmethod
    def load(cls, path):
        with open(path, 'r', encoding='utf-8') as f:
            d = json.load(f)
        return cls(d['a'], d['b'], d.get('prior', 0.5), d.get('normalised', False))


def cllr_from_sums(sums, NT, NN):
    """The cost of the LLR from the sums of one evaluation at (a, b) WITHOUT a prior offset: (S0_tar / NT + S0_non / NN) / (2 ln 2)."""
    sums = np.asarray(sums, dtype=np.float64).reshape(2, 6)
    return float((sums[0, 0] / NT + sums[1, 0] / NN) / (2.0 * LN2))


def objective(sums, NT, NN, prior=0.5):
    """J, its gradient (2,) and its Hessian (2, 2) in (a, b) from the twelve sums (docs/calibration.md writes them out)."""
    S = np.asarray(sums, dtype=np.float64).reshape(2, 6)
    wt, wn = prior / NT, (1.0 - prior) / NN
    J = wt * S[0, 0] + wn * S[1, 0]
    g = np.array([-wt * S[0, 2] + wn * S[1, 2], -wt * S[0, 1] + wn * S[1, 1]])
    haa, hab, hbb = wt * S[0, 5] + wn * S[1, 5], wt * S[0, 4] + wn * S[1, 4], wt * S[0, 3] + wn * S[1, 3]
    return float(J), g, np.array([[haa, hab], [hab, hbb]])


def newton_fit(sums_at, NT, NN, prior=0.5, max_iter=50):
    """Newton's method on J from (a, b) = (1, 0).  ``sums_at(a, b')`` returns the (2, 6) sums at llr + tau = a s + b'.  Step
    d = -H^-1 g, halved until J falls by 1e-4 t (-g.d); stops when -g.d / 2 < 1e-12 or after max_iter steps.
    -> (a, b, sums at (a, b + tau), iterations, evaluations, converged)."""
    tau = _logit(prior)
    a, b = 1.0, 0.0
    S = sums_at(a, b + tau)
    evaluations, iterations, converged = 1, 0, False
    while True:
        J, g, H = objective(S, NT, NN, prior)
        det = H[0, 0] * H[1, 1] - H[0, 1] * H[0, 1]
        if not (np.isfinite(S).all() and H[0, 0] > 0.0 and det > 0.0):
            break                               # separable in the limit, or nearly: no Newton step exists
        d = np.array([-(H[1, 1] * g[0] - H[0, 1] * g[1]) / det, -(H[0, 0] * g[1] - H[0, 1] * g[0]) / det])
        dec = float(-(g[0] * d[0] + g[1] * d[1]))
        if dec / 2.0 < 1e-12:
            converged = True
            break
        if iterations >= max_iter:
            break
        t, taken = 1.0, False
        while t >= 2.0 ** -40:
            na, nb = a + t * d[0], b + t * d[1]
            if not (math.isfinite(na) and math.isfinite(nb)):
                break
            nS = sums_at(na, nb + tau)
            evaluations += 1
            nJ = objective(nS, NT, NN, prior)[0]
            if nJ <= J - 1e-4 * t * dec:        # false for a NaN
                a, b, S, taken = na, nb, nS, True
                break
            t /= 2.0
        if not taken:
            break
        iterations += 1
    return a, b, S, iterations, evaluations, converged


def min_cllr_from_ranks(targets, hist):
    """The Cllr of the best monotone map of the scores, from the (targets, hist) of the fused trial scorer alone: float64, O(NT).
    The ranks define the sequence hist[0] non-targets, target 0, hist[1] non-targets, target 1, ..., hist[NT] non-targets (a
    non-target equal to a target stands before it); pool-adjacent-violators over weighted blocks, a run of non-targets being one
    block that is never expanded.  A block of y targets among w pairs has the posterior p = y / w and
    llr = logit(p) - logit(NT / (NT + NN)); blocks with p = 0 or p = 1 contribute 0."""
    hist = np.asarray(hist, dtype=np.int64).reshape(-1)
    NT = hist.shape[0] - 1
    if NT != np.asarray(targets).reshape(-1).shape[0]:
        raise ValueError(f'min_cllr_from_ranks: {hist.shape[0]} bins for {np.asarray(targets).size} targets')
    NN = int(hist.sum())
    if NT == 0 or NN == 0:
        raise ValueError('min_cllr_from_ranks: no target or no non-target pairs')
    # the non-empty bins cut the targets into runs: block k of the sequence is (bins[k] non-targets, then the targets up to the next
    # non-empty bin)
    at = np.flatnonzero(hist)
    runs = np.diff(np.concatenate((at, [NT]))).tolist()         # the targets after each non-empty bin
    nons = hist[at].tolist()
    ws, ys = [], []                                             # the stack of blocks: pairs, targets among them (exact integers)
    if at[0] > 0:
        ws.append(int(at[0]))
        ys.append(int(at[0]))                                   # the targets below every non-target
    for n, m in zip(nons, runs):
        for w, y in ((n, 0), (m, m)):
            if w == 0:
                continue
            while ws and ys[-1] * w >= y * ws[-1]:              # the block before is no lower: pool
                w += ws.pop()
                y += ys.pop()
            ws.append(w)
            ys.append(y)
    w, y = np.asarray(ws, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    mixed = (y > 0) & (y < w)
    y, n = y[mixed], (w - y)[mixed]
    odds = (y * NN) / (n * NT)                                  # exp(llr)
    cost = (y / NT) * np.log1p(1.0 / odds) + (n / NN) * np.log1p(odds)
    return float(cost.sum() / (2.0 * LN2))


def fit_calibration(enroll_features, enroll_labels, trials_features, trials_labels, prior=0.5, score_norm=None, max_iter=50):
    """Fits llr = a s + b on every (trial, enrol) pair -> (Calibration, info).  info: cllr (of the fitted LLRs), min_cllr (of the
    ranking), cllr_raw (the scores used as LLRs: a = 1, b = 0), iterations, evaluations, converged, NT, NN.  One TrialRanks serves the
    fit and min_cllr; nothing proportional to Nt Ne exists on the device or the host.  ``score_norm``: a ScoreNorm, or None for
    ppvector.get_score_norm() as evaluate_trials (None by default: raw cosines); the result records ``normalised``.  A fit that cannot
    converge (classes separable in the limit or nearly so, a non-finite sum, max_iter reached) returns the last iterate with
    converged = False and a RuntimeWarning."""
    import ppvector
    from ppvector.metric.metrics import TrialRanks, _host_labels, _label_plan
    if not 0.0 < float(prior) < 1.0:
        raise ValueError(f'fit_calibration: prior = {prior} outside (0, 1)')
    tl, el = _host_labels(trials_labels), _host_labels(enroll_labels)
    NT = _label_plan(tl, el)[4]
    NN = int(np.asarray(tl).size) * int(np.asarray(el).size) - NT
    if NT == 0 or NN == 0:
        raise ValueError(f'fit_calibration: {NT} target and {NN} non-target pairs: both classes are needed')
    if score_norm is None:
        score_norm = ppvector.get_score_norm()
    r = TrialRanks(trials_features, tl, enroll_features, el, score_norm=score_norm)
    first = []                                  # the sums of the first evaluation, at (1, tau): the raw scores' when tau = 0

    def sums_at(a, b):
        S = r.calib_sums(a, b)
        if not first:
            first.append(S)
        return S

    a, b, S, iterations, evaluations, converged = newton_fit(sums_at, NT, NN, float(prior), int(max_iter))
    if not converged:
        warnings.warn(f'fit_calibration: no convergence after {iterations} steps (a = {a}, b = {b}): the classes are separable, or '
                      'nearly so, or a sum is not finite', RuntimeWarning, stacklevel=2)
    S_raw = first[0]
    if _logit(float(prior)) != 0.0:             # cllr and cllr_raw are defined without the prior's offset: two more passes
        S_raw, S = r.calib_sums(1.0, 0.0), r.calib_sums(a, b)
        evaluations += 2
    info = dict(cllr=cllr_from_sums(S, NT, NN), min_cllr=min_cllr_from_ranks(r.targets.cpu().numpy(), r.hist.cpu().numpy()),
                cllr_raw=cllr_from_sums(S_raw, NT, NN), iterations=iterations, evaluations=evaluations, converged=converged,
                NT=NT, NN=NN)
    return Calibration(a, b, prior=prior, normalised=score_norm is not None), info
