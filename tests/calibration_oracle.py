"""Helpers of the score calibration's tests (ppvector/metric/calibration.py, csrc/calibrate.hip; docs/calibration.md is the contract),
NumPy float64 throughout and nothing imported from the package: the twelve sums by brute force over an explicit score matrix (each
sum an exactly rounded math.fsum, with the sum of the terms' magnitudes beside it for the bound), the objective with its gradient and
Hessian, the Newton fit restated, Cllr, and minCllr by expanding every non-target and running a plain pool-adjacent-violators.
"""
import math

import numpy as np

LN2 = math.log(2.0)
U = 2.0 ** -53          # the unit round-off of float64


def logit(p):
    return math.log(p / (1.0 - p))


def terms(scores, target, a, b):
    """scores (any shape; float32 values are widened exactly), target flags, llr + tau = a s + b -> (6, n) float64 terms of every pair
    in the order softplus(u), sigma(u), sigma(u) s, w, w s, w s^2, and the flattened flags.  u = -(a s + b) for a target, a s + b
    otherwise, the product and the sum each rounded on its own (as the device takes them); e = exp(-|u|)."""
    s = np.asarray(scores).astype(np.float64).reshape(-1)
    target = np.asarray(target, bool).reshape(-1)
    p = np.float64(a) * s
    y = p + np.float64(b)
    u = np.where(target, -y, y)
    e = np.exp(-np.abs(u))
    hi = 1.0 / (1.0 + e)
    lo = e * hi
    t0 = np.maximum(u, 0.0) + np.log1p(e)
    t1 = np.where(u >= 0, hi, lo)
    t3 = hi * lo
    t2 = t1 * s
    t4 = t3 * s
    t5 = t4 * s
    return np.stack([t0, t1, t2, t3, t4, t5]), target


def sums(scores, target, a, b, exact=True):
    """-> (sums (2, 6), magnitudes (2, 6), pairs (2,)): targets first; sums[c, k] the exactly rounded sum of term k over class c,
    magnitudes[c, k] the sum of |term|, pairs[c] the number of pairs of the class.  ``exact=False``: NumPy's pairwise sums instead of
    math.fsum, for timing the host path at sizes where a Python-level sum is out of the question (tools/calibration_probe.py)."""
    t, target = terms(scores, target, a, b)
    out, mag = np.zeros((2, 6)), np.zeros((2, 6))
    add = math.fsum if exact else np.sum
    for c, m in enumerate((target, ~target)):
        for k in range(6):
            out[c, k] = add(t[k, m])
            mag[c, k] = add(np.abs(t[k, m]))
    return out, mag, np.array([int(target.sum()), int((~target).sum())])


def sums_bound(mag, pairs, ulps=64):
    """|device - oracle| <= (Pc + ulps) 2^-53 sum |term|: the worst case of a float64 sum of Pc terms in any order, and `ulps` units for
    the chain of functions inside a term."""
    return (np.asarray(pairs, np.float64)[:, None] + ulps) * U * np.asarray(mag)


def objective(S, NT, NN, prior=0.5):
    """J, gradient (2,), Hessian (2, 2) in (a, b) from the sums."""
    S = np.asarray(S, np.float64).reshape(2, 6)
    wt, wn = prior / NT, (1.0 - prior) / NN
    J = wt * S[0, 0] + wn * S[1, 0]
    g = np.array([-wt * S[0, 2] + wn * S[1, 2], -wt * S[0, 1] + wn * S[1, 1]])
    H = np.array([[wt * S[0, 5] + wn * S[1, 5], wt * S[0, 4] + wn * S[1, 4]], [wt * S[0, 4] + wn * S[1, 4], wt * S[0, 3] + wn * S[1, 3]]])
    return float(J), g, H


def cllr(scores, target, a=1.0, b=0.0):
    """The cost of llr = a s + b."""
    S, _, n = sums(scores, target, a, b)
    return float((S[0, 0] / n[0] + S[1, 0] / n[1]) / (2.0 * LN2))


def fit(scores, target, prior=0.5, max_iter=50, exact=True):
    """Newton from (1, 0): d = -H^-1 g, halved until J falls by 1e-4 t (-g.d); stops at -g.d / 2 < 1e-12.
    -> (a, b, iterations, evaluations, converged)."""
    target = np.asarray(target, bool).reshape(-1)
    NT, NN = int(target.sum()), int((~target).sum())
    tau = logit(prior)
    a, b = 1.0, 0.0
    S = sums(scores, target, a, b + tau, exact)[0]
    evaluations, iterations = 1, 0
    while True:
        J, g, H = objective(S, NT, NN, prior)
        det = H[0, 0] * H[1, 1] - H[0, 1] * H[0, 1]
        if not (np.isfinite(S).all() and H[0, 0] > 0 and det > 0):
            return a, b, iterations, evaluations, False
        d = np.array([-(H[1, 1] * g[0] - H[0, 1] * g[1]) / det, -(H[0, 0] * g[1] - H[0, 1] * g[0]) / det])
        dec = float(-(g[0] * d[0] + g[1] * d[1]))
        if dec / 2.0 < 1e-12:
            return a, b, iterations, evaluations, True
        if iterations >= max_iter:
            return a, b, iterations, evaluations, False
        t = 1.0
        while True:
            if t < 2.0 ** -40:
                return a, b, iterations, evaluations, False
            na, nb = a + t * d[0], b + t * d[1]
            nS = sums(scores, target, na, nb + tau, exact)[0]
            evaluations += 1
            if objective(nS, NT, NN, prior)[0] <= J - 1e-4 * t * dec:
                a, b, S = na, nb, nS
                break
            t /= 2.0
        iterations += 1


def min_cllr_expanded(scores, target):
    """minCllr with every pair its own item: the pairs in the ranks' order (score ascending, a non-target before an equal target),
    pool-adjacent-violators on the 0 / 1 labels one item at a time, a block's llr = logit(p) - logit(NT / (NT + NN)), the Cllr of
    those; blocks with p = 0 or p = 1 cost nothing."""
    scores, target = np.asarray(scores).reshape(-1), np.asarray(target, bool).reshape(-1)
    y = target[np.lexsort((target, scores))].astype(np.int64)
    NT, NN = int(y.sum()), int((1 - y).sum())
    blocks = []                                 # [items, targets]
    for v in y.tolist():
        blocks.append([1, v])
        while len(blocks) > 1 and blocks[-2][1] * blocks[-1][0] >= blocks[-1][1] * blocks[-2][0]:
            w, t = blocks.pop()
            blocks[-1][0] += w
            blocks[-1][1] += t
    prior_logit = logit(NT / (NT + NN))
    cost_t = cost_n = 0.0
    for w, t in blocks:
        if t == 0 or t == w:
            continue
        llr = logit(t / w) - prior_logit
        cost_t += t * math.log1p(math.exp(-llr))
        cost_n += (w - t) * math.log1p(math.exp(llr))
    return (cost_t / NT + cost_n / NN) / (2.0 * LN2)
