"""Helpers of the fused trial scorer's tests (ppvector/metric/metrics.py: trial_ranks, eer_dcf_from_ranks, evaluate_trials_fused;
csrc/trial_ranks.hip): the CPU derivation of (targets, hist) from a list of scores, the oracle's EER / minDCF / threshold on the
order the fused scorer defines (score ascending, a non-target before an equal target), and the input families of the GPU tests.
"""
import numpy as np

from oracle import scoring as S

TOL = 1e-6      # absolute, on a cosine: the bound of tests/gallery_oracle.py and tests/test_gpu_kernels.py::test_cosine_scores


def scores64(trials, enroll):
    """(Nt, Ne) float64 cosines; a zero row scores 0."""
    def unit(x):
        x = np.asarray(x, np.float64)
        n = np.linalg.norm(x, axis=1, keepdims=True)
        return np.divide(x, n, out=np.zeros_like(x), where=n > 0)
    return unit(trials) @ unit(enroll).T


def is_target(trial_labels, enroll_labels):
    return np.asarray(trial_labels)[:, None] == np.asarray(enroll_labels)[None, :]


def ranks_from_scores(scores, target):
    """All scores and their target flags -> (targets ascending, hist (NT + 1) int64): hist[b] = #{non-targets s: #{t < s} == b}."""
    scores, target = np.asarray(scores).reshape(-1), np.asarray(target, bool).reshape(-1)
    t = np.sort(scores[target])
    bins = np.searchsorted(t, scores[~target], side='left')
    return t, np.bincount(bins, minlength=len(t) + 1).astype(np.int64)


def oracle_metrics(scores, target):
    """oracle.scoring's fnr_fpr / eer / min_dcf on the scores ordered by (score, non-target before target) -> (eer, min_dcf,
    score at hi).  fnr_fpr sorts its input once more with np.argsort, which may reorder equal scores; it is therefore given the
    POSITIONS in the order just established instead of the scores -- every rate depends on the order alone -- and eer() takes the
    threshold from the ordered scores."""
    scores, target = np.asarray(scores).reshape(-1), np.asarray(target, bool).reshape(-1)
    order = np.lexsort((target, scores))
    s, y = scores[order], target[order].astype(np.int64)
    fnr, fpr, _ = S.fnr_fpr(np.arange(len(s), dtype=np.float64), y)
    e, thr = S.eer(fnr, fpr, s)
    return float(e), float(S.min_dcf(fnr, fpr)), thr


def score_at(where, scores, target):
    """The score that ``where`` of eer_dcf_from_ranks names, from the full list."""
    scores, target = np.asarray(scores).reshape(-1), np.asarray(target, bool).reshape(-1)
    t = np.sort(scores[target])
    if where[0] == 't':
        return t[where[1]]
    non = scores[~target]
    inside = np.sort(non[np.searchsorted(t, non, side='left') == where[1]])
    return inside[where[2] - 1]


def _labels(rs, Nt, Ne, nspk):
    """Enrol labels uniform in [0, nspk); trial labels uniform in [0, nspk + 2): two trial speakers are never enrolled."""
    el = rs.randint(0, nspk, Ne)
    return rs.randint(0, nspk + 2, Nt), el


def lattice_case(Nt, Ne, D, nspk, moved, seed):
    """Rows of exactly 16 entries +-1 and D - 16 zeros: every length is 4, every cosine a multiple of 1/16, every product and partial
    sum a dyadic rational that f32 holds: any evaluation order gives the float64 score exactly, and scores tie across the classes.
    A speaker is such a row; an utterance is its speaker's row with ``moved`` of the 16 set to zero and ``moved`` of the then-zero
    positions set to +-1.  -> trials (Nt, D) f32, trial labels, enroll (Ne, D) f32, enrol labels."""
    rs = np.random.RandomState(seed)

    def speaker():
        r = np.zeros(D, np.float32)
        r[rs.choice(D, 16, replace=False)] = rs.choice([-1.0, 1.0], 16)
        return r

    def utterance(base):
        r = base.copy()
        r[rs.choice(np.flatnonzero(r), moved, replace=False)] = 0.0
        r[rs.choice(np.flatnonzero(r == 0), moved, replace=False)] = rs.choice([-1.0, 1.0], moved)
        return r

    tl, el = _labels(rs, Nt, Ne, nspk)
    spk = [speaker() for _ in range(nspk + 2)]
    enroll = np.stack([utterance(spk[l]) for l in el])
    trials = np.stack([utterance(spk[l]) for l in tl])
    assert ((trials != 0).sum(1) == 16).all() and ((enroll != 0).sum(1) == 16).all()
    return trials, tl, enroll, el


def band_case(Nt, Ne, D, nspk, seed):
    """Centroids: unit Gaussian rows; an embedding: 1.8 D^(-1/4) centroid + N(0, 1/D) noise, float32."""
    rs = np.random.RandomState(seed)
    cen = rs.standard_normal((nspk + 2, D))
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    tl, el = _labels(rs, Nt, Ne, nspk)

    def emb(labels):
        return (1.8 * D ** -0.25 * cen[labels] + rs.standard_normal((len(labels), D)) / np.sqrt(D)).astype(np.float32)

    return emb(tl), tl, emb(el), el


def check_band(targets, hist, s64, target, tol=TOL):
    """The acceptance of (targets, hist) against float64 scores that are no lattice: NT and the total exact, sorted targets within tol
    elementwise, and for every j  #{non-targets <= t64[j] - 2 tol} <= C[j] <= #{non-targets <= t64[j] + 2 tol}  (a counted pair has
    s <= t[j], and each side is within tol of its float64 value).  Returns the largest |target - float64|."""
    s64, target = np.asarray(s64, np.float64).reshape(-1), np.asarray(target, bool).reshape(-1)
    t64, non = np.sort(s64[target]), np.sort(s64[~target])
    assert targets.dtype == np.float32 and hist.dtype == np.int64
    assert targets.shape == t64.shape and hist.shape == (len(t64) + 1,), (targets.shape, hist.shape, t64.shape)
    assert (hist >= 0).all() and int(hist.sum()) == len(non), (int(hist.sum()), len(non))
    assert (np.diff(targets) >= 0).all(), 'targets are not ascending'
    err = np.abs(targets.astype(np.float64) - t64)
    assert (err <= tol).all(), f'target off by {err.max():.3e} at {err.argmax()}'
    C = np.cumsum(hist)[:-1]
    low = np.searchsorted(non, t64 - 2 * tol, side='right')
    high = np.searchsorted(non, t64 + 2 * tol, side='right')
    bad = np.flatnonzero((C < low) | (C > high))
    assert bad.size == 0, f'C[{bad[0]}] = {C[bad[0]]} outside [{low[bad[0]]}, {high[bad[0]]}]'
    return float(err.max()) if err.size else 0.0
