"""float64 oracle of the 1:N speaker search (ppvector/infer_utils/gallery.py, csrc/gallery.hip) and its acceptance criterion.

The reference (ppvector/predict.py:154-187): ``audio_feature_mean`` = the mean embedding of every user, ``__retrieval`` = sklearn's
``cosine_similarity`` of the query against all of them, ``argmax``, ``>= threshold``.
"""
import numpy as np

TOL = 1e-6      # absolute, on a cosine: an f32 fma chain over unit vectors errs by <= ~1.5e-7 sum|a_i b_i| <= 1.5e-7, the two
#                 normalisations add a few ulp each; tests/test_gpu_kernels.py::test_cosine_scores holds vp_cosine_scores_f32 to the same


def _unit(x):
    x = np.asarray(x, np.float64)
    n = np.linalg.norm(x, axis=-1, keepdims=True)
    return np.divide(x, n, out=np.zeros_like(x), where=n > 0)


def centroids(features, names):
    """-> (users in order of first appearance, (U, D) float64 unit means of their rows; a zero mean gives a zero row)."""
    features = np.asarray(features, np.float64)
    users = list(dict.fromkeys(names))
    means = np.stack([features[[i for i, n in enumerate(names) if n == u]].mean(axis=0) for u in users])
    return users, _unit(means)


def scores(queries, cen):
    """(Q, U) float64 cosines; a zero query or a zero centroid scores 0."""
    return _unit(queries) @ _unit(cen).T


def topk(queries, cen, k):
    """-> (idx (Q, k) int64, score (Q, k) float64) by score descending, then index ascending; past U: -1 / -inf."""
    s = scores(queries, cen)
    Q, U = s.shape
    idx = np.full((Q, k), -1, np.int64)
    val = np.full((Q, k), -np.inf)
    for q in range(Q):
        order = np.lexsort((np.arange(U), -s[q]))[:k]
        idx[q, :len(order)] = order
        val[q, :len(order)] = s[q, order]
    return idx, val


def check_topk(idx, score, scores64, k, tol=TOL):
    """Raises AssertionError unless (idx, score) (Q, k) is an acceptable top-k of the float64 scores (Q, U).  No exclusions:
      * shape, and the tail past min(k, U) is -1 / -inf (and only the tail);
      * every returned score is within tol of the float64 score of the returned index;
      * each row is ordered by (returned) score descending, then index ascending;
      * no index appears twice;
      * every row NOT returned has a float64 score <= the returned k-th score + 2 tol.
    Returns the largest |returned score - float64 score|."""
    idx, score, scores64 = np.asarray(idx), np.asarray(score), np.asarray(scores64, np.float64)
    Q, U = scores64.shape
    assert idx.shape == (Q, k) and score.shape == (Q, k), (idx.shape, score.shape, (Q, k))
    n = min(k, U)
    worst = 0.0
    for q in range(Q):
        assert (idx[q, n:] == -1).all() and np.isneginf(score[q, n:]).all(), f'query {q}: tail past U is not -1 / -inf'
        ri, rs = idx[q, :n].astype(np.int64), score[q, :n].astype(np.float64)
        assert ((ri >= 0) & (ri < U)).all(), f'query {q}: index out of range {ri}'
        err = np.abs(rs - scores64[q, ri])
        assert (err <= tol).all(), f'query {q}: score off by {err.max():.3e} at index {ri[err.argmax()]}'
        worst = max(worst, float(err.max()) if n else 0.0)
        for a in range(n - 1):
            assert rs[a] > rs[a + 1] or (rs[a] == rs[a + 1] and ri[a] < ri[a + 1]), \
                f'query {q}: positions {a}, {a + 1} out of order: ({rs[a]!r}, {ri[a]}), ({rs[a + 1]!r}, {ri[a + 1]})'
        assert len(set(ri.tolist())) == n, f'query {q}: an index appears twice: {ri}'
        if n < U:
            rest = np.ones(U, bool)
            rest[ri] = False
            over = scores64[q, rest].max() - rs[n - 1]
            assert over <= 2 * tol, f'query {q}: a row that was not returned beats the k-th score by {over:.3e}'
    return worst
