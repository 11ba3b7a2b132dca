"""The float64 oracle of the 1:N speaker search and its acceptance criterion, tested on their own, and the host-only refusals of
vp_gallery_topk_f32 (no device is needed for any of it)."""
import numpy as np
import pytest

from tests import gallery_oracle as og


def _library(seed=0, users=7, D=24):
    rs = np.random.RandomState(seed)
    counts = rs.randint(1, 4, users)
    names = [f'u{u}' for u, c in enumerate(counts) for _ in range(c)]
    order = rs.permutation(len(names))
    names = [names[i] for i in order]
    feats = rs.standard_normal((len(names), D))
    queries = rs.standard_normal((5, D))
    return names, feats, queries


def test_k1_is_the_reference_retrieval():
    """predict.py:154-187 restated literally: per-user mean, normalise, cosine, argmax, >= threshold."""
    names, feats, queries = _library()
    users, cen = og.centroids(feats, names)
    idx, val = og.topk(queries, cen, 1)
    threshold = 0.1
    for q, x in enumerate(queries):
        means = np.stack([np.mean([feats[i] for i, n in enumerate(names) if n == u], axis=0) for u in users])
        a = x / np.linalg.norm(x)
        b = means / np.linalg.norm(means, axis=1, keepdims=True)
        sim = b @ a                                       # cosine_similarity(features, feature)
        best = int(np.argmax(sim))
        assert idx[q, 0] == best
        assert abs(val[q, 0] - sim[best]) < 1e-14
        assert (val[q, 0] >= threshold) == (sim[best] >= threshold)
    assert users == list(dict.fromkeys(names))


def test_topk_order_ties_and_tail():
    cen = np.eye(4)[[0, 1, 1, 2]]                         # rows 1 and 2 are equal
    idx, val = og.topk(np.asarray([[0.0, 1.0, 0.0, 0.0]]), cen, 6)
    assert idx[0].tolist() == [1, 2, 0, 3, -1, -1]
    assert val[0, :4].tolist() == [1.0, 1.0, 0.0, 0.0] and np.isneginf(val[0, 4:]).all()
    idx, val = og.topk(np.zeros((1, 4)), cen, 2)          # a zero query scores 0 against everything
    assert idx[0].tolist() == [0, 1] and val[0].tolist() == [0.0, 0.0]


@pytest.fixture(scope='module')
def good():
    rs = np.random.RandomState(3)
    s = rs.uniform(-1, 1, (3, 40))
    k = 5
    idx = np.stack([np.lexsort((np.arange(40), -r))[:k] for r in s])
    val = np.take_along_axis(s, idx, 1)
    return s, k, idx.astype(np.int32), val.astype(np.float64)


def test_check_topk_accepts_the_exact_answer(good):
    s, k, idx, val = good
    assert og.check_topk(idx, val, s, k) == 0.0


def test_check_topk_rejects_a_wrong_index(good):
    s, k, idx, val = good
    idx = idx.copy()
    worst = int(np.argmin(s[1]))
    idx[1, 2] = worst                                     # its float64 score is far from the score returned with it
    with pytest.raises(AssertionError, match='score off'):
        og.check_topk(idx, val, s, k)


def test_check_topk_rejects_a_dropped_better_row(good):
    s, k, idx, val = good
    order = np.lexsort((np.arange(40), -s[0]))
    idx, val = idx.copy(), val.copy()
    idx[0] = order[1:k + 1]                               # the best row is missing; everything returned is consistent
    val[0] = s[0, idx[0]]
    with pytest.raises(AssertionError, match='not returned'):
        og.check_topk(idx, val, s, k)


def test_check_topk_rejects_an_unsorted_list(good):
    s, k, idx, val = good
    idx, val = idx.copy(), val.copy()
    idx[2, [0, 3]] = idx[2, [3, 0]]
    val[2, [0, 3]] = val[2, [3, 0]]
    with pytest.raises(AssertionError, match='out of order'):
        og.check_topk(idx, val, s, k)


def test_check_topk_rejects_a_repeated_index():
    s = np.asarray([[0.5, 0.5, 0.1, 0.0]])
    idx = np.asarray([[0, 0]], np.int32)                  # sorted as far as the scores go, scores right: only the repeat is wrong
    val = np.asarray([[0.5, 0.5]])
    with pytest.raises(AssertionError):
        og.check_topk(idx, val, s, 2)
    idx = np.asarray([[1, 0]], np.int32)                  # the tie in the wrong index order
    with pytest.raises(AssertionError, match='out of order'):
        og.check_topk(idx, val, s, 2)


def test_check_topk_accepts_a_swap_closer_than_tol():
    s = np.asarray([[0.9, 0.5 + 4e-7, 0.5, 0.1]])
    # an f32 search may see rows 1 and 2 the other way round: returned scores descending, each within tol of its float64 score
    idx = np.asarray([[0, 2, 1]], np.int32)
    val = np.asarray([[0.9, 0.5 + 3e-7, 0.5 + 1e-7]])
    assert og.check_topk(idx, val, s, 3) <= og.TOL
    # ... and may return row 2 instead of row 1 at the cut
    assert og.check_topk(idx[:, :2], val[:, :2], s, 2) <= og.TOL
    with pytest.raises(AssertionError):                   # but not a row 1e-5 worse
        og.check_topk(np.asarray([[0, 2]], np.int32), np.asarray([[0.9, 0.5]]), np.asarray([[0.9, 0.5 + 1e-5, 0.5, 0.1]]), 2)


def test_check_topk_wants_the_tail_past_U():
    s = np.asarray([[0.3, 0.7]])
    ok_i, ok_s = np.asarray([[1, 0, -1]], np.int32), np.asarray([[0.7, 0.3, -np.inf]])
    assert og.check_topk(ok_i, ok_s, s, 3) == 0.0
    with pytest.raises(AssertionError, match='tail'):
        og.check_topk(np.asarray([[1, 0, 0]], np.int32), np.asarray([[0.7, 0.3, 0.3]]), s, 3)


def test_workspace_query_refuses_on_the_host():
    """vp_gallery_topk_workspace_bytes is a host-only call: 0 for every unsupported shape, positive and growing with Q otherwise."""
    from ppvector import _native as N
    lib = N.load_library()
    ws = lib.vp_gallery_topk_workspace_bytes
    assert ws(1, 1000, 190, 1) == 0                       # D % 4 != 0
    assert ws(1, 1000, 1028, 1) == 0                      # D > 1024
    assert ws(1, 1000, 192, 0) == 0                       # k = 0
    assert ws(1, 1000, 192, 33) == 0                      # k = 33
    assert ws(1, (1 << 31) // 192 + 1, 192, 1) == 0       # U D >= 2^31
    assert ws(1, 1 << 21, 1024, 1) == 0                   # U D == 2^31
    assert ws(1, (1 << 21) - 1, 1024, 32) > 0
    sizes = [ws(Q, 100000, 192, 10) for Q in (1, 32, 33, 256)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert ws(1, 1, 4, 1) > 0 and ws(1, 1000, 1024, 32) > 0
    # the entry point refuses the same shapes before it touches a device (no context, no pointers)
    assert lib.vp_gallery_topk_f32(None, None, 1, None, 1000, 190, 1, None, None, None, 0, None) == N.VP_EUNSUP
    assert lib.vp_gallery_topk_f32(None, None, 1, None, 1000, 192, 33, None, None, None, 0, None) == N.VP_EUNSUP
    assert N.VP_GALLERY_SLAB == 128
