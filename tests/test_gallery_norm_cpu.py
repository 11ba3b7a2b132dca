"""The host half of the search on normalised scores (docs/gallery.md, docs/score_norm.md): the helper's top-k on z against a
brute-force sort, the host-only refusals of vp_gallery_topk_norm_f32, vp_cohort_stats_split_f32 and vp_unit_rows_f32, and the grid of
the split statistics as include/vpmi.h states it.  No device is needed."""
import numpy as np
import pytest

from tests import gallery_norm_oracle as ogn


def test_topk_z_equals_a_brute_force_sort():
    ties = 0
    for seed in range(40):
        rs = np.random.RandomState(seed)
        Q, U, k = rs.randint(1, 9), rs.randint(1, 60), int(rs.choice([1, 5, 32]))
        z = rs.standard_normal((Q, U)).astype(np.float32 if seed % 2 else np.float64)
        if seed % 3 == 0:
            z = np.round(z * 2) / 2                         # a coarse grid: blocks of equal z
        z[:, rs.randint(0, U, max(1, U // 4))] = z[:, :1]   # planted ties with row 0, in every row
        idx, val = ogn.topk_z(z, k)
        assert idx.shape == val.shape == (Q, k) and val.dtype == z.dtype
        for q in range(Q):
            brute = sorted(range(U), key=lambda u: (-z[q, u], u))[:k]
            n = len(brute)
            assert idx[q, :n].tolist() == brute and (val[q, :n] == z[q, brute]).all(), (seed, q)
            assert (idx[q, n:] == -1).all() and np.isneginf(val[q, n:]).all()
            ties += int((np.diff(val[q, :n]) == 0).any())
    assert ties >= 40, ties                                 # a property of the inputs: the tie rule is exercised


def test_z_matrices_agree_on_exact_inputs():
    """On lattice rows every cosine and every statistic's sum is exact: the float32 restatement is the rounding of the definition's
    statistics, and its z is within the helper's own bound of the float64 z."""
    from tests import gallery_oracle as og
    from tests import score_norm_oracle as osn
    from tests import trial_ranks_oracle as ot
    x, _, c, _ = ot.lattice_case(5 + 40, 129, 20, 6, 5, seed=7)
    q, g = x[:5], x[5:]
    z64, bound, (qm, qs), (um, us) = ogn.z_matrix64(q, g, c, 20)
    s = og.scores(q, g)
    assert (s * 16 == np.round(s * 16)).all()
    z32 = ogn.z_matrix32(s.astype(np.float32), osn.topn_stats32(og.scores(q, c), 20), osn.topn_stats32(og.scores(g, c), 20))
    assert z32.dtype == np.float32 and (np.abs(z32 - z64) <= bound).all()


def test_entry_points_refuse_on_the_host():
    from ppvector import _native as N
    lib = N.load_library()
    cap = N.VP_COHORT_SPLIT_MAX_Q
    ws = lib.vp_cohort_stats_split_workspace_bytes
    for Q, C, D, top_n in [(0, 20, 192, 5), (10, 0, 192, 5), (10, 20, 192, 0), (10, 20, 6, 5), (10, 20, 1028, 5), (cap + 1, 20, 192, 5)]:
        if top_n:
            assert ws(Q, C, D) == 0, (Q, C, D)
        # before any pointer or context is touched
        assert lib.vp_cohort_stats_split_f32(None, None, Q, None, C, D, top_n, None, None, None, 0, None) == N.VP_EUNSUP, (Q, C, D, top_n)
    assert ws(cap, 20, 192) > 0 and ws(1, 1, 4) > 0
    assert lib.vp_cohort_stats_split_f32(None, None, 10, None, 20, 192, 5, None, None, None, 0, None) == N.VP_EINVAL
    assert lib.vp_unit_rows_f32(None, None, 0, 192, None, None) == N.VP_EUNSUP
    assert lib.vp_unit_rows_f32(None, None, 5, 6, None, None) == N.VP_EUNSUP
    assert lib.vp_unit_rows_f32(None, None, 5, 192, None, None) == N.VP_EINVAL

    wsg = lib.vp_gallery_topk_workspace_bytes

    def norm(Q, U, D, k, *ptrs):
        a = list(ptrs) + [None] * (9 - len(ptrs))           # queries, centroids, four statistics, idx, score, ws
        return lib.vp_gallery_topk_norm_f32(None, a[0], Q, a[1], U, D, k, a[2], a[3], a[4], a[5], a[6], a[7], a[8], 0, None)
    for Q, U, D, k in [(3, 10, 6, 1), (3, 10, 1028, 1), (3, 10, 192, 0), (3, 10, 192, 33), (0, 10, 192, 1), (3, 0, 192, 1)]:
        assert wsg(Q, U, D, k) == 0, (Q, U, D, k)
        assert norm(Q, U, D, k) == N.VP_EUNSUP, (Q, U, D, k)
        assert lib.vp_gallery_topk_f32(None, None, Q, None, U, D, k, None, None, None, 0, None) == N.VP_EUNSUP
    assert norm(3, 10, 192, 5) == N.VP_EINVAL


def test_split_grid_is_what_the_header_states():
    from ppvector import _native as N
    lib = N.load_library()
    slabs, cap = N.VP_COHORT_SPLIT_SLABS, N.VP_COHORT_SPLIT_MAX_RANGES
    ws = lib.vp_cohort_stats_split_workspace_bytes
    edges = [(1, 1), (128, 1), (128 * slabs, 1), (128 * slabs + 1, 2), (128 * slabs * 3, 3), (128 * slabs * cap, cap),
             (128 * slabs * cap + 1, (slabs * cap + 1 + slabs) // (slabs + 1))]
    for C, ranges in edges:
        assert ogn.split_ranges(C, slabs, cap)[1] == ranges, (C, ranges)
        for Q in (1, 32, 33, 70):
            for D in (20, 192, 1016, 1020, 1024):
                assert ws(Q, C, D) == ogn.split_workspace_bytes(Q, C, D, slabs, cap), (Q, C, D)
    # ranges enters the workspace with 640 bytes a tile: the query implies it, and it depends on neither Q nor D
    for C, ranges in edges:
        for D in (20, 1024):
            assert (ws(1, C, D) - ws(1, 1, D)) // 640 + 1 == ranges == (ws(70, C, D) - ws(70, 1, D)) // (3 * 640) + 1
