"""Helpers of the tests of the search on normalised scores (csrc/gallery.hip: vp_gallery_topk_norm_f32; docs/gallery.md, "Search on
normalised scores"): the z of every (query, gallery row) pair, in float64 from the definition and as the float32 restatement of the
device's arithmetic, and the top-k of a z matrix by (z descending, row ascending).  The gallery row is the enrolment, the query the
trial.  Built from tests/gallery_oracle.py (cosines) and tests/score_norm_oracle.py (statistics, z); nothing is restated here.
"""
import numpy as np

from tests import gallery_oracle as og
from tests import score_norm_oracle as osn


def z_matrix64(queries, gallery, cohort, top_n):
    """-> (z (Q, U) float64, its per-pair bound, (mean, std) of the queries, (mean, std) of the gallery rows), all from float64
    cosines: the definition."""
    s = og.scores(queries, gallery)
    qm, qs = osn.topn_stats(og.scores(queries, cohort), top_n)
    um, us = osn.topn_stats(og.scores(gallery, cohort), top_n)
    return osn.z64(s, um, us, qm, qs), osn.z_bound(s, um, us, qm, qs), (qm, qs), (um, us)


def z_matrix32(s, qstats, ustats):
    """The device's z of exact float32 cosines s (Q, U) from float32 (mean, std) of the queries and of the gallery rows."""
    return osn.z32(s, ustats[0], osn.recip_std(ustats[1]), qstats[0], osn.recip_std(qstats[1]))


def topk_z(z, k):
    """z (Q, U) -> (idx (Q, k) int64, score (Q, k) of z's dtype) by z descending, then row ascending; past U: -1 / -inf."""
    z = np.asarray(z)
    Q, U = z.shape
    idx = np.full((Q, k), -1, np.int64)
    val = np.full((Q, k), -np.inf, z.dtype)
    for q in range(Q):
        order = np.lexsort((np.arange(U), -z[q]))[:k]
        idx[q, :len(order)] = order
        val[q, :len(order)] = z[q, order]
    return idx, val


def split_ranges(C, slabs, max_ranges, slab=128):
    """include/vpmi.h's statement of vp_cohort_stats_split_f32's grid: -> (slabs_per_wg, ranges), from C alone."""
    n = -(-C // slab)
    per = max(slabs, -(-n // max_ranges))
    return per, -(-n // per)


def split_workspace_bytes(Q, C, D, slabs, max_ranges):
    """... and of its workspace: ceil(Q / 32) (P (2^W + 2) 128 + 640 ranges), W = 8 and P = 4, or W = 7 and P = 5 for D >= 1020."""
    W, P = (7, 5) if D >= 1020 else (8, 4)
    return -(-Q // 32) * (P * (2 ** W + 2) * 128 + 640 * split_ranges(C, slabs, max_ranges)[1])
