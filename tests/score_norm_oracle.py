"""Helpers of the score normalisation's tests (ppvector/metric/score_norm.py, csrc/cohort_stats.hip, csrc/score_norm.h;
docs/score_norm.md is the contract): the float64 top-N statistics by a full sort, the float32 restatement of r and z with one NumPy
operation per line (each rounded as the device rounds it), a NumPy emulation of the kernel's digit-counting selection, and the
per-pair error bound of z.
"""
import numpy as np

from tests.trial_ranks_oracle import TOL

STD_FLOOR = np.float32(1e-6)


def topn_stats(scores, top_n):
    """scores (Q, C), float32 or float64 -> (mean, std) float64 (Q,): N = min(top_n, C), T = the N largest of a row by a full sort,
    mean = sum T / N, std = sqrt(max(sum T^2 / N - mean^2, 0)) in float64, every operation on its own."""
    s = np.asarray(scores).astype(np.float64)
    n = min(int(top_n), s.shape[1])
    top = -np.sort(-s, axis=1)[:, :n]
    s1 = top.sum(axis=1)
    s2 = (top * top).sum(axis=1)
    mean = s1 / n
    m2 = s2 / n
    mm = mean * mean
    var = m2 - mm
    return mean, np.sqrt(np.maximum(var, 0.0))


def topn_stats32(scores, top_n):
    """topn_stats, each statistic rounded once to float32: what the device returns when its sums are exact."""
    mean, std = topn_stats(scores, top_n)
    return mean.astype(np.float32), std.astype(np.float32)


def recip_std(std):
    std = np.asarray(std, np.float32)
    floored = np.maximum(std, STD_FLOOR)
    return np.float32(1.0) / floored


def z32(s, mean_e, r_e, mean_t, r_t):
    """The device's z: s (Nt, Ne) float32 cosines, enrolment statistics (Ne,), trial statistics (Nt,), all float32 -> (Nt, Ne)."""
    s = np.asarray(s, np.float32)
    mean_e, r_e = np.asarray(mean_e, np.float32)[None, :], np.asarray(r_e, np.float32)[None, :]
    mean_t, r_t = np.asarray(mean_t, np.float32)[:, None], np.asarray(r_t, np.float32)[:, None]
    de = s - mean_e
    pe = de * r_e
    dt = s - mean_t
    pt = dt * r_t
    both = pe + pt
    out = np.float32(0.5) * both
    assert out.dtype == np.float32
    return out


def z64(s, mean_e, std_e, mean_t, std_t):
    """The definition in float64 (the floor included)."""
    s = np.asarray(s, np.float64)
    pe = (s - mean_e[None, :]) / np.maximum(std_e, float(STD_FLOOR))[None, :]
    pt = (s - mean_t[:, None]) / np.maximum(std_t, float(STD_FLOOR))[:, None]
    return 0.5 * (pe + pt)


def z_bound(s, mean_e, std_e, mean_t, std_t, tol=TOL):
    """Per pair: 0.5 sum over x in {e, t} of (3 tol / sigma_x + 2 tol |s - mu_x| / sigma_x^2) + 2^-21 (|p_e| + |p_t| + 1), from the
    float64 quantities: first-order propagation of tol on s and 2 tol on each of mu and sigma, then six float32 roundings."""
    s = np.asarray(s, np.float64)
    de, dt = s - mean_e[None, :], s - mean_t[:, None]
    se, st = std_e[None, :], std_t[:, None]
    first = 0.5 * ((3 * tol / se + 2 * tol * np.abs(de) / se ** 2) + (3 * tol / st + 2 * tol * np.abs(dt) / st ** 2))
    return first + 2.0 ** -21 * (np.abs(de / se) + np.abs(dt / st) + 1.0)


def order_key(s):
    """vp_order_key (csrc/common.h): the bits of a float32 as a uint32 that orders as the float does."""
    u = np.asarray(s, np.float32).view(np.uint32)
    return np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_score(key):
    key = np.uint32(key)
    bits = key ^ np.uint32(0x80000000) if key >> 31 else ~key
    return np.asarray([bits], np.uint32).view(np.float32)[0]


def select_by_digits(scores, n, digit_bits):
    """cohort_stats_kernel's selection on one row of float32 scores: the key of the n-th largest, digit by digit from the top (a
    histogram of the digit over the scores whose key agrees with the prefix above it; the first digit, from the largest down, at which
    the count reaches the rank that is left) -> (the n-th largest score, #{scores above it}, the number of passes)."""
    keys = order_key(scores).astype(np.uint64)
    prefix, left, top, passes = 0, int(n), 32, 0
    while top > 0:
        bits = min(digit_bits, top)
        sh = top - bits
        cand = keys[(keys >> top) == (prefix >> top)] if top < 32 else keys
        hist = np.bincount(((cand >> sh) & ((1 << bits) - 1)).astype(np.int64), minlength=1 << bits)
        seen = 0
        for d in range((1 << bits) - 1, -1, -1):
            if seen + hist[d] >= left:
                break
            seen += hist[d]
        prefix |= d << sh
        left -= seen
        top = sh
        passes += 1
    return key_score(prefix), int(n) - left, passes


def stats_from_selection(scores, n, digit_bits):
    """The kernel's sums: the scores above the n-th largest, and the n-th largest n - #above times -> (mean, std) float32."""
    scores = np.asarray(scores, np.float32)
    thr, above, _ = select_by_digits(scores, n, digit_bits)
    top = np.concatenate([scores[order_key(scores) > order_key(thr)], np.full(n - above, thr, np.float32)]).astype(np.float64)
    assert top.shape == (n,)
    mean, std = topn_stats(top[None, :], n)
    return np.float32(mean[0]), np.float32(std[0]), np.sort(top)[::-1]
