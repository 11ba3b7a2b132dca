"""The host half of the score normalisation (docs/score_norm.md): the digit-counting selection of csrc/cohort_stats.hip, emulated in
NumPy, against a full sort; the host-only refusals of the new entry points; the default of the switch.  No device is needed."""
import numpy as np
import pytest

from tests import score_norm_oracle as osn


def _score_list(seed):
    """1 .. 700 float32 scores in [-1, 1] and a top_n below, at or above their number; every other seed on a coarse grid (multiples
    of 1/8 or 1/16): dozens of exact ties, at the n-th place too."""
    rs = np.random.RandomState(seed)
    c = rs.randint(1, 701)
    s = np.clip(rs.standard_normal(c) * 0.3, -1, 1)
    if seed % 2:
        s = np.round(s * (8, 16)[seed // 2 % 2]) / (8, 16)[seed // 2 % 2]
    if seed % 5 == 0:
        s[rs.randint(0, c, max(1, c // 10))] = 0.0          # zeros among negative and positive scores
    n = (1, max(1, c // 3), c, c + 7, 300)[seed % 5]
    return s.astype(np.float32), min(n, c)


@pytest.mark.parametrize('digit_bits', [8, 7])
def test_digit_counting_selection_equals_the_full_sort(digit_bits):
    cut_ties = 0
    for seed in range(100):
        s, n = _score_list(seed)
        full = np.sort(s)[::-1][:n]
        thr, above, passes = osn.select_by_digits(s, n, digit_bits)
        assert passes == (4 if digit_bits == 8 else 5)
        # the selection orders by key, where +0.0 stands above -0.0 (np.round leaves both in the grid lists): equal as scores
        assert thr == full[-1] and above == int((osn.order_key(s) > osn.order_key(thr)).sum()), (seed, thr, full[-1], above)
        mean, std, top = osn.stats_from_selection(s, n, digit_bits)
        assert (top == full.astype(np.float64)).all(), seed                     # the same multiset: ties need no rule
        ref = osn.topn_stats32(s[None, :], n)
        if seed % 2:                                                            # grid scores: every sum is exact, the same bits
            assert mean == ref[0][0] and std == ref[1][0], (seed, mean, ref)
        else:
            assert abs(float(mean) - float(ref[0][0])) <= 1e-7 and abs(float(std) - float(ref[1][0])) <= 1e-7, seed
        cut_ties += int((s == thr).sum()) > n - int((s > thr).sum())
    # a property of the lists, not of the code: in 22 of them the n-th place cuts through a block of equal scores
    assert cut_ties >= 20, cut_ties


def test_restatement_of_r_and_z():
    std = np.asarray([0.0, 5e-7, 1e-6, 0.25], np.float32)
    r = osn.recip_std(std)
    assert r.dtype == np.float32 and r[0] == r[1] == r[2] == np.float32(1.0) / np.float32(1e-6) and r[3] == 4.0
    s = np.asarray([[0.5, -0.25]], np.float32)
    z = osn.z32(s, np.asarray([0.25, 0.0], np.float32), np.asarray([4.0, 2.0], np.float32), np.asarray([0.0], np.float32),
                np.asarray([2.0], np.float32))
    assert (z == np.asarray([[1.0, -0.5]], np.float32)).all()
    z64 = osn.z64(s, np.asarray([0.25, 0.0]), np.asarray([0.25, 0.5]), np.asarray([0.0]), np.asarray([0.5]))
    assert (z64 == z).all()


def test_entry_points_refuse_on_the_host():
    from ppvector import _native as N
    lib = N.load_library()
    ws = lib.vp_cohort_stats_workspace_bytes
    for Q, C, D, top_n in [(0, 20, 192, 5), (10, 0, 192, 5), (10, 20, 192, 0), (10, 20, 6, 5), (10, 20, 1028, 5)]:
        if top_n:
            assert ws(Q, C, D) == 0, (Q, C, D)
        # before any pointer or context is touched
        assert lib.vp_cohort_stats_f32(None, None, Q, None, C, D, top_n, None, None, None, 0, None) == N.VP_EUNSUP, (Q, C, D, top_n)
    assert ws(10, 20, 192) == 20 * 192 * 4 and ws(1, 1, 4) > 0 and ws(100000, 10000, 1024) > 0
    assert ws(10, 20, 192) == ws(100000, 20, 192)                               # the unit cohort and nothing else
    assert lib.vp_cohort_stats_f32(None, None, 10, None, 20, 192, 5, None, None, None, 0, None) == N.VP_EINVAL
    assert lib.vp_score_norm_recip_f32(None, None, 0, None, None) == N.VP_EUNSUP
    assert lib.vp_score_norm_recip_f32(None, None, 4, None, None) == N.VP_EINVAL
    assert lib.vp_score_norm_apply_f32(None, None, 0, 5, None, None, None, None, None) == N.VP_EUNSUP
    assert lib.vp_score_norm_apply_f32(None, None, 5, 5, None, None, None, None, None) == N.VP_EINVAL
    # the normalised passes refuse what the plain ones refuse
    for Nt, Ne, D, NT in [(10, 20, 190, 5), (10, 20, 1028, 5), (10, 20, 192, 0), (0, 20, 192, 5), (10, 0, 192, 5)]:
        assert lib.vp_trial_ranks_targets_norm_f32(None, None, None, None, Nt, None, None, None, Ne, D, NT, None, None, None, None,
                                                   None, None, 0, None) == N.VP_EUNSUP
        assert lib.vp_trial_ranks_counts_norm_f32(None, None, Nt, None, Ne, D, None, NT, None, None, None, None, None, None, 0,
                                                  None) == N.VP_EUNSUP
        assert lib.vp_trial_ranks_select_norm_f32(None, None, Nt, None, Ne, D, NT, 0.0, 1.0, 0, 0, None, None, None, None, None, None,
                                                  0, None) == N.VP_EUNSUP


def test_switch_defaults_to_none():
    import inspect

    import ppvector
    from ppvector.metric import metrics
    assert ppvector.get_score_norm() is None
    for fn in (metrics.evaluate_trials, metrics.evaluate_trials_fused):
        assert inspect.signature(fn).parameters['score_norm'].default is None
    assert inspect.signature(metrics.TrialRanks.__init__).parameters['score_norm'].default is None
    with pytest.raises(ValueError):
        ppvector.set_score_norm('as-norm')
    ppvector.set_score_norm(None)
    assert ppvector.get_score_norm() is None


def test_cpu_tensors_are_refused():
    from ppvector import _native as N
    from ppvector.metric.score_norm import cohort_stats
    x = np.ones((3, 8), np.float32)
    with pytest.raises(N.VpmiError):
        cohort_stats(x, x)
    from ppvector.metric.metrics import evaluate_trials
    with pytest.raises(N.VpmiError):                        # the argument is accepted; the CPU tensors are what is refused
        evaluate_trials(x, [0, 1, 2], x, [0, 1, 2], score_norm=None)
