"""The host half of the fused trial scorer: eer_dcf_from_ranks against oracle.scoring bit for bit, the label bookkeeping that places
the targets, the host-only refusals of csrc/trial_ranks.hip, and the scorer switch.  No device is needed for any of it."""
import numpy as np
import pytest

from tests import trial_ranks_oracle as ot


def _score_list(seed):
    """5 .. 400 scores, two overlapping classes with at least two members each; every other seed on a coarse grid (multiples of 1/50
    after scaling by 4, 10 or 50): dozens of exact ties, within and across the classes."""
    rs = np.random.RandomState(seed)
    n = rs.randint(5, 401)
    target = rs.uniform(size=n) < rs.uniform(0.1, 0.6)
    target[:2], target[2:4] = True, False
    scores = rs.standard_normal(n) * 0.25 + np.where(target, rs.uniform(0.1, 0.6), 0.0)
    if seed % 2:
        scores = np.round(scores * (4, 10, 50)[seed // 2 % 3]) / 50
    p = rs.permutation(n)
    return scores[p], target[p]


@pytest.mark.parametrize('block', range(6))
def test_from_ranks_equals_the_oracle_bit_for_bit(block):
    from ppvector.metric.metrics import eer_dcf_from_ranks
    tied = on_target = on_nontarget = 0
    for seed in range(40 * block, 40 * block + 40):         # 240 lists in all
        scores, target = _score_list(seed)
        t, hist = ot.ranks_from_scores(scores, target)
        eer, dcf, where = eer_dcf_from_ranks(t, hist)
        ref_eer, ref_dcf, ref_thr = ot.oracle_metrics(scores, target)
        assert eer == ref_eer and dcf == ref_dcf, (seed, eer, ref_eer, dcf, ref_dcf)
        assert ot.score_at(where, scores, target) == ref_thr, (seed, where)
        tied += int(np.isin(scores[~target], t).sum())
        on_target += where[0] == 't'
        on_nontarget += where[0] == 'n'
    assert tied >= 24 and on_target and on_nontarget, (tied, on_target, on_nontarget)     # both kinds of `hi`, cross-class ties


def test_other_costs_and_priors():
    from oracle import scoring as S
    from ppvector.metric.metrics import eer_dcf_from_ranks
    scores, target = _score_list(11)
    t, hist = ot.ranks_from_scores(scores, target)
    order = np.lexsort((target, scores))
    fnr, fpr, _ = S.fnr_fpr(np.arange(len(scores), dtype=np.float64), target[order].astype(np.int64))
    for p, cm, cf in ((0.05, 1, 1), (0.001, 10, 1), (0.5, 1, 5)):
        assert eer_dcf_from_ranks(t, hist, p, cm, cf)[1] == float(S.min_dcf(fnr, fpr, p, cm, cf))


def test_a_bin_may_hold_more_than_any_array_could():
    """Perfect separation with 3 * 10^12 non-targets below the lowest target: `hi` is the largest of them, found by bisection."""
    from ppvector.metric.metrics import eer_dcf_from_ranks
    n = 3 * 10 ** 12
    eer, dcf, where = eer_dcf_from_ranks(np.asarray([0.5, 0.6, 0.7], np.float32), np.asarray([n, 0, 0, 0]))
    assert where == ('n', 0, n) and eer == 0.0 and dcf == 0.0


def test_degenerate_inputs_raise():
    from ppvector.metric.metrics import eer_dcf_from_ranks
    with pytest.raises(ValueError):                         # no target: the reference divides by np.sum(tgt) == 0
        eer_dcf_from_ranks(np.zeros(0, np.float32), np.asarray([5]))
    with pytest.raises(ValueError):                         # no non-target
        eer_dcf_from_ranks(np.asarray([0.1, 0.2], np.float32), np.zeros(3, np.int64))
    with pytest.raises(ValueError):                         # hi == 0: the only target is the lowest score
        eer_dcf_from_ranks(np.asarray([0.5], np.float32), np.asarray([0, 3]))
    with pytest.raises(ValueError):                         # hi == 0: the only non-target is the lowest score
        eer_dcf_from_ranks(np.asarray([0.5, 0.6], np.float32), np.asarray([1, 0, 0]))
    with pytest.raises(ValueError):                         # hist is not NT + 1 long
        eer_dcf_from_ranks(np.asarray([0.5, 0.6], np.float32), np.asarray([1, 2]))


def test_label_plan_places_every_target_once():
    from ppvector.metric.metrics import _label_plan
    rs = np.random.RandomState(4)
    tl, el = rs.randint(-3, 9, 57) * 1000003, rs.randint(-3, 7, 131) * 1000003       # labels of any integer kind; some not enrolled
    t_id, e_id, off, rank, NT = _label_plan(tl, el)
    assert t_id.dtype == e_id.dtype == rank.dtype == np.int32 and off.dtype == np.int64
    same = tl[:, None] == el[None, :]
    assert ((t_id[:, None] == e_id[None, :]) == same).all() and NT == same.sum()
    places = (off[:, None] + rank[None, :])[same]
    assert sorted(places.tolist()) == list(range(NT))


def test_workspace_query_refuses_on_the_host():
    from ppvector import _native as N
    lib = N.load_library()
    ws = lib.vp_trial_ranks_workspace_bytes
    bad = [(10, 20, 190, 5), (10, 20, 1028, 5), (10, 20, 192, 0), (10, 20, 192, (1 << 24) + 1), (0, 20, 192, 5), (10, 0, 192, 5)]
    for Nt, Ne, D, NT in bad:                               # D % 4, D > 1024, NT = 0, NT > 2^24, no rows
        assert ws(Nt, Ne, D, NT) == 0, (Nt, Ne, D, NT)
        # the entry points refuse the same shapes before they touch a device (no context, no pointers)
        assert lib.vp_trial_ranks_targets_f32(None, None, None, None, Nt, None, None, None, Ne, D, NT, None, None, 0, None) == N.VP_EUNSUP
        assert lib.vp_trial_ranks_counts_f32(None, None, Nt, None, Ne, D, None, NT, None, None, 0, None) == N.VP_EUNSUP
        assert lib.vp_trial_ranks_select_f32(None, None, Nt, None, Ne, D, NT, 0.0, 1.0, 0, 0, None, None, 0, None) == N.VP_EUNSUP
    assert ws(1, 1, 4, 1) > 0 and ws(10, 20, 1024, 1 << 24) > 0
    # the unit rows of both sides and nothing else: linear in Nt + Ne, independent of NT
    assert ws(100000, 10000, 192, 300000) == ws(100000, 10000, 192, 1) <= (110000 * 192 * 4) + 512
    assert ws(200, 100, 192, 7) > ws(100, 100, 192, 7)


def test_scorer_switch():
    import ppvector
    assert ppvector.get_trial_scorer() == 'matrix'
    try:
        ppvector.set_trial_scorer('fused')
        assert ppvector.get_trial_scorer() == 'fused'
        ppvector.set_trial_scorer('matrix')
        for bad in ('gpu', 'Fused', '', None):
            with pytest.raises(ValueError):
                ppvector.set_trial_scorer(bad)
        assert ppvector.get_trial_scorer() == 'matrix'
    finally:
        ppvector.set_trial_scorer('matrix')


def test_fused_scorer_refuses_cpu_tensors():
    from ppvector import _native as N
    from ppvector.metric.metrics import trial_ranks
    x = np.ones((3, 8), np.float32)
    with pytest.raises(N.VpmiError):
        trial_ranks(x, [0, 1, 2], x, [0, 1, 2])
