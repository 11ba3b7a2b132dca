"""The fused trial scorer on the GPU (csrc/trial_ranks.hip, ppvector/metric/metrics.py) against the CPU derivation and oracle.scoring
(tests/trial_ranks_oracle.py).  Shapes are the smallest at which the kernels can go wrong: every edge of the 32-trial tile, the
32-row wave tile and the 128-row slab, more than one workgroup both ways, D with and without a tail of four, the largest LDS request
(D = 1024), both searches (all targets in LDS; pivots in LDS and the rest in global memory) and counts on both sides of the LDS
window.  No case has more than 65 x 384 pairs."""
import numpy as np
import pytest
import torch

from tests import trial_ranks_oracle as ot

pytestmark = pytest.mark.gpu

TOL = ot.TOL


@pytest.fixture(scope='module')
def M():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: these tests must run on an MI355X (no CPU fallback exists)')
    from ppvector.metric import metrics
    return metrics


def _ranks(M, trials, tl, enroll, el, **kw):
    r = M.TrialRanks(torch.as_tensor(trials).cuda(), tl, torch.as_tensor(enroll).cuda(), el, **kw)
    return r, r.targets.cpu().numpy(), r.hist.cpu().numpy()


def _same_bits(a, b):
    return a[0].shape == b[0].shape and (a[0].view(np.int32) == b[0].view(np.int32)).all() and (a[1] == b[1]).all()


# ------------------------------------------------------------------------------------------------ exact family
LATTICE = [     # (Nt, Ne, D, nspk, moved), seed 7
    (33, 129, 32, 6, 5),
    (31, 128, 64, 5, 8),
    (65, 257, 192, 12, 5),          # all but a few non-targets in ONE bin: the selection may not collect a bin
    (65, 257, 192, 12, 8),
    (32, 384, 1024, 20, 8),
    (1, 130, 20, 3, 5),
    (65, 384, 1024, 1, 12),         # NT = 9 600 beside the largest tile: pivots in LDS, the rest of the search in global memory, and
    #                                 bins past the LDS window (6 528 bins at D = 1024) that count straight into global memory
]


@pytest.mark.parametrize('Nt,Ne,D,nspk,moved', LATTICE)
def test_lattice_inputs_are_exact(M, Nt, Ne, D, nspk, moved):
    trials, tl, enroll, el = ot.lattice_case(Nt, Ne, D, nspk, moved, seed=7)
    target = ot.is_target(tl, el)
    s = ot.scores64(trials, enroll)
    assert (s * 16 == np.round(s * 16)).all()               # every cosine is a multiple of 1/16: float32 holds it exactly
    s = s.astype(np.float32)
    t_ref, h_ref = ot.ranks_from_scores(s, target)
    assert len(t_ref) >= 1
    r, targets, hist = _ranks(M, trials, tl, enroll, el)
    assert targets.dtype == np.float32 and hist.dtype == np.int64
    assert targets.shape == t_ref.shape and (targets == t_ref).all()
    assert hist.shape == h_ref.shape and (hist == h_ref).all()
    ties = np.intersect1d(t_ref, s[~target]).size
    ref = ot.oracle_metrics(s, target)
    eer, dcf, where = M.eer_dcf_from_ranks(targets, hist)
    got = M.evaluate_trials_fused(torch.as_tensor(enroll).cuda(), el, torch.as_tensor(trials).cuda(), tl)
    print(f'[trial ranks lattice {(Nt, Ne, D, nspk, moved)}] NT {len(t_ref)} NN {int(h_ref.sum())} EER {ref[0]:.4f} hi at {where} '
          f'of {int(h_ref[where[1]])}; {ties} score levels shared by targets and non-targets')
    assert got == (ref[0], ref[1], float(ref[2])), (got, ref)
    assert (eer, dcf) == ref[:2]
    # the k-th non-target of the fullest bin (first, middle, last) and of the last non-empty bin, against the full list
    non = s[~target]
    bins = np.searchsorted(t_ref, non, side='left')
    for b in {int(np.argmax(h_ref)), int(np.flatnonzero(h_ref)[-1])}:
        inside = np.sort(non[bins == b])
        for k in sorted({1, (len(inside) + 1) // 2, len(inside)}):
            assert r.kth_nontarget(b, k) == inside[k - 1], (b, k)
    with pytest.raises(ValueError):
        r.kth_nontarget(int(np.argmax(h_ref)), int(h_ref.max()) + 1)


# ------------------------------------------------------------------------------------------------ band family
@pytest.fixture(scope='module')
def band():
    """(97, 640, 192, 40): shared by the property tests; never modified."""
    trials, tl, enroll, el = ot.band_case(97, 640, 192, 40, seed=7)
    return trials, tl, enroll, el, ot.scores64(trials, enroll), ot.is_target(tl, el)


def test_band_small(M):
    trials, tl, enroll, el = ot.band_case(70, 300, 20, 25, seed=7)
    _, targets, hist = _ranks(M, trials, tl, enroll, el)
    worst = ot.check_band(targets, hist, ot.scores64(trials, enroll), ot.is_target(tl, el))
    print(f'[trial ranks band (70, 300, 20, 25)] NT {len(targets)} largest |target - float64| {worst:.3e}')


def test_band(M, band):
    trials, tl, enroll, el, s64, target = band
    r, targets, hist = _ranks(M, trials, tl, enroll, el)
    worst = ot.check_band(targets, hist, s64, target)
    print(f'[trial ranks band (97, 640, 192, 40)] NT {len(targets)} largest |target - float64| {worst:.3e}')
    # the selection inside a bin: k-th smallest, in order, inside (t[b-1], t[b]].  The bins cut the non-targets in ascending order,
    # so it is the (hist[0] + ... + hist[b-1] + k)-th smallest non-target of all: within tol of the float64 non-target of that rank
    non = np.sort(s64[~target])
    C = np.concatenate(([0], np.cumsum(hist)))
    full = np.flatnonzero(hist)
    for b in {int(full[0]), int(np.argmax(hist)), int(full[len(full) // 2]), int(full[-1])}:
        n = int(hist[b])
        ks = sorted({1, (n + 1) // 2, n})
        got = [r.kth_nontarget(b, k) for k in ks]
        assert got == sorted(got) and (b == 0 or got[0] > targets[b - 1]) and (b == len(targets) or got[-1] <= targets[b])
        for k, g in zip(ks, got):
            assert abs(g - non[C[b] + k - 1]) <= TOL, (b, k, g, non[C[b] + k - 1])


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_small_random_case_is_exact(M, seed):
    trials, tl, enroll, el = ot.band_case(5, 7, 4, 2, seed)
    target = ot.is_target(tl, el)
    s64 = ot.scores64(trials, enroll)
    gap = np.abs(s64[target][:, None] - s64[~target][None, :]).min()
    assert gap >= 4 * TOL, gap                              # no non-target can change sides of a target within the tolerance
    s = s64.astype(np.float32)
    t_ref, h_ref = ot.ranks_from_scores(s, target)
    _, targets, hist = _ranks(M, trials, tl, enroll, el)
    assert (hist == h_ref).all() and np.abs(targets.astype(np.float64) - np.sort(s64[target])).max() <= TOL
    ref = ot.oracle_metrics(s, target)
    got = M.evaluate_trials_fused(torch.as_tensor(enroll).cuda(), el, torch.as_tensor(trials).cuda(), tl)
    assert got[:2] == ref[:2] and abs(got[2] - float(ref[2])) <= TOL, (got, ref)


# ------------------------------------------------------------------------------------------------ properties
def test_row_order_does_not_matter(M, band):
    trials, tl, enroll, el, _, _ = band
    base = _ranks(M, trials, tl, enroll, el)[1:]
    rs = np.random.RandomState(3)
    pe, pt = rs.permutation(len(el)), rs.permutation(len(tl))
    assert _same_bits(base, _ranks(M, trials, tl, enroll[pe], el[pe])[1:])
    assert _same_bits(base, _ranks(M, trials[pt], tl[pt], enroll, el)[1:])
    assert _same_bits(base, _ranks(M, trials[pt], tl[pt], enroll[pe], el[pe])[1:])


def test_two_runs_same_bits(M, band):
    trials, tl, enroll, el, _, _ = band
    assert _same_bits(_ranks(M, trials, tl, enroll, el)[1:], _ranks(M, trials, tl, enroll, el)[1:])


@pytest.mark.parametrize('Nt,Ne', [(97, 640), (65, 257), (32, 128), (31, 1)])
def test_nothing_is_read_past_the_lists_or_from_the_workspace(M, band, Nt, Ne):
    """NaN rows behind Nt / Ne in larger buffers and a workspace pre-filled with NaN: the bits of the tight call."""
    from ppvector import _native as N
    trials, tl, enroll, el, s64, target = band
    if not target[:Nt, :Ne].any():
        pytest.fail('the cut has no target pair')
    tight = _ranks(M, trials[:Nt].copy(), tl[:Nt], enroll[:Ne].copy(), el[:Ne])[1:]
    big_t = np.full((Nt + 40, 192), np.nan, np.float32)
    big_e = np.full((Ne + 50, 192), np.nan, np.float32)
    big_t[:Nt], big_e[:Ne] = trials[:Nt], enroll[:Ne]
    need = N.lib().vp_trial_ranks_workspace_bytes(Nt, Ne, 192, len(tight[0]))
    assert need > 0
    ws = torch.full((need // 4 + 64,), float('nan'), dtype=torch.float32, device='cuda').view(torch.uint8)
    loose = _ranks(M, big_t, np.concatenate([tl[:Nt], tl[:40]]), big_e, np.concatenate([el[:Ne], el[:50]]), Nt=Nt, Ne=Ne, ws=ws)[1:]
    assert _same_bits(tight, loose)
    ot.check_band(tight[0], tight[1], s64[:Nt, :Ne], target[:Nt, :Ne])


def test_zero_rows_score_zero(M):
    trials, tl, enroll, el = ot.band_case(33, 129, 20, 4, seed=5)
    trials, enroll = trials.copy(), enroll.copy()
    zt = int(np.flatnonzero(tl < 4)[0])                     # a trial whose speaker is enrolled
    ze = int(np.flatnonzero(el != tl[zt])[0])               # an enrol row of another speaker with trials of its own
    trials[zt], enroll[ze] = 0.0, 0.0
    target = ot.is_target(tl, el)
    s64 = ot.scores64(trials, enroll)
    r, targets, hist = _ranks(M, trials, tl, enroll, el)
    ot.check_band(targets, hist, s64, target)
    zero_targets = int(target[zt].sum() + target[:, ze].sum())
    zero_nontargets = int((~target[zt]).sum() + (~target[:, ze]).sum()) - 1
    assert zero_targets >= 2 and (targets == 0.0).sum() == zero_targets
    # the non-targets that are exactly 0 stand in the bin of 0.0 itself: below the first zero target, above every negative one
    b = int(np.searchsorted(targets, 0.0, side='left'))
    assert hist[b] >= zero_nontargets
    assert r.kth_nontarget(b, int(hist[b])) == 0.0          # ... and are the largest of that bin


def test_the_switch_routes_evaluate_trials(M, band):
    import ppvector
    trials, tl, enroll, el, _, _ = band
    args = (torch.as_tensor(enroll).cuda(), el, torch.as_tensor(trials).cuda(), tl)
    fused = M.evaluate_trials_fused(*args)
    matrix = M.evaluate_trials(*args)
    before = ppvector.get_trial_scorer()
    ppvector.set_trial_scorer('fused')
    try:
        assert M.evaluate_trials(*args) == fused
    finally:
        ppvector.set_trial_scorer(before)
    assert M.evaluate_trials(*args) == matrix
    print(f'[trial scorers] fused {fused} matrix {matrix}')


def test_unsupported_shapes_raise(M):
    from ppvector import _native as N
    x = torch.ones((3, 6), device='cuda')
    with pytest.raises(N.VpmiError):                        # D % 4 != 0
        M.trial_ranks(x, [0, 1, 2], x, [0, 1, 2])
    x = torch.ones((3, 8), device='cuda')
    with pytest.raises(N.VpmiError):                        # no target pair
        M.trial_ranks(x, [0, 1, 2], x, [3, 4, 5])
