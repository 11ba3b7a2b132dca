"""Adaptive score normalisation on the GPU (csrc/cohort_stats.hip, csrc/score_norm.h, the normalised passes of csrc/trial_ranks.hip,
ppvector/metric/score_norm.py) against tests/score_norm_oracle.py; docs/score_norm.md is the contract.  Shapes: every edge of the
32-column tile, the 32-row wave tile and the 128-row slab, D with and without the tail of four, both digit widths (D = 1024 is the
largest LDS request and the 7-bit path), top_n below, at and above C.  No case has more than 97 x 640 pairs.

Observed on an MI355X (the tests print these; docs/score_norm.md has the table): band family, largest |mean - float64| 2.6e-08 and
5.3e-09, |std - float64| 1.7e-08 and 6.5e-09, against the derived 2e-06; largest |z - float64| of the normalised matrix 1.3e-06 (exact
family) and 2.0e-06 (band family), at most 0.041 of the per-pair bound."""
import numpy as np
import pytest
import torch

from tests import score_norm_oracle as osn
from tests import trial_ranks_oracle as ot

pytestmark = pytest.mark.gpu

TOL = ot.TOL

EXACT = [       # (Q, C, D, nspk, moved, top_n), lattice_case seed 7; the second list is the cohort
    (33, 129, 32, 6, 5, 20),
    (31, 128, 64, 5, 8, 128),
    (65, 257, 192, 12, 5, 300),
    (65, 257, 192, 12, 8, 64),
    (32, 384, 1024, 20, 8, 300),
    (65, 384, 1024, 1, 12, 100),
]
FLOOR = [       # the same; rows with std = 0: 33, 5 and 3
    (33, 129, 32, 6, 5, 1),
    (5, 1, 20, 3, 5, 4),
    (32, 127, 20, 3, 5, 2),
]
BAND = [        # (Q, C, D, nspk, top_n, seed), band_case
    (70, 300, 20, 10, 50, 3),
    (97, 640, 192, 30, 300, 3),
]


@pytest.fixture(scope='module')
def SN():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: these tests must run on an MI355X (no CPU fallback exists)')
    from ppvector.metric import score_norm
    return score_norm


@pytest.fixture(scope='module')
def M():
    from ppvector.metric import metrics
    return metrics


def _gpu(a):
    return torch.as_tensor(a).cuda()


def _stats(SN, x, cohort, top_n, **kw):
    mean, std = SN.cohort_stats(_gpu(x), _gpu(cohort), top_n, **kw)
    assert mean.dtype == std.dtype == torch.float32 and mean.is_cuda and std.is_cuda
    return mean.cpu().numpy(), std.cpu().numpy()


def _same_bits(a, b):
    return all(x.shape == y.shape and (x.view(np.int32) == y.view(np.int32)).all() for x, y in zip(a, b))


_CASES = {}


def _lattice(Q, C, D, nspk, moved):
    """lattice_case once per shape (never modified): trials, labels, cohort = enrol list, labels, exact float32 cosines both ways."""
    key = (Q, C, D, nspk, moved)
    if key not in _CASES:
        x, xl, c, cl = ot.lattice_case(Q, C, D, nspk, moved, seed=7)
        s = ot.scores64(x, c)
        cc = ot.scores64(c, c)
        assert (s * 16 == np.round(s * 16)).all() and (cc * 16 == np.round(cc * 16)).all()
        _CASES[key] = (x, xl, c, cl, s.astype(np.float32), cc.astype(np.float32))
    return _CASES[key]


def _band(Q, C, D, nspk, seed):
    key = ('band', Q, C, D, nspk, seed)
    if key not in _CASES:
        x, xl, c, cl = ot.band_case(Q, C, D, nspk, seed)
        _CASES[key] = (x, xl, c, cl, ot.scores64(x, c), ot.scores64(c, c))
    return _CASES[key]


# ------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize('Q,C,D,nspk,moved,top_n', EXACT)
def test_exact_statistics(SN, Q, C, D, nspk, moved, top_n):
    x, _, c, _, s, _ = _lattice(Q, C, D, nspk, moved)
    ref = osn.topn_stats32(s, top_n)
    assert ref[1].min() >= 0.0136                           # no floor in this family
    n = min(top_n, C)
    nth = -np.sort(-s, axis=1)[:, n - 1]
    cut = int(((s >= nth[:, None]).sum(1) > n).sum())       # rows whose n-th place lies inside a block of equal scores
    got = _stats(SN, x, c, top_n)
    print(f'[score norm exact {(Q, C, D, nspk, moved, top_n)}] std {ref[1].min():.4f} .. {ref[1].max():.4f}; {cut} of {Q} rows cut ties')
    assert _same_bits(got, ref), (np.abs(got[0] - ref[0]).max(), np.abs(got[1] - ref[1]).max())
    assert _same_bits(_stats(SN, x, c, top_n), ref)                                     # a second run
    assert _same_bits(_stats(SN, x, c[np.random.RandomState(3).permutation(C)], top_n), ref)    # the cohort's order
    # NaN rows behind Q and C in larger buffers, a workspace pre-filled with NaN
    from ppvector import _native as N
    big_x = np.full((Q + 40, D), np.nan, np.float32)
    big_c = np.full((C + 50, D), np.nan, np.float32)
    big_x[:Q], big_c[:C] = x, c
    need = N.lib().vp_cohort_stats_workspace_bytes(Q, C, D)
    assert need == (C * D * 4 + 255) // 256 * 256
    ws = torch.full((need // 4 + 64,), float('nan'), dtype=torch.float32, device='cuda').view(torch.uint8)
    assert _same_bits(_stats(SN, big_x, big_c, top_n, Q=Q, C=C, ws=ws), ref)


@pytest.mark.parametrize('Q,C,D,nspk,moved,top_n', FLOOR)
def test_floor(SN, Q, C, D, nspk, moved, top_n):
    x, _, c, _, s, cc = _lattice(Q, C, D, nspk, moved)
    ref = osn.topn_stats32(s, top_n)
    zero = int((ref[1] == 0).sum())
    assert zero == {1: 33, 4: 5, 2: 3}[top_n]
    got = _stats(SN, x, c, top_n)
    assert _same_bits(got, ref)
    # z of the rows against the cohort as enrolments: finite, and the restatement's bits (r is 10^6 where std is below the floor)
    sn = SN.ScoreNorm(_gpu(c), top_n)
    cref = osn.topn_stats32(cc, top_n)
    z = sn.normalise(_gpu(s.copy()), _gpu(x), _gpu(c)).cpu().numpy()
    want = osn.z32(s, cref[0], osn.recip_std(cref[1]), ref[0], osn.recip_std(ref[1]))
    assert np.isfinite(z).all() and (z.view(np.int32) == want.view(np.int32)).all()
    print(f'[score norm floor {(Q, C, D, nspk, moved, top_n)}] {zero} rows with std = 0, |z| up to {np.abs(z).max():.4g}')


def test_zero_row(SN):
    x, _, c, _, s, _ = _lattice(33, 129, 32, 6, 5)
    x = x.copy()
    x[7] = 0.0
    mean, std = _stats(SN, x, c, 20)
    ref = osn.topn_stats32(s, 20)
    assert mean[7] == 0.0 and std[7] == 0.0
    keep = np.arange(33) != 7
    assert _same_bits((mean[keep], std[keep]), (ref[0][keep], ref[1][keep]))


@pytest.mark.parametrize('Q,C,D,nspk,top_n,seed', BAND)
def test_band_statistics(SN, Q, C, D, nspk, top_n, seed):
    """Every score is within TOL of its float64 value; order statistics, and the standard deviation of the sorted top-N vector, are
    1-Lipschitz in the sup norm; a second TOL covers the rounding to float32."""
    x, _, c, _, s64, _ = _band(Q, C, D, nspk, seed)
    mean64, std64 = osn.topn_stats(s64, top_n)
    mean, std = _stats(SN, x, c, top_n)
    em, es = np.abs(mean - mean64).max(), np.abs(std - std64).max()
    print(f'[score norm band {(Q, C, D, nspk, top_n, seed)}] std64 {std64.min():.3f} .. {std64.max():.3f}; largest |mean - float64| '
          f'{em:.3e}, |std - float64| {es:.3e} (bound {2 * TOL:.0e})')
    assert em <= 2 * TOL and es <= 2 * TOL
    assert _same_bits(_stats(SN, x, c, top_n), (mean, std))


def test_unsupported_shapes_raise(SN):
    from ppvector import _native as N
    with pytest.raises(N.VpmiError):                        # D % 4 != 0
        SN.cohort_stats(torch.ones((3, 6), device='cuda'), torch.ones((5, 6), device='cuda'))
    with pytest.raises(N.VpmiError):                        # top_n = 0
        SN.cohort_stats(torch.ones((3, 8), device='cuda'), torch.ones((5, 8), device='cuda'), top_n=0)
    with pytest.raises(N.VpmiError):                        # a host cohort_stats call
        SN.cohort_stats(torch.ones((3, 8)), torch.ones((5, 8), device='cuda'))


# ------------------------------------------------------------------------------------------------ the normalised matrix
def _z_reference(s64, cc64, top_n):
    """float64 z of every (trial, enrolment = cohort row) pair and its bound, from the oracle's own quantities."""
    mt, st = osn.topn_stats(s64, top_n)
    me, se = osn.topn_stats(cc64, top_n)
    assert min(st.min(), se.min()) >= 0.01                  # first-order propagation is valid
    return osn.z64(s64, me, se, mt, st), osn.z_bound(s64, me, se, mt, st)


def _matrix_case(kind, case):
    if kind == 'exact':
        Q, C, D, nspk, moved, top_n = case
        x, xl, c, cl, s, cc = _lattice(Q, C, D, nspk, moved)
        return x, xl, c, cl, s.astype(np.float64), cc.astype(np.float64), top_n
    Q, C, D, nspk, top_n, seed = case
    return _band(Q, C, D, nspk, seed) + (top_n,)


@pytest.mark.parametrize('kind,case', [('exact', c) for c in EXACT] + [('band', c) for c in BAND])
def test_normalised_matrix(SN, M, kind, case):
    x, _, c, _, s64, cc64, top_n = _matrix_case(kind, case)
    z64, bound = _z_reference(s64, cc64, top_n)
    sn = SN.ScoreNorm(_gpu(c), top_n)
    z = sn.normalise(M.cosine_score_matrix(_gpu(x), _gpu(c)), _gpu(x), _gpu(c)).cpu().numpy()
    err = np.abs(z - z64)
    print(f'[score norm matrix {kind} {case}] largest |z - float64| {err.max():.3e}, bound there {bound.reshape(-1)[err.argmax()]:.3e}, '
          f'smallest bound {bound.min():.3e}, largest err / bound {(err / bound).max():.3f}')
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------ the fused scorer
def _ranks(M, x, xl, c, cl, sn):
    r = M.TrialRanks(_gpu(x), xl, _gpu(c), cl, score_norm=sn)
    return r, r.targets.cpu().numpy(), r.hist.cpu().numpy()


@pytest.mark.parametrize('Q,C,D,nspk,moved,top_n', EXACT)
def test_fused_exact(SN, M, Q, C, D, nspk, moved, top_n):
    x, xl, c, cl, s, cc = _lattice(Q, C, D, nspk, moved)
    target = ot.is_target(xl, cl)
    sn = SN.ScoreNorm(_gpu(c), top_n)
    # the z matrix in NumPy float32 from the device's own statistics (bit-exact: test_exact_statistics) and the exact cosines
    (tm, ts), (em, es) = [tuple(t.cpu().numpy() for t in sn.stats(_gpu(a))) for a in (x, c)]
    assert _same_bits((tm, ts, em, es), osn.topn_stats32(s, top_n) + osn.topn_stats32(cc, top_n))
    z = osn.z32(s, em, osn.recip_std(es), tm, osn.recip_std(ts))
    t_ref, h_ref = ot.ranks_from_scores(z, target)
    r, targets, hist = _ranks(M, x, xl, c, cl, sn)
    assert targets.dtype == np.float32 and targets.shape == t_ref.shape and (targets.view(np.int32) == t_ref.view(np.int32)).all()
    assert hist.shape == h_ref.shape and (hist == h_ref).all()
    ref = ot.oracle_metrics(z, target)
    got = M.evaluate_trials_fused(_gpu(c), cl, _gpu(x), xl, score_norm=sn)
    print(f'[score norm fused {(Q, C, D, nspk, moved, top_n)}] NT {len(t_ref)} NN {int(h_ref.sum())} EER {ref[0]:.4f} minDCF {ref[1]:.4f} '
          f'threshold {float(ref[2]):.6f}; {len(np.unique(z))} distinct z')
    assert got == (ref[0], ref[1], float(ref[2])), (got, ref)
    non = z[~target]
    bins = np.searchsorted(t_ref, non, side='left')
    b = int(np.argmax(h_ref))
    inside = np.sort(non[bins == b])
    for k in sorted({1, (len(inside) + 1) // 2, len(inside)}):
        assert r.kth_nontarget(b, k) == inside[k - 1], (b, k)


@pytest.mark.parametrize('Q,C,D,nspk,top_n,seed', BAND)
def test_fused_band(SN, M, Q, C, D, nspk, top_n, seed):
    x, xl, c, cl, s64, cc64 = _band(Q, C, D, nspk, seed)
    z64, bound = _z_reference(s64, cc64, top_n)
    _, targets, hist = _ranks(M, x, xl, c, cl, SN.ScoreNorm(_gpu(c), top_n))
    worst = ot.check_band(targets, hist, z64, ot.is_target(xl, cl), tol=float(bound.max()))
    print(f'[score norm fused band {(Q, C, D, nspk, top_n, seed)}] NT {len(targets)} largest |target - float64| {worst:.3e} '
          f'(tol {bound.max():.3e})')


def test_without_normalisation_nothing_changes(SN, M):
    """score_norm=None: both scorers give the bits they give without the argument, and the cosines' ranks."""
    import ppvector
    x, xl, c, cl, s, _ = _lattice(65, 257, 192, 12, 8)
    assert ppvector.get_score_norm() is None
    plain = _ranks(M, x, xl, c, cl, None)[1:]
    r = M.TrialRanks(_gpu(x), xl, _gpu(c), cl)
    assert r.stats is None and _same_bits(plain[:1], (r.targets.cpu().numpy(),)) and (plain[1] == r.hist.cpu().numpy()).all()
    t_ref, h_ref = ot.ranks_from_scores(s, ot.is_target(xl, cl))
    assert (plain[0] == t_ref).all() and (plain[1] == h_ref).all()
    args = (_gpu(c), cl, _gpu(x), xl)
    before = ppvector.get_trial_scorer()
    try:
        for scorer in ('matrix', 'fused'):
            ppvector.set_trial_scorer(scorer)
            assert M.evaluate_trials(*args) == M.evaluate_trials(*args, score_norm=None)
        assert M.evaluate_trials_fused(*args) == M.evaluate_trials_fused(*args, score_norm=None) == M.evaluate_trials(*args)
        # ... and the default of the switch is what evaluate_trials takes when it is handed none
        sn = SN.ScoreNorm(_gpu(c), 64)
        ppvector.set_score_norm(sn)
        try:
            assert M.evaluate_trials(*args) == M.evaluate_trials_fused(*args, score_norm=sn) != M.evaluate_trials_fused(*args)
        finally:
            ppvector.set_score_norm(None)
    finally:
        ppvector.set_trial_scorer(before)


# ------------------------------------------------------------------------------------------------ the trainer
def _write_wav(path, pcm):
    import wave
    with wave.open(path, 'wb') as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(np.asarray(pcm, np.int16).tobytes())


def _configs(root, score_norm):
    eval_conf = dict(batch_size=2, max_duration=20)
    if score_norm is not None:
        eval_conf['score_norm'] = score_norm
    return dict(
        dataset_conf=dict(dataset=dict(min_duration=0.3, max_duration=2, sample_rate=16000, use_dB_normalization=True, target_dB=-20),
                          sampler=dict(batch_size=4, shuffle=True, drop_last=True), dataLoader=dict(num_workers=2),
                          eval_conf=eval_conf,
                          train_list=f'{root}/train_list.txt', enroll_list=f'{root}/enroll_list.txt', trials_list=f'{root}/trials_list.txt',
                          is_use_pksampler=False, sample_per_id=4),
        preprocess_conf=dict(feature_method='Fbank', method_args=dict(sr=16000, n_mels=80)),
        model_conf=dict(model='TDNN', model_args=dict(embd_dim=192, pooling_type='ASP'),
                        classifier=dict(classifier_type='Cosine', num_speakers=2, num_blocks=0)),
        loss_conf=dict(loss='AAMLoss', loss_args=dict(margin=0.2, scale=32, easy_margin=False, label_smoothing=0.0),
                       use_margin_scheduler=True, margin_scheduler_args=dict(initial_margin=0.0, final_margin=0.3)),
        optimizer_conf=dict(optimizer='Adam', optimizer_args=dict(weight_decay=1e-6), scheduler='WarmupCosineSchedulerLR',
                            scheduler_args=dict(learning_rate=2e-3, min_lr=1e-5, warmup_epoch=1)),
        train_conf=dict(enable_amp=False, max_epoch=1, log_interval=1))


def test_trainer_cohort_and_evaluate(SN, M, golden_dir, tmp_path):
    """The four reference WAVs (two speakers): extract_cohort on the training list, then evaluate() configured with that cohort
    against evaluate_trials on the same embeddings.  The model is the trainer's freshly initialised one: nothing is trained."""
    from ppvector.trainer import PPVectorTrainer
    root = str(tmp_path)
    pcm = np.load(f'{golden_dir}/wavs_3s.npz')['pcm']                       # a_1, a_2, b_1, b_2 (3 s each)
    lists = {'train': [], 'enroll': [], 'trials': []}
    for r, spk in ((0, 0), (1, 0), (2, 1), (3, 1)):
        for k, (a, b) in enumerate(((0, 48000), (4000, 44000), (8000, 30000))):
            p = f'{root}/train_{r}_{k}.wav'
            _write_wav(p, pcm[r, a:b])
            lists['train'].append(f'{p}\t{spk}')
        for name, (a, b) in (('enroll', (0, 24000)), ('trials', (24000, 48000))):
            p = f'{root}/{name}_{r}.wav'
            _write_wav(p, pcm[r, a:b])
            lists[name].append(f'{p}\t{spk}')
    for name, lines in lists.items():
        open(f'{root}/{name}_list.txt', 'w').write('\n'.join(lines) + '\n')
    cohort_path = f'{root}/cohort/cohort.npy'
    tr = PPVectorTrainer(_configs(root, dict(cohort=cohort_path, top_n=300)), use_gpu=True)
    cohort = tr.extract_cohort(f'{root}/train_list.txt', save_path=cohort_path)
    assert cohort.shape == (2, 192) and cohort.dtype == np.float32 and np.isfinite(cohort).all()
    assert (np.load(cohort_path) == cohort).all()
    got = tr.evaluate()
    tr.model.eval()
    backbone = tr.model if len(tr.model) == 1 else tr.model[0]
    enroll, el = tr._embed(tr.enroll_loader, tr.enroll_dataset, backbone)
    trials, tl = tr._embed(tr.trials_loader, tr.trials_dataset, backbone)
    tr.model.train()
    want = M.evaluate_trials(enroll, el.cpu().numpy(), trials, tl.cpu().numpy(), score_norm=SN.ScoreNorm(_gpu(cohort), 300))
    plain = M.evaluate_trials(enroll, el.cpu().numpy(), trials, tl.cpu().numpy())
    print(f'[score norm trainer] evaluate() with the cohort {got}, evaluate_trials {want}, raw cosines {plain}')
    assert got == want and all(np.isfinite(got))
    # absent from the configuration: evaluate() is the raw-cosine evaluation
    assert PPVectorTrainer(_configs(root, None), use_gpu=True)._score_norm() is None
