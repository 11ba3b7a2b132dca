"""Score calibration on the GPU (csrc/calibrate.hip, TrialRanks.calib_sums, ppvector/metric/calibration.py, the trainer's and the
predictor's doors) against tests/calibration_oracle.py; docs/calibration.md is the contract.  Shapes: every edge of the 32-column
tile and the 128-row slab, a shape whose trial tiles are split over several workgroups (read from the partials query), D with and
without the tail of four up to the largest LDS request; (a, b) up to |u| of about 90 and 200, which only the stable forms of softplus
and sigma survive.  No case has more than 33 x 1000 pairs.

The bound of a sum (tests/calibration_oracle.py::sums_bound) is derived, not fitted: (Pc + 64) 2^-53 sum |term| -- the worst case
of a float64 sum of Pc terms in any order, and 64 ulps for the functions inside a term.  The tests print the largest
|device - oracle| / bound they meet; docs/calibration.md has the table."""
import ctypes
import math
import warnings
import wave

import numpy as np
import pytest
import torch

from tests import calibration_oracle as oc
from tests import score_norm_oracle as osn
from tests import trial_ranks_oracle as ot

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2), (31, 127), (32, 128), (33, 129), (65, 257), (33, 1000)]       # the last: a trial tile over four workgroups
DIMS = [16, 64, 192, 1024]
AB = [(1.0, 0.0), (9.3, -3.5), (146.0, -59.0), (-4.0, 2.0)]


@pytest.fixture(scope='module')
def M():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: these tests must run on an MI355X (no CPU fallback exists)')
    from ppvector.metric import metrics
    return metrics


@pytest.fixture(scope='module')
def C():
    from ppvector.metric import calibration
    return calibration


def _gpu(a):
    return torch.as_tensor(a).cuda()


_CASES = {}


def _lattice(Nt, Ne, D, moved=5, nspk=6, plant=False):
    """lattice_case once per shape (never modified) -> trials, labels, enrol rows, labels, the exact float32 cosines.  Every label
    pattern has a target and a non-target; (1, 2) gets them by hand.  ``plant``: enrol rows 0 .. 3 become trial 0, its negative,
    trial 1 and its negative, labelled so that each class has a pair with s = 1 and one with s = -1."""
    key = (Nt, Ne, D, moved, nspk, plant)
    if key not in _CASES:
        x, xl, c, cl = ot.lattice_case(Nt, Ne, D, nspk, moved, seed=11)
        if Nt == 1:
            xl, cl = np.array([4]), np.array([4, 2])
        elif plant:
            c[0], c[1], c[2], c[3] = x[0], -x[0], x[1], -x[1]
            cl[0], cl[1], cl[2], cl[3] = xl[0], (xl[0] + 1) % 6, (xl[1] + 1) % 6, xl[1]
        s = ot.scores64(x, c)
        assert (s * 16 == np.round(s * 16)).all()
        target = ot.is_target(xl, cl)
        assert target.any() and (~target).any()
        _CASES[key] = (x, xl, c, cl, s.astype(np.float32))
    return _CASES[key]


def _check(name, got, scores, target, a, b, extra=None):
    """got (2, 6) against the oracle's sums of `scores` within sums_bound (+ extra) -> the largest |device - oracle| / bound."""
    want, mag, pairs = oc.sums(scores, target, a, b)
    bound = oc.sums_bound(mag, pairs) + (0.0 if extra is None else extra(pairs))
    err = np.abs(got - want)
    assert got.shape == (2, 6) and got.dtype == np.float64 and np.isfinite(got).all()
    ratio = float(np.max(np.where(err > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
    print(f'[calibration {name} a={a} b={b}] pairs {pairs.tolist()} largest |device - oracle| / bound {ratio:.3e}, '
          f'largest relative error {np.max(err / np.maximum(mag, 1e-300)):.3e}')
    assert (err <= bound).all(), (name, a, b, err, bound)
    return ratio


# ------------------------------------------------------------------------------------------------ 1. lattice, exact scores
@pytest.mark.parametrize('D', DIMS)
@pytest.mark.parametrize('Nt,Ne', SHAPES)
def test_sums_on_exact_scores(M, Nt, Ne, D):
    """Every cosine is a multiple of 1/16 that the device and the oracle hold alike, and a s + b is two rounded operations on both
    sides: u is the same number, and what is left is the functions inside a term and the order of the additions."""
    from ppvector import _native as N
    x, xl, c, cl, s = _lattice(Nt, Ne, D, plant=True)
    target = ot.is_target(xl, cl)
    workgroups = N.lib().vp_trial_calib_partials_bytes(Nt, Ne, D) // 96
    tiles = (Nt + 31) // 32
    assert workgroups % tiles == 0 and workgroups // tiles == {2: 1, 127: 1, 128: 1, 129: 1, 257: 2, 1000: 4}[Ne]
    r = M.TrialRanks(_gpu(x), xl, _gpu(c), cl)
    assert r.stats is None
    for a, b in AB:
        _check(f'exact {(Nt, Ne, D)}', r.calib_sums(a, b), s, target, a, b)
    if Nt > 1:                                              # the third pair drives |u| to 87 and 205, in both directions, in both classes
        y = 146.0 * s.astype(np.float64) - 59.0
        assert y[target].max() == y[~target].max() == 87.0 and y[target].min() == y[~target].min() == -205.0


def test_sums_with_zero_rows(M):
    """A zero row scores 0 against everything and counts as a pair, as in the ranks."""
    x, xl, c, cl, _ = _lattice(65, 257, 192)
    x, c = x.copy(), c.copy()
    x[[3, 40]] = 0.0
    c[[5, 128, 256]] = 0.0
    s = ot.scores64(x, c).astype(np.float32)
    assert (s[3] == 0).all() and (s[:, 128] == 0).all()
    r = M.TrialRanks(_gpu(x), xl, _gpu(c), cl)
    for a, b in AB:
        _check('zero rows', r.calib_sums(a, b), s, ot.is_target(xl, cl), a, b)


# ------------------------------------------------------------------------------------------------ 2. the same bits twice
@pytest.mark.parametrize('Nt,Ne,D', [(65, 257, 192), (33, 1000, 64)])
def test_same_bits_twice(M, Nt, Ne, D):
    x, xl, c, cl, _ = _lattice(Nt, Ne, D)
    r = M.TrialRanks(_gpu(x), xl, _gpu(c), cl)
    first = r.calib_sums(9.3, -3.5).copy()
    again = r.calib_sums(9.3, -3.5).copy()
    assert first.tobytes() == again.tobytes()
    r._calib_partials.fill_(0xff)                           # NaN bytes in every partial and in the result: all of them are rewritten
    r._calib_out.fill_(float('nan'))
    assert r.calib_sums(9.3, -3.5).tobytes() == first.tobytes()
    assert M.TrialRanks(_gpu(x), xl, _gpu(c), cl).calib_sums(9.3, -3.5).tobytes() == first.tobytes()   # another object, other buffers
    assert r.calib_sums(1.0, 0.0).tobytes() != first.tobytes()


def test_entry_point_refuses_before_launching(M):
    """Non-finite a or b and buffers one byte short are VP_EINVAL, and nothing is written."""
    from ppvector import _native as N
    x, xl, c, cl, _ = _lattice(33, 129, 64)
    r = M.TrialRanks(_gpu(x), xl, _gpu(c), cl)
    r.calib_sums(1.0, 0.0)
    r._calib_out.fill_(-7.0)
    lib = N.lib()

    def call(a, b, partials_bytes=None, ws_bytes=None):
        ab = (ctypes.c_double * 2)(a, b)
        return lib.vp_trial_calib_sums_f32(r._ctx, r._tl.data_ptr(), r.Nt, r._el.data_ptr(), r.Ne, r.D, ctypes.addressof(ab),
                                           r._calib_out.data_ptr(), r._calib_partials.data_ptr(),
                                           r._calib_partials.numel() if partials_bytes is None else partials_bytes,
                                           r._ws.data_ptr(), r._ws.numel() if ws_bytes is None else ws_bytes, N.stream_ptr())

    for a, b in ((float('nan'), 0.0), (1.0, float('inf')), (float('-inf'), 0.0)):
        assert call(a, b) == N.VP_EINVAL
        with pytest.raises(N.VpmiError):
            r.calib_sums(a, b)
    assert call(1.0, 0.0, partials_bytes=r._calib_partials.numel() - 1) == N.VP_EINVAL
    assert call(1.0, 0.0, ws_bytes=lib.vp_trial_ranks_workspace_bytes(r.Nt, r.Ne, r.D, r.NT) - 1) == N.VP_EINVAL
    torch.cuda.synchronize()
    assert (r._calib_out.cpu().numpy() == -7.0).all()
    assert call(1.0, 0.0) == N.VP_OK


# ------------------------------------------------------------------------------------------------ 3. Gaussian inputs
@pytest.mark.parametrize('Nt,Ne', [(65, 257), (33, 1000)])
def test_sums_on_gaussian_rows(M, Nt, Ne):
    """The device's cosine differs from scores64 by at most (D + 2) 2^-24, and a term's derivative in s is at most |a| + 2, so
    |sum - oracle| <= Pc (|a| + 2) (D + 2) 2^-24 beside the bound of the exact test.  LOOSE BY DESIGN: it catches a slab that was
    not walked or a pair put into the wrong class, not a rounding."""
    D = 192
    x, xl, c, cl = ot.band_case(Nt, Ne, D, 8, seed=5)
    s64, target = ot.scores64(x, c), ot.is_target(xl, cl)
    r = M.TrialRanks(_gpu(x), xl, _gpu(c), cl)
    for a, b in AB:
        got = r.calib_sums(a, b)
        _check(f'gaussian {(Nt, Ne, D)}', got, s64, target, a, b,
               extra=lambda pairs: (pairs[:, None] * (abs(a) + 2.0) * (D + 2) * 2.0 ** -24) * np.ones((2, 6)))
        if a == 1.0:
            # what the bound is for: a sum that leaves the last slab out is far outside it (on the terms that do not vanish)
            want, mag, pairs = oc.sums(s64, target, a, b)
            slack = oc.sums_bound(mag, pairs) + pairs[:, None] * (abs(a) + 2.0) * (D + 2) * 2.0 ** -24
            short = oc.sums(s64[:, :Ne - Ne % 128], target[:, :Ne - Ne % 128], a, b)[0]
            assert (np.abs(short - want)[:, :2] > 10 * slack[:, :2]).all()


# ------------------------------------------------------------------------------------------------ 4. with a ScoreNorm
@pytest.mark.parametrize('top_n', [64, 300])
def test_sums_with_score_norm(M, C, top_n):
    """z from the device's own statistics (TrialRanks.stats) and the exact lattice cosines, restated in float32 one operation per
    line (score_norm_oracle.z32): the oracle's z has the device's bits.  top_n below and above the cohort's 257 rows."""
    from ppvector.metric.score_norm import ScoreNorm
    x, xl, c, cl, s = _lattice(65, 257, 192, moved=8, nspk=12)
    target = ot.is_target(xl, cl)
    sn = ScoreNorm(_gpu(c), top_n)
    r = M.TrialRanks(_gpu(x), xl, _gpu(c), cl, score_norm=sn)
    tm, tr, em, er = (t.cpu().numpy() for t in r.stats)
    z = osn.z32(s, em, er, tm, tr)
    t_ref, _ = ot.ranks_from_scores(z, target)
    assert (r.targets.cpu().numpy().view(np.int32) == t_ref.view(np.int32)).all()        # the ranks see the same z
    for a, b in AB:
        _check(f'score norm top_n={top_n}', r.calib_sums(a, b), z, target, a, b)
    assert not np.array_equal(r.calib_sums(1.0, 0.0), M.TrialRanks(_gpu(x), xl, _gpu(c), cl).calib_sums(1.0, 0.0))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        cal, info = C.fit_calibration(_gpu(c), cl, _gpu(x), xl, score_norm=sn)
    assert cal.normalised is True and math.isfinite(cal.a) and math.isfinite(cal.b)
    a, b, iterations, evaluations, converged = oc.fit(z, target)
    print(f'[calibration score norm top_n={top_n}] fit a {cal.a:.6f} b {cal.b:.6f} (oracle {a:.6f} {b:.6f}) in {info["iterations"]} '
          f'steps, Cllr {info["cllr"]:.6f} min {info["min_cllr"]:.6f} raw {info["cllr_raw"]:.6f}')
    assert (info['iterations'], info['converged']) == (iterations, converged)
    assert abs(cal.a - a) <= 1e-9 * abs(a) and abs(cal.b - b) <= 1e-9 * abs(b)
    cal0, _ = C.fit_calibration(_gpu(c), cl, _gpu(x), xl)
    assert cal0.normalised is False


# ------------------------------------------------------------------------------------------------ 5. the fit
def test_fit_against_the_oracle(M, C):
    """Overlapping classes whose device scores the host can restate: lattice utterances with 11 of their speaker's 16 entries moved
    (band_case's Gaussian rows have no cosine the host reproduces bit for bit, and 1e-9 on (a, b) needs the same scores on both
    sides).  Both sides take the same Newton steps from sums that differ by the bound of the exact test, a few 1e-16 relative; a step
    is d = -H^-1 g with a condition number of H of a few hundred here, so the iterates separate by about 1e-13 relative: (a, b)
    within 1e-9 relative and Cllr (whose gradient vanishes at the fit) within 1e-12 absolute."""
    x, xl, c, cl, s = _lattice(65, 257, 192, moved=11, nspk=6)
    target = ot.is_target(xl, cl)
    cal, info = C.fit_calibration(_gpu(c), cl, _gpu(x), xl)
    a, b, iterations, evaluations, converged = oc.fit(s, target)
    cllr, raw = oc.cllr(s, target, a, b), oc.cllr(s, target)
    t, hist = M.trial_ranks(_gpu(x), xl, _gpu(c), cl)
    print(f'[calibration fit] NT {info["NT"]} NN {info["NN"]}: a {cal.a!r} b {cal.b!r} (oracle {a!r} {b!r}), {info["iterations"]} steps '
          f'{info["evaluations"]} evaluations; Cllr {info["cllr"]!r} (oracle {cllr!r}) raw {info["cllr_raw"]:.6f} min {info["min_cllr"]:.6f}; '
          f'|a - oracle| / |a| {abs(cal.a - a) / abs(a):.2e} |b - oracle| / |b| {abs(cal.b - b) / abs(b):.2e} '
          f'|Cllr - oracle| {abs(info["cllr"] - cllr):.2e}')
    assert info['NT'] == int(target.sum()) and info['NN'] == int((~target).sum())
    assert info['converged'] and converged and info['iterations'] == iterations <= 50 and info['evaluations'] == evaluations
    assert abs(cal.a - a) <= 1e-9 * abs(a) and abs(cal.b - b) <= 1e-9 * abs(b)
    assert abs(info['cllr'] - cllr) <= 1e-12 and abs(info['cllr_raw'] - raw) <= 1e-12
    assert info['min_cllr'] == C.min_cllr_from_ranks(t, hist) == pytest.approx(oc.min_cllr_expanded(s, target), rel=1e-12)
    assert 0.0 < info['min_cllr'] <= info['cllr'] < info['cllr_raw'] and cal.normalised is False and cal.prior == 0.5
    assert 0.05 < float((s[target].mean() - s[~target].mean())) and s[target].min() < s[~target].max()   # the classes do overlap


def test_fit_on_gaussian_rows_and_with_a_prior(M, C):
    """band_case: nothing to compare bit for bit, so the properties: convergence within the cap, min_cllr from the same ranks, the
    order min_cllr <= cllr <= cllr_raw, the oracle's fit on the float64 cosines nearby, and a prior other than 1/2."""
    x, xl, c, cl = ot.band_case(97, 640, 192, 30, seed=3)
    s64, target = ot.scores64(x, c), ot.is_target(xl, cl)
    t, hist = M.trial_ranks(_gpu(x), xl, _gpu(c), cl)
    a, b, iterations, _, converged = oc.fit(s64, target)
    for prior in (0.5, 0.05):
        cal, info = C.fit_calibration(_gpu(c), cl, _gpu(x), xl, prior=prior)
        print(f'[calibration fit gaussian P={prior}] a {cal.a:.6f} b {cal.b:.6f} (float64 cosines, P=0.5: {a:.6f} {b:.6f}) in '
              f'{info["iterations"]} steps, {info["evaluations"]} evaluations; Cllr {info["cllr"]:.6f} raw {info["cllr_raw"]:.6f} '
              f'min {info["min_cllr"]:.6f}')
        assert info['converged'] and info['iterations'] <= 50 and cal.prior == prior
        assert info['min_cllr'] == C.min_cllr_from_ranks(t, hist)
        assert info['min_cllr'] <= info['cllr'] <= info['cllr_raw']
        if prior == 0.5:
            # a cosine moves by at most (D + 2) 2^-24 = 1.2e-5: the fit moves by about a times that relative to the scores' spread
            assert converged and abs(cal.a - a) <= 1e-3 * abs(a) and abs(cal.b - b) <= 1e-3 * abs(b)
            assert abs(info['cllr'] - oc.cllr(s64, target, a, b)) <= 1e-4


# ------------------------------------------------------------------------------------------------ 6. end to end
def _write_wav(path, pcm):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(np.asarray(pcm, np.int16).tobytes())


def _configs(root):
    return dict(
        dataset_conf=dict(dataset=dict(min_duration=0.3, max_duration=2, sample_rate=16000, use_dB_normalization=True, target_dB=-20),
                          sampler=dict(batch_size=4, shuffle=True, drop_last=True), dataLoader=dict(num_workers=2),
                          eval_conf=dict(batch_size=2, max_duration=20),
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


def test_trainer_and_predictor_end_to_end(M, C, golden_dir, tmp_path):
    """The four reference WAVs (two speakers), cut into eight enrolment and eight trial segments: PPVectorTrainer.calibrate on the
    trainer's freshly initialised model (nothing is trained), the JSON it writes, and PPVectorPredictor's calibrated pair scores."""
    from ppvector.metric.score_norm import ScoreNorm
    from ppvector.predict import PPVectorPredictor
    from ppvector.trainer import PPVectorTrainer
    root = str(tmp_path)
    pcm = np.load(f'{golden_dir}/wavs_3s.npz')['pcm']                       # a_1, a_2, b_1, b_2 (3 s each)
    lists = {'train': [], 'enroll': [], 'trials': []}
    for r, spk in ((0, 0), (1, 0), (2, 1), (3, 1)):
        p = f'{root}/train_{r}.wav'
        _write_wav(p, pcm[r])
        lists['train'].append(f'{p}\t{spk}')
        for name, cuts in (('enroll', ((0, 16000), (16000, 32000))), ('trials', ((32000, 48000), (8000, 24000)))):
            for k, (a, b) in enumerate(cuts):
                p = f'{root}/{name}_{r}_{k}.wav'
                _write_wav(p, pcm[r, a:b])
                lists[name].append(f'{p}\t{spk}')
    for name, lines in lists.items():
        open(f'{root}/{name}_list.txt', 'w').write('\n'.join(lines) + '\n')
    tr = PPVectorTrainer(_configs(root), use_gpu=True)
    assert tr.eval_cllr is None and tr.eval_min_cllr is None
    before = tr.evaluate()
    path = f'{root}/calibration/cal.json'
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)                     # 32 + 32 pairs of an untrained model may well be separable
        cal = tr.calibrate(save_path=path)
    print(f'[calibration trainer] {cal}, Cllr {tr.eval_cllr:.6f} min {tr.eval_min_cllr:.6f}; evaluate() {before}')
    assert isinstance(cal, C.Calibration) and cal.normalised is False and cal.prior == 0.5
    assert all(math.isfinite(v) for v in (cal.a, cal.b, tr.eval_cllr, tr.eval_min_cllr)) and 0.0 <= tr.eval_min_cllr <= tr.eval_cllr
    assert C.Calibration.load(path) == cal
    assert tr.evaluate() == before                                          # evaluate() is what it was
    # the same numbers from the embeddings evaluate() scores
    tr.model.eval()
    backbone = tr.model if len(tr.model) == 1 else tr.model[0]
    enroll, el = tr._embed(tr.enroll_loader, tr.enroll_dataset, backbone)
    trials, tl = tr._embed(tr.trials_loader, tr.trials_dataset, backbone)
    tr.model.train()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        cal2, info = C.fit_calibration(enroll, el.cpu().numpy(), trials, tl.cpu().numpy())
    assert cal2 == cal and (info['cllr'], info['min_cllr']) == (tr.eval_cllr, tr.eval_min_cllr) and info['NT'] == info['NN'] == 32

    pred = PPVectorPredictor(_configs(root), model_path={k: v.detach().cpu() for k, v in tr.model.state_dict().items()})
    w1, w2 = f'{root}/enroll_0_0.wav', f'{root}/trials_1_0.wav'
    with pytest.raises(ValueError):                                         # none set
        pred.contrast_llr(w1, w2)
    with pytest.raises(ValueError):
        pred.contrast_probability(w1, w2)
    pred.set_calibration(path)                                              # a path
    assert pred.calibration == cal
    s = pred.contrast(w1, w2)
    llr = pred.contrast_llr(w1, w2)
    assert isinstance(llr, float) and llr == cal.a * s + cal.b
    assert pred.contrast_probability(w1, w2) == cal.posterior(s) and pred.contrast_probability(w1, w2, p_target=0.01) == cal.posterior(s, 0.01)
    assert 0.0 <= pred.contrast_probability(w1, w2, p_target=0.01) <= pred.contrast_probability(w1, w2) <= 1.0
    assert pred.contrast(w1, w2) == s                                       # contrast does not look at the calibration
    # a calibration of normalised scores without a score norm, and the other way round
    pred.set_calibration(C.Calibration(cal.a, cal.b, normalised=True))
    with pytest.raises(ValueError):
        pred.contrast_llr(w1, w2)
    cohort = np.random.RandomState(0).standard_normal((5, 192)).astype(np.float32)
    pred.set_score_norm(ScoreNorm(_gpu(cohort), 3), threshold=0.0)
    z = pred.contrast(w1, w2)
    assert z != s and pred.contrast_llr(w1, w2) == cal.a * z + cal.b
    pred.set_calibration(cal)
    with pytest.raises(ValueError):
        pred.contrast_llr(w1, w2)
    pred.set_score_norm(None)
    assert pred.contrast_llr(w1, w2) == llr
    pred.set_calibration(None)
    with pytest.raises(ValueError):
        pred.contrast_llr(w1, w2)
    with pytest.raises(ValueError):
        pred.set_calibration(3.5)
    # the cooperative stop flag
    tr.stop_eval = True
    assert tr.calibrate() is None and tr.evaluate() == (-1, -1, -1)
