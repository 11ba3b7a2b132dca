"""GPU tests of the sample-rate conversion (csrc/resample.hip, ppvector/data_utils/wave_batch.py resample_waves, the 'gpu' resampler in
PPVectorTrainer and PPVectorPredictor; docs/resample.md) against the float64 closed form of tests/resample_oracle.py.

Bounds.  Kernel: max|got - ref64| <= 8 e_cpu32 + 2^-21 max|ref64| per row, e_cpu32 = max|scipy.signal.resample_poly(x32) - ref64| --
the form docs/augment_wave.md uses for reverb: what the host's own float32 path reaches, times a factor for another summation order,
plus the rounding of the table and of the result.  Impulses: bit for bit.  Trainer: max|feature(gpu) - feature(host)| <= 8 e_ref, e_ref
the feature difference between host float32 and host float64 resampling.  Predictor: 1e-4 of cosine 1, the project's score bar."""
import random
import wave

import numpy as np
import pytest
import torch
from scipy.signal import resample_poly

import ppvector
from tests import resample_oracle as ro

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def N():
    from ppvector import _native as N
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    N.load_library()
    return N


@pytest.fixture(autouse=True)
def host_resampler_afterwards():
    yield
    ppvector.set_resampler('host')


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def gpu_resample(xs, up, down):
    """resample_waves on rows that all sit at (up, down): rates (down, up) have that ratio whenever gcd(up, down) = 1."""
    from ppvector.data_utils.wave_batch import resample_waves
    return [y.cpu().numpy() for y in resample_waves([dev(x) for x in xs], [down] * len(xs), up)]


def raw_call(N, srcs, lens, new_lens, dsts, up, down, table, taps=None, B=None, max_new_len=None, null=()):
    """vp_resample_poly_f32 straight through the binding on device tensors the caller laid out; `null` names arguments passed as NULL."""
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device='cuda')
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device='cuda')
    sp, dp, ld, nd = i64([s.data_ptr() for s in srcs]), i64([d.data_ptr() for d in dsts]), i32(lens), i32(new_lens)
    ctx = N.ctx()
    args = dict(ctx=ctx, srcs=sp.data_ptr(), lens=ld.data_ptr(), new_lens=nd.data_ptr(), dsts=dp.data_ptr(), B=len(srcs) if B is None else B,
                max_new_len=max(new_lens) if max_new_len is None else max_new_len, up=up, down=down, table=table.data_ptr(),
                taps=int(table.shape[1]) if taps is None else taps, stream=N.stream_ptr())
    for k in null:
        args[k] = None
    rc = N.lib().vp_resample_poly_f32(*args.values())
    torch.cuda.synchronize()
    return rc


@pytest.fixture(scope='module')
def cases(N):
    """{(up, down): [(x32, ref64, e_cpu32)] over edge_lengths}, computed once and left unchanged."""
    out = {}
    for up, down in ro.PAIRS:
        tile = N.lib().vp_resample_tile(up, down)
        assert tile == 1024
        rng = np.random.RandomState(up * 1000 + down)
        rows = []
        for n in ro.edge_lengths(up, down, tile):
            x = (0.1 * rng.standard_normal(n)).astype(np.float32)
            ref = ro.closed_form(x, up, down)
            cpu32 = resample_poly(x, up, down)
            assert cpu32.dtype == np.float32 and cpu32.shape == ref.shape
            rows.append((x, ref, float(np.max(np.abs(cpu32.astype(np.float64) - ref)))))
        out[(up, down)] = rows
    return out


# ------------------------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize('up,down', ro.PAIRS)
def test_matches_float64_closed_form_at_tile_edges(N, cases, up, down):
    rows = cases[(up, down)]
    tile = N.lib().vp_resample_tile(up, down)
    Ms = [r[1].shape[0] for r in rows]
    assert Ms[0] == ro.out_len(1, up, down) and max(Ms) > 2 * tile and any(tile - 2 <= m < tile for m in Ms) and any(tile < m <= tile + 2 for m in Ms)
    for (x, ref, e_cpu32), got in zip(rows, gpu_resample([r[0] for r in rows], up, down)):
        assert got.dtype == np.float32 and got.shape == ref.shape
        err, top = float(np.max(np.abs(got.astype(np.float64) - ref))), float(np.max(np.abs(ref)))
        print(f'resample ({up}, {down}) n {x.shape[0]} M {ref.shape[0]}: gpu err {err:.3e}  e_cpu32 {e_cpu32:.3e}  max|ref| {top:.3e}  '
              f'err/max|ref| {err / top:.3e}')
        assert err <= 8.0 * e_cpu32 + 2.0 ** -21 * top, (up, down, x.shape[0], err, e_cpu32, top)


# ----------------------------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize('up,down', ro.PAIRS)
def test_unit_impulses_pick_their_table_entries_bit_for_bit(N, up, down):
    """x = delta at sample 0 and at sample n - 1: y[m] is the float32 filter tap h[m down + half - i up] or zero -- one product by 1.0
    and zeros; pins the phase, the centre and both edges."""
    h, half = ro.design(up, down)
    h32 = h.astype(np.float32)
    tile = N.lib().vp_resample_tile(up, down)
    xs, want = [], []
    for n in (1, 2, ro.n_with_out_len(tile + 1, up, down)):
        for at in sorted({0, n - 1}):
            x = np.zeros(n, np.float32)
            x[at] = 1.0
            k = np.arange(ro.out_len(n, up, down), dtype=np.int64) * down + half - at * up
            xs.append(x)
            want.append(np.where((k >= 0) & (k <= 2 * half), h32[np.clip(k, 0, 2 * half)], np.float32(0.0)))
    for x, w, got in zip(xs, want, gpu_resample(xs, up, down)):
        assert got.shape == w.shape and np.array_equal(bits(got), bits(w)), (up, down, x.shape[0], int(np.argmax(x)))
        assert np.count_nonzero(w) >= 1


# ------------------------------------------------------------------------------------------- batch invariance and containment
@pytest.mark.parametrize('up,down', ((160, 441), (1, 3), (2, 1)))
def test_ragged_batch_is_the_single_calls_and_stays_inside_its_rows(N, cases, up, down):
    from ppvector.data_utils.wave_batch import phase_table
    xs = [r[0] for r in cases[(up, down)]]
    singles = [gpu_resample([x], up, down)[0] for x in xs]
    for s, b in zip(singles, gpu_resample(xs, up, down)):
        assert np.array_equal(bits(s), bits(b))
    # every source a slice inside a NaN frame, every destination a slice of a NaN frame: the same bits, the frame untouched
    lens = [x.shape[0] for x in xs]
    new_lens = [ro.out_len(n, up, down) for n in lens]
    gap = 37
    src_frame = torch.full((sum(lens) + gap * (len(xs) + 1),), float('nan'), dtype=torch.float32, device='cuda')
    dst_frame = torch.full((sum(new_lens) + gap * (len(xs) + 1),), float('nan'), dtype=torch.float32, device='cuda')
    srcs, dsts, so, do = [], [], gap, gap
    for x, n, m in zip(xs, lens, new_lens):
        src_frame[so:so + n] = dev(x)
        srcs.append(src_frame[so:so + n])
        dsts.append(dst_frame[do:do + m])
        so, do = so + n + gap, do + m + gap
    table = dev(phase_table(up, down))
    assert raw_call(N, srcs, lens, new_lens, dsts, up, down, table) == N.VP_OK
    for s, d in zip(singles, dsts):
        assert np.array_equal(bits(s), bits(d.cpu().numpy()))
    frame = dst_frame.cpu().numpy()
    inside = np.zeros(frame.shape[0], bool)
    do = gap
    for m in new_lens:
        inside[do:do + m] = True
        do += m + gap
    assert np.isnan(frame[~inside]).all() and not np.isnan(frame[inside]).any() and (~inside).sum() == gap * (len(xs) + 1)


# ------------------------------------------------------------------------------------------------------------ long recording
def test_long_recording_indexes_past_2_31(N):
    """One row with m down > 2^31 at 44.1 kHz -> 16 kHz: the last 4096 outputs against the closed form on the tail."""
    up, down = 160, 441
    M_want = 4_900_000                                              # 4.9e6 x 441 = 2.16e9 > 2^31
    n = ro.n_with_out_len(M_want, up, down)
    M = ro.out_len(n, up, down)
    assert (M - 1) * down > 2 ** 31
    x = (0.1 * np.random.RandomState(5).standard_normal(n)).astype(np.float32)
    got = gpu_resample([x], up, down)[0]
    assert got.shape == (M,)
    ref = ro.closed_form(x, up, down, M - 4096, M)
    # the host's float32 path on a tail that starts on a multiple of `down` samples (its outputs are the whole row's, shifted by a
    # multiple of `up`), far enough back that its own left edge is out of reach
    i0 = (n - 4096 * down // up - 40 * down) // down * down
    cpu32 = resample_poly(x[i0:], up, down)[-4096:]
    e_cpu32 = float(np.max(np.abs(cpu32.astype(np.float64) - ref)))
    err, top = float(np.max(np.abs(got[-4096:].astype(np.float64) - ref))), float(np.max(np.abs(ref)))
    print(f'long row n {n} M {M}: gpu err {err:.3e}  e_cpu32 {e_cpu32:.3e}  max|ref| {top:.3e}')
    assert e_cpu32 < 1e-6 * top                                      # the shifted tail is the same signal
    assert err <= 8.0 * e_cpu32 + 2.0 ** -21 * top
    head = ro.closed_form(x[:4096 * 3 + 200], up, down, 0, 4096)
    assert np.max(np.abs(got[:4096].astype(np.float64) - head)) <= 8.0 * e_cpu32 + 2.0 ** -21 * top


# ------------------------------------------------------------------------------------------------------------------ contract
def test_bad_arguments_return_einval_and_write_nothing(N):
    from ppvector.data_utils.wave_batch import phase_table
    up, down, n = 1, 3, 500
    m = ro.out_len(n, up, down)
    x = dev((0.1 * np.random.RandomState(1).standard_normal(n)).astype(np.float32))
    o = torch.full((m,), 7.0, dtype=torch.float32, device='cuda')
    table = dev(phase_table(up, down))
    good = dict(srcs=[x], lens=[n], new_lens=[m], dsts=[o], up=up, down=down, table=table)
    for name in ('ctx', 'srcs', 'lens', 'new_lens', 'dsts', 'table'):
        assert raw_call(N, **good, null=(name,)) == N.VP_EINVAL, name
    assert b'resample_poly' in N.lib().vp_last_error(N.ctx())
    for bad in (dict(B=0), dict(B=-1), dict(B=65536), dict(max_new_len=0), dict(up=0), dict(up=-1), dict(down=0), dict(down=-3),
                dict(up=1025), dict(down=1025), dict(taps=60), dict(taps=62), dict(taps=0)):
        assert raw_call(N, **{**good, **bad}) == N.VP_EINVAL, bad
    table2 = dev(phase_table(2, 3))                                   # (2, 3) wants ceil(61 / 2) = 31 taps, not (1, 3)'s 61
    assert raw_call(N, **{**good, 'up': 2, 'table': table2, 'taps': 61}) == N.VP_EINVAL
    assert float(o.min()) == 7.0 and float(o.max()) == 7.0
    assert raw_call(N, **good) == N.VP_OK                             # ... and the good call does write
    ref = ro.closed_form(x.cpu().numpy(), up, down)
    assert np.max(np.abs(o.cpu().numpy() - ref)) < 1e-5 * np.max(np.abs(ref))


def test_equal_rates_pass_through_and_a_pair_past_the_cap_takes_the_host_function(N, monkeypatch):
    from ppvector.data_utils import wave_batch as W
    from ppvector.predict import AudioSegment
    rng = np.random.RandomState(9)
    xs = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (3000, 2000, 1000, 4000)]
    waves = [dev(x) for x in xs]
    calls = []
    real = AudioSegment.resample

    def counted(self, rate):
        calls.append((self.sample_rate, rate))
        return real(self, rate)

    monkeypatch.setattr(AudioSegment, 'resample', counted)
    out = W.resample_waves(waves, [16000, 16001, 8000, 16000], 16000)      # 16001 -> 16000: up 16000, down 16001, past the cap of 1024
    assert out[0] is waves[0] and out[3] is waves[3] and calls == [(16001, 16000)]
    host = AudioSegment(xs[1], 16001)
    real(host, 16000)
    assert np.array_equal(bits(out[1].cpu().numpy()), bits(host.samples)) and out[1].is_cuda
    ref = ro.closed_form(xs[2], 2, 1)
    assert out[2].shape == (2000,) and np.max(np.abs(out[2].cpu().numpy() - ref)) < 1e-5 * np.max(np.abs(ref))
    same = W.resample_waves(waves, [16000] * 4, 16000)
    assert all(a is b for a, b in zip(same, waves))
    # a mixed batch: one launch per source rate, every row what its single call gives
    mixed = W.resample_waves(waves, [8000, 48000, 8000, 44100], 16000)
    for x, y, rate in zip(xs, mixed, (8000, 48000, 8000, 44100)):
        single = W.resample_waves([dev(x)], [rate], 16000)[0]
        assert np.array_equal(bits(y.cpu().numpy()), bits(single.cpu().numpy()))
    assert mixed[0].untyped_storage().data_ptr() == mixed[3].untyped_storage().data_ptr()      # views of one allocation


# ------------------------------------------------------------------------------------------------------- trainer end to end
def _write_wav(path, x, sr):
    pcm = np.clip(np.round(np.asarray(x) * 32768.0), -32768, 32767).astype(np.int16)
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr); w.writeframes(pcm.tobytes())


def _trainer_configs(root):
    return dict(
        dataset_conf=dict(dataset=dict(min_duration=0.3, max_duration=3, sample_rate=16000, use_dB_normalization=True, target_dB=-20),
                          sampler=dict(batch_size=4, shuffle=True, drop_last=True), dataLoader=dict(num_workers=2),
                          eval_conf=dict(batch_size=2, max_duration=20),
                          train_list=f'{root}/list.txt', enroll_list=f'{root}/list.txt', trials_list=f'{root}/list.txt',
                          is_use_pksampler=False, sample_per_id=4),
        preprocess_conf=dict(feature_method='Fbank', method_args=dict(sr=16000, n_mels=80)),
        model_conf=dict(model='TDNN', model_args=dict(embd_dim=192, pooling_type='ASP'),
                        classifier=dict(classifier_type='Cosine', num_speakers=3, num_blocks=0)),
        loss_conf=dict(loss='AAMLoss', loss_args=dict(margin=0.2, scale=32, easy_margin=False, label_smoothing=0.0)),
        optimizer_conf=dict(optimizer='Adam', optimizer_args=dict(weight_decay=1e-6), scheduler='WarmupCosineSchedulerLR',
                            scheduler_args=dict(learning_rate=2e-3, min_lr=1e-5, warmup_epoch=1)),
        train_conf=dict(enable_amp=False, max_epoch=1, log_interval=1))


def test_trainer_features_gpu_resampler_vs_host(N, tmp_path):
    """PPVectorTrainer._features over white-noise WAVs at 8 k, 16 k and 48 k: 'gpu' mode against 'host' mode, the bound from the
    host alone (float32 against float64 resampling of the same files, both through the same featurizer)."""
    from ppvector.data_utils.featurizer import AudioFeaturizer
    from ppvector.data_utils.reader import PPVectorDataset
    from ppvector.predict import AudioSegment
    from ppvector.trainer import PPVectorTrainer
    rng = np.random.RandomState(21)
    files = ((8000, 9000), (16000, 20000), (48000, 60001), (8000, 12345), (48000, 40000))
    rows = []
    for i, (sr, n) in enumerate(files):
        _write_wav(tmp_path / f'u{i}.wav', 0.1 * rng.standard_normal(n), sr)
        rows.append(f'{tmp_path}/u{i}.wav\t{i % 3}')
    (tmp_path / 'list.txt').write_text('\n'.join(rows) + '\n')
    tr = PPVectorTrainer(_trainer_configs(str(tmp_path)), use_gpu=True)
    tr.audio_featurizer = AudioFeaturizer('Fbank', dict(sr=16000, n_mels=80))

    def run(mode, samples=None):
        ppvector.set_resampler(mode)
        ds = PPVectorDataset(f'{tmp_path}/list.txt', tr.audio_featurizer, max_duration=3, min_duration=0.3, mode='extract_feature')
        random.seed(4)
        items = [ds[i] for i in range(len(files))]
        if samples is not None:
            items = [dict(it, samples=s) for it, s in zip(items, samples)]
        feats, labels = tr._features(items, ds)
        return items, feats.cpu().numpy(), labels.cpu().numpy(), tr._last_frames

    it_h, f_h, l_h, fr_h = run('host')
    it_g, f_g, l_g, fr_g = run('gpu')
    assert all('sample_rate' not in it for it in it_h) and [it['sample_rate'] for it in it_g] == [sr for sr, _ in files]
    assert [it['samples'].shape[0] for it in it_g] == [n for _, n in files]
    assert f_h.shape == f_g.shape and np.array_equal(l_h, l_g) and fr_h == fr_g and fr_h is not None and len(set(fr_h)) > 1
    # the reference's own error: the same files resampled in float64 and rounded, through the same path
    samples64 = []
    for i, (sr, _) in enumerate(files):
        seg = AudioSegment.from_file(f'{tmp_path}/u{i}.wav')
        up, down = ro.ratio(sr, 16000)
        samples64.append(seg.samples if sr == 16000 else resample_poly(seg.samples.astype(np.float64), up, down).astype(np.float32))
    _, f_64, _, fr_64 = run('host', samples64)
    assert fr_64 == fr_h
    e_ref = float(np.max(np.abs(f_h - f_64)))
    err = float(np.max(np.abs(f_g - f_h)))
    print(f'trainer features: max|gpu - host| {err:.3e}  e_ref (host f32 vs f64 resampling) {e_ref:.3e}  max|feature| {np.max(np.abs(f_h)):.3e}')
    assert e_ref > 0.0 and err <= 8.0 * e_ref, (err, e_ref)


# ----------------------------------------------------------------------------------------------------- predictor end to end
@pytest.fixture(scope='module')
def predictor():
    from oracle import models as om
    from ppvector.predict import PPVectorPredictor
    from ppvector.utils.utils import dict_to_object
    cfg = dict_to_object(dict(
        dataset_conf=dict(dataset=dict(min_duration=0.3, max_duration=3, sample_rate=16000, use_dB_normalization=True, target_dB=-20)),
        preprocess_conf=dict(feature_method='Fbank', method_args=dict(sr=16000, n_mels=80)),
        model_conf=dict(model='EcapaTdnn', model_args=dict(embd_dim=192, pooling_type='ASP', channels=[512, 512, 512, 512, 1536]))))
    state = {'0.' + k: v for k, v in om.ecapa_params(80, seed=1000).items()}
    return PPVectorPredictor(cfg, model_path=state)


def _cos(a, b):
    return float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))


def _refuse(*a, **k):
    raise AssertionError('scipy.signal.resample_poly was called under the gpu resampler')


def test_predictor_gpu_resampler_scores_as_host(N, predictor, monkeypatch):
    import scipy.signal
    from oracle import fbank as ofb
    from ppvector.predict import AudioSegment
    w8, w16, w48 = (ofb.synth_waves(1, n, seed=s, lowpass=0.9)[0] for n, s in ((16000, 31), (40000, 32), (120000, 33)))
    segments = lambda: [AudioSegment(w8.copy(), 8000), AudioSegment(w16.copy(), 16000), AudioSegment(w48.copy(), 48000)]
    host_single = [predictor.predict(w8.copy(), sample_rate=8000), predictor.predict(w48.copy(), sample_rate=48000)]
    host_at_rate = predictor.predict_batch([w8.copy(), w16.copy(), w48.copy()], sample_rate=16000)      # all at the dataset's rate
    host_mixed = predictor.predict_batch(segments())
    ppvector.set_resampler('gpu')
    monkeypatch.setattr(scipy.signal, 'resample_poly', _refuse)
    gpu_single = [predictor.predict(w8.copy(), sample_rate=8000), predictor.predict(w48.copy(), sample_rate=48000)]
    # input at the dataset's rate takes today's path, bit for bit; other rates are converted on the device, among rows that are not
    assert np.array_equal(predictor.predict_batch([w8.copy(), w16.copy(), w48.copy()], sample_rate=16000), host_at_rate)
    gpu_mixed = predictor.predict_batch(segments())
    assert gpu_mixed.shape == host_mixed.shape == (3, 192)
    for name, hs, gs in (('predict', host_single, gpu_single), ('predict_batch', host_mixed, gpu_mixed)):
        for h, g in zip(hs, gs):
            print(f'{name}: 1 - cos(host, gpu) = {1.0 - _cos(h, g):.3e}')
            assert abs(1.0 - _cos(h, g)) <= 1e-4


def test_diarization_gpu_resampler_returns_the_host_segments(N, predictor, monkeypatch):
    import scipy.signal
    from oracle import fbank as ofb
    a, b = ofb.synth_waves(2, 240000, seed=41, lowpass=0.97), ofb.synth_waves(2, 240000, seed=42, lowpass=0.5)
    rec = np.concatenate([a[0], b[0], 0.5 * a[1], 2.0 * b[1]]).astype(np.float32)      # 20 s at 48 kHz: two dark and two bright stretches
    vad = [(0.5, 9.0), (10.0, 19.2), (19.4, 19.9)]
    host = predictor.speaker_diarization(rec.copy(), sample_rate=48000, speaker_num=2, vad_segments=vad)
    ppvector.set_resampler('gpu')
    monkeypatch.setattr(scipy.signal, 'resample_poly', _refuse)
    gpu = predictor.speaker_diarization(rec.copy(), sample_rate=48000, speaker_num=2, vad_segments=vad)
    assert len(host) >= 2 and gpu == host
