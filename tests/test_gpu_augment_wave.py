"""GPU tests of the noise / reverb waveform augmentation (csrc/augment.hip noise_mix_kernel, csrc/reverb.hip;
ppvector/data_utils/wave_batch.py noise_perturb / reverb_perturb; the reference's reader.py:159-162) against the float64 oracle
tests/augment_wave_oracle.py: the kernels alone, the chain in front of assemble_waves, the trainer with both libraries
configured, and the argument checks of the C ABI.

Bounds.  Noise: max|got - ref| <= 1e-5 max|ref| per utterance -- two f32 tree reductions over at most 5 000 values and one
exp10f stay under 2e-6 relative.  Reverb: measured in the test against what a float32 FFT convolution on the CPU reaches,
max|got - ref64| <= 8 e_cpu32 + 2^-21 max|ref64| with e_cpu32 = max|scipy.signal.fftconvolve(x32, h32)[:n] - ref64| (the factor
covers f32 twiddle tables and another summation order over the partitions).  The case sizes sit on the edges of the
partition P = 2048."""
import logging
import wave

import numpy as np
import pytest
import torch

from tests import augment_wave_oracle as ow

pytestmark = pytest.mark.gpu

P = 2048
REVERB_SHAPES = ((1, 1), (P - 1, 1), (P, P), (P + 1, P + 1), (5000, 3000), (2 * P + 1, 3 * P + 1))


@pytest.fixture(scope='module')
def N():
    from ppvector import _native as N
    assert torch.cuda.is_available(), 'GPU tests need a visible MI355X'
    N.load_library()
    return N


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _rir(rng, Lr):
    """An exponentially decaying Gaussian response, unit energy in float64, stored float32 (what the reader hands over)."""
    h = rng.standard_normal(Lr) * np.exp(-np.arange(Lr) / (0.15 * Lr + 1.0))
    return ow.unit_energy(h).astype(np.float32)


@pytest.fixture(scope='module')
def reverb_cases():
    """[(x32, h32, ref64, e_cpu32)] for REVERB_SHAPES, computed once and left unchanged."""
    from scipy.signal import fftconvolve
    rng = np.random.RandomState(77)
    cases = []
    for n, Lr in REVERB_SHAPES:
        x = (0.1 * rng.standard_normal(n)).astype(np.float32)
        h = _rir(rng, Lr)
        ref = ow.convolve_cut(x, h)
        cpu32 = fftconvolve(x, h)[:n]
        assert cpu32.dtype == np.float32
        cases.append((x, h, ref, float(np.max(np.abs(cpu32.astype(np.float64) - ref)))))
    return cases


# ----------------------------------------------------------------------------------------------------------------- noise
def test_noise_perturb_matches_oracle_in_one_ragged_launch(N):
    from ppvector.data_utils.wave_batch import noise_perturb
    rng = np.random.RandomState(31)
    #        n     Ln    start  snr_dB
    spec = ((1000, 300, 0, 10.0),          # shorter file: wrap-padded, level over the padded n samples
            (1000, 1000, 0, 30.0),         # the same length: the whole file
            (1000, 5000, 3999, 50.0),      # longer file: a segment, level over the WHOLE file
            (257, 1, 0, 10.0),             # a one-sample file
            (1000, 300, 0, 30.0))          # an all-zero utterance: the 1e-20 floor of rms_dB
    xs = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n, _, _, _ in spec]
    xs[4][:] = 0.0
    nzs = [(0.05 * rng.standard_normal(Ln) + 0.01).astype(np.float32) for _, Ln, _, _ in spec]
    # rows 1 and 4 of the launch are not selected
    order = [0, None, 1, 2, None, 3, 4]
    plain = (0.1 * rng.standard_normal(777)).astype(np.float32)
    waves = [dev(plain) if k is None else dev(xs[k]) for k in order]
    noises = [None if k is None else dev(nzs[k]) for k in order]
    snrs = [0.0 if k is None else spec[k][3] for k in order]
    starts = [0 if k is None else spec[k][2] for k in order]
    out = noise_perturb(waves, noises, snrs, starts)
    torch.cuda.synchronize()
    assert len(out) == len(order)
    for row, k in enumerate(order):
        if k is None:
            assert out[row] is waves[row]
            continue
        assert out[row] is not waves[row] and out[row].dtype == torch.float32 and out[row].shape == waves[row].shape
        assert torch.equal(waves[row].cpu(), torch.from_numpy(xs[k]))                      # the source is left alone
        ref = ow.add_noise(xs[k], nzs[k], spec[k][3], spec[k][2])
        err, top = float(np.max(np.abs(out[row].cpu().numpy().astype(np.float64) - ref))), float(np.max(np.abs(ref)))
        print(f'noise case {k}: n={spec[k][0]} Ln={spec[k][1]} err/max|ref| = {err / top:.3e}')
        assert top > 0.0 and err <= 1e-5 * top, (k, err, top)
    with pytest.raises(N.VpmiError):
        noise_perturb([torch.zeros(10)], [torch.zeros(4)], [10.0], [0])
    with pytest.raises(N.VpmiError):
        noise_perturb([torch.zeros(10).cuda()], [torch.zeros(4)], [10.0], [0])


# ---------------------------------------------------------------------------------------------------------------- reverb
def _check_reverb(got, case, tag):
    x, h, ref, e32 = case
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == x.shape
    err, top = float(np.max(np.abs(got.astype(np.float64) - ref))), float(np.max(np.abs(ref)))
    bound = 8.0 * e32 + 2.0 ** -21 * top
    print(f'reverb {tag} n={len(x)} Lr={len(h)}: err/max|ref| = {err / top:.3e}  e_cpu32/max|ref| = {e32 / top:.3e}  bound/max|ref| = {bound / top:.3e}')
    assert err <= bound, (tag, len(x), len(h), err, bound)


@pytest.fixture(scope='module')
def reverb_singles(reverb_cases):
    """Every case run alone: [tensor]."""
    from ppvector.data_utils.wave_batch import reverb_perturb
    outs = []
    for x, h, _, _ in reverb_cases:
        w = dev(x)
        o = reverb_perturb([w], [dev(h)])[0]
        assert o is not w
        outs.append(o)
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize('i', range(len(REVERB_SHAPES)), ids=[f'n{n}-Lr{Lr}' for n, Lr in REVERB_SHAPES])
def test_reverb_single_utterance_matches_float64(N, reverb_cases, reverb_singles, i):
    _check_reverb(reverb_singles[i], reverb_cases[i], 'single')


def test_reverb_ragged_batch_is_bit_identical_and_reads_only_what_it_wrote(N, reverb_cases, reverb_singles):
    from ppvector.data_utils import wave_batch as wb
    plain = dev(np.linspace(-1, 1, 333, dtype=np.float32))
    waves = [dev(c[0]) for c in reverb_cases] + [plain]
    rirs = [dev(c[1]) for c in reverb_cases] + [None]
    out = wb.reverb_perturb(waves, rirs)
    torch.cuda.synchronize()
    assert out[-1] is plain                                                                 # not selected: the same object
    for i, case in enumerate(reverb_cases):
        assert out[i] is not waves[i] and torch.equal(waves[i].cpu(), torch.from_numpy(case[0]))
        _check_reverb(out[i], case, 'batched')
        assert torch.equal(out[i], reverb_singles[i]), f'case {i}: batched differs from the single-utterance launch'
    # once more over a workspace full of NaN: nothing may change
    assert wb._reverb_ws.bufs
    for buf in wb._reverb_ws.bufs.values():
        buf[:buf.numel() // 4 * 4].view(torch.float32).fill_(float('nan'))
    again = wb.reverb_perturb(waves, rirs)
    torch.cuda.synchronize()
    for i in range(len(reverb_cases)):
        assert torch.equal(again[i], out[i]), f'case {i}: the result depends on the workspace\'s old contents'
    with pytest.raises(N.VpmiError):
        wb.reverb_perturb([torch.zeros(10)], [torch.zeros(4)])


# -------------------------------------------------------------------------------------------------------------- pipeline
def test_noise_reverb_then_assemble_waves_normalises_the_augmented_signal(N):
    """noise_perturb -> reverb_perturb -> assemble_waves against oracle.augment.wave_batch over the oracle-augmented waves:
    the dB normalisation must see the AUGMENTED signal's level (the reference augments before it normalises, reader.py:94-98).
    Tolerance: the one assemble_waves' own test uses (tests/test_gpu_kernels.py)."""
    from oracle import augment as oa
    from ppvector.data_utils.wave_batch import assemble_waves, noise_perturb, reverb_perturb
    rng = np.random.RandomState(41)
    lens = (30000, 16001, 52000)
    xs = [(s * rng.standard_normal(n)).astype(np.float32) for n, s in zip(lens, (0.1, 0.02, 0.3))]
    nzs = [(0.2 * rng.standard_normal(7001)).astype(np.float32), None, (0.05 * rng.standard_normal(60000)).astype(np.float32)]
    snrs, nstarts = [12.0, 0.0, 25.0], [0, 0, 4321]
    hs = [None, _rir(rng, 3000), _rir(rng, 5000)]
    starts = [100, 0, 4000]
    aug = []
    for x, z, snr, ns, h in zip(xs, nzs, snrs, nstarts, hs):
        y = np.asarray(x, np.float64) if z is None else ow.add_noise(x, z, snr, ns)
        aug.append(y if h is None else ow.convolve_cut(y, h))
    ref, nv = oa.wave_batch(aug, L=48000, starts=starts, normalize=True, target_db=-20.0)
    plain, _ = oa.wave_batch(xs, L=48000, starts=starts, normalize=True, target_db=-20.0)
    waves = [dev(x) for x in xs]
    waves = noise_perturb(waves, [None if z is None else dev(z) for z in nzs], snrs, nstarts)
    waves = reverb_perturb(waves, [None if h is None else dev(h) for h in hs])
    out, ratio = assemble_waves(waves, max_len=48000, starts=starts, target_dB=-20.0)
    got = out.cpu().numpy()
    err, top = float(np.max(np.abs(got - ref))), float(np.max(np.abs(ref)))
    print(f'pipeline: err/max|ref| = {err / top:.3e}')
    assert err < 5e-6 * top, (err, top)
    assert np.array_equal((ratio.cpu().numpy() * 48000).round().astype(np.int32), nv)
    assert np.max(np.abs(plain - ref)) > 1e-2 * top                                        # the augmentation is not a no-op here


# --------------------------------------------------------------------------------------------------------------- trainer
def _write_wav(path, pcm, sr=16000):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr); w.writeframes(np.asarray(pcm, np.int16).tobytes())


def _configs(root, max_epoch):
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
        train_conf=dict(enable_amp=False, max_epoch=max_epoch, log_interval=1))


def test_trainer_trains_with_noise_and_reverb_libraries(golden_dir, tmp_path, caplog, monkeypatch):
    """Two TDNN training steps with a noise directory of two WAVs and a reverb directory of one, both at prob 1: every utterance goes
    through both kernels, the loss stays finite and nothing is reported as not built."""
    import ppvector.trainer as T
    root = str(tmp_path)
    pcm = np.load(f'{golden_dir}/wavs_3s.npz')['pcm']                       # a_1, a_2, b_1, b_2 (3 s each)
    train = []
    for spk, rows in ((0, (0, 1)), (1, (2, 3))):
        for r in rows:
            for k, (a, b) in enumerate(((0, 48000), (4000, 44000))):
                p = f'{root}/s{spk}_{r}_{k}.wav'
                _write_wav(p, pcm[r, a:b])
                train.append(f'{p}\t{spk}')
    for name, rows in (('enroll', ((0, 0), (2, 1))), ('trials', ((1, 0), (3, 1)))):
        lines = []
        for r, spk in rows:
            p = f'{root}/{name}_{r}.wav'
            _write_wav(p, pcm[r])
            lines.append(f'{p}\t{spk}')
        open(f'{root}/{name}_list.txt', 'w').write('\n'.join(lines) + '\n')
    open(f'{root}/train_list.txt', 'w').write('\n'.join(train) + '\n')
    rng = np.random.RandomState(3)
    import os
    os.makedirs(f'{root}/noise')
    os.makedirs(f'{root}/reverb')
    _write_wav(f'{root}/noise/short.wav', rng.standard_normal(9000) * 2000)                # wrap-padded under every utterance
    _write_wav(f'{root}/noise/long.wav', rng.standard_normal(80000) * 500)                 # a random segment
    _write_wav(f'{root}/reverb/room.wav', rng.standard_normal(6000) * np.exp(-np.arange(6000) / 900.0) * 9000)
    aug = dict(speed=dict(prob=0.0), volume=dict(prob=0.0, min_gain_dBFS=-15, max_gain_dBFS=15),
               noise=dict(prob=1.0, noise_dir=f'{root}/noise', min_snr_dB=10, max_snr_dB=50),
               reverb=dict(prob=1.0, reverb_dir=f'{root}/reverb'),
               spec_aug=dict(prob=0.5, freq_mask_ratio=0.1, n_freq_masks=1, time_mask_ratio=0.05, n_time_masks=1, max_time_warp=0))
    seen = dict(noise=0, rir=0)
    real_noise, real_reverb = T.noise_perturb, T.reverb_perturb

    def count_noise(waves, noises, snrs, starts):
        seen['noise'] += sum(z is not None for z in noises)
        return real_noise(waves, noises, snrs, starts)

    def count_reverb(waves, rirs):
        seen['rir'] += sum(h is not None for h in rirs)
        return real_reverb(waves, rirs)

    monkeypatch.setattr(T, 'noise_perturb', count_noise)
    monkeypatch.setattr(T, 'reverb_perturb', count_reverb)
    log = logging.getLogger('ppvector')
    log.addHandler(caplog.handler)
    try:
        with caplog.at_level(logging.WARNING, logger='ppvector'):
            tr = T.PPVectorTrainer(_configs(root, 1), use_gpu=True, data_augment_configs=aug)
            tr.train(save_model_path=f'{root}/models', resume_model=None, pretrained_model=None, do_eval=False)
    finally:
        log.removeHandler(caplog.handler)
    assert tr.train_step == 2 and tr.train_loss is not None and np.isfinite(tr.train_loss)
    assert seen == dict(noise=8, rir=8)
    assert tr.train_dataset.noise_conf is not None and len(tr.train_dataset.noise_conf['files']) == 2
    assert not any('not built' in r.getMessage() for r in caplog.records)


# ------------------------------------------------------------------------------------------------------- argument errors
def test_bad_arguments_return_einval_and_write_nothing(N):
    lib = N.lib()
    ctx = N.ctx()
    n, Ln = 500, 100
    x = dev((0.1 * np.random.RandomState(1).standard_normal(n)).astype(np.float32))
    z = dev((0.1 * np.random.RandomState(2).standard_normal(Ln)).astype(np.float32))
    o = torch.full((n,), 7.0, dtype=torch.float32, device='cuda')
    i64 = lambda v: torch.tensor([v], dtype=torch.int64, device='cuda')
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device='cuda')
    sp, zp, dp, ld, zd, sd = i64(x.data_ptr()), i64(z.data_ptr()), i64(o.data_ptr()), i32(n), i32(Ln), i32(0)
    snr = torch.tensor([20.0], dtype=torch.float32, device='cuda')
    st = N.stream_ptr()
    good = [ctx, sp.data_ptr(), ld.data_ptr(), zp.data_ptr(), zd.data_ptr(), sd.data_ptr(), snr.data_ptr(), dp.data_ptr(), 1, st]
    for pos in (1, 2, 3, 4, 6, 7):                                                           # each required pointer as NULL
        args = list(good)
        args[pos] = None
        assert lib.vp_noise_mix_f32(*args) == N.VP_EINVAL
        assert b'noise_mix' in lib.vp_last_error(ctx)
    for B in (0, -1, 65536):
        args = list(good)
        args[8] = B
        assert lib.vp_noise_mix_f32(*args) == N.VP_EINVAL
    assert lib.vp_noise_mix_f32(None, *good[1:]) == N.VP_EINVAL
    torch.cuda.synchronize()
    assert float(o.min()) == 7.0 and float(o.max()) == 7.0
    assert lib.vp_noise_mix_f32(*good) == N.VP_OK                                            # ... and the good call does write
    torch.cuda.synchronize()
    assert float((o - 7.0).abs().min()) > 0.0

    o.fill_(7.0)
    need = int(lib.vp_reverb_workspace_bytes(1, n, Ln))
    assert need == 1 * (1 + 1) * 2056 * 8
    assert lib.vp_reverb_workspace_bytes(0, n, Ln) == 0 and lib.vp_reverb_workspace_bytes(1, 0, Ln) == 0
    assert lib.vp_reverb_workspace_bytes(3, 2 * P + 1, P) == 3 * (3 + 1) * 2056 * 8
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    good = [ctx, sp.data_ptr(), ld.data_ptr(), zp.data_ptr(), zd.data_ptr(), dp.data_ptr(), 1, n, Ln, ws.data_ptr(), need, st]
    for pos in (1, 2, 3, 4, 5, 9):
        args = list(good)
        args[pos] = None
        assert lib.vp_reverb_f32(*args) == N.VP_EINVAL
        assert b'reverb' in lib.vp_last_error(ctx)
    for pos, bad in ((6, 0), (6, 65536), (7, 0), (8, 0), (10, need - 1)):                    # B, max_len, max_rir_len, a byte short
        args = list(good)
        args[pos] = bad
        assert lib.vp_reverb_f32(*args) == N.VP_EINVAL
    assert lib.vp_reverb_f32(None, *good[1:]) == N.VP_EINVAL
    torch.cuda.synchronize()
    assert float(o.min()) == 7.0 and float(o.max()) == 7.0 and int(ws.max()) == 0
    assert lib.vp_reverb_f32(*good) == N.VP_OK
    torch.cuda.synchronize()
    ref = ow.convolve_cut(x.cpu().numpy(), z.cpu().numpy())
    assert np.max(np.abs(o.cpu().numpy() - ref)) < 1e-5 * np.max(np.abs(ref))
