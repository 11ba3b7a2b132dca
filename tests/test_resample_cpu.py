"""CPU tests of the sample-rate conversion's host side (docs/resample.md): the float64 closed form of tests/resample_oracle.py against
scipy.signal.resample_poly, the phase table ppvector/data_utils/wave_batch.py designs for the kernel, the ppvector.set_resampler
switch, and PPVectorDataset under both resamplers -- the same draws and the same eval order, native-rate samples under 'gpu'."""
import random
import wave

import numpy as np
import pytest
from scipy.signal import resample_poly

import ppvector
from ppvector.data_utils import wave_batch as W
from ppvector.data_utils.featurizer import AudioFeaturizer
from ppvector.data_utils.reader import PPVectorDataset
from ppvector.utils.utils import dict_to_object
from tests import resample_oracle as ro

RATE_PAIRS = tuple((r, 16000) for r in ro.RATES_TO_16K) + ((16000, 8000),)
LENGTHS = (1, 2, 7, 441, 1000, 5003)


@pytest.fixture(autouse=True)
def host_resampler_afterwards():
    yield
    ppvector.set_resampler('host')


@pytest.mark.parametrize('src,dst', RATE_PAIRS)
def test_closed_form_is_resample_poly(src, dst):
    up, down = ro.ratio(src, dst)
    rng = np.random.RandomState(src % 1000)
    for n in LENGTHS:
        x = rng.standard_normal(n)
        want = resample_poly(x, up, down)
        got = ro.closed_form(x, up, down)
        assert got.shape == want.shape == (ro.out_len(n, up, down),)
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (src, dst, n)
        assert W.resample_len(n, up, down) == want.shape[0] and W.resample_ratio(src, dst) == (up, down)
    # a stretch of outputs computed on its own is the same stretch
    x = rng.standard_normal(5003)
    M = ro.out_len(5003, up, down)
    assert np.array_equal(ro.closed_form(x, up, down, M - 50, M), ro.closed_form(x, up, down)[M - 50:])


def test_phase_table_taken_apart_gives_back_the_filter():
    taps = {(2, 1): 21, (1, 3): 61, (160, 441): 56, (320, 441): 28}        # 8 k, 48 k, 44.1 k and 22.05 k -> 16 k
    taps[ro.ratio(11025, 16000)] = 21
    for (up, down), J in taps.items():
        h, half = ro.design(up, down)
        P = W.phase_table(up, down)
        assert P.dtype == np.float32 and P.shape == (up, J) and J == ro.taps_per_phase(up, down) and P.flags['C_CONTIGUOUS']
        flat = P.T.reshape(-1)                                           # flat[p + j up] = P[p][j]
        assert np.array_equal(flat[:2 * half + 1], h.astype(np.float32)) and not flat[2 * half + 1:].any()
        h2, half2 = W.resample_filter(up, down)
        assert half2 == half and np.array_equal(h2, h)
    # the length rule at awkward sizes
    for n, (up, down), M in ((1, (1, 3), 1), (3, (1, 3), 1), (4, (1, 3), 2), (441, (160, 441), 160), (442, (160, 441), 161), (5, (2, 1), 10)):
        assert W.resample_len(n, up, down) == M == resample_poly(np.ones(n), up, down).shape[0]


def test_the_kernel_tile_query():
    from ppvector import _native as N
    lib = N.load_library()
    for up, down in ro.PAIRS + ((1, 6), (441, 160), (147, 640)):
        assert lib.vp_resample_tile(up, down) == 1024
    # where the table and a tile's span would pass 160 KB of LDS the tile shrinks: table + span <= 40960 floats, one more output would not fit
    for up, down in ((1, 1024), (2, 1023), (3, 1024), (1024, 1), (1023, 1024), (7, 1000)):
        T = lib.vp_resample_tile(up, down)
        J = ro.taps_per_phase(up, down)
        table = 0 if up == 1 else up * (J | 1)
        assert 1 <= T <= 1024 and table + (T - 1) * down // up + 1 + J <= 40960, (up, down, T)
        assert T == 1024 or table + T * down // up + 1 + J > 40960, (up, down, T)
    for up, down in ((0, 1), (1, 0), (-1, 2), (1025, 1), (1, 1025)):
        assert lib.vp_resample_tile(up, down) == 0


def test_the_switch_defaults_to_host_and_validates():
    assert ppvector.get_resampler() == 'host'
    ppvector.set_resampler('gpu')
    assert ppvector.get_resampler() == 'gpu'
    for bad in ('cpu', 'GPU', '', None, 1):
        with pytest.raises(ValueError):
            ppvector.set_resampler(bad)
    assert ppvector.get_resampler() == 'gpu'
    ppvector.set_resampler('host')
    assert ppvector.get_resampler() == 'host'


def test_resample_waves_refuses_cpu_tensors():
    import torch
    from ppvector import _native as N
    with pytest.raises(N.VpmiError):
        W.resample_waves([torch.zeros(100)], [8000], 16000)
    with pytest.raises(N.VpmiError):
        W.resample_waves([], [], 16000)


def _wav(path, n, sr, seed, channels=1):
    pcm = (np.random.RandomState(seed).standard_normal((n, channels)) * 3000).astype(np.int16)
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(channels); w.setsampwidth(2); w.setframerate(sr); w.writeframes(pcm.tobytes())


def test_dataset_draws_and_orders_alike_under_both_resamplers(tmp_path):
    fz = AudioFeaturizer('Fbank', dict(sr=16000, n_mels=80))
    #          rate   frames (file)                       seconds
    files = ((8000, 30000), (16000, 70000), (48000, 200001), (48000, 24000), (8000, 2001), (44100, 150000), (16000, 20000), (48000, 96001))
    rows = []
    for i, (sr, n) in enumerate(files):
        _wav(tmp_path / f'u{i}.wav', n, sr, seed=i, channels=2 if i == 5 else 1)
        rows.append(f'{tmp_path}/u{i}.wav\t{i % 3}')
    lst = tmp_path / 'list.txt'
    lst.write_text('\n'.join(rows) + '\n')
    (tmp_path / 'noise').mkdir()
    _wav(tmp_path / 'noise' / 'long.wav', 100000, 16000, seed=50)
    _wav(tmp_path / 'noise' / 'long48.wav', 400000, 48000, seed=51)         # a noise file at another rate: host-resampled in both modes
    aug = dict_to_object(dict(speed=dict(prob=0.7, speed_perturb_3_class=True), volume=dict(prob=0.5, min_gain_dBFS=-15, max_gain_dBFS=15),
                              noise=dict(prob=0.8, noise_dir=str(tmp_path / 'noise'), min_snr_dB=10, max_snr_dB=50), reverb=None, spec_aug=None))
    at_16k = [ro.out_len(n, *ro.ratio(sr, 16000)) for sr, n in files]

    def run(mode):
        ppvector.set_resampler(mode)
        ds = PPVectorDataset(str(lst), fz, max_duration=3, min_duration=0.3, mode='train', aug_conf=aug, num_speakers=3)
        random.seed(11)
        items = [ds[i] for i in range(len(files)) for _ in range(3)]
        ev = PPVectorDataset(str(lst), fz, max_duration=20, min_duration=0.3, mode='eval')
        ex = PPVectorDataset(str(lst), fz, max_duration=100, min_duration=0.3, mode='extract_feature')
        return items, list(ev.lines), [int(l) for l in ev.labels], [ex[i] for i in range(len(files))]

    host, host_order, host_labels, host_ex = run('host')
    gpu, gpu_order, gpu_labels, gpu_ex = run('gpu')
    assert host_order == gpu_order and host_labels == gpu_labels
    assert [host_order.index(r + '\n') for r in rows] == list(np.argsort(np.argsort([m / 16000.0 for m in at_16k], kind='stable')))
    assert len({it['start'] for it in host}) > 3 and len({it['speed'] for it in host}) == 3 and any('noise' in it for it in host)
    for a, b in zip(host, gpu):
        assert set(a) == {'samples', 'speed', 'start', 'gain_dB', 'label'} | ({'noise', 'snr_dB', 'noise_start'} if 'noise' in a else set())
        assert set(b) == set(a) | {'sample_rate'}
        for key in ('speed', 'start', 'gain_dB', 'label', 'snr_dB', 'noise_start'):
            assert a.get(key) == b.get(key), key
        if 'noise' in a:
            assert np.array_equal(a['noise'], b['noise'])
    # 'gpu' items hold the file's own samples; utterance 4 (2001 samples at 8 kHz = 0.25 s) is under min_duration in both modes and
    # falls through to the next entry, file 5 (stereo: the mean of its channels)
    for i, (sr, n) in enumerate(files):
        for it_h, it_g in ((host[3 * i], gpu[3 * i]), (host_ex[i], gpu_ex[i])):
            k = 5 if i == 4 else i
            assert it_g['sample_rate'] == files[k][0] and it_g['samples'].shape == (files[k][1],) and it_g['samples'].dtype == np.float32
            assert it_h['samples'].shape == (at_16k[k],)
            if files[k][0] == 16000:
                assert np.array_equal(it_h['samples'], it_g['samples'])
