"""CPU tests of the noise / reverb augmentation's host side: the float64 oracle (tests/augment_wave_oracle.py) checked against
closed forms, and the draws PPVectorDataset.__getitem__ makes for them (ppvector/data_utils/reader.py; the reference's
reader.py:159-162).  No GPU: items are raw host data."""
import random
import wave

import numpy as np

from ppvector.data_utils.featurizer import AudioFeaturizer
from ppvector.data_utils.reader import PPVectorDataset
from ppvector.utils.utils import dict_to_object
from tests import augment_wave_oracle as ow


def _wav(path, pcm, sr=16000):
    pcm = np.asarray(pcm, np.int16)
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1 if pcm.ndim == 1 else pcm.shape[1]); w.setsampwidth(2); w.setframerate(sr); w.writeframes(pcm.tobytes())


def _noise_pcm(n, seed, scale=3000):
    return (np.random.RandomState(seed).standard_normal(n) * scale).astype(np.int16)


# --------------------------------------------------------------------------------------------------------- oracle self-checks
def test_oracle_reverb_closed_forms():
    x = np.random.RandomState(0).standard_normal(50)
    assert np.array_equal(ow.reverb(x, [1.0]), x)                                    # a unit impulse is the identity
    d = ow.reverb(x, [0.0, 0.0, 1.0])                                                # [0, 0, 1] delays by two samples
    assert np.array_equal(d[:2], [0.0, 0.0]) and np.array_equal(d[2:], x[:-2])
    rir = np.random.RandomState(1).standard_normal(17) * np.exp(-np.arange(17) / 4.0)
    assert np.max(np.abs(ow.reverb(x, 37.5 * rir) - ow.reverb(x, rir))) < 1e-12     # the response's scale does not matter
    assert abs(float(np.sum(ow.unit_energy(rir) ** 2)) - 1.0) < 1e-12
    assert np.array_equal(ow.reverb(x, np.zeros(9)), x)                              # an all-zero response: untouched


def test_oracle_add_noise_realises_the_snr():
    rng = np.random.RandomState(2)
    x = 0.1 * rng.standard_normal(1000)
    for Ln, snr in ((300, 10.0), (1, 30.0), (999, 50.0)):                            # Ln < n: wrap-padded, level over those n samples
        noise = 0.3 * rng.standard_normal(Ln) + 0.01
        added = ow.add_noise(x, noise, snr, 0) - x
        assert np.allclose(added / added[0] * noise[0], noise[np.arange(1000) % Ln], rtol=1e-9, atol=1e-12)
        realised = 10.0 * np.log10(np.mean(x * x) / np.mean(added * added))
        assert abs(realised - snr) < 1e-9, (Ln, realised)
    # Ln >= n: the level is the WHOLE file's, the segment starts at `start`
    noise = 0.2 * rng.standard_normal(5000)
    y = ow.add_noise(x, noise, 20.0, 3999)
    g = 10.0 ** ((ow.rms_db(x) - ow.rms_db(noise) - 20.0) / 20.0)
    assert np.max(np.abs(y - (x + g * noise[3999:4999]))) < 1e-15
    assert abs(ow.noise_gain_db(np.zeros(10), noise, 10.0) - (-200.0 - ow.rms_db(noise) - 10.0)) < 1e-12      # silence: the 1e-20 floor
    assert ow.noise_gain_db(np.ones(10), np.zeros(4), -200.0) == 300.0               # the clamp: 0 - (-200) + 200 = 400 dB -> 300


# ------------------------------------------------------------------------------------------------------------ reader draws
def _dataset(tmp_path, aug, lens=(48000, 20000, 70000)):
    fz = AudioFeaturizer('Fbank', dict(sr=16000, n_mels=80))
    rows = []
    for i, n in enumerate(lens):
        _wav(tmp_path / f'u{i}.wav', _noise_pcm(n, i))
        rows.append(f'{tmp_path}/u{i}.wav\t{i % 3}')
    lst = tmp_path / 'list.txt'
    lst.write_text('\n'.join(rows) + '\n')
    return PPVectorDataset(str(lst), fz, max_duration=3, min_duration=0.3, mode='train', aug_conf=dict_to_object(aug), num_speakers=3)


def test_reader_draws_noise_and_reverb(tmp_path):
    nd, rd = tmp_path / 'noise', tmp_path / 'reverb'
    (nd / 'sub').mkdir(parents=True)
    rd.mkdir()
    _wav(nd / 'short.wav', _noise_pcm(5000, 10))                                     # shorter than every utterance: wrap-padded
    _wav(nd / 'sub' / 'long.wav', _noise_pcm(100000, 11))                            # longer than every utterance: a random segment
    (nd / 'readme.txt').write_text('not audio')
    t = np.arange(400)
    left = (np.random.RandomState(12).standard_normal(400) * np.exp(-t / 80.0) * 8000).astype(np.int16)
    _wav(rd / 'room.wav', np.stack([left, np.zeros(400, np.int16)], axis=1), sr=8000)    # stereo, 8 kHz
    aug = dict(speed=dict(prob=1.0, speed_perturb_3_class=False), volume=None,
               noise=dict(prob=1.0, noise_dir=str(nd), min_snr_dB=10, max_snr_dB=50), reverb=dict(prob=1.0, reverb_dir=str(rd)), spec_aug=None)
    ds = _dataset(tmp_path, aug)
    assert [p[len(str(nd)) + 1:] for p in ds.noise_conf['files']] == ['short.wav', 'sub/long.wav'] and len(ds.reverb_conf['files']) == 1
    random.seed(5)
    seen = set()
    for k in range(30):
        it = ds[k % 3]
        n = it['samples'].shape[0] if it['speed'] == 1.0 else int(it['samples'].shape[0] / it['speed'])     # the perturbed length
        assert it['noise'].dtype == np.float32 and it['noise'].ndim == 1 and 10.0 <= it['snr_dB'] <= 50.0
        Ln = it['noise'].shape[0]
        assert Ln in (5000, 100000)
        seen.add(Ln)
        if Ln < n:
            assert it['noise_start'] == 0
        else:
            assert isinstance(it['noise_start'], int) and 0 <= it['noise_start'] <= Ln - n
        h = it['rir']
        assert h.dtype == np.float32 and h.ndim == 1 and abs(float(np.sum(h.astype(np.float64) ** 2)) - 1.0) < 1e-6
        assert abs(h.shape[0] - 800) <= 1                                            # 400 samples at 8 kHz -> 16 kHz, one channel
        assert set(it) == {'samples', 'speed', 'start', 'gain_dB', 'label', 'noise', 'snr_dB', 'noise_start', 'rir'}
    assert seen == {5000, 100000}
    starts = {ds[1]['noise_start'] for _ in range(40)}                               # 20 000-sample utterance: both files get drawn
    assert len(starts) > 5
    # the first channel alone, not the channel mean: the silent right channel would halve the response before the scaling hides it,
    # so compare with the decoded left channel directly
    from ppvector.predict import AudioSegment
    seg = AudioSegment(left, 8000)
    seg.resample(16000)
    ref = ow.unit_energy(seg.samples).astype(np.float32)
    assert np.max(np.abs(ds[0]['rir'] - ref)) < 1e-6
    # eval mode never augments
    fz = AudioFeaturizer('Fbank', dict(sr=16000, n_mels=80))
    ev = PPVectorDataset(str(tmp_path / 'list.txt'), fz, max_duration=20, mode='eval', aug_conf=dict_to_object(aug))
    assert set(ev[0]) == {'samples', 'speed', 'start', 'gain_dB', 'label'}


def test_all_zero_rir_is_dropped(tmp_path):
    rd = tmp_path / 'reverb'
    rd.mkdir()
    _wav(rd / 'dead.wav', np.zeros(100, np.int16))
    ds = _dataset(tmp_path, dict(speed=None, volume=None, noise=None, reverb=dict(prob=1.0, reverb_dir=str(rd)), spec_aug=None))
    assert ds.reverb_conf is not None and 'rir' not in ds[0]


def test_no_stray_random_draws_without_libraries(tmp_path):
    """Sections at prob 0, or pointing at empty / missing directories, consume no random number: a seeded run draws what a run with
    noise=None, reverb=None draws."""
    empty = tmp_path / 'empty'
    empty.mkdir()
    (empty / 'notes.txt').write_text('no audio here')
    full = tmp_path / 'full'
    full.mkdir()
    _wav(full / 'n.wav', _noise_pcm(3000, 20))
    base = dict(speed=dict(prob=0.7, speed_perturb_3_class=True), volume=dict(prob=0.6, min_gain_dBFS=-15, max_gain_dBFS=15), spec_aug=None)
    variants = dict(
        none=dict(noise=None, reverb=None),
        prob0=dict(noise=dict(prob=0.0, noise_dir=str(full), min_snr_dB=10, max_snr_dB=50), reverb=dict(prob=0.0, reverb_dir=str(full))),
        empty=dict(noise=dict(prob=1.0, noise_dir=str(empty), min_snr_dB=10, max_snr_dB=50), reverb=dict(prob=1.0, reverb_dir=str(empty))),
        missing=dict(noise=dict(prob=1.0, noise_dir=str(tmp_path / 'nowhere')), reverb=dict(prob=1.0, reverb_dir='')))
    seqs = {}
    for name, extra in variants.items():
        ds = _dataset(tmp_path, dict(base, **extra))
        assert ds.noise_conf is None and ds.reverb_conf is None
        random.seed(11)
        items = [ds[k % 3] for k in range(24)]
        assert all('noise' not in it and 'rir' not in it for it in items)
        seqs[name] = [(it['start'], it['gain_dB'], it['speed'], it['label']) for it in items]
    assert len({s[0] for s in seqs['none']}) > 3                                     # the sequence does exercise the crop draw
    assert seqs['prob0'] == seqs['none'] and seqs['empty'] == seqs['none'] and seqs['missing'] == seqs['none']
