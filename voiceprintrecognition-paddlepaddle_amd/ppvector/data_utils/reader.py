"""Dataset of the training / evaluation lists (ppvector/data_utils/reader.py:16-163), re-cut for a GPU front end.

The reference's __getitem__ runs, per utterance on a CPU worker: decode -> resample -> waveform augmentation -> dB
normalisation -> crop -> Fbank -> SpecAugment (reader.py:72-109).  Here the worker threads only decode / resample and draw
the random numbers (crop start, volume gain); everything from the dB normalisation on runs batched on the MI355X
(data_utils/wave_batch.py -> AudioFeaturizer -> SpecAugmentor.batch).  __getitem__ therefore returns the RAW utterance:

    audio list entry  -> dict(samples float32 (n,), speed float, start int, gain_dB float, label int
                              [, noise float32 (Ln,), snr_dB float, noise_start int] [, rir float32 (Lr,), unit energy])
    '.npy' list entry -> dict(feature float32 (T, F) cropped to max_feature_len (:78-83), label int)

Under ppvector.set_resampler('gpu') (docs/resample.md) the workers do not resample either: `samples` are at the file's own rate and
the item carries one more key, `sample_rate`; the trainer converts the uploaded batch (wave_batch.resample_waves).  Every length used
here -- the min_duration check, the length after the speed change, the noise start, the crop start -- is then ceil(n up / down), the
length resample_poly would have given, so the same seed draws the same numbers in both modes, and the eval-mode sort reads each WAV
header's frame count instead of decoding the file.  Noise and impulse-response files keep the host conversion in both modes: the
responses are cached after their float64 scaling and the noise level rule is stated on the decoded, resampled file.

List format, min_duration skipping (:89-91), the eval-mode length sort (:121-139), train-mode random crop (yeaudio
AudioSegment.crop: a uniform random start, 0 otherwise) follow the reference.  Speed perturbation (SpeedPerturbAugmentor:
rate drawn from {1.0, 0.9, 1.1}, optional 3-class label offset) is drawn here and applied on the GPU; the crop start is drawn on
the PERTURBED length, as the reference crops after it augments.  Noise and reverb perturbation (NoisePerturbAugmentor /
ReverbPerturbAugmentor, reader.py:159-162; yeaudio is third party and not installed: restated from its published behaviour
[3P-memory], PARITY UNPINNED) are drawn here in the reference's order -- after speed and volume, before the crop: the noise
file, snr_dB = uniform(min_snr_dB, max_snr_dB) and the segment start (int(uniform(0, Ln/sr - n/sr) * sr) on the perturbed
length n; 0 and no draw when the file is shorter and gets wrap-padded), then the impulse-response file.  The worker decodes
the chosen files (first channel, resampled to the dataset's rate), scales the impulse response to unit energy in float64
(an all-zero one is dropped: the utterance stays as it is) and hands them over; the mix and the convolution run on the GPU
(data_utils/wave_batch.py noise_perturb / reverb_perturb).  An augmentor whose section is None, whose prob is <= 0 or whose
directory is missing or holds no WAV file draws nothing, as upstream's is a no-op without its library.
Volume: the reference applies the volume gain BEFORE noise and reverb; the noise gain is relative to the utterance's level and
the convolution is linear, so the whole result just scales by that gain (the 300 dB clamp never binds on real audio).  The
gain therefore stays where it was: applied by vp_wave_batch_f32 when dB normalisation is off, ignored when it is on.
"""
import os
import random
import threading

import wave

import numpy as np

import ppvector
from ppvector.data_utils.wave_batch import SPEEDS, resample_len, resample_ratio
from ppvector.predict import AudioSegment


def _wav_files(root):
    """Every WAV file under root, recursive, sorted (the order the host's file draw indexes)."""
    return sorted(os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs if f.lower().endswith('.wav'))


class PPVectorDataset:
    def __init__(self, data_list_path, audio_featurizer, max_duration=3, min_duration=0.5, mode='train', sample_rate=16000,
                 aug_conf=None, num_speakers=None, use_dB_normalization=True, target_dB=-20):
        assert mode in ['train', 'eval', 'extract_feature']
        self.data_list_path, self.mode = data_list_path, mode
        self.max_duration, self.min_duration = max_duration, min_duration
        self._target_sample_rate = sample_rate
        self._use_dB_normalization, self._target_dB = use_dB_normalization, target_dB
        self.num_speakers = num_speakers
        self.audio_featurizer = audio_featurizer
        self.volume_conf = self.spec_augment = self.speed_conf = self.noise_conf = self.reverb_conf = None
        self._rir_cache, self._rir_lock = {}, threading.Lock()      # __getitem__ runs on the loader's worker threads
        self.max_samples = int(self.max_duration * self._target_sample_rate)
        self.max_feature_len = self.get_crop_feature_len()
        with open(self.data_list_path, 'r', encoding='utf-8') as f:
            self.lines = [l for l in f.readlines() if l.strip()]
        self.labels = [np.int64(line.strip().split('\t')[1]) for line in self.lines]
        if mode == 'train' and aug_conf is not None:
            self.get_augmentor(aug_conf)
        if self.mode == 'eval':
            self.sort_list()

    def _decode(self, path):
        seg = AudioSegment.from_file(path)
        if seg.sample_rate != self._target_sample_rate and ppvector.get_resampler() == 'host':
            seg.resample(self._target_sample_rate)
        return seg

    def _resampled_len(self, n, sample_rate):
        """Samples an utterance of n samples at sample_rate has at the dataset's rate -- resample_poly's ceil(n up / down)."""
        if sample_rate == self._target_sample_rate:
            return int(n)
        return resample_len(n, *resample_ratio(sample_rate, self._target_sample_rate))

    def __getitem__(self, idx):
        data_path, spk_id = self.lines[idx].strip().split('\t')
        spk_id = int(spk_id)
        if data_path.endswith('.npy'):
            feature = np.load(data_path)
            if feature.shape[0] > self.max_feature_len:
                crop_start = random.randint(0, feature.shape[0] - self.max_feature_len) if self.mode == 'train' else 0
                feature = feature[crop_start:crop_start + self.max_feature_len, :]
            return dict(feature=np.ascontiguousarray(feature, dtype=np.float32), label=spk_id)
        on_gpu = ppvector.get_resampler() == 'gpu'
        seg = self._decode(data_path)
        # the utterance's length at the dataset's rate: under the 'gpu' resampler the samples are still at the file's rate, and every
        # length below is taken from this count, so that a seeded run draws the same numbers in both modes
        n_at_rate = self._resampled_len(seg.samples.shape[0], seg.sample_rate)
        if self.mode in ('train', 'extract_feature') and n_at_rate / float(self._target_sample_rate) < self.min_duration:
            return self.__getitem__(idx + 1 if idx < len(self.lines) - 1 else 0)
        speed, gain = 1.0, 0.0
        if self.mode == 'train' and self.speed_conf is not None and random.random() < self.speed_conf['prob']:
            speed_idx = random.randint(0, 2)
            speed = SPEEDS[speed_idx]
            if self.speed_conf['speed_perturb_3_class']:
                spk_id = spk_id + self.num_speakers * speed_idx
        if self.mode == 'train' and self.volume_conf is not None and random.random() < self.volume_conf['prob']:
            gain = random.uniform(self.volume_conf['min_gain_dBFS'], self.volume_conf['max_gain_dBFS'])
        n = n_at_rate if speed == 1.0 else int(n_at_rate / speed)                            # length after the speed change
        extra = dict(sample_rate=seg.sample_rate) if on_gpu else {}
        if self.mode == 'train' and self.noise_conf is not None and random.random() < self.noise_conf['prob']:
            path = random.choice(self.noise_conf['files'])
            snr = random.uniform(self.noise_conf['min_snr_dB'], self.noise_conf['max_snr_dB'])
            noise = self._decode_first_channel(path)
            sr = float(self._target_sample_rate)
            if noise.shape[0] > 0:                                                            # a file without samples adds nothing
                ns = 0 if noise.shape[0] < n else int(random.uniform(0.0, noise.shape[0] / sr - n / sr) * sr)
                extra.update(noise=noise, snr_dB=snr, noise_start=ns)
        if self.mode == 'train' and self.reverb_conf is not None and random.random() < self.reverb_conf['prob']:
            rir = self._unit_rir(random.choice(self.reverb_conf['files']))
            if rir is not None:
                extra['rir'] = rir
        start = 0
        if self.mode == 'train' and n > self.max_samples:
            start = int(random.uniform(0.0, n / float(self._target_sample_rate) - self.max_duration) * self._target_sample_rate)
        return dict(samples=seg.samples, speed=speed, start=start, gain_dB=gain, label=spk_id, **extra)

    def _decode_first_channel(self, path):
        """A noise / impulse-response file as yeaudio reads it: first channel, resampled to the dataset's rate, float32."""
        seg = AudioSegment.from_file(path, channel=0)
        if seg.sample_rate != self._target_sample_rate:
            seg.resample(self._target_sample_rate)
        return np.ascontiguousarray(seg.samples, dtype=np.float32)

    def _unit_rir(self, path, cache_size=64):
        """h = rir / sqrt(sum rir^2) in float64, stored as float32 (AudioSegment.reverb's scaling, done once per file: the GPU kernel
        is a pure convolution).  None for an all-zero or empty file.  Decoded responses are kept per dataset, oldest dropped first."""
        with self._rir_lock:
            if path not in self._rir_cache:
                h = self._decode_first_channel(path).astype(np.float64)
                e = float(np.sum(h * h))
                while len(self._rir_cache) >= cache_size:
                    self._rir_cache.pop(next(iter(self._rir_cache)))
                self._rir_cache[path] = (h / np.sqrt(e)).astype(np.float32) if e > 0.0 else None
            return self._rir_cache[path]

    def __len__(self):
        return len(self.lines)

    def get_crop_feature_len(self):
        """Frames of a max_duration utterance (reader.py:115-119), from the featurizer's framing arithmetic."""
        return int(self.audio_featurizer.num_frames(self.max_samples))

    def sort_list(self):
        lengths = []
        for line in self.lines:
            data_path, _ = line.split('\t')
            if data_path.endswith('.npy'):
                lengths.append(np.load(data_path, mmap_mode='r').shape[0])
            elif ppvector.get_resampler() == 'gpu':     # the duration at the dataset's rate from the WAV header: nothing is decoded
                with wave.open(data_path, 'rb') as w:
                    lengths.append(self._resampled_len(w.getnframes(), w.getframerate()) / float(self._target_sample_rate))
            else:
                lengths.append(self._decode(data_path).duration)
        self.lines = [self.lines[i] for i in np.argsort(lengths, kind='stable')]
        self.labels = [np.int64(line.strip().split('\t')[1]) for line in self.lines]

    def get_augmentor(self, aug_conf):
        from ppvector.data_utils.spec_aug import SpecAugmentor
        spd = aug_conf.get('speed')
        if spd is not None and float(spd.get('prob', 0.0)) > 0:
            self.speed_conf = dict(prob=float(spd['prob']), speed_perturb_3_class=bool(spd.get('speed_perturb_3_class', False)))
        for name in ('noise', 'reverb'):
            c = aug_conf.get(name) if hasattr(aug_conf, 'get') else None
            if c is None or float(c.get('prob', 0.0)) <= 0:
                continue
            lib_dir = c.get(f'{name}_dir', '')
            files = _wav_files(lib_dir) if lib_dir and os.path.isdir(lib_dir) else []
            if not files:
                continue      # as upstream: without its library of noise / impulse-response files the augmentor is a no-op
            if name == 'noise':
                self.noise_conf = dict(prob=float(c['prob']), min_snr_dB=float(c.get('min_snr_dB', 10)),
                                       max_snr_dB=float(c.get('max_snr_dB', 50)), files=files)
            else:
                self.reverb_conf = dict(prob=float(c['prob']), files=files)
        vol = aug_conf.get('volume')
        if vol is not None and float(vol.get('prob', 0.0)) > 0:
            self.volume_conf = dict(prob=float(vol['prob']), min_gain_dBFS=float(vol.get('min_gain_dBFS', -15)),
                                    max_gain_dBFS=float(vol.get('max_gain_dBFS', 15)))
        if aug_conf.get('spec_aug') is not None:
            self.spec_augment = SpecAugmentor(**aug_conf['spec_aug'])
