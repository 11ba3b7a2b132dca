"""PPVectorPredictor on the MI355X engine -- the inference API of ppvector/predict.py:24-396.

Hot path (what runs in HIP): ``predict`` (:218-233), ``predict_batch`` (:235-269: zero-padded waveforms, ratio
mask, one featurizer call, backbone in chunks), ``contrast`` (:271-283) and the 1:N search of ``recognition``
(:173-187, :337-342) -- Fbank+CMN, backbone forward and cosine scoring all go through libvpmi.
Host bookkeeping kept in Python as in the reference: audio decoding / resampling / dB normalisation
(``_load_audio`` :189-216, yeaudio semantics restated for PCM WAV + ndarray input; under ``ppvector.set_resampler('gpu')`` a recording
that is not at the dataset's rate is uploaded as decoded and converted and normalised on the device instead -- ``_load_waves``,
docs/resample.md -- in ``predict``, ``predict_batch``, ``vad`` and ``speaker_diarization``; ``register`` keeps the host path), the user index
(pickle ``audio_indexes.bin`` with the reference's key names, :86-109).  The per-user means the search runs over (:154-164) are kept
as unit centroids in a device matrix (``ppvector/infer_utils/gallery.py``, docs/gallery.md) in step with the index: a query
computes and uploads nothing but its own embedding.
``speaker_diarization`` (:366-396): the windows are cut, padded and normalised on the GPU from one upload of the recording, embedded
by the same featurizer + backbone, and clustered through the pruned-affinity and Laplacian kernels (``ppvector/infer_utils``).  The
reference's model-based voice-activity detection in front of it is not built: the caller passes the speech regions, or sets this
project's own energy detector with ``set_vad`` (``ppvector/infer_utils/vad.py``, docs/vad.md), which finds them on the same upload.
"""
import io
import os
import pickle
import shutil
import wave
from io import BufferedReader

import numpy as np
import torch
import yaml
from torch import nn

from ppvector.data_utils.featurizer import AudioFeaturizer
from ppvector.data_utils.wave_batch import assemble_waves, resample_waves
from ppvector.infer_utils.gallery import SpeakerGallery
from ppvector.infer_utils.speaker_diarization import SpeakerDiarization, chunk_batch
from ppvector.metric.metrics import cosine_score_matrix
from ppvector.models import build_model
from ppvector.utils.utils import dict_to_object


class AudioSegment:
    """Minimal stand-in for yeaudio.audio.AudioSegment (mono float32 samples in [-1, 1])."""

    def __init__(self, samples, sample_rate):
        samples = np.asarray(samples)
        if samples.dtype.kind in 'iu':
            samples = samples.astype(np.float32) / float(2 ** (8 * samples.dtype.itemsize - 1))
        samples = samples.astype(np.float32)
        if samples.ndim == 2:                      # (frames, channels) -> mono
            samples = samples.mean(axis=1)
        self.samples, self.sample_rate = samples, int(sample_rate)

    @classmethod
    def from_file(cls, f, channel=None):
        """channel: keep that one channel of a multi-channel file (None = the mean of all)."""
        with wave.open(f, 'rb') as w:
            n, ch, sw, sr = w.getnframes(), w.getnchannels(), w.getsampwidth(), w.getframerate()
            raw = w.readframes(n)
        if sw not in (1, 2, 4):
            raise Exception(f'不支持该数据类型: {8 * sw}-bit PCM')
        dt = {1: np.uint8, 2: np.int16, 4: np.int32}[sw]
        x = np.frombuffer(raw, dtype=dt)
        if sw == 1:
            x = (x.astype(np.int16) - 128).astype(np.int8)
        x = x.reshape(-1, ch)
        return cls(x if channel is None else x[:, channel], sr)

    @classmethod
    def from_bytes(cls, b):
        return cls.from_file(io.BytesIO(b))

    @classmethod
    def from_ndarray(cls, x, sample_rate=16000):
        return cls(x, sample_rate)

    @property
    def duration(self):
        return self.samples.shape[0] / float(self.sample_rate)

    @property
    def rms_db(self):
        return 10.0 * np.log10(max(float(np.mean(self.samples.astype(np.float64) ** 2)), 1e-20))

    def resample(self, target_sample_rate):
        from math import gcd
        from scipy.signal import resample_poly
        g = gcd(int(target_sample_rate), self.sample_rate)
        self.samples = resample_poly(self.samples, int(target_sample_rate) // g, self.sample_rate // g).astype(np.float32)
        self.sample_rate = int(target_sample_rate)

    def normalize(self, target_db=-20, max_gain_db=300.0):
        gain = min(target_db - self.rms_db, max_gain_db)
        self.samples = (self.samples * (10.0 ** (gain / 20.0))).astype(np.float32)


class PPVectorPredictor:
    def __init__(self, configs, threshold=0.6, audio_db_path=None, model_path='models/CAMPPlus_Fbank/best_model/',
                 use_gpu=True):
        """声纹识别预测工具 (same arguments as the reference; ``use_gpu`` must be True: no CPU fallback)."""
        if not use_gpu:
            raise RuntimeError('the MI355X engine has no CPU path (use_gpu=False is not available)')
        assert torch.cuda.is_available(), 'GPU不可用'
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.threshold = threshold
        if isinstance(configs, str):
            with open(configs, 'r', encoding='utf-8') as f:
                configs = yaml.load(f.read(), Loader=yaml.FullLoader)
        self.configs = dict_to_object(configs)
        self._audio_featurizer = AudioFeaturizer(feature_method=self.configs.preprocess_conf.feature_method,
                                                 method_args=self.configs.preprocess_conf.get('method_args', {}))
        backbone = build_model(input_size=self._audio_featurizer.feature_dim, configs=self.configs)
        self.predictor = nn.Sequential(backbone)
        if isinstance(model_path, dict):                       # an in-memory state dict ("0.<...>" keys)
            state = model_path
        else:
            if not os.path.exists(model_path):
                raise Exception("模型文件不存在，请检查{}是否存在！".format(model_path))
            if os.path.isdir(model_path):                      # the reference's checkpoint directory (predict.py:61-62)
                model_path = os.path.join(model_path, 'model.pdparams')
            assert os.path.exists(model_path), f"{model_path} 模型不存在！"
            from ppvector.utils.checkpoint import load_pdparams
            state = load_pdparams(model_path)
        state = {k: torch.as_tensor(np.asarray(v)) if not isinstance(v, torch.Tensor) else v for k, v in state.items()}
        own = self.predictor.state_dict()
        # load_pretrained semantics (utils/checkpoint.py:11-42): keep what matches by name and shape
        self.predictor.load_state_dict({k: v for k, v in state.items() if k in own and tuple(v.shape) == tuple(own[k].shape)},
                                       strict=False)
        self.predictor.to(self.device).eval()
        self.audio_feature = None
        self.users_name, self.users_audio_path = [], []
        self.gallery = None                                    # SpeakerGallery, made with the first enrolled embedding's width
        self.score_norm = None                                 # a ScoreNorm: set_score_norm (docs/gallery.md)
        self._cosine_threshold = None                          # the threshold in force when the score norm was set
        self.calibration = None                                # a Calibration: set_calibration (docs/calibration.md)
        self.audio_db_path = audio_db_path
        self.speaker_diarize = SpeakerDiarization()
        self._vad = None                                       # an EnergyVad: set_vad (docs/vad.md)
        if self.audio_db_path is not None:
            self.audio_indexes_path = os.path.join(audio_db_path, "audio_indexes.bin")
            self.__load_audio_db(self.audio_db_path)

    # ------------------------------------------------------------------ voice-print index (host bookkeeping)
    def __load_audio_indexes(self):
        if not os.path.exists(self.audio_indexes_path):
            return
        with open(self.audio_indexes_path, "rb") as f:
            indexes = pickle.load(f)
        for name, feature, path in zip(indexes["users_name"], indexes["faces_feature"], indexes["users_image_path"]):
            if not os.path.exists(path):
                continue
            self.users_name.append(name)
            self.users_audio_path.append(path)
            self.audio_feature = feature[None] if self.audio_feature is None else np.vstack((self.audio_feature, feature))
        if self.audio_feature is not None:
            self.__gallery().rebuild(self.users_name, self.audio_feature)

    def __gallery(self):
        if self.gallery is None:
            self.gallery = SpeakerGallery(self.audio_feature.shape[1], self.device)
            self.gallery.set_score_norm(self.score_norm)
        return self.gallery

    def set_score_norm(self, score_norm, threshold=None):
        """Adaptive score normalisation for ``recognition``, ``recognition_batch``, ``contrast`` and the ``search_audio_db`` branch
        (no counterpart in the reference; docs/gallery.md): with a ``ScoreNorm`` they return, and threshold on, z.  ``threshold``
        is the operating point on z and has to be given: a z is not a cosine, the constructor's threshold does not carry over.
        ``set_score_norm(None)`` restores the cosine search and the threshold that was in force before."""
        from ppvector.metric.score_norm import ScoreNorm
        if score_norm is None:
            if self.score_norm is not None:
                self.threshold = self._cosine_threshold
            self.score_norm = self._cosine_threshold = None
        else:
            if not isinstance(score_norm, ScoreNorm):
                raise ValueError(f'set_score_norm: a ScoreNorm or None, got {type(score_norm).__name__}')
            if threshold is None:
                raise TypeError('set_score_norm: a threshold on z has to be given with a ScoreNorm (a z is not a cosine)')
            if self.score_norm is None:
                self._cosine_threshold = self.threshold
            self.score_norm = score_norm
            self.threshold = threshold
        if self.gallery is not None:
            self.gallery.set_score_norm(self.score_norm)

    def __gallery_set(self, user_name):
        """One user's row of the gallery from that user's rows of ``audio_feature``."""
        rows = [i for i, n in enumerate(self.users_name) if n == user_name]
        self.__gallery().set_user(user_name, self.audio_feature[rows])

    def __search(self, features, top_k=1):
        """(Q, D) embeddings -> host (idx, score) arrays (Q, top_k) of the best enrolled users (``self.gallery.names[idx]``)."""
        idx, score = self.gallery.search(torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32)).to(self.device), top_k)
        return idx.cpu().numpy(), score.cpu().numpy()

    def __write_index(self):
        with open(self.audio_indexes_path, "wb") as f:
            pickle.dump({"users_name": self.users_name, "faces_feature": self.audio_feature,
                         "users_image_path": self.users_audio_path}, f)

    def __load_audio_db(self, audio_db_path):
        self.__load_audio_indexes()
        os.makedirs(audio_db_path, exist_ok=True)
        todo = []
        for name in sorted(os.listdir(audio_db_path)):
            audio_dir = os.path.join(audio_db_path, name)
            if not os.path.isdir(audio_dir):
                continue
            for file in sorted(os.listdir(audio_dir)):
                p = os.path.join(audio_dir, file).replace('\\', '/')
                if p not in self.users_audio_path:
                    todo.append((name, p))
        for name, p in todo:
            feat = self.predict(p)
            self.users_name.append(name)
            self.users_audio_path.append(p)
            self.audio_feature = feat[None] if self.audio_feature is None else np.vstack((self.audio_feature, feat))
        for name in dict.fromkeys(n for n, _ in todo):
            self.__gallery_set(name)
        if todo:
            self.__write_index()

    # ------------------------------------------------------------------ audio front end (host)
    def _load_audio(self, audio_data, sample_rate=16000):
        return self._finish_audio(self._decode_audio(audio_data, sample_rate))

    def _decode_audio(self, audio_data, sample_rate=16000):
        if isinstance(audio_data, str):
            seg = AudioSegment.from_file(audio_data)
        elif isinstance(audio_data, BufferedReader):
            seg = AudioSegment.from_file(audio_data)
        elif isinstance(audio_data, np.ndarray):
            seg = AudioSegment.from_ndarray(audio_data, sample_rate)
        elif isinstance(audio_data, bytes):
            seg = AudioSegment.from_bytes(audio_data)
        elif isinstance(audio_data, AudioSegment):
            seg = audio_data
        else:
            raise Exception(f'不支持该数据类型，当前数据类型为：{type(audio_data)}')
        return seg

    def _finish_audio(self, seg):
        ds = self.configs.dataset_conf.dataset
        assert seg.duration >= ds.min_duration, f'音频太短，最小应该为{ds.min_duration}s，当前音频为{seg.duration}s'
        if seg.sample_rate != ds.sample_rate:
            seg.resample(ds.sample_rate)
        if ds.use_dB_normalization:
            seg.normalize(target_db=ds.target_dB)
        return seg

    def _native_segment(self, audio_data, sample_rate):
        """(segment, audio): under the 'gpu' resampler (docs/resample.md), for input that is not at the dataset's rate, `segment` is the
        decoded recording at its own rate, to be uploaded as it is and converted, then normalised, on the device (``_load_waves``).
        Otherwise `segment` is None and `audio` is what ``_load_audio`` takes, to do what it always did -- the input itself under the
        host resampler, the decoded segment for a recording that is already at the dataset's rate."""
        import ppvector
        if ppvector.get_resampler() != 'gpu':
            return None, audio_data
        seg = self._decode_audio(audio_data, sample_rate)
        return (seg, None) if seg.sample_rate != self.configs.dataset_conf.dataset.sample_rate else (None, seg)

    def _load_waves(self, segs):
        """What ``_finish_audio`` does to native-rate segments, on the device: the duration check, one upload each at the file's rate,
        resample_waves, then the dB normalisation over the whole converted recording by vp_wave_batch_f32.  Returns
        ((len(segs), L) f32 rows zero-padded to the longest, [samples of each row])."""
        ds = self.configs.dataset_conf.dataset
        for seg in segs:
            assert seg.duration >= ds.min_duration, f'音频太短，最小应该为{ds.min_duration}s，当前音频为{seg.duration}s'
        waves = resample_waves([self._upload(seg) for seg in segs], [seg.sample_rate for seg in segs], ds.sample_rate)
        batch, _ = assemble_waves(waves, use_dB_normalization=bool(ds.use_dB_normalization), target_dB=float(ds.target_dB))
        return batch, [int(w.numel()) for w in waves]

    def _load_recording(self, audio_data, sample_rate):
        """(segment, samples on the device) of a whole recording for ``vad`` / ``speaker_diarization``.  Converted on the device, the
        segment is a stand-in at the dataset's rate whose ``samples`` have the converted length and no storage: the chunk table reads
        only lengths, and no host copy of the converted recording is made."""
        native, audio_data = self._native_segment(audio_data, sample_rate)
        if native is None:
            seg = self._load_audio(audio_data=audio_data, sample_rate=sample_rate)
            return seg, self._upload(seg)
        batch, (n,) = self._load_waves([native])
        stand_in = AudioSegment.__new__(AudioSegment)           # (the constructor would copy the samples)
        stand_in.samples = np.broadcast_to(np.float32(0.0), (n,))
        stand_in.sample_rate = int(self.configs.dataset_conf.dataset.sample_rate)
        return stand_in, batch[0]

    # ------------------------------------------------------------------ hot path
    def predict(self, audio_data, sample_rate=16000):
        """预测一个音频的特征 -> (embd_dim,) float32."""
        native, audio_data = self._native_segment(audio_data, sample_rate)
        if native is not None:
            x, _ = self._load_waves([native])
        else:
            seg = self._load_audio(audio_data=audio_data, sample_rate=sample_rate)
            x = torch.from_numpy(seg.samples).to(self.device).unsqueeze(0)
        feat = self._audio_featurizer(x, want_bf16=self._want_bf16())
        return self.predictor(feat).cpu().numpy()[0]

    def predict_batch(self, audios_data, sample_rate=16000, batch_size=32):
        """预测一批音频的特征: zero-pad the WAVEFORMS to the longest, ratio mask, as the reference does."""
        native, audios_data = zip(*[self._native_segment(a, sample_rate) for a in audios_data])
        on_gpu = [i for i, s in enumerate(native) if s is not None]
        host = [i for i, s in enumerate(native) if s is None]
        waves = [self._load_audio(audio_data=audios_data[i], sample_rate=sample_rate).samples for i in host]
        converted, lens = self._load_waves([native[i] for i in on_gpu]) if on_gpu else (None, [])
        longest = max([w.shape[0] for w in waves] + lens)
        inputs = np.zeros((len(waves), longest), dtype=np.float32)
        ratios = [0.0] * len(native)
        for k, (i, w) in enumerate(zip(host, waves)):
            inputs[k, :w.shape[0]] = w
            ratios[i] = w.shape[0] / longest
        x = torch.from_numpy(inputs).to(self.device)
        if on_gpu:                                             # the rows converted on the device, zero-padded, among the others
            rows = torch.zeros((len(native), longest), dtype=torch.float32, device=self.device)
            rows[torch.tensor(host, dtype=torch.int64, device=self.device)] = x
            rows[torch.tensor(on_gpu, dtype=torch.int64, device=self.device), :converted.shape[1]] = converted
            x = rows
            for i, n in zip(on_gpu, lens):
                ratios[i] = n / longest
        r = torch.tensor(ratios, dtype=torch.float32, device=self.device)
        feat = self._audio_featurizer(x, r)
        outs = [self.predictor(feat[i:i + batch_size].contiguous()).cpu().numpy() for i in range(0, len(native), batch_size)]
        return np.concatenate(outs, axis=0)

    def contrast(self, audio_data1, audio_data2):
        """声纹对比 -> cosine similarity; with a score norm set, the z of the pair (the first as trial, the second as enrolment)."""
        f = np.stack([self.predict(audio_data1), self.predict(audio_data2)])
        a, b = torch.from_numpy(f[:1]).to(self.device), torch.from_numpy(f[1:]).to(self.device)
        s = cosine_score_matrix(a, b)
        if self.score_norm is not None:
            s = self.score_norm.normalise(s.contiguous(), a, b)
        return float(s[0, 0])

    # ------------------------------------------------------------------ calibrated pair scores (docs/calibration.md)
    def set_calibration(self, calibration):
        """A ``Calibration``, the path of one saved as JSON, or None (no counterpart in the reference): what ``contrast_llr`` and
        ``contrast_probability`` map the pair score with.  ``contrast``, ``recognition*`` and ``register`` do not look at it."""
        from ppvector.metric.calibration import Calibration
        if isinstance(calibration, (str, os.PathLike)):
            calibration = Calibration.load(calibration)
        if calibration is not None and not isinstance(calibration, Calibration):
            raise ValueError(f'set_calibration: a Calibration, a path or None, got {type(calibration).__name__}')
        self.calibration = calibration

    def _calibration(self, what):
        cal = self.calibration
        if cal is None:
            raise ValueError(f'{what}: no calibration is set (set_calibration)')
        if cal.normalised != (self.score_norm is not None):
            raise ValueError(f'{what}: the calibration was fitted on {"normalised scores" if cal.normalised else "raw cosines"}, '
                             f'and a score norm is {"not set" if self.score_norm is None else "set"}')
        return cal

    def contrast_llr(self, audio_data1, audio_data2):
        """The log-likelihood ratio (natural log) of "same speaker" for the pair: a s + b of the score ``contrast`` returns."""
        return self._calibration('contrast_llr').llr(self.contrast(audio_data1, audio_data2))

    def contrast_probability(self, audio_data1, audio_data2, p_target=0.5):
        """The posterior probability of "same speaker" for the pair, for a target prior p_target."""
        return self._calibration('contrast_probability').posterior(self.contrast(audio_data1, audio_data2), p_target=p_target)

    def _want_bf16(self):
        import ppvector
        return ppvector.get_compute_dtype() == 'bfloat16'

    # ------------------------------------------------------------------ 1:N
    def register(self, audio_data, user_name: str, sample_rate=16000):
        """声纹注册."""
        seg = self._load_audio(audio_data=audio_data, sample_rate=sample_rate)
        feat = self.predict(audio_data=seg)
        if self.audio_db_path is not None:
            d = os.path.join(self.audio_db_path, user_name)
            os.makedirs(d, exist_ok=True)
            path = os.path.join(d, f'{len(os.listdir(d))}.wav').replace('\\', '/')
            pcm = np.clip(seg.samples * 32768.0, -32768, 32767).astype(np.int16)
            with wave.open(path, 'wb') as w:
                w.setnchannels(1); w.setsampwidth(2); w.setframerate(seg.sample_rate); w.writeframes(pcm.tobytes())
        else:
            path = f'<memory:{len(self.users_name)}>'
        self.users_name.append(user_name)
        self.users_audio_path.append(path)
        self.audio_feature = feat[None] if self.audio_feature is None else np.vstack((self.audio_feature, feat))
        self.__gallery_set(user_name)
        if self.audio_db_path is not None:
            self.__write_index()
        return True, "注册成功"

    def recognition(self, audio_data, threshold=None, sample_rate=16000):
        """声纹识别 -> (name, score) of the best enrolled user, or (None, None) under the threshold."""
        if threshold:
            self.threshold = threshold
        if self.audio_feature is None:
            return None, None
        feat = self.predict(audio_data, sample_rate=sample_rate)
        idx, score = self.__search(feat[None])
        i, s = int(idx[0, 0]), float(score[0, 0])
        if i >= 0 and s >= self.threshold:
            return self.gallery.names[i], round(s, 5)
        return None, None

    def recognition_batch(self, audios_data, threshold=None, sample_rate=16000, batch_size=32, top_k=1):
        """声纹识别 of a batch: one list per utterance of up to ``top_k`` (name, score) pairs at or above the threshold, best first
        (empty when nothing passes).  The embeddings are ``predict_batch``'s, as the reference's ``__retrieval`` takes a batch."""
        if threshold:
            self.threshold = threshold
        if self.audio_feature is None:
            return [[] for _ in audios_data]
        feats = self.predict_batch(audios_data, sample_rate=sample_rate, batch_size=batch_size)
        idx, score = self.__search(feats, top_k)
        names = self.gallery.names
        return [[(names[i], round(float(s), 5)) for i, s in zip(ri, rs) if i >= 0 and s >= self.threshold]
                for ri, rs in zip(idx, score)]

    def get_users(self):
        return self.users_name

    # ------------------------------------------------------------------ diarization
    def _upload(self, audio_segment):
        return torch.from_numpy(np.ascontiguousarray(audio_segment.samples, dtype=np.float32)).to(self.device)

    def chunk_embeddings(self, audio_segment, table, batch_size=32, wave=None):
        """Embeddings (N, embd_dim) of the windows ``table`` (rows ``[start_s, end_s, first_sample, end_sample]``) of a loaded
        recording: one upload (``wave``: the samples already on the device, when the caller has them there), the windows cut /
        zero-padded / dB-normalised by vp_chunk_batch_f32 as ``_load_audio`` would do to each of them, then the featurizer (all rows
        have one length: no ratio mask) and the backbone in slices of ``batch_size``."""
        ds = self.configs.dataset_conf.dataset
        if wave is None:
            wave = self._upload(audio_segment)
        offsets = np.asarray([[row[2], row[3]] for row in table], dtype=np.int32)
        chunks = chunk_batch(wave, offsets, self.speaker_diarize.chunk_len, normalize=bool(ds.use_dB_normalization),
                             target_db=float(ds.target_dB))
        outs = []
        for i in range(0, chunks.shape[0], batch_size):
            feat = self._audio_featurizer(chunks[i:i + batch_size])
            outs.append(self.predictor(feat).cpu().numpy())
        return np.concatenate(outs, axis=0)

    _NO_VAD = ('voice-activity detection (yeaudio AudioSegment.vad) is not built on the HIP engine: '
               'pass the speech regions as vad_segments=[(start_s, end_s), ...]')

    def set_vad(self, vad):
        """An ``EnergyVad`` (no counterpart in the reference; docs/vad.md): ``speaker_diarization`` without ``vad_segments`` then takes
        the speech regions from it.  ``set_vad(None)``, the default: such a call raises, as it always did."""
        from ppvector.infer_utils.vad import EnergyVad
        if vad is not None and not isinstance(vad, EnergyVad):
            raise ValueError(f'set_vad: an EnergyVad or None, got {type(vad).__name__}')
        self._vad = vad

    def _vad_regions(self, seg, wave):
        """The detector's regions of a loaded recording as ``segments`` can take them: it reads times to the millisecond and wants the
        regions inside the recording and apart, so an end is rounded DOWN to the millisecond and stops where the next region starts
        (a region ends with its last frame's window, which can reach past the first frame of a region that starts right after it)."""
        vad = self._vad
        if vad.sample_rate != seg.sample_rate:
            raise ValueError(f'the detector was made for {vad.sample_rate} Hz, the recording is loaded at {seg.sample_rate} Hz')
        regions, _ = vad.regions(wave)
        out = []
        for i, (start, end) in enumerate(regions):
            if i + 1 < len(regions):
                end = min(end, regions[i + 1][0])
            out.append((start, int(end * 1000.0 + 1e-6) / 1000.0))     # 11.3 s is 11299.999... ms in binary
        return out

    def vad(self, audio_data, sample_rate=16000):
        """The speech regions [(start_s, end_s)] the detector set with ``set_vad`` finds in the recording as ``_load_audio`` loads it --
        what ``speaker_diarization`` uses when it is given no ``vad_segments``."""
        if getattr(self, '_vad', None) is None:
            raise NotImplementedError(self._NO_VAD)
        seg, wave = self._load_recording(audio_data, sample_rate)
        return self._vad_regions(seg, wave)

    def speaker_diarization(self, audio_data, sample_rate=16000, speaker_num=None, search_audio_db=False, vad_segments=None):
        """说话人日志识别 -> [dict(speaker, start, end)] (predict.py:366-396).

        ``vad_segments``: the speech regions as (start_s, end_s) pairs, the one argument the reference does not have.  Its own
        regions come from yeaudio's model-based ``AudioSegment.vad``, which is not built here; without ``vad_segments`` the call raises,
        unless a detector was set with ``set_vad``: then the regions are that detector's, found on the upload the windows are cut from.
        """
        if vad_segments is None and getattr(self, '_vad', None) is None:      # (before anything else: also on a bare instance)
            raise NotImplementedError(self._NO_VAD)
        seg, wave = self._load_recording(audio_data, sample_rate)
        if vad_segments is None:
            vad_segments = self._vad_regions(seg, wave)
        table = self.speaker_diarize.segments(seg, vad_segments)
        features = self.chunk_embeddings(seg, table, wave=wave)
        labels, spk_center_embeddings = self.speaker_diarize.clustering(features, speaker_num=speaker_num)
        outputs = self.speaker_diarize.postprocess(table, labels)
        if search_audio_db:
            assert self.audio_feature is not None, "数据库中没有音频数据，请先指定说话人特征数据库或者注册说话人"
            idx, score = self.__search(spk_center_embeddings)
            users = self.gallery.names
            names = [users[j] if j >= 0 and s >= self.threshold else None for j, s in zip(idx[:, 0], score[:, 0])]
            outputs = [dict(speaker=names[o['speaker']] if names[o['speaker']] else f"陌生人{o['speaker']}",
                            start=o['start'], end=o['end']) for o in outputs]
        return outputs

    def remove_user(self, user_name):
        if user_name not in self.users_name:
            return False
        keep = [i for i, n in enumerate(self.users_name) if n != user_name]
        if self.audio_db_path is not None:
            shutil.rmtree(os.path.join(self.audio_db_path, user_name), ignore_errors=True)
        self.users_name = [self.users_name[i] for i in keep]
        self.users_audio_path = [self.users_audio_path[i] for i in keep]
        self.audio_feature = self.audio_feature[keep] if keep else None
        self.gallery.remove(user_name)
        if self.audio_db_path is not None:
            self.__write_index()
        return True
