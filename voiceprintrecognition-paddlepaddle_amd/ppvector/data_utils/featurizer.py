"""AudioFeaturizer on the MI355X engine.

Mirrors ppvector/data_utils/featurizer.py:7-80 (constructor arguments, call signature,
``feature_dim``, the exceptions for unknown methods).  'Fbank' (KaldiFbank, featurizer.py:83-101)
runs in one fused HIP pipeline (csrc/fbank.hip): framing, DC removal, pre-emphasis, Povey window,
512-point FFT, Kaldi mel bank, log, time-mean subtraction and the length mask.
"""
import ctypes as C
import math

import torch
from torch import nn

from ppvector import _native as N

_KALDI_KW = {'sr': 'sample_rate', 'n_mels': 'n_mels', 'frame_length': 'frame_length_ms',
             'frame_shift': 'frame_shift_ms', 'preemphasis_coefficient': 'preemph',
             'remove_dc_offset': 'remove_dc', 'low_freq': 'low_freq', 'high_freq': 'high_freq'}
_KALDI_FIXED = {'dither': 0.0, 'window_type': 'povey', 'snip_edges': True, 'use_energy': False,
                'use_log_fbank': True, 'use_power': True, 'round_to_power_of_two': True,
                'subtract_mean': False, 'htk_compat': False, 'raw_energy': True, 'channel': -1,
                'vtln_warp': 1.0, 'energy_floor': 1.0, 'blackman_coeff': 0.42, 'vtln_low': 100.0,
                'vtln_high': -500.0}


def _f32(x):
    return C.c_float(x).value


def _fbank_pcm16_covered(o):
    """Whether vp_fbank_cmn_pcm16 takes these options: the 16-bit loads exist in the four-frames-per-wave kernel only, which wants
    an even frame shift (4-byte aligned sample pairs) and a mel bank that fits its padded round layout -- csrc/fbank.hip,
    build_tables: rounds of 16 filters, taps padded to the round's longest filter rounded up to 4, at most F16_MAX_TAPS = 32 per
    round and F16_MAX_WPAD = 1536 floats in all.  Decided here, up front, so that int16 input of an option set the entry does not
    cover is widened first instead of failing in the library (the paddleaudio default n_mels=23 at 16 kHz is such a bank).  Option
    sets the library refuses altogether report False: the float entry then raises its own error."""
    win = int(_f32(_f32(o.sample_rate * o.frame_length_ms) * _f32(0.001)))          # the library's float32 products, truncated
    shift = int(_f32(_f32(o.sample_rate * o.frame_shift_ms) * _f32(0.001)))
    nfft = 1
    while nfft < win:
        nfft <<= 1
    if nfft != 512 or win < 2 or shift < 1 or shift & 1 or not 1 <= o.n_mels <= 128:
        return False

    def mel(f):
        return 1127.0 * math.log(1.0 + f / 700.0)
    hi = o.high_freq if o.high_freq > 0.0 else o.high_freq + 0.5 * o.sample_rate
    mlo = mel(o.low_freq)
    delta = (mel(hi) - mlo) / (o.n_mels + 1)
    bins = [mel(o.sample_rate / nfft * k) for k in range(nfft // 2)]
    taps = []
    for m in range(o.n_mels):
        l, c, r = mlo + m * delta, mlo + (m + 1) * delta, mlo + (m + 2) * delta
        nz = [k for k, x in enumerate(bins) if min((x - l) / (c - l), (r - x) / (r - c)) > 0.0]
        taps.append(nz[-1] - nz[0] + 1 if nz else 0)
    padded = [max(4, (max(taps[i:i + 16]) + 3) // 4 * 4) for i in range(0, o.n_mels, 16)]
    return max(padded) <= 32 and 16 * sum(padded) <= 1536


class AudioFeaturizer(nn.Module):
    """音频特征器 (feature_method: 'Fbank' on the HIP engine).

    :param feature_method: 所使用的预处理方法
    :param method_args: 预处理方法的参数
    """

    def __init__(self, feature_method='MelSpectrogram', method_args={}):
        super().__init__()
        self._method_args = method_args
        self._feature_method = feature_method
        if feature_method == 'Fbank':
            self._opts = self._fbank_opts(method_args)
            self._pcm16_ok = _fbank_pcm16_covered(self._opts)
        elif feature_method == 'MelSpectrogram':
            self._opts = self._mel_opts(method_args)
        elif feature_method == 'LogMelSpectrogram':
            self._opts = self._mel_opts(method_args, log=True)
        elif feature_method == 'MFCC':
            args = dict(method_args)
            self._n_mfcc = int(args.pop('n_mfcc', 40))
            self._opts = self._mel_opts(args, log=True)
            if self._n_mfcc > self._opts.n_mels:
                raise AssertionError('n_mfcc cannot be larger than n_mels: %d vs %d' % (self._n_mfcc, self._opts.n_mels))
            self._dct = None
        elif feature_method == 'Spectrogram':
            self._opts = None       # known to the reference; not built on the HIP engine yet
        else:
            raise Exception(f'预处理方法 {self._feature_method} 不存在!')
        self._ws = N.Workspace()

    @staticmethod
    def _fbank_opts(method_args):
        o = N.FbankOpts()
        N.lib().vp_fbank_default_opts(C.byref(o))
        for k, v in dict(method_args).items():
            if k in _KALDI_KW:
                setattr(o, _KALDI_KW[k], type(getattr(o, _KALDI_KW[k]))(v))
            elif k in _KALDI_FIXED:
                if v != _KALDI_FIXED[k]:
                    raise NotImplementedError(f'Fbank option {k}={v} is not built on the HIP engine')
            else:
                raise TypeError(f"fbank() got an unexpected keyword argument '{k}'")
        return o

    @staticmethod
    def _mel_opts(method_args, log=False):
        """paddle.audio.features.MelSpectrogram keyword surface (defaults: sr 22050, n_fft 2048, hop_length 512,
        win_length None, window 'hann', power 2.0, center True, pad_mode 'reflect', n_mels 64, f_min 50.0,
        f_max None, htk False, norm 'slaney').  log=True: paddle.audio.features.LogMelSpectrogram (featurizer.py:20-21) =
        the same mel spectrogram through power_to_db(ref_value=1.0, amin=1e-10, top_db=None); its n_fft default is 512."""
        o = N.MelOpts()
        N.lib().vp_mel_default_opts(C.byref(o))
        if log:
            o.log_db, o.n_fft = 1, 512
        names = {'sr': 'sample_rate', 'n_fft': 'n_fft', 'hop_length': 'hop_length', 'win_length': 'win_length',
                 'n_mels': 'n_mels', 'f_min': 'f_min', 'f_max': 'f_max', 'power': 'power'}
        if log:
            names.update(ref_value='ref_value', amin='amin')
        fixed = {'window': 'hann', 'center': True, 'pad_mode': 'reflect', 'htk': False, 'norm': 'slaney', 'dtype': 'float32'}
        if log:
            fixed['top_db'] = None
        for k, v in dict(method_args).items():
            if k in names:
                if v is None:
                    v = 0
                setattr(o, names[k], type(getattr(o, names[k]))(v))
            elif k in fixed:
                if v != fixed[k]:
                    raise NotImplementedError(f'MelSpectrogram option {k}={v} is not built on the HIP engine')
            else:
                raise TypeError(f"__init__() got an unexpected keyword argument '{k}'")
        if dict(method_args).get('hop_length') is None:              # paddle: hop_length defaults to win_length // 4
            o.hop_length = (o.win_length or o.n_fft) // 4
        if o.f_max > 0.5 * o.sample_rate:
            raise ValueError(f'f_max {o.f_max} is above the Nyquist frequency of sr {o.sample_rate}')
        return o

    def num_frames(self, n_samples):
        if self._feature_method in ('MelSpectrogram', 'LogMelSpectrogram', 'MFCC'):
            return N.lib().vp_mel_num_frames(C.byref(self._opts), int(n_samples))
        return N.lib().vp_fbank_num_frames(C.byref(self._opts), int(n_samples))

    def forward(self, waveforms, input_lens_ratio=None, want_bf16=False):
        """waveforms (L,) or (B, L) float32 on the GPU -> (B, T, F) float32.

        With want_bf16 the bf16 copy the bf16 network consumes is produced by the same kernel and
        attached to the result as ``._vp_bf16``.
        """
        if self._opts is None:
            raise NotImplementedError(f'feature_method {self._feature_method} is not built on the HIP engine yet '
                                      '(Fbank is); there is no CPU fallback')
        if waveforms.dim() == 1:
            waveforms = waveforms.unsqueeze(0)
        if not waveforms.is_cuda:
            raise N.VpmiError('AudioFeaturizer needs GPU tensors: the engine has no CPU fallback')
        # 16-bit PCM as decoded (torch.int16): widened inside the Fbank frame kernel (x 1 / 32768, what the reference's readers do on
        # the host), so an upload in front of this call carries half the bytes; other methods, an odd row length and Fbank options
        # the 16-bit entry does not cover (_fbank_pcm16_covered) widen first
        pcm16 = (waveforms.dtype == torch.int16 and self._feature_method == 'Fbank' and waveforms.shape[-1] % 2 == 0
                 and self._pcm16_ok)
        if waveforms.dtype == torch.int16 and not pcm16:
            waveforms = waveforms.float() * (1.0 / 32768.0)
        wav = waveforms.contiguous() if pcm16 else waveforms.contiguous().float()
        B, L = wav.shape
        lib, ctx = N.lib(), N.ctx(wav.device)
        mel = self._feature_method in ('MelSpectrogram', 'LogMelSpectrogram', 'MFCC')
        T = (lib.vp_mel_num_frames if mel else lib.vp_fbank_num_frames)(C.byref(self._opts), L)
        if T <= 0:
            raise ValueError(f'{L} samples are shorter than one analysis window')
        F = self._opts.n_mels
        out = torch.empty((B, T, F), dtype=torch.float32, device=wav.device)
        out16 = torch.empty((B, T, F), dtype=torch.bfloat16, device=wav.device) if want_bf16 else None
        ratio = None
        if input_lens_ratio is not None:
            ratio = input_lens_ratio.to(device=wav.device, dtype=torch.float32).contiguous()
        nws = (lib.vp_mel_workspace_bytes if mel else lib.vp_fbank_workspace_bytes)(C.byref(self._opts), B, L)
        ws = self._ws.get(nws, wav.device)
        if pcm16:
            N.check(lib.vp_fbank_cmn_pcm16(ctx, N.ptr(wav), 1.0 / 32768.0, N.ptr(ratio), B, L, C.byref(self._opts), N.ptr(out), N.ptr(out16),
                                           N.ptr(ws), ws.numel(), N.stream_ptr()), ctx)
        else:
            fn = lib.vp_melspec_cmn_f32 if mel else lib.vp_fbank_cmn_f32
            N.check(fn(ctx, N.ptr(wav), N.ptr(ratio), B, L, C.byref(self._opts), N.ptr(out), N.ptr(out16), N.ptr(ws),
                       ws.numel(), N.stream_ptr()), ctx)
        if self._feature_method == 'MFCC':
            out, out16 = self._mfcc(out, want_bf16)
        if out16 is not None:
            out._vp_bf16 = out16
        return out

    def _mfcc(self, logmel, want_bf16):
        """paddle.audio.features.MFCC (featurizer.py:26-27): log-mel @ create_dct(n_mfcc, n_mels, norm='ortho').  The DCT is
        linear, so it commutes with the mean subtraction and the zeroed rows already applied to the log-mel features (B, T, n_mels).
        Returns (mfcc (B, T, n_mfcc) f32, its bf16 cast or None)."""
        B, T, F = logmel.shape
        lib, ctx = N.lib(), N.ctx(logmel.device)
        if self._dct is None or self._dct.device != logmel.device:
            n = torch.arange(F, dtype=torch.float64)
            k = torch.arange(self._n_mfcc, dtype=torch.float64).unsqueeze(1)
            dct = torch.cos(math.pi / F * (n + 0.5) * k)
            dct[0] *= 1.0 / math.sqrt(2.0)
            self._dct = (dct * math.sqrt(2.0 / F)).t().contiguous().float().to(logmel.device)        # (n_mels, n_mfcc)
        mf = torch.empty((B, T, self._n_mfcc), dtype=torch.float32, device=logmel.device)
        N.check(lib.vp_dense_f32(ctx, N.ptr(logmel), F, N.ptr(self._dct), 1, None, B * T, self._n_mfcc, F, N.VP_ACT_NONE, N.ptr(mf),
                                 self._n_mfcc, N.stream_ptr()), ctx)
        mf16 = torch.empty_like(mf, dtype=torch.bfloat16) if want_bf16 else None
        if mf16 is not None:
            N.check(lib.vp_cast_f32_bf16(ctx, N.ptr(mf), N.ptr(mf16), mf.numel(), N.stream_ptr()), ctx)
        return mf, mf16

    def forward_ragged(self, waveforms, n_samples, want_bf16=False):
        """The training loader's semantics for a ragged batch: utterance b occupies the first n_samples[b] samples of row b;
        it is featurised as if alone (time mean over ITS frames -- the reference's per-utterance call, reader.py:102-103) and
        the rows past its last frame are zero (collate_fn.py:5-23).  Returns (features (B, T, F), input_lens (B,) int64).
        One batched launch for every built method: 'Fbank', and the mel family ('MelSpectrogram', 'LogMelSpectrogram', 'MFCC'
        with its DCT over the whole batch), whose rows equal the utterance's own forward() bit for bit.  With want_bf16 the
        bf16 copy is attached as ``._vp_bf16``.  A mel-family utterance of n_fft/2 samples or fewer cannot be reflect-padded and
        raises, as its own forward() does; lengths that arrive as a GPU tensor cost one readback of their minimum for that."""
        if self._opts is None:
            raise NotImplementedError(f'feature_method {self._feature_method} is not built on the HIP engine yet '
                                      '(Fbank is); there is no CPU fallback')
        if not waveforms.is_cuda:
            raise N.VpmiError('AudioFeaturizer needs GPU tensors: the engine has no CPU fallback')
        wav = waveforms.contiguous().float()
        B, L = wav.shape
        mel = self._feature_method != 'Fbank'
        if mel:
            shortest = min(int(torch.as_tensor(n_samples).min()), L)
            if shortest <= self._opts.n_fft // 2:
                raise N.VpmiError(f'libvpmi error {N.VP_EINVAL}: melspec: {shortest} samples are too few for reflect padding of '
                                  f'{self._opts.n_fft // 2}')
        ns = torch.as_tensor(n_samples).to(device=wav.device, dtype=torch.int32).contiguous()
        lib, ctx = N.lib(), N.ctx(wav.device)
        T = (lib.vp_mel_num_frames if mel else lib.vp_fbank_num_frames)(C.byref(self._opts), L)
        if T <= 0:
            raise ValueError(f'{L} samples are shorter than one analysis window')
        F = self._opts.n_mels
        mfcc = self._feature_method == 'MFCC'
        out = torch.empty((B, T, F), dtype=torch.float32, device=wav.device)
        out16 = torch.empty((B, T, F), dtype=torch.bfloat16, device=wav.device) if want_bf16 and not mfcc else None
        nf = torch.empty((B,), dtype=torch.int32, device=wav.device)
        nws = (lib.vp_mel_workspace_bytes if mel else lib.vp_fbank_workspace_bytes)(C.byref(self._opts), B, L)
        ws = self._ws.get(nws, wav.device)
        fn = lib.vp_melspec_cmn_ragged_f32 if mel else lib.vp_fbank_cmn_ragged_f32
        N.check(fn(ctx, N.ptr(wav), N.ptr(ns), B, L, C.byref(self._opts), N.ptr(out), N.ptr(out16), N.ptr(nf), N.ptr(ws), ws.numel(),
                   N.stream_ptr()), ctx)
        if mfcc:
            out, out16 = self._mfcc(out, want_bf16)             # zero rows stay zero: the DCT has no bias
        if out16 is not None:
            out._vp_bf16 = out16
        return out, nf.to(torch.int64)

    @property
    def feature_dim(self):
        """返回特征大小"""
        if self._feature_method == 'LogMelSpectrogram':
            return self._method_args.get('n_mels', 128)
        elif self._feature_method == 'MelSpectrogram':
            return self._method_args.get('n_mels', 64)
        elif self._feature_method == 'Spectrogram':
            return self._method_args.get('n_fft', 512) // 2 + 1
        elif self._feature_method == 'MFCC':
            return self._method_args.get('n_mfcc', 40)
        elif self._feature_method == 'Fbank':
            return self._method_args.get('n_mels', 23)
        else:
            raise Exception('没有{}预处理方法'.format(self._feature_method))
