"""Reference, planted signals and case tables for the featurizer option sweep (tests/test_featurizer_oracle_cpu.py,
tests/test_gpu_featurizer_options.py).  TEST INFRASTRUCTURE ONLY.

The reference is oracle/fbank.py run in float64.  Nothing of the operation is restated here except
  * `kernel_class`: which frame kernel csrc/fbank.hip picks for an option set (the rule of build_tables / launch_frames),
  * `fbank_f64` and the mutations of `mel_feat`: float64 restatements with switchable MUTATIONS, used only to show that a subtly
    wrong kernel would move the output by far more than the bound the GPU tests assert (with no mutation they equal the oracle,
    which is tested),
  * `mel_feat` in float32: the float32 restatement of the mel family (the oracle's log-mel and MFCC always go through float64).
"""
import math

import numpy as np

from oracle import fbank as ofb

F32_EPS = float(np.finfo(np.float32).eps)

# ------------------------------------------------------------------------------------------------------------- Fbank cases
# (id, method args, window / shift in samples, kernel class).  Classes: '13' / '16' = fbank_frames16_kernel<13 / 16>, 'old' =
# fbank_frames_kernel (the bank does not fit the four-frames-per-wave layout).
FBANK_CASES = [
    ('m80', dict(sr=16000, n_mels=80), 400, 160, '13'),
    ('m80_win385', dict(sr=16000, n_mels=80, frame_length=24.0625), 385, 160, '13'),
    ('m80_win416', dict(sr=16000, n_mels=80, frame_length=26.0), 416, 160, '13'),
    ('m64_win320', dict(sr=16000, n_mels=64, frame_length=20.0), 320, 160, '16'),
    ('m80_win512', dict(sr=16000, n_mels=80, frame_length=32.0, frame_shift=12.5), 512, 200, '16'),
    ('m80_win480_shift161', dict(sr=16000, n_mels=80, frame_length=30.0, frame_shift=10.0625), 480, 161, '16'),
    ('m40_win257_shift80', dict(sr=16000, n_mels=40, frame_length=16.0625, frame_shift=5.0), 257, 80, '16'),
    ('sr8k_m40_band', dict(sr=8000, n_mels=40, frame_length=50.0, frame_shift=20.0, low_freq=100.0, high_freq=-200.0), 400, 160, '13'),
    ('sr8k_m80_win320', dict(sr=8000, n_mels=80, frame_length=40.0), 320, 80, '16'),
    ('m128_8rounds', dict(sr=16000, n_mels=128, low_freq=0.0, high_freq=7600.0), 400, 160, '13'),
    ('m48_narrow', dict(sr=16000, n_mels=48, low_freq=300.0, high_freq=3400.0), 400, 160, '13'),
    ('m96_high-4000', dict(sr=16000, n_mels=96, high_freq=-4000.0), 400, 160, '13'),
    ('m23', dict(sr=16000, n_mels=23), 400, 160, 'old'),
    ('m16', dict(sr=16000, n_mels=16), 400, 160, 'old'),
    ('m1', dict(sr=16000, n_mels=1), 400, 160, 'old'),
    # preemphasis x DC removal over one <13>, one <16> and one fallback case
    ('m80_pre0', dict(sr=16000, n_mels=80, preemphasis_coefficient=0.0), 400, 160, '13'),
    ('m80_nodc', dict(sr=16000, n_mels=80, remove_dc_offset=False), 400, 160, '13'),
    ('m80_pre0_nodc', dict(sr=16000, n_mels=80, preemphasis_coefficient=0.0, remove_dc_offset=False), 400, 160, '13'),
    ('m64_win320_pre0', dict(sr=16000, n_mels=64, frame_length=20.0, preemphasis_coefficient=0.0), 320, 160, '16'),
    ('m64_win320_nodc', dict(sr=16000, n_mels=64, frame_length=20.0, remove_dc_offset=False), 320, 160, '16'),
    ('m64_win320_pre0_nodc', dict(sr=16000, n_mels=64, frame_length=20.0, preemphasis_coefficient=0.0, remove_dc_offset=False), 320, 160, '16'),
    ('m23_pre0', dict(sr=16000, n_mels=23, preemphasis_coefficient=0.0), 400, 160, 'old'),
    ('m23_nodc', dict(sr=16000, n_mels=23, remove_dc_offset=False), 400, 160, 'old'),
    ('m23_pre0_nodc', dict(sr=16000, n_mels=23, preemphasis_coefficient=0.0, remove_dc_offset=False), 400, 160, 'old'),
]
FBANK_IDS = [c[0] for c in FBANK_CASES]
FBANK_BY_ID = {c[0]: c for c in FBANK_CASES}

# csrc/fbank.hip
F16_MAX_TAPS, F16_MAX_WPAD, F16_MAX_ROUNDS, FB_NFFT, FRAMES_PER_WG = 32, 1536, 8, 512, 16


def fbank_opts(args):
    o = dict(ofb.FBANK_DEFAULTS)
    o.update(args)
    return o


def geometry(args):
    o = fbank_opts(args)
    return ofb.frame_geometry(o['sr'], o['frame_length'], o['frame_shift'])


def kernel_class(args):
    """'13', '16' or 'old' by the rule of build_tables (rounds of 16 filters, taps padded to the round's longest filter rounded up
    to 4, at most F16_MAX_TAPS per round and F16_MAX_WPAD in all) and launch_frames (NP1 = 13 iff ceil(win / 32) == 13)."""
    o = fbank_opts(args)
    win, _, nfft = geometry(args)
    assert nfft == FB_NFFT
    bank = ofb.mel_banks(o['n_mels'], nfft, o['sr'], o['low_freq'], o['high_freq'])[:, :nfft // 2]
    taps = []
    for row in bank:
        nz = np.nonzero(row > 0.0)[0]
        taps.append(int(nz[-1] - nz[0] + 1) if len(nz) else 0)
    nr = (o['n_mels'] + 15) // 16
    ok, wpad = nr <= F16_MAX_ROUNDS, 0
    for r in range(nr):
        mx = max(4, (max(taps[16 * r:16 * r + 16]) + 3) // 4 * 4)
        ok = ok and mx <= F16_MAX_TAPS
        wpad += 16 * mx
    if not (ok and wpad <= F16_MAX_WPAD):
        return 'old'
    return '13' if (win + 31) // 32 == 13 else '16'


def pcm16_covered(args, L):
    """vp_fbank_cmn_pcm16 covers: the four-frames-per-wave kernels, an even shift, an even row length."""
    return kernel_class(args) != 'old' and geometry(args)[1] % 2 == 0 and L % 2 == 0


def exercised_classes():
    """Every kernel the case table reaches, PCM16 instantiations included."""
    out = set()
    for _, args, _, shift, _ in FBANK_CASES:
        k = kernel_class(args)
        out.add(k)
        if k != 'old' and shift % 2 == 0:
            out.add('pcm16_' + k)
    return out


def fbank_lengths(win, shift, sr):
    """T = 1; T = 1 with a tail no frame covers; T = 2; T = 16, 17, 33 (the FRAMES_PER_WG edges); about 0.5 s."""
    return [win, win + shift - 1, win + shift, win + 15 * shift, win + 16 * shift + 3, win + 32 * shift, sr // 2 + 7]


# ------------------------------------------------------------------------------------------------------------ planted signals
SIGNALS = ('white', 'lowpass', 'dc', 'tone', 'ramp', 'impulses', 'silence')


def signals(L, shift, sr, seed):
    """(7, L) float32, |x| <= 1, each over a noise floor (no mel bin at the float32 FFT noise floor, where float32 and float64
    legitimately disagree by O(1) in the log); the last row is digital silence."""
    rng = np.random.RandomState(seed)
    n = rng.standard_normal((6, L))
    t = np.arange(L, dtype=np.float64)
    lp = np.empty(L)
    acc = 0.0
    for i in range(L):
        acc = 0.9 * acc + 0.1 * n[1, i]
        lp[i] = acc
    imp = np.zeros(L)
    imp[::shift] = 0.9
    x = np.stack([
        0.1 * n[0],                                                          # white noise, -20 dBFS
        0.1 * lp / max(np.sqrt(np.mean(lp ** 2)), 1e-12),                    # one-pole low-passed noise, -20 dBFS
        0.5 + 0.01 * n[2],                                                   # DC handling
        0.5 * np.sin(2.0 * math.pi * 1000.0 * t / sr) + 5e-4 * n[3],         # window shape, bin placement
        np.linspace(-0.8, 0.8, L) + 0.01 * n[4],                             # the DC divisor
        imp + 1e-4 * n[5],                                                   # frame placement
        np.zeros(L)])
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def pcm_of(x):
    """float signals -> int16 PCM and the samples a reader widens them to."""
    pcm = np.clip(np.round(x.astype(np.float64) * 32767.0), -32768, 32767).astype(np.int16)
    return pcm, pcm.astype(np.float32) * np.float32(1.0 / 32768.0)


# ------------------------------------------------------------------------------------------------------------------- bounds
def deviation(got, ref):
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    return float(d.max()), float(d.mean())


def bound(e32, ref, margin, cap):
    """(max, mean) bounds: margin x the float32 restatement's own deviation from float64 plus ten float32 ulps of the largest
    |output|, never looser than `cap` = what the existing tests of the method assert.  margin: one number or (for max, for mean)."""
    floor = 10.0 * F32_EPS * float(np.max(np.abs(ref)))
    mmax, mmean = margin if isinstance(margin, tuple) else (margin, margin)
    return min(mmax * e32[0] + floor, cap[0]), min(mmean * e32[1] + floor, cap[1])


FBANK_CAP = (2e-3, 2e-5)          # tests/test_gpu_kernels.py::test_fbank_matches_oracle
MARGIN = 4.0
# Without pre-emphasis the max deviation needs 8: it is set by a handful of far mel bins of the 1 kHz tone row, 60 dB and more below
# the tone (pre-emphasis would lift the noise floor there by up to 30 dB), where any float32 FFT is off by eps x the TONE's magnitude
# and the largest such error over the case is an extreme value that depends on the factorisation.  Two float32 FFTs on the CPU
# (NumPy's pocketfft, torch.fft) disagree there by up to 5.8 x in max on these cases, 1.2 - 3.3 x on the others, while the means
# agree within 2.2 x everywhere; the kernel (16 x 16 in registers) measured 4.6 - 7.2 x in max, 1.8 x in mean
# (docs/featurizer_options.md).  The mean keeps 4 and the cap of 2e-3 holds.
MARGIN_MAX_NO_PREEMPH = 8.0


def fbank_margin(args):
    if fbank_opts(args)['preemphasis_coefficient'] == 0.0:
        return (MARGIN_MAX_NO_PREEMPH, MARGIN)
    return (MARGIN, MARGIN)


def fbank_ref(x, args, ratio=None, dtype=np.float64):
    return ofb.featurize(np.asarray(x, dtype), ratio, method_args=args, dtype=dtype)


def fbank_ragged_ref(x, lens, args, dtype=np.float64):
    """Per-utterance featurise, then zero-pad to the longest row's frame count (reader + collate_fn)."""
    win, shift, _ = geometry(args)
    T = ofb.num_frames(x.shape[1], win, shift)
    out = np.zeros((len(lens), T, fbank_opts(args)['n_mels']), dtype)
    nf = []
    for b, n in enumerate(lens):
        f = fbank_ref(x[b:b + 1, :n], args, dtype=dtype)[0]
        out[b, :len(f)] = f
        nf.append(len(f))
    return out, nf


# ----------------------------------------------------------------------------------------------- mutable float64 restatements
FBANK_MUTATIONS = ('dc_div_nfft', 'dc_skipped', 'preemph_ignored', 'window_periodic', 'window_short', 'frame_start+1', 'nyquist_weight',
                   'bank_shift', 'low_freq_ignored', 'high_freq_ignored')


def fbank_f64(x, args, mutation=None):
    """(B, L') -> (B, T, F) float64 with CMN; L' may hold one sample more than the length featurised (for 'frame_start+1'), T is
    that of L = x.shape[1] - 1."""
    o = fbank_opts(args)
    dflt = ofb.FBANK_DEFAULTS
    win, shift, nfft = geometry(args)
    x = np.asarray(x, np.float64)
    T = ofb.num_frames(x.shape[1] - 1, win, shift)
    idx = np.arange(T)[:, None] * shift + np.arange(win)[None, :] + (1 if mutation == 'frame_start+1' else 0)
    fr = x[:, idx]                                                            # (B, T, win)
    if o['remove_dc_offset'] and mutation != 'dc_skipped':
        fr = fr - fr.sum(axis=2, keepdims=True) / (nfft if mutation == 'dc_div_nfft' else win)
    pc = dflt['preemphasis_coefficient'] if mutation == 'preemph_ignored' else o['preemphasis_coefficient']
    if pc != 0.0:
        fr = fr - pc * np.concatenate([fr[:, :, :1], fr[:, :, :-1]], axis=2)
    n = np.arange(win, dtype=np.float64)
    if mutation == 'window_periodic':
        w = (0.5 - 0.5 * np.cos(2.0 * math.pi * n / win)) ** 0.85
    elif mutation == 'window_short':
        w = np.concatenate([ofb.povey_window(win - 1), [0.0]])
    else:
        w = ofb.povey_window(win)
    fr = np.concatenate([fr * w, np.zeros(fr.shape[:2] + (nfft - win,))], axis=2)
    pw = np.abs(np.fft.rfft(fr, axis=2)) ** 2
    lo = dflt['low_freq'] if mutation == 'low_freq_ignored' else o['low_freq']
    hi = dflt['high_freq'] if mutation == 'high_freq_ignored' else o['high_freq']
    bank = ofb.mel_banks(o['n_mels'], nfft, o['sr'], lo, hi)
    if mutation == 'nyquist_weight':                                          # the bank evaluated one bin too far: the Nyquist column
        bank = bank.copy()                                                    # takes the weight of its neighbour
        bank[:, -1] = bank[:, -2]
    if mutation == 'bank_shift':
        bank = np.roll(bank, 1, axis=1)
    e = np.log(np.maximum(pw @ bank.T, o['eps']))
    return e - e.mean(axis=1, keepdims=True)


def fbank_mutations_for(args):
    """The mutations that are not the identity on this option set."""
    o = fbank_opts(args)
    d = ofb.FBANK_DEFAULTS
    win, _, nfft = geometry(args)
    skip = set()
    if not o['remove_dc_offset']:
        skip |= {'dc_div_nfft', 'dc_skipped'}
    if win == nfft:
        skip.add('dc_div_nfft')
    if o['preemphasis_coefficient'] == d['preemphasis_coefficient']:
        skip.add('preemph_ignored')
    if o['low_freq'] == d['low_freq']:
        skip.add('low_freq_ignored')
    if o['high_freq'] == d['high_freq']:
        skip.add('high_freq_ignored')
    if ofb.mel_banks(o['n_mels'], nfft, o['sr'], o['low_freq'], o['high_freq'])[:, -2].max() == 0.0:
        skip.add('nyquist_weight')                                            # no filter reaches the last bin: nothing to leak
    return [m for m in FBANK_MUTATIONS if m not in skip]


# --------------------------------------------------------------------------------------------------------------- mel family
# (id, feature_method, method args, L)
MEL_CASES = [
    ('mel512_p2', 'MelSpectrogram', dict(sr=16000, n_fft=512, hop_length=160, win_length=400, n_mels=80, f_min=20.0, power=2.0), 4007),
    ('mel512_p1', 'MelSpectrogram', dict(sr=16000, n_fft=512, hop_length=160, win_length=400, n_mels=80, f_min=20.0, power=1.0), 4007),
    ('mel512_p1.5_win401', 'MelSpectrogram', dict(sr=16000, n_fft=512, hop_length=160, win_length=401, n_mels=80, f_min=20.0, power=1.5), 4007),
    ('mel1024_p2_fmax7000', 'MelSpectrogram', dict(sr=16000, n_fft=1024, hop_length=320, win_length=1024, n_mels=64, f_min=50.0, f_max=7000.0), 6001),
    ('mel1024_p1_hop161', 'MelSpectrogram', dict(sr=16000, n_fft=1024, hop_length=161, win_length=1024, n_mels=64, f_min=50.0, power=1.0), 6001),
    ('mel1024_p1.5', 'MelSpectrogram', dict(sr=16000, n_fft=1024, hop_length=320, win_length=800, n_mels=64, f_min=50.0, power=1.5), 6001),
    ('mel2048_p2', 'MelSpectrogram', dict(sr=22050, n_fft=2048, hop_length=512, n_mels=64, power=2.0), 9001),
    ('mel2048_p1', 'MelSpectrogram', dict(sr=22050, n_fft=2048, hop_length=512, n_mels=64, power=1.0), 9001),
    ('mel2048_p1.5', 'MelSpectrogram', dict(sr=22050, n_fft=2048, hop_length=512, n_mels=64, power=1.5), 9001),
    ('mel512_sr8k_fmax3800', 'MelSpectrogram', dict(sr=8000, n_fft=512, hop_length=80, win_length=200, n_mels=40, f_min=20.0, f_max=3800.0), 2400),
    ('mel512_shortest', 'MelSpectrogram', dict(sr=16000, n_fft=512, hop_length=160, win_length=400, n_mels=80, f_min=20.0), 257),
    ('logmel_ref_amin', 'LogMelSpectrogram', dict(sr=16000, hop_length=160, n_mels=80, ref_value=0.5, amin=1e-8), 4007),
    ('mfcc_full', 'MFCC', dict(sr=16000, n_mfcc=40, n_fft=512, hop_length=160, n_mels=40, f_min=20.0), 4007),
]
MEL_IDS = [c[0] for c in MEL_CASES]
MEL_BY_ID = {c[0]: c for c in MEL_CASES}
# what the existing tests assert: linear mel relative to the largest |reference| (test_gpu_featurizer_ragged.py), log-mel in dB and
# MFCC absolute (test_gpu_kernels.py); the mean of the linear metric is left to the e32 rule
MEL_CAP = {'MelSpectrogram': (2e-5, 2e-5), 'LogMelSpectrogram': (5e-2, 1e-3), 'MFCC': (0.2, 5e-3)}
MEL_MUTATIONS = ('power_ignored', 'f_max_ignored', 'lpad_rounded_up')


def _dct(n_mfcc, n_mels, dtype):
    n = np.arange(n_mels, dtype=np.float64)
    k = np.arange(n_mfcc, dtype=np.float64)[:, None]
    d = np.cos(math.pi / n_mels * (n + 0.5) * k)
    d[0] *= 1.0 / math.sqrt(2.0)
    return (d * math.sqrt(2.0 / n_mels)).astype(dtype)


def mel_feat(x, method, args, dtype, ratio=None, mutation=None):
    """AudioFeaturizer.forward of the mel family in `dtype` THROUGHOUT (the oracle's log-mel and MFCC go through float64 whatever
    the dtype, so their float32 run is no float32 restatement); float64 equals the oracle (tested).  Mutations: see MEL_MUTATIONS."""
    a = dict(args)
    n_mfcc = a.pop('n_mfcc', 40)
    ref_value, amin = a.pop('ref_value', 1.0), a.pop('amin', 1e-10)
    if method != 'MelSpectrogram':
        a.setdefault('n_fft', 512)
    if mutation == 'power_ignored':
        a['power'] = 2.0
    if mutation == 'f_max_ignored':
        a['f_max'] = None
    feats = []
    for w in np.asarray(x, dtype):
        if mutation == 'lpad_rounded_up':
            m = _mel_lpad_up(w, a)
        else:
            m = ofb.mel_spectrogram(w, dtype=dtype, **a)
        if method != 'MelSpectrogram':
            m = (dtype(10.0) * np.log10(np.maximum(m, dtype(amin))) - dtype(10.0 * math.log10(max(ref_value, amin)))).astype(dtype)
        if method == 'MFCC':
            m = (m @ _dct(n_mfcc, m.shape[1], dtype).T).astype(dtype)
        feats.append(m)
    f = np.stack(feats)
    f = f - f.mean(axis=1, keepdims=True, dtype=dtype)
    if ratio is not None:
        T = f.shape[1]
        lens = (np.asarray(ratio, np.float32) * np.float32(T)).astype(np.int32)
        f = np.where((np.arange(T)[None, :] < lens[:, None])[:, :, None], f, np.zeros_like(f))
    return f.astype(dtype)


def _mel_lpad_up(w, a):
    """mel_spectrogram in float64 with the window's zero padding rounded the other way (ceil instead of floor on the left)."""
    o = dict(ofb.MEL_DEFAULTS)
    o.update(a)
    n_fft, wl, hop = int(o['n_fft']), int(o['win_length'] or o['n_fft']), int(o['hop_length'])
    x = np.asarray(w, np.float64)
    xp = np.pad(x, (n_fft // 2, n_fft // 2), mode='reflect')
    T = 1 + len(x) // hop
    n = np.arange(wl, dtype=np.float64)
    lpad = (n_fft - wl + 1) // 2
    win = np.pad(0.5 - 0.5 * np.cos(2.0 * math.pi * n / wl), (lpad, n_fft - wl - lpad))
    fr = xp[np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]] * win
    pw = np.abs(np.fft.rfft(fr, axis=1)) ** o['power']
    return pw @ ofb.slaney_mel_bank(o['sr'], n_fft, o['n_mels'], o['f_min'], o['f_max']).T


def mel_oracle(x, method, args, ratio=None):
    """The float64 reference: oracle/fbank.py."""
    log = {'MelSpectrogram': False, 'LogMelSpectrogram': True, 'MFCC': 'mfcc'}[method]
    return ofb.featurize_mel(np.asarray(x, np.float64), ratio, method_args=args, dtype=np.float64, log=log)


def mel_mutations_for(args):
    out = []
    if args.get('power', 2.0) != 2.0:
        out.append('power_ignored')
    if args.get('f_max') is not None:
        out.append('f_max_ignored')
    wl = args.get('win_length')
    if wl is not None and (args.get('n_fft', 512) - wl) % 2 == 1:
        out.append('lpad_rounded_up')
    return out


def mel_metric(got, ref, method):
    """(max, mean) deviation in the metric the existing tests of the method use: linear mel relative to the largest |reference| of
    the batch (the errors scale with the features before the time mean is taken off, so a per-utterance scale of the features
    after it would say nothing), log-mel in dB and MFCC absolute."""
    mx, mn = deviation(got, ref)
    if method == 'MelSpectrogram':
        s = float(np.max(np.abs(ref))) or 1.0
        return mx / s, mn / s
    return mx, mn


def mel_bound(e32, ref, method, margin=MARGIN):
    cap = MEL_CAP[method]
    floor = 10.0 * F32_EPS * (1.0 if method == 'MelSpectrogram' else float(np.max(np.abs(ref))))
    return min(margin * e32[0] + floor, cap[0]), min(margin * e32[1] + floor, cap[1])
