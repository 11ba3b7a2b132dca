"""CPU tests of the featurizer option sweep's reference (tests/featurizer_oracle.py, oracle/fbank.py): the float64 reference
pinned, one frame per option set, against a direct O(N K) DFT written here from the Kaldi / librosa definitions; the integer frame
geometry of the C library against the oracle's; and the proof that the GPU tests' bounds would catch a subtly wrong kernel: each
listed mutation of the float64 reference moves some planted signal by at least ten times the bound of its case.
"""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import fbank as ofb
from tests import featurizer_oracle as fo


# ------------------------------------------------------------------------------------------------------------ the case table
def test_case_table_classes_and_geometry():
    for cid, args, win, shift, cls in fo.FBANK_CASES:
        assert fo.geometry(args) == (win, shift, 512), cid
        assert fo.kernel_class(args) == cls, (cid, fo.kernel_class(args))
    assert fo.exercised_classes() == {'13', '16', 'old', 'pcm16_13', 'pcm16_16'}
    # the edges the table claims: NP1 = 13 exactly for win 385 .. 416; eight rounds; the odd shift is not PCM16 material
    assert [(w + 31) // 32 for w in (384, 385, 416, 417)] == [12, 13, 13, 14]
    assert not fo.pcm16_covered(fo.FBANK_BY_ID['m80_win480_shift161'][1], 4000)
    assert not fo.pcm16_covered(fo.FBANK_BY_ID['m23'][1], 4000) and fo.pcm16_covered(fo.FBANK_BY_ID['m80'][1], 4000)
    assert not fo.pcm16_covered(fo.FBANK_BY_ID['m80'][1], 4001)


def test_signals_are_what_they_claim():
    x = fo.signals(4000, 160, 16000, seed=3)
    assert x.shape == (7, 4000) and x.dtype == np.float32 and np.max(np.abs(x)) <= 1.0
    assert abs(float(np.sqrt(np.mean(x[0].astype(np.float64) ** 2))) - 0.1) < 0.01
    assert abs(float(x[2].mean()) - 0.5) < 1e-2 and np.all(x[6] == 0.0)
    assert np.all(x[5, ::160] > 0.89) and np.max(np.abs(np.delete(x[5], np.arange(0, 4000, 160)))) < 1e-3
    assert np.array_equal(x, fo.signals(4000, 160, 16000, seed=3))
    # silence: the log floor minus its own mean -- zero up to the rounding of a T-term mean of equal values
    ref = fo.fbank_ref(x[6:], dict(sr=16000, n_mels=80))
    assert np.max(np.abs(ref)) <= 8 * np.finfo(np.float64).eps * abs(math.log(1e-7))


# --------------------------------------------------------------------------------------- the float64 reference, independently
def _kaldi_mel(f):
    return 1127.0 * math.log(1.0 + f / 700.0)


def direct_fbank_frame(wave, t, sr=16000, n_mels=23, frame_length=25.0, frame_shift=10.0, preemphasis_coefficient=0.97,
                       remove_dc_offset=True, low_freq=20.0, high_freq=0.0):
    """Frame t of Kaldi's log-mel filterbank energies in float64: loops and a DFT sum, no helper of the oracle."""
    win, shift = int(sr * frame_length * 0.001), int(sr * frame_shift * 0.001)
    nfft = 1
    while nfft < win:
        nfft *= 2
    fr = [float(v) for v in wave[t * shift:t * shift + win]]
    if remove_dc_offset:
        mean = sum(fr) / win
        fr = [v - mean for v in fr]
    fr = [fr[i] - preemphasis_coefficient * fr[max(i - 1, 0)] for i in range(win)]
    fr = [fr[i] * (0.5 - 0.5 * math.cos(2.0 * math.pi * i / (win - 1))) ** 0.85 for i in range(win)]
    fr = np.asarray(fr + [0.0] * (nfft - win))
    k = np.arange(nfft // 2)[:, None]                                        # bins 0 .. nfft/2 - 1: Nyquist carries no weight
    power = np.abs(np.exp(-2j * math.pi * k * np.arange(nfft)[None, :] / nfft) @ fr) ** 2
    if high_freq <= 0.0:
        high_freq += 0.5 * sr
    lo, hi = _kaldi_mel(low_freq), _kaldi_mel(high_freq)
    d = (hi - lo) / (n_mels + 1)
    out = np.zeros(n_mels)
    for m in range(n_mels):
        l, c, r = lo + m * d, lo + (m + 1) * d, lo + (m + 2) * d
        e = 0.0
        for b in range(nfft // 2):
            x = _kaldi_mel(b * sr / nfft)
            if l < x < r:
                e += power[b] * ((x - l) / (c - l) if x <= c else (r - x) / (r - c))
        out[m] = math.log(max(e, 1e-7))
    return out


@pytest.mark.parametrize('cid', fo.FBANK_IDS)
def test_fbank_reference_matches_a_direct_dft(cid):
    _, args, win, shift, _ = fo.FBANK_BY_ID[cid]
    x = fo.signals(win + 3 * shift + 5, shift, args['sr'], seed=17)
    for row in (1, 3, 4):                                                    # low-passed noise, tone, ramp
        ref = ofb.kaldi_fbank(x[row], dtype=np.float64, **args)
        assert ref.shape == (4, args['n_mels'])
        for t in (0, 3):
            assert np.max(np.abs(ref[t] - direct_fbank_frame(x[row], t, **args))) <= 1e-10, (cid, row, t)


def _slaney_hz(m):
    return 200.0 / 3 * m if m < 15.0 else 1000.0 * math.exp(math.log(6.4) / 27.0 * (m - 15.0))


def _slaney_mel(f):
    return f / (200.0 / 3) if f < 1000.0 else 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


def direct_mel_frame(wave, t, sr=22050, n_fft=2048, hop_length=512, win_length=None, n_mels=64, f_min=50.0, f_max=None, power=2.0):
    """Frame t of librosa's mel spectrogram (center, reflect, periodic Hann centred in the FFT frame, Slaney scale and norm)."""
    wl = win_length or n_fft
    L = len(wave)

    def sample(i):                                                           # reflect without repeating the edge sample
        i = -i if i < 0 else i
        return float(wave[2 * (L - 1) - i if i >= L else i])
    lpad = (n_fft - wl) // 2
    fr = np.zeros(n_fft)
    for i in range(wl):
        fr[lpad + i] = sample(t * hop_length - n_fft // 2 + lpad + i) * (0.5 - 0.5 * math.cos(2.0 * math.pi * i / wl))
    k = np.arange(n_fft // 2 + 1)[:, None]
    mag = np.abs(np.exp(-2j * math.pi * k * np.arange(n_fft)[None, :] / n_fft) @ fr) ** power
    f_max = 0.5 * sr if f_max is None else f_max
    mlo, mhi = _slaney_mel(f_min), _slaney_mel(f_max)
    edges = [_slaney_hz(mlo + (mhi - mlo) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    out = np.zeros(n_mels)
    for m in range(n_mels):
        for b in range(n_fft // 2 + 1):
            f = b * sr / n_fft
            w = min((f - edges[m]) / (edges[m + 1] - edges[m]), (edges[m + 2] - f) / (edges[m + 2] - edges[m + 1]))
            if w > 0.0:
                out[m] += mag[b] * w * 2.0 / (edges[m + 2] - edges[m])
    return out


@pytest.mark.parametrize('cid', [c for c in fo.MEL_IDS if fo.MEL_BY_ID[c][1] == 'MelSpectrogram'])
def test_mel_reference_matches_a_direct_dft(cid):
    _, _, args, L = fo.MEL_BY_ID[cid]
    x = fo.signals(L, args['hop_length'], args['sr'], seed=19)
    for row in (1, 3):
        ref = ofb.mel_spectrogram(x[row], dtype=np.float64, **args)
        T = 1 + L // args['hop_length']
        assert ref.shape == (T, args['n_mels'])
        for t in (0, T - 1):                                                 # both frames reflect
            d = direct_mel_frame(x[row], t, **args)
            assert np.max(np.abs(ref[t] - d)) <= 1e-10 * max(1.0, float(np.max(d))), (cid, row, t)


@pytest.mark.parametrize('cid', fo.MEL_IDS)
def test_mel_restatement_in_float64_is_the_oracle(cid):
    """fo.mel_feat exists for its float32 run; in float64 it must be the oracle, log-mel and MFCC epilogues included."""
    _, method, args, L = fo.MEL_BY_ID[cid]
    x = fo.signals(L, args['hop_length'], args['sr'], seed=23)
    ratio = np.linspace(1.0, 0.3, len(x)).astype(np.float32)
    a, b = fo.mel_feat(x, method, args, np.float64, ratio), fo.mel_oracle(x, method, args, ratio)
    assert a.shape == b.shape and np.max(np.abs(a - b)) <= 1e-9 * max(1.0, float(np.max(np.abs(b))))


def test_mel_shortest_length_gives_two_frames():
    """L = n_fft/2 + 1 is the shortest length reflect padding allows (paddle and librosa refuse one fewer; NumPy's pad does not, so
    the refusal itself is pinned on the engine, in the GPU tests)."""
    _, _, args, L = fo.MEL_BY_ID['mel512_shortest']
    assert L == args['n_fft'] // 2 + 1
    assert ofb.mel_spectrogram(np.ones(L, np.float32), dtype=np.float64, **args).shape == (2, 80)


def test_pcm16_routing_rule_matches_the_kernel_class():
    """AudioFeaturizer decides up front whether int16 input takes the 16-bit entry; its rule must be the library's."""
    from ppvector.data_utils import featurizer as fz
    for cid, args, _, _, _ in fo.FBANK_CASES:
        assert fz._fbank_pcm16_covered(fz.AudioFeaturizer._fbank_opts(args)) == fo.pcm16_covered(args, 4000), cid
    for args in (dict(sr=16000, n_mels=80, frame_length=40.0), dict(sr=16000, n_mels=129)):      # refused by the library
        assert not fz._fbank_pcm16_covered(fz.AudioFeaturizer._fbank_opts(args))


# -------------------------------------------------------------------------------------------------------- integer geometry
def test_library_frame_counts_agree_with_the_oracle():
    """vp_fbank_num_frames / vp_mel_num_frames (float32 products truncated in C) against frame_geometry (double in Python), at the
    lengths around every frame boundary the GPU tests use."""
    from ppvector import _native as N
    from ppvector.data_utils.featurizer import AudioFeaturizer
    lib = N.lib()
    for cid, args, win, shift, _ in fo.FBANK_CASES:
        o = AudioFeaturizer._fbank_opts(args)
        for L in [win - 1, 1] + [l + d for l in fo.fbank_lengths(win, shift, args['sr']) for d in (-1, 0, 1)] + [win + 63 * shift]:
            assert lib.vp_fbank_num_frames(C.byref(o), L) == ofb.num_frames(L, win, shift), (cid, L)
    for cid, method, args, L in fo.MEL_CASES:
        a = dict(args)
        a.pop('n_mfcc', None)
        o = AudioFeaturizer._mel_opts(a, log=method != 'MelSpectrogram')
        for n in (L - 1, L, L + 1, args['hop_length'] - 1, args['hop_length'], 10 * args['hop_length'] - 1):
            assert lib.vp_mel_num_frames(C.byref(o), n) == 1 + n // args['hop_length'], (cid, n)


# ------------------------------------------------------------------------------------------------------ mutation sensitivity
def _fbank_signals(cid, extra=0):
    _, args, win, shift, _ = fo.FBANK_BY_ID[cid]
    return args, fo.signals(win + 32 * shift + extra, shift, args['sr'], seed=29)


@pytest.mark.parametrize('cid', fo.FBANK_IDS)
def test_fbank_bound_and_mutation_sensitivity(cid):
    """With no mutation fo.fbank_f64 is the oracle; every mutation that is not the identity on this option set moves at least one
    planted signal by >= 10 x the max bound the GPU parity test asserts for the case (margin x e32 + floor with the case's margin, capped at 2e-3)."""
    args, x1 = _fbank_signals(cid, extra=1)
    x = x1[:, :-1]
    ref = fo.fbank_ref(x, args)
    assert np.max(np.abs(fo.fbank_f64(x1, args) - ref)) <= 1e-10
    e32 = fo.deviation(fo.fbank_ref(x, args, dtype=np.float32), ref)
    bmax, bmean = fo.bound(e32, ref, fo.fbank_margin(args), fo.FBANK_CAP)
    assert 0.0 < bmax <= 2e-3 and 0.0 < bmean <= 2e-5
    muts = fo.fbank_mutations_for(args)
    assert {'window_periodic', 'window_short', 'frame_start+1', 'bank_shift'} <= set(muts)
    moved = {}
    for m in muts:
        d = np.abs(fo.fbank_f64(x1, args, m) - ref).reshape(len(x), -1).max(axis=1)
        moved[m] = float(d.max())
        assert d[6] <= 1e-12                                                # silence stays the floor under every mutation
    print(f'{cid}: e32 max {e32[0]:.2e} mean {e32[1]:.2e}  bound {bmax:.2e}/{bmean:.2e}  moved ' +
          ' '.join(f'{k} {v:.2e}' for k, v in moved.items()))
    weak = {k: v for k, v in moved.items() if v < 10.0 * bmax}
    assert not weak, (weak, bmax)


def test_fbank_mutation_list_is_complete_over_the_table():
    """Every listed mutation is applied to at least one <13>, one <16> and one fallback case."""
    seen = {m: set() for m in fo.FBANK_MUTATIONS}
    for _, args, _, _, cls in fo.FBANK_CASES:
        for m in fo.fbank_mutations_for(args):
            seen[m].add(cls)
    for m in ('dc_div_nfft', 'dc_skipped', 'preemph_ignored', 'window_periodic', 'window_short', 'frame_start+1', 'nyquist_weight', 'bank_shift'):
        assert seen[m] == {'13', '16', 'old'}, (m, seen[m])
    assert seen['low_freq_ignored'] and seen['high_freq_ignored']


@pytest.mark.parametrize('cid', [c for c in fo.MEL_IDS if fo.mel_mutations_for(fo.MEL_BY_ID[c][2])])
def test_mel_mutation_sensitivity(cid):
    _, method, args, L = fo.MEL_BY_ID[cid]
    x = fo.signals(L, args['hop_length'], args['sr'], seed=31)
    ref = fo.mel_oracle(x, method, args)
    e32 = fo.mel_metric(fo.mel_feat(x, method, args, np.float32), ref, method)
    bmax, _ = fo.mel_bound(e32, ref, method)
    for m in fo.mel_mutations_for(args):
        moved = fo.mel_metric(fo.mel_feat(x, method, args, np.float64, mutation=m), ref, method)[0]
        print(f'{cid}: e32 {e32[0]:.2e} bound {bmax:.2e} {m} moved {moved:.2e}')
        assert moved >= 10.0 * bmax, (m, moved, bmax)


def test_mel_mutations_cover_power_fmax_and_odd_window():
    seen = set()
    for _, _, args, _ in fo.MEL_CASES:
        seen |= set(fo.mel_mutations_for(args))
    assert seen == set(fo.MEL_MUTATIONS)
