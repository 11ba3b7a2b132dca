"""Ragged batches of the mel family in one launch (vp_melspec_cmn_ragged_f32, AudioFeaturizer.forward_ragged) and
PPVectorTrainer.extract_features(batch_size=...).

The contract is the training loader's (reader.py:102-103 + collate_fn.py:5-23): every utterance featurised alone, features
zero-padded to the longest.  References are built that way from the oracle, one utterance at a time.  The samples past each
utterance's end are NaN in the GPU input: a kept value that read one would be NaN.  Row b must also equal, bit for bit, what the
dense entry point returns for that utterance alone.  Run with -m gpu on an MI355X.
"""
import ctypes as C
import os
import wave

import numpy as np
import pytest
import torch

from oracle import augment as oa
from oracle import fbank as ofb

pytestmark = pytest.mark.gpu

ARGS_512 = dict(sr=16000, n_fft=512, hop_length=160, win_length=400, n_mels=80, f_min=20.0)
ARGS_README = dict(sr=16000, n_fft=1024, hop_length=320, win_length=1024, n_mels=64, f_min=50.0)      # README.md:288-296
ARGS_DEFAULT = dict(sr=22050, n_mels=64)                                  # class defaults: n_fft 2048, hop 512 (2-wave kernel)
# 5120 samples at hop 160: the shortest legal utterance (2 frames), a last frame that exactly fills a 16-frame tile, one frame into
# the next tile, a length one sample short of a new frame; frames 33, 2, 16, 17, 16, 26
LENS_5120 = [5120, 257, 2400, 2560, 2559, 4001]


@pytest.fixture(scope='module')
def N():
    from ppvector import _native as N
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: these tests must run on an MI355X (no CPU fallback exists)')
    N.ctx(0)
    return N


def dev(x):
    return torch.as_tensor(np.asarray(x)).cuda().contiguous()


def poisoned(w, lens):
    """w with NaN past each utterance's end."""
    p = w.copy()
    for b, n in enumerate(lens):
        p[b, n:] = np.nan
    return p


def per_utterance_reference(w, lens, args, **kw):
    """The oracle on each utterance alone, then the oracle's collate: (per-utterance features, padded batch, input_lens)."""
    per = [ofb.featurize_mel(w[b:b + 1, :n], method_args=args, **kw)[0] for b, n in enumerate(lens)]
    ref, _, ref_lens = oa.collate([(f, 0) for f in per])
    return per, ref, ref_lens


def check_padding_and_alone(fz, w, lens, got, got_lens, ref, ref_lens, bits=True):
    """input_lens, zero rows, and (bits) bit identity of every row, and of its bf16 copy, with the utterance's own forward()."""
    assert got_lens.dtype == torch.int64 and np.array_equal(got_lens.cpu().numpy(), ref_lens)
    assert tuple(got.shape) == ref.shape and tuple(got._vp_bf16.shape) == ref.shape
    same = []
    for b, n in enumerate(lens):
        tb = int(ref_lens[b])
        assert float(got[b, tb:].abs().max() if tb < got.shape[1] else 0.0) == 0.0
        assert float(got._vp_bf16[b, tb:].float().abs().max() if tb < got.shape[1] else 0.0) == 0.0
        alone = fz(dev(w[b:b + 1, :n]), want_bf16=True)
        assert alone.shape[1] == tb
        same.append(torch.equal(got[b, :tb], alone[0]) and torch.equal(got._vp_bf16[b, :tb], alone._vp_bf16[0]))
    if bits:
        assert all(same), same
    return same


@pytest.mark.parametrize('args,L,lens', [
    (ARGS_512, 5120, LENS_5120),
    (ARGS_README, 9600, [9600, 513, 5120, 640]),
    (ARGS_DEFAULT, 16384, [16384, 1025, 8192, 8191]),
], ids=['n_fft512', 'n_fft1024', 'n_fft2048'])
def test_ragged_mel_is_per_utterance_featurise_then_collate(N, args, L, lens):
    """MelSpectrogram, one option set per kernel instantiation, against the float64 oracle per utterance and against the utterance
    featurised alone on the GPU (bit for bit, f32 and bf16)."""
    from ppvector.data_utils.featurizer import AudioFeaturizer
    w = ofb.synth_waves(len(lens), L, seed=L % 97, lowpass=0.9)
    per, ref, ref_lens = per_utterance_reference(w, lens, args, dtype=np.float64)
    fz = AudioFeaturizer('MelSpectrogram', args)
    got, got_lens = fz.forward_ragged(dev(poisoned(w, lens)), torch.tensor(lens), want_bf16=True)
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    assert np.all(np.isfinite(g))
    for b, r in enumerate(per):
        scale = np.max(np.abs(r))
        err = np.max(np.abs(g[b, :len(r)] - r))
        col = np.max(np.abs(g[b, :len(r)].astype(np.float64).mean(axis=0)))
        print(f'mel n_fft {fz._opts.n_fft} utt {b} ({lens[b]} samples, {len(r)} frames): max err / scale {err / scale:.3e}  '
              f'column mean / scale {col / scale:.3e}')
        assert err < 2e-5 * scale, err / scale           # f32 FFT round-off relative to the utterance's dynamic range
        assert col <= 1e-6 * scale, col / scale          # own-frame CMN: f32 round-off of a sum of T_b values
    check_padding_and_alone(fz, w, lens, got, got_lens, ref, ref_lens)


def test_ragged_log_mel(N):
    """LogMelSpectrogram (n_fft defaults to 512): oracle tolerances of the dense test, per utterance; the amin floor on digital
    silence; bit identity with the alone form."""
    from ppvector.data_utils.featurizer import AudioFeaturizer
    args = dict(sr=16000, hop_length=160, n_mels=80)
    w = ofb.synth_waves(len(LENS_5120), 5120, seed=31, lowpass=0.5)
    w[0, 2560:] = 0.0                                                      # digital silence: the amin floor (-100 dB)
    per, ref, ref_lens = per_utterance_reference(w, LENS_5120, args, log=True)
    fz = AudioFeaturizer('LogMelSpectrogram', args)
    got, got_lens = fz.forward_ragged(dev(poisoned(w, LENS_5120)), torch.tensor(LENS_5120), want_bf16=True)
    g = got.cpu().numpy()
    assert np.all(np.isfinite(g))
    for b, r in enumerate(per):
        d = np.abs(g[b, :len(r)] - r)
        col = np.max(np.abs(g[b, :len(r)].astype(np.float64).mean(axis=0)))
        print(f'log-mel utt {b}: max {d.max():.3e} mean {d.mean():.3e} column mean {col:.3e}')
        assert d.max() < 5e-2 and d.mean() < 1e-3, (d.max(), d.mean())
        assert col < 1e-4
    check_padding_and_alone(fz, w, LENS_5120, got, got_lens, ref, ref_lens)


def test_ragged_mfcc(N):
    """MFCC: the DCT over the whole batch; zero rows stay zero.  Bit identity with the alone form depends on vp_dense_f32
    treating rows independently: it is printed, not gated."""
    from ppvector.data_utils.featurizer import AudioFeaturizer
    args = dict(sr=16000, n_mfcc=20, n_fft=512, hop_length=160, n_mels=40, f_min=20.0)
    w = ofb.synth_waves(len(LENS_5120), 5120, seed=41, lowpass=0.6)
    per, ref, ref_lens = per_utterance_reference(w, LENS_5120, args, log='mfcc')
    fz = AudioFeaturizer('MFCC', args)
    got, got_lens = fz.forward_ragged(dev(poisoned(w, LENS_5120)), torch.tensor(LENS_5120), want_bf16=True)
    g = got.cpu().numpy()
    assert g.shape[2] == 20 and np.all(np.isfinite(g))
    for b, r in enumerate(per):
        d = np.abs(g[b, :len(r)] - r)
        print(f'mfcc utt {b}: max {d.max():.3e} mean {d.mean():.3e}')
        assert d.max() < 0.2 and d.mean() < 5e-3, (d.max(), d.mean())
    assert np.max(np.abs(got._vp_bf16.float().cpu().numpy() - g)) <= np.max(np.abs(g)) * 2 ** -8 + 1e-6
    same = check_padding_and_alone(fz, w, LENS_5120, got, got_lens, ref, ref_lens, bits=False)
    print('mfcc rows bit-identical to the alone form:', same)


def test_ragged_entry_point_edge_rows(N):
    """vp_melspec_cmn_ragged_f32 itself: rows of 0, n_fft/2 and L + 100 samples beside ordinary ones, NaN in the workspace, in the
    outputs and past every utterance's end; the workspace contract; B = 1 with n = L against the dense entry point."""
    from ppvector.data_utils.featurizer import AudioFeaturizer
    lib, ctx = N.lib(), N.ctx(0)
    o = AudioFeaturizer._mel_opts(ARGS_512)
    L, F = 5120, 80
    ns = [5120, 0, 256, L + 100, 2400, 3000]
    kept = [min(n, L) for n in ns]
    B = len(ns)
    T = lib.vp_mel_num_frames(C.byref(o), L)
    w = ofb.synth_waves(B, L, seed=51, lowpass=0.9)
    wav = dev(poisoned(w, kept))
    nws = lib.vp_mel_workspace_bytes(C.byref(o), B, L)

    def nan_ws(nbytes):
        return torch.full(((nbytes + 3) // 4,), float('nan'), dtype=torch.float32, device='cuda')

    def dense(x):
        x = dev(x)
        b, l = x.shape
        out = torch.full((b, lib.vp_mel_num_frames(C.byref(o), l), F), float('nan'), device='cuda')
        out16 = torch.empty(out.shape, dtype=torch.bfloat16, device='cuda')
        n1 = lib.vp_mel_workspace_bytes(C.byref(o), b, l)
        ws = nan_ws(n1)
        N.check(lib.vp_melspec_cmn_f32(ctx, N.ptr(x), None, b, l, C.byref(o), N.ptr(out), N.ptr(out16), N.ptr(ws), n1, N.stream_ptr()), ctx)
        return out, out16

    def ragged(x, n_samples, ws_bytes=None):
        b, l = x.shape
        t = lib.vp_mel_num_frames(C.byref(o), l)
        out = torch.full((b, t, F), float('nan'), device='cuda')
        out16 = torch.full((b, t, F), float('nan'), dtype=torch.bfloat16, device='cuda')
        nf = torch.full((b,), -7, dtype=torch.int32, device='cuda')
        n1 = lib.vp_mel_workspace_bytes(C.byref(o), b, l)
        n_dev, ws = dev(np.asarray(n_samples, np.int32)), nan_ws(n1)
        rc = lib.vp_melspec_cmn_ragged_f32(ctx, N.ptr(x), N.ptr(n_dev), b, l, C.byref(o), N.ptr(out), N.ptr(out16), N.ptr(nf), N.ptr(ws),
                                           n1 if ws_bytes is None else ws_bytes, N.stream_ptr())
        torch.cuda.synchronize()
        return rc, out, out16, nf

    rc, out, out16, nf = ragged(wav, ns)
    torch.cuda.synchronize()
    assert rc == N.VP_OK
    frames = [1 + n // 160 if n > 256 else 0 for n in kept]
    assert nf.tolist() == frames == [33, 0, 0, 33, 16, 19]
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(out16.float()).all())
    for b, tb in enumerate(frames):
        assert float(out[b, tb:].abs().max() if tb < T else 0.0) == 0.0 and float(out16[b, tb:].float().abs().max() if tb < T else 0.0) == 0.0
        if tb:                                             # the over-long row is clamped to L; the neighbours of the empty rows are intact
            d, d16 = dense(w[b:b + 1, :kept[b]])
            assert torch.equal(out[b, :tb], d[0]) and torch.equal(out16[b, :tb], d16[0]), b
    assert ragged(wav, ns, ws_bytes=nws - 1)[0] == N.VP_EWORKSPACE
    rc, o1, o16, n1 = ragged(wav[:1], [L])
    d, d16 = dense(w[:1])
    assert rc == N.VP_OK and n1.tolist() == [T] and torch.equal(o1, d) and torch.equal(o16, d16)


def test_ragged_mel_refuses_an_utterance_too_short_to_reflect(N):
    """An utterance of n_fft/2 samples raises what its own forward() raises, for lengths on the host and on the GPU."""
    from ppvector.data_utils.featurizer import AudioFeaturizer
    fz = AudioFeaturizer('MelSpectrogram', ARGS_512)
    w = dev(ofb.synth_waves(2, 5120, seed=61))
    with pytest.raises(N.VpmiError) as alone:
        fz(w[1:2, :256])
    for lens in ([5120, 256], torch.tensor([5120, 256]).cuda()):
        with pytest.raises(N.VpmiError) as batched:
            fz.forward_ragged(w, lens)
        assert type(batched.value) is type(alone.value)
    got, lens = fz.forward_ragged(w, [5120, 257])         # one sample more is legal
    assert lens.tolist() == [33, 2]


# --------------------------------------------------------------------------------------- extract_features(batch_size=...)
def _write_wav(path, pcm):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(np.asarray(pcm, np.int16).tobytes())


def _extract(root, method, method_args, batch_size):
    from ppvector.trainer import PPVectorTrainer
    cfg = dict(dataset_conf=dict(dataset=dict(min_duration=0.3, max_duration=2, sample_rate=16000, use_dB_normalization=True, target_dB=-20),
                                 train_list=f'{root}/train_list.txt', enroll_list=f'{root}/enroll_list.txt',
                                 trials_list=f'{root}/trials_list.txt'),
               preprocess_conf=dict(feature_method=method, method_args=method_args))
    save = f'{root}/features_{method}_{batch_size}'
    PPVectorTrainer(cfg, use_gpu=True).extract_features(save_dir=save, max_duration=100, batch_size=batch_size)
    out, paths = {}, []
    for name in ('train', 'enroll', 'trials'):
        lines = open(f'{root}/{name}_list_features.txt').read().strip().split('\n')
        paths += [l.split('\t')[0] for l in lines]
        # a line is '<save_dir>/<label>/<milliseconds>_<index>.npy\t<label>': the clock and the directory of this run aside, it names
        # the utterance's index and label
        keys = [(os.path.relpath(os.path.dirname(p), save), os.path.basename(p).split('_', 1)[1], lab)
                for p, lab in (l.split('\t') for l in lines)]
        out[name] = (keys, [np.load(l.split('\t')[0]) for l in lines])
    assert len(set(paths)) == len(paths)            # the lists share save_dir and labels: no file of one may replace another's
    return out


@pytest.mark.parametrize('method,method_args', [('MelSpectrogram', ARGS_README), ('Fbank', dict(sr=16000, n_mels=80))])
def test_extract_features_in_batches_writes_the_same_files(golden_dir, tmp_path, method, method_args):
    """Six WAVs of unequal length (batches of 4 + 2, both ragged; the enroll list is one ragged batch of 2, the trials list an
    equal-length one): the same list lines in the same order and the same array shapes as one utterance at a time.  Values: bit for
    bit for MelSpectrogram; for Fbank within the tolerance of the ragged-Fbank test (its ragged and dense means are summed in
    different orders)."""
    root = str(tmp_path)
    pcm = np.load(f'{golden_dir}/wavs_3s.npz')['pcm']
    cuts = ((0, 0, 48000), (1, 4000, 34000), (2, 100, 16101), (3, 0, 8000), (0, 1, 48000), (2, 20000, 40000))
    lines = []
    for k, (r, a, b) in enumerate(cuts):
        _write_wav(f'{root}/u{k}.wav', pcm[r, a:b])
        lines.append(f'{root}/u{k}.wav\t{k % 2}')
    open(f'{root}/train_list.txt', 'w').write('\n'.join(lines) + '\n')
    open(f'{root}/enroll_list.txt', 'w').write('\n'.join(lines[1:3]) + '\n')
    open(f'{root}/trials_list.txt', 'w').write('\n'.join([lines[0], lines[0]]) + '\n')
    one = _extract(root, method, method_args, 1)
    four = _extract(root, method, method_args, 4)
    for name, n in (('train', 6), ('enroll', 2), ('trials', 2)):
        (k1, f1), (k4, f4) = one[name], four[name]
        assert len(k1) == n and k1 == k4
        for x, y in zip(f1, f4):
            assert x.shape == y.shape and x.dtype == y.dtype == np.float32
            if method == 'MelSpectrogram':
                assert np.array_equal(x, y)
            else:
                d = np.abs(x - y)
                assert d.max() < 2e-3 and d.mean() < 2e-5, (d.max(), d.mean())
    assert [f.shape[0] for f in one['train'][1]] == [1 + (b - a) // 320 if method == 'MelSpectrogram' else 1 + (b - a - 400) // 160
                                                     for _, a, b in cuts]
