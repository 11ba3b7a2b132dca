"""The Fbank and mel featurizers (csrc/fbank.hip, csrc/melspec.hip) over their option surface against float64: every kernel
instantiation -- fbank_frames16_kernel<13> and <16>, float and PCM16, and the fallback fbank_frames_kernel --, the persistent tile
loop, the table cache, int16 routing and the samples no frame covers.  Cases, signals and bounds: tests/featurizer_oracle.py; that
the bounds would catch a subtly wrong kernel: tests/test_featurizer_oracle_cpu.py.  Measured kernel / e32 ratios:
docs/featurizer_options.md.  Run with -m gpu on an MI355X.
"""
import math

import numpy as np
import pytest
import torch

from tests import featurizer_oracle as fo

pytestmark = pytest.mark.gpu

LOG_FLOOR = abs(math.log(1e-7))
# digital silence: every frame is the log floor, the output the floor minus a float32 mean of T equal values
SILENCE_TOL = 8 * fo.F32_EPS * LOG_FLOOR


@pytest.fixture(scope='module')
def N():
    from ppvector import _native as N
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: these tests must run on an MI355X (no CPU fallback exists)')
    N.ctx(0)
    return N


def dev(x):
    return torch.as_tensor(np.asarray(x)).cuda().contiguous()


def fbank(args):
    from ppvector.data_utils.featurizer import AudioFeaturizer
    return AudioFeaturizer('Fbank', args)


def twin_ok(out):
    g = out.float().cpu().numpy()
    return np.max(np.abs(out._vp_bf16.float().cpu().numpy() - g)) <= np.max(np.abs(g)) * 2 ** -8 + 1e-6


def check_fbank(tag, args, got, ref, r32, worst):
    """The e32 rule: kernel vs float64 within margin x (float32 restatement vs float64) + ten ulps, capped at the existing bound."""
    e32, dv = fo.deviation(r32, ref), fo.deviation(got, ref)
    bmax, bmean = fo.bound(e32, ref, fo.fbank_margin(args), fo.FBANK_CAP)
    if e32[0] > 0.0:
        worst[0], worst[1] = max(worst[0], dv[0] / e32[0]), max(worst[1], dv[1] / e32[1])
    print(f'{tag}: kernel max {dv[0]:.3e} mean {dv[1]:.3e}  e32 max {e32[0]:.3e} mean {e32[1]:.3e}  bound {bmax:.3e} / {bmean:.3e}')
    assert np.all(np.isfinite(got)), tag
    assert dv[0] <= bmax and dv[1] <= bmean, (tag, dv, e32, (bmax, bmean))


def test_case_table_reaches_every_kernel(N):
    """The parametrised tests below run FBANK_CASES; the table must hold <13>, <16>, the fallback kernel and both PCM16 forms, and
    the featurizer's own routing must agree with it."""
    assert fo.exercised_classes() == {'13', '16', 'old', 'pcm16_13', 'pcm16_16'}
    for cid, args, _, _, cls in fo.FBANK_CASES:
        assert fo.kernel_class(args) == cls
        assert fbank(args)._pcm16_ok == fo.pcm16_covered(args, 4000), cid


# ------------------------------------------------------------------------------------------------------------- Fbank parity
@pytest.mark.parametrize('cid', fo.FBANK_IDS)
def test_fbank_parity(N, cid):
    _, args, win, shift, cls = fo.FBANK_BY_ID[cid]
    fz = fbank(args)
    ratio = np.linspace(1.0, 0.2, 7).astype(np.float32)
    worst = [0.0, 0.0]
    for L in fo.fbank_lengths(win, shift, args['sr']):
        x = fo.signals(L, shift, args['sr'], seed=100 + L)
        T = 1 + (L - win) // shift
        for r in (None, ratio):
            ref, r32 = fo.fbank_ref(x, args, r), fo.fbank_ref(x, args, r, dtype=np.float32)
            out = fz(dev(x), None if r is None else dev(r), want_bf16=True)
            got = out.cpu().numpy()
            assert got.shape == ref.shape == (7, T, args['n_mels'])
            check_fbank(f'{cid} <{cls}> L {L} T {T} mask {r is not None}', args, got, ref, r32, worst)
            assert twin_ok(out)
            assert np.max(np.abs(got[6])) <= SILENCE_TOL and np.max(np.abs(ref[6])) <= 1e-12
            if r is not None:
                for b, n in enumerate((ratio * np.float32(T)).astype(np.int32)):
                    assert np.all(got[b, n:] == 0.0)
    print(f'RATIO fbank {cid} <{cls}>: kernel / e32 max {worst[0]:.2f} mean {worst[1]:.2f}')


def test_fbank_refusals_are_loud(N):
    x = dev(fo.signals(4000, 160, 16000, seed=1)[:2])
    for args in (dict(sr=16000, n_mels=80, frame_length=40.0),        # win 640 -> nfft 1024
                 dict(sr=16000, n_mels=129),
                 dict(sr=16000, n_mels=80, frame_length=0.0625)):     # win 1
        fz = fbank(args)
        with pytest.raises(N.VpmiError):
            fz(x)
        with pytest.raises(N.VpmiError):
            fz((x * 32767.0).to(torch.int16))
        with pytest.raises(N.VpmiError):
            fz.forward_ragged(x, [4000, 3000])
    with pytest.raises(ValueError):
        fbank(dict(sr=16000, n_mels=80))(x[:, :399])


# -------------------------------------------------------------------------------------------------------------------- PCM16
@pytest.mark.parametrize('cid', fo.FBANK_IDS)
def test_fbank_int16_input(N, cid):
    """Covered option sets (four-frames-per-wave kernel, even shift, even L): the 16-bit entry, bit-equal to the float entry over
    the widened samples, bf16 twin included.  Every other option set, and an odd L: the same tensor as widening by hand, no error."""
    _, args, win, shift, cls = fo.FBANK_BY_ID[cid]
    fz = fbank(args)
    L = (win + 17 * shift + 3) // 2 * 2
    pcm, wf = fo.pcm_of(fo.signals(L, shift, args['sr'], seed=7))
    ratio = np.linspace(1.0, 0.3, 7).astype(np.float32)
    covered = fo.pcm16_covered(args, L)
    assert fz._pcm16_ok == covered
    for r in (None, ratio):
        rr = None if r is None else dev(r)
        a = fz(dev(pcm), rr, want_bf16=True)
        b = fz(dev(wf), rr, want_bf16=True)
        assert a.dtype == torch.float32 and torch.equal(a, b) and torch.equal(a._vp_bf16, b._vp_bf16)
    check_fbank(f'{cid} <{cls}> int16 ({"16-bit entry" if covered else "widened first"})', args, a.cpu().numpy(), fo.fbank_ref(wf, args, ratio),
                fo.fbank_ref(wf, args, ratio, dtype=np.float32), [0.0, 0.0])
    odd = fz(dev(pcm[:, :L - 1]), want_bf16=True)
    assert torch.equal(odd, fz(dev(wf[:, :L - 1])))


# ------------------------------------------------------------------------------------------------------------------- ragged
RAGGED_CASES = ['m80', 'm64_win320', 'm23']


def ragged_lens(L, win, shift):
    return [L, win, win + shift - 1, int(0.6 * L), L - 1]


@pytest.mark.parametrize('cid', RAGGED_CASES)
def test_fbank_ragged(N, cid):
    _, args, win, shift, cls = fo.FBANK_BY_ID[cid]
    L = args['sr'] // 2
    lens = ragged_lens(L, win, shift)
    x = fo.signals(L, shift, args['sr'], seed=13)[:5]
    ref, nf = fo.fbank_ragged_ref(x, lens, args)
    r32, _ = fo.fbank_ragged_ref(x, lens, args, dtype=np.float32)
    junk = x.copy()
    for b, n in enumerate(lens):
        junk[b, n:] = 0.7
    out, got_lens = fbank(args).forward_ragged(dev(junk), torch.tensor(lens), want_bf16=True)
    got = out.cpu().numpy()
    assert got_lens.tolist() == nf and got.shape == ref.shape
    worst = [0.0, 0.0]
    check_fbank(f'{cid} <{cls}> ragged', args, got, ref, r32, worst)
    print(f'RATIO fbank-ragged {cid} <{cls}>: kernel / e32 max {worst[0]:.2f} mean {worst[1]:.2f}')
    assert twin_ok(out)
    for b, n in enumerate(nf):
        assert np.all(got[b, n:] == 0.0)


# ----------------------------------------------------------------------------------------------------------- unread samples
@pytest.mark.parametrize('cid', ['m80', 'm64_win320', 'm23'])
def test_fbank_samples_no_frame_covers_do_not_matter(N, cid):
    """Rectangular batch: the tail after the last frame (shift - 1 samples), NaN one row at a time, changes no bit of the output.
    A NaN INSIDE the last frame's window poisons that frame, hence (through the time mean) that utterance and no other."""
    _, args, win, shift, _ = fo.FBANK_BY_ID[cid]
    fz = fbank(args)
    tail = win + 4 * shift
    x = fo.signals(tail + shift - 1, shift, args['sr'], seed=41)[:4]
    x[:, tail:] = 0.0
    base = fz(dev(x), want_bf16=True)
    assert bool(torch.isfinite(base).all())
    for b in range(4):
        p = x.copy()
        p[b, tail:] = np.nan
        out = fz(dev(p), want_bf16=True)
        assert torch.equal(out, base) and torch.equal(out._vp_bf16, base._vp_bf16), (cid, b)
        p = x.copy()
        p[b, tail - 1] = np.nan                        # the last sample of the last frame: in no other frame (shift < win)
        out = fz(dev(p))
        assert bool(torch.isnan(out[b]).all())
        keep = [i for i in range(4) if i != b]
        assert torch.equal(out[keep], base[keep])


@pytest.mark.parametrize('cid', RAGGED_CASES)
def test_fbank_ragged_padding_does_not_matter(N, cid):
    """Ragged batch: whatever lies past n_samples[b] -- NaN, then +Inf --, the output is bit-equal to the run with zeros there."""
    _, args, win, shift, _ = fo.FBANK_BY_ID[cid]
    fz = fbank(args)
    L = args['sr'] // 2
    lens = ragged_lens(L, win, shift)
    x = fo.signals(L, shift, args['sr'], seed=43)[:5]
    for b, n in enumerate(lens):
        x[b, n:] = 0.0
    base, base_lens = fz.forward_ragged(dev(x), torch.tensor(lens), want_bf16=True)
    assert bool(torch.isfinite(base).all())
    for poison in (np.nan, np.inf):
        p = x.copy()
        for b, n in enumerate(lens):
            p[b, n:] = poison
        out, out_lens = fz.forward_ragged(dev(p), torch.tensor(lens), want_bf16=True)
        assert torch.equal(out_lens, base_lens)
        assert torch.equal(out, base) and torch.equal(out._vp_bf16, base._vp_bf16), (cid, poison)


# ---------------------------------------------------------------------------------------------------------- persistent loop
@pytest.mark.parametrize('cid', ['m80', 'm64_win320'])
def test_fbank_persistent_tile_loop(N, cid):
    """T = 64 (4 tiles per row) and enough rows for two full trips of the resident grid (3 workgroups per CU) and a partial third;
    a different signal per row, so a tile delivered to the wrong (row, tile) shows.  Against float64, and bit-equal to the same rows
    in batches of 5, which never take a second trip."""
    _, args, win, shift, cls = fo.FBANK_BY_ID[cid]
    fz = fbank(args)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = (2 * 3 * cus + 1 + 3) // 4
    assert 4 * B >= 2 * 3 * cus + 1
    L, sr = win + 63 * shift, args['sr']
    rng = np.random.RandomState(59)
    t = np.arange(L, dtype=np.float64)
    freq = 200.0 + (0.45 * sr - 200.0) * np.arange(B) / B                   # a tone of its own per row, over its own noise
    x = (0.1 * rng.standard_normal((B, L)) + 0.3 * np.sin(2.0 * math.pi * freq[:, None] * t[None, :] / sr)).astype(np.float32)
    ref, r32 = fo.fbank_ref(x, args), fo.fbank_ref(x, args, dtype=np.float32)
    xd = dev(x)
    out = fz(xd, want_bf16=True)
    got = out.cpu().numpy()
    assert got.shape == (B, 64, args['n_mels'])
    worst = [0.0, 0.0]
    check_fbank(f'{cid} <{cls}> persistent B {B} ({cus} CUs)', args, got, ref, r32, worst)
    print(f'RATIO fbank-persistent {cid} <{cls}>: kernel / e32 max {worst[0]:.2f} mean {worst[1]:.2f}')
    small = torch.cat([fz(xd[i:i + 5]) for i in range(0, B, 5)])
    assert torch.equal(small, out)


# -------------------------------------------------------------------------------------------------------------- table cache
@pytest.mark.parametrize('a,b', [
    (dict(sr=16000, n_mels=80), dict(sr=16000, n_mels=80, high_freq=-500.0)),
    (dict(sr=16000, n_mels=80), dict(sr=16000, n_mels=80, preemphasis_coefficient=0.0)),
    (dict(sr=16000, n_mels=64), dict(sr=16000, n_mels=64, frame_length=20.0)),
], ids=['high_freq', 'preemph', 'frame_length'])
def test_fbank_table_cache_flips(N, a, b):
    """One context, A then B then A: the A results bit-equal, B equal to B from a fresh AudioFeaturizer, each within the bound of its
    OWN reference (stale tables would give the other's numbers)."""
    x = fo.signals(4000, 160, 16000, seed=47)
    xd = dev(x)
    fa, fb_ = fbank(a), fbank(b)
    a1, b1, a2 = fa(xd), fb_(xd), fa(xd)
    b2 = fbank(b)(xd)
    assert torch.equal(a1, a2) and torch.equal(b1, b2)
    for tag, args, got in (('A', a, a1), ('B', b, b1)):
        check_fbank(f'cache {tag}', args, got.cpu().numpy(), fo.fbank_ref(x, args), fo.fbank_ref(x, args, dtype=np.float32), [0.0, 0.0])
    assert a1.shape != b1.shape or not torch.equal(a1, b1)


@pytest.mark.parametrize('a,b', [('mel512_p2', 'mel512_p1'), ('mel1024_p2_fmax7000', None)], ids=['power', 'f_max'])
def test_mel_table_cache_flips(N, a, b):
    from ppvector.data_utils.featurizer import AudioFeaturizer
    _, method, args_a, L = fo.MEL_BY_ID[a]
    args_b = fo.MEL_BY_ID[b][2] if b else {k: v for k, v in args_a.items() if k != 'f_max'}
    x = fo.signals(L, args_a['hop_length'], args_a['sr'], seed=53)
    xd = dev(x)
    fa, fb_ = AudioFeaturizer(method, args_a), AudioFeaturizer(method, args_b)
    a1, b1, a2 = fa(xd), fb_(xd), fa(xd)
    b2 = AudioFeaturizer(method, args_b)(xd)
    assert torch.equal(a1, a2) and torch.equal(b1, b2) and not torch.equal(a1, b1)
    for tag, args, got in (('A', args_a, a1), ('B', args_b, b1)):
        check_mel(f'mel cache {tag}', method, got.cpu().numpy(), fo.mel_oracle(x, method, args), fo.mel_feat(x, method, args, np.float32),
                  [0.0, 0.0])


# --------------------------------------------------------------------------------------------------------------- mel family
def check_mel(tag, method, got, ref, r32, worst):
    e32, dv = fo.mel_metric(r32, ref, method), fo.mel_metric(got, ref, method)
    bmax, bmean = fo.mel_bound(e32, ref, method)
    if e32[0] > 0.0:
        worst[0], worst[1] = max(worst[0], dv[0] / e32[0]), max(worst[1], dv[1] / e32[1])
    print(f'{tag}: kernel max {dv[0]:.3e} mean {dv[1]:.3e}  e32 max {e32[0]:.3e} mean {e32[1]:.3e}  bound {bmax:.3e} / {bmean:.3e}')
    assert np.all(np.isfinite(got)), tag
    assert dv[0] <= bmax and dv[1] <= bmean, (tag, dv, e32, (bmax, bmean))


@pytest.mark.parametrize('cid', fo.MEL_IDS)
def test_mel_family_parity(N, cid):
    """Rectangular (with and without the length mask) and ragged, under the e32 rule in the metric of the method's existing tests."""
    from ppvector.data_utils.featurizer import AudioFeaturizer
    _, method, args, L = fo.MEL_BY_ID[cid]
    fz = AudioFeaturizer(method, args)
    hop, n_fft = args['hop_length'], args.get('n_fft', 512)
    F = args.get('n_mfcc', args['n_mels']) if method == 'MFCC' else args['n_mels']
    x = fo.signals(L, hop, args['sr'], seed=61)
    ratio = np.linspace(1.0, 0.2, 7).astype(np.float32)
    worst = [0.0, 0.0]
    for r in (None, ratio):
        ref, r32 = fo.mel_oracle(x, method, args, r), fo.mel_feat(x, method, args, np.float32, r)
        out = fz(dev(x), None if r is None else dev(r), want_bf16=True)
        got = out.cpu().numpy()
        assert got.shape == ref.shape == (7, 1 + L // hop, F)
        check_mel(f'{cid} L {L} mask {r is not None}', method, got, ref, r32, worst)
        assert twin_ok(out)
    if method == 'MelSpectrogram':
        assert np.all(got[6] == 0.0)                                          # silence: zero power, zero mean
    lens = [L, n_fft // 2 + 1, max(n_fft // 2 + 1, int(0.6 * L)), max(n_fft // 2 + 1, L - 1)]
    xr = x[:4].copy()
    ref = np.zeros((4, 1 + L // hop, F))
    r32 = np.zeros_like(ref)
    for b, n in enumerate(lens):
        f = fo.mel_oracle(xr[b:b + 1, :n], method, args)[0]
        ref[b, :len(f)] = f
        r32[b, :len(f)] = fo.mel_feat(xr[b:b + 1, :n], method, args, np.float32)[0]
        xr[b, n:] = np.nan
    out, out_lens = fz.forward_ragged(dev(xr), torch.tensor(lens), want_bf16=True)
    got = out.cpu().numpy()
    assert out_lens.tolist() == [1 + n // hop for n in lens]
    check_mel(f'{cid} ragged', method, got, ref, r32, worst)
    for b, n in enumerate(out_lens.tolist()):
        assert np.all(got[b, n:] == 0.0)
    print(f'RATIO mel {cid}: kernel / e32 max {worst[0]:.2f} mean {worst[1]:.2f}')


@pytest.mark.parametrize('cid', ['mel512_p2', 'mel1024_p1.5', 'logmel_ref_amin', 'mfcc_full'])
def test_mel_nan_inside_a_frame_poisons_that_utterance_only(N, cid):
    """As for Fbank: the reference's power_to_db is maximum(x, amin), which keeps a NaN; a floor that swallowed it would turn a
    NaN sample into -100 dB frames.  Through the time mean every row of the utterance is NaN; the others keep every bit."""
    from ppvector.data_utils.featurizer import AudioFeaturizer
    _, method, args, L = fo.MEL_BY_ID[cid]
    fz = AudioFeaturizer(method, args)
    x = fo.signals(L, args['hop_length'], args['sr'], seed=71)[:4]
    base = fz(dev(x))
    assert bool(torch.isfinite(base).all())
    x[2, L // 2] = np.nan
    out = fz(dev(x))
    assert bool(torch.isnan(out[2]).all()) and torch.equal(out[[0, 1, 3]], base[[0, 1, 3]])


def test_mel_refuses_what_cannot_be_reflect_padded(N):
    from ppvector.data_utils.featurizer import AudioFeaturizer
    _, method, args, L = fo.MEL_BY_ID['mel512_shortest']
    fz = AudioFeaturizer(method, args)
    x = dev(fo.signals(L, 160, 16000, seed=67)[:2])
    assert fz(x).shape == (2, 2, 80)
    with pytest.raises(N.VpmiError):
        fz(x[:, :L - 1])
