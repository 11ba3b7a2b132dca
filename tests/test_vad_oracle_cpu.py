"""The energy voice-activity detector, the parts that need no GPU: the restatement tests/vad_oracle.py against hand-checked cases of
every rule, frame counts, the seconds conversion, EnergyVad's argument validation, the binding, and the predictor's use of a detector."""
import numpy as np
import pytest

from tests import vad_oracle as ov

SR = 16000


def _e(*parts):
    """Planted energies: (level, count) pairs."""
    return np.concatenate([np.full(n, v, np.float32) for v, n in parts])


def test_frame_counts_at_the_window_edges():
    from ppvector import _native as N
    from ppvector.infer_utils.vad import EnergyVad
    lib = N.load_library()
    vad = EnergyVad()
    assert (vad.win, vad.hop) == (400, 160)
    for win, hop in ((400, 160), (401, 161), (200, 80), (7, 7), (4096, 1)):
        for n, want in ((win - 1, 0), (win, 1), (win + hop - 1, 1), (win + hop, 2), (0, 0), (win + 10 * hop, 11)):
            assert ov.num_frames(n, win, hop) == want == lib.vp_vad_num_frames(n, win, hop), (win, hop, n)
    for n in (399, 400, 559, 560, 192000):
        assert vad.num_frames(n) == ov.num_frames(n, 400, 160)
    assert lib.vp_vad_num_frames(1000, 0, 160) == 0 and lib.vp_vad_num_frames(1000, 400, 0) == 0 and lib.vp_vad_num_frames(-1, 400, 160) == 0
    assert lib.vp_vad_workspace_bytes(12000, 4) == 16 * (12000 // 64 + 4 + 1) and lib.vp_vad_workspace_bytes(0, 1) == 32
    assert lib.vp_vad_workspace_bytes(-1, 1) == 0 and lib.vp_vad_workspace_bytes(10, 0) == 0


def test_the_four_symbols_are_in_the_binding():
    from ppvector import _native as N
    lib = N.load_library()
    for name in ('vp_vad_num_frames', 'vp_vad_frame_db_f32', 'vp_vad_workspace_bytes', 'vp_vad_regions_f32'):
        assert name in N.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert len(N._PROTOS['vp_vad_frame_db_f32'][1]) == 10 and len(N._PROTOS['vp_vad_regions_f32'][1]) == 19
    assert N._PROTOS['vp_vad_workspace_bytes'] == (N.c_size_t, [N.C.c_longlong, N.c_int])


def test_frame_db_hand_checked():
    """A constant frame has no energy left after the mean is removed: exactly -100.  +-a alternating, c = 0: mean 0, p = a^2.  With
    pre-emphasis c: y[0] = a (1 - c), every other |y| = a (1 + c)."""
    win, hop = 8, 4
    assert np.array_equal(ov.frame_db(np.full(20, 0.7), win, hop, 0.97), np.full(4, -100.0))
    assert np.array_equal(ov.frame_db(np.zeros(8, np.float32), win, hop, 0.0), np.full(1, -100.0))
    assert abs(ov.frame_db(np.zeros(8, np.float32), win, hop, 0.0, dtype=np.float32)[0] + 100.0) < 1e-5      # f32 log10: an ulp off
    a = 0.25
    x = a * np.where(np.arange(16) % 2, -1.0, 1.0)
    assert np.allclose(ov.frame_db(x, win, hop, 0.0), 10 * np.log10(a * a), atol=1e-12)
    c = 0.5
    p = (a * a * (1 - c) ** 2 + 7 * a * a * (1 + c) ** 2) / 8
    assert np.allclose(ov.frame_db(x, win, hop, c), 10 * np.log10(p), atol=1e-12)
    # a DC offset changes nothing in float64, and the float32 restatement stays close under it
    rng = np.random.RandomState(0)
    q = 3e-4 * rng.standard_normal(2000)
    assert np.abs(ov.frame_db(q + 0.5, 400, 160, 0.97) - ov.frame_db(q, 400, 160, 0.97)).max() < 1e-6
    x32 = (q + 0.5).astype(np.float32)
    assert np.abs(ov.frame_db(x32, 400, 160, 0.97, dtype=np.float32) - ov.frame_db(x32, 400, 160, 0.97)).max() < 1e-4
    assert ov.frame_db(np.zeros(399), 400, 160, 0.97).shape == (0,)


def test_order_statistics_and_thresholds():
    e = np.arange(11, dtype=np.float32) * 10 - 100                    # -100 .. 0
    assert [ov.rank(p, 11) for p in (0.0, 0.1, 0.95, 1.0, 0.25)] == [0, 1, 9, 10, 2]
    assert ov.rank(0.1, 12) == 1 and ov.rank(0.95, 2) == 0            # floor, and (double) of the f32 0.1 = 0.100000001...
    assert ov.rank(0.1, 21) == 2                                      # the f32 0.1 is over a tenth: 2.00000003 -> 2
    fl, pk, on, off = ov.thresholds(e, 0.1, 0.95, 6.0, 0.5, 0.25)
    assert (fl, pk, on, off) == (-90.0, -10.0, -50.0, -70.0) and all(isinstance(v, np.float32) for v in (fl, pk, on, off))
    fl, pk, on, off = ov.thresholds(e, 0.1, 0.95, 30.0, 0.5, 0.25)    # the margin wins over offset r = 20
    assert (on, off) == (-50.0, -60.0)
    fl, pk, on, off = ov.thresholds(_e((-50.0, 10), (-20.0, 10)), 0.1, 0.95, 6.0, 0.0, 0.0)
    assert (fl, pk, on, off) == (-50.0, -20.0, -44.0, -44.0)
    # ranks inside a run of tied values; F = 1; F = 0
    assert ov.thresholds(_e((-100.0, 50), (-30.0, 3)), 0.1, 0.95, 6.0, 0.5, 0.5)[:2] == (-100.0, -100.0)
    assert ov.regions(np.float32([-40.0]))[0][:2] == (-40.0, -40.0)
    assert ov.regions(np.zeros(0, np.float32)) == ((0.0, 0.0, 0.0, 0.0), [])


def test_hysteresis_hand_checked():
    on, off = np.float32(-44.0), np.float32(-60.0)
    mid = -50.0
    st = ov.hysteresis(_e((mid, 2), (-30.0, 2), (mid, 3), (-70.0, 1), (mid, 2), (-44.0, 1), (np.nextafter(np.float32(-44), np.float32(-100)), 1),
                          (-60.0, 1), (np.nextafter(np.float32(-60), np.float32(-100)), 1), (mid, 1)), on, off)
    #           mid at the start is silence | speech | mid after speech stays | silence | mid after silence stays | exactly on: speech |
    #           just under on: undecided, stays speech | exactly off: not under it, stays | just under off: silence | mid stays silence
    assert st == [False, False, True, True, True, True, True, False, False, False, True, True, True, False, False]


def test_clean_up_rules_hand_checked():
    T, F_ = True, False

    def states(*parts):
        return [s for s, n in parts for _ in range(n)]

    # 5: gaps of min_gap - 1 are filled, of min_gap and more are not; silence at either end never is
    s = states((F_, 2), (T, 5), (F_, 2), (T, 5), (F_, 3), (T, 5), (F_, 4), (T, 5), (F_, 1))
    assert ov.clean(s, 3, 1, 0) == [(2, 14), (17, 22), (26, 31)]
    # 6: after the gap fill, runs under min_speech go; the fill happens first, so two short bursts a short gap apart survive together
    s = states((F_, 3), (T, 2), (F_, 5), (T, 3), (F_, 5), (T, 4), (F_, 5), (T, 1), (F_, 1), (T, 1), (F_, 2))
    assert ov.clean(s, 2, 3, 0) == [(10, 13), (18, 22), (27, 30)]
    assert ov.clean(s, 1, 1, 0) == [tuple(r) for r in ov.runs(s)] == [(3, 5), (10, 13), (18, 22), (27, 28), (29, 30)]
    # 7: padding clipped at both ends; padded runs that touch or overlap merge, one frame apart they do not
    s = states((T, 3), (F_, 10), (T, 3), (F_, 4), (T, 3), (F_, 5), (T, 2))
    assert ov.clean(s, 1, 1, 2) == [(0, 5), (11, 25), (26, 30)]
    s = states((F_, 5), (T, 2), (F_, 5), (T, 2), (F_, 5))
    assert ov.clean(s, 1, 1, 2) == [(3, 9), (10, 16)] and ov.clean(s, 1, 1, 3) == [(2, 17)]
    # speech throughout, nothing at all
    assert ov.clean([T] * 7, 3, 3, 2) == [(0, 7)] and ov.clean([F_] * 7, 3, 3, 2) == [] and ov.clean([], 3, 3, 2) == []
    # never more than ceil(F / 2) regions
    assert len(ov.clean([T, F_] * 5 + [T], 1, 1, 0)) == 6


def test_regions_end_to_end_on_planted_energies():
    e = _e((-60.0, 40), (-20.0, 50), (-60.0, 5), (-20.0, 30), (-60.0, 60), (-20.0, 3), (-60.0, 40))
    thr, reg = ov.regions(e, 0.1, 0.95, 6.0, 0.5, 0.25, min_gap=10, min_speech=5, pad=4)
    assert thr == (-60.0, -20.0, -40.0, -50.0)
    assert reg == [(36, 129)]                                         # the 5-frame gap filled, the 3-frame burst dropped, 4 frames of padding


def test_seconds_conversion():
    from ppvector.infer_utils.vad import EnergyVad
    vad = EnergyVad()
    n = 400 + 99 * 160 + 37                                           # 100 frames and a tail of 37 samples no frame covers
    assert vad.num_frames(n) == 100
    assert vad.to_seconds(10, 20, n) == (10 * 160 / SR, (19 * 160 + 400) / SR) == ov.to_seconds(10, 20, n, 400, 160, SR)
    assert vad.to_seconds(0, 1, n) == (0.0, 400 / SR)
    assert vad.to_seconds(90, 100, n) == (90 * 160 / SR, n / SR) == ov.to_seconds(90, 100, n, 400, 160, SR)       # b == F: the tail stays
    assert vad.to_seconds(98, 99, n) == (98 * 160 / SR, (98 * 160 + 400) / SR)
    v8 = EnergyVad(sample_rate=8000)
    assert (v8.win, v8.hop) == (200, 80) and v8.to_seconds(1, 3, 1000) == (80 / 8000, (2 * 80 + 200) / 8000)


def test_energy_vad_arguments():
    from ppvector.infer_utils.vad import EnergyVad
    v = EnergyVad()
    assert (v.min_gap, v.min_run, v.pad) == (30, 25, 10) and (v.preemph, v.floor_pct, v.peak_pct) == (0.97, 0.10, 0.95)
    assert (v.margin_db, v.onset, v.offset) == (6.0, 0.35, 0.25)
    v = EnergyVad(min_silence=0.0, min_speech=0.0, pad=0.0)
    assert (v.min_gap, v.min_run, v.pad) == (1, 1, 0)                 # no clean-up
    assert EnergyVad(min_silence=0.125, hop_ms=10).min_gap == round(12.5) == 12
    for bad in (dict(sample_rate=0), dict(frame_ms=5, hop_ms=10), dict(hop_ms=0), dict(frame_ms=300), dict(preemph=1.0), dict(preemph=-0.1),
                dict(floor_pct=-0.1), dict(floor_pct=0.96), dict(peak_pct=1.1), dict(onset=0.2), dict(offset=-0.1), dict(onset=1.5),
                dict(margin_db=-1.0), dict(margin_db=float('nan')), dict(min_silence=-1.0), dict(min_speech=-0.1), dict(pad=-0.1)):
        with pytest.raises(ValueError):
            EnergyVad(**bad)


def test_energy_vad_has_no_cpu_path():
    import torch
    from ppvector import _native as N
    from ppvector.infer_utils.vad import EnergyVad
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    with pytest.raises(N.VpmiError):
        EnergyVad().regions(np.zeros(16000, np.float32))


def test_speaker_diarization_asks_the_detector_only_without_vad_segments(monkeypatch):
    """A stub detector: called once, with the uploaded waveform, exactly when vad_segments is None; an explicit vad_segments wins;
    after set_vad(None) the call raises as it always did."""
    from ppvector.infer_utils.vad import EnergyVad, Thresholds
    from ppvector.predict import AudioSegment, PPVectorPredictor

    class Stub(EnergyVad):
        calls = []

        def regions(self, waves):
            self.calls.append(waves)
            return [(0.5, 3.0), (2.99, 7.0004)], Thresholds(0.0, 0.0, 0.0, 0.0)

    pred = PPVectorPredictor.__new__(PPVectorPredictor)
    seen = {}
    monkeypatch.setattr(pred, '_load_audio', lambda audio_data, sample_rate=16000: AudioSegment(audio_data, sample_rate), raising=False)
    monkeypatch.setattr(pred, '_upload', lambda seg: ('device', seg.samples.shape[0]), raising=False)

    class Diarize:
        def segments(self, seg, vad_segments):
            seen['regions'] = list(vad_segments)
            return [[0.0, 1.5, 0, 24000]]

        def clustering(self, features, speaker_num=None):
            return np.array([0]), np.zeros((1, 4), np.float32)

        def postprocess(self, table, labels):
            return [dict(speaker=0, start=0.0, end=1.5)]

    pred.speaker_diarize = Diarize()

    def chunk_embeddings(seg, table, batch_size=32, wave=None):
        seen['wave'] = wave
        return np.zeros((1, 4), np.float32)

    monkeypatch.setattr(pred, 'chunk_embeddings', chunk_embeddings, raising=False)
    rec = np.zeros(SR * 8, np.float32)
    with pytest.raises(ValueError):
        pred.set_vad(object())
    stub = Stub()
    pred.set_vad(stub)
    out = pred.speaker_diarization(rec)
    assert out == [dict(speaker=0, start=0.0, end=1.5)]
    assert stub.calls == [('device', SR * 8)] and seen['wave'] == ('device', SR * 8)      # one upload, shared
    # as segments() can take them: an end stops at the next start and is rounded down to the millisecond
    assert seen['regions'] == [(0.5, 2.99), (2.99, 7.0)]
    assert pred.vad(rec) == [(0.5, 2.99), (2.99, 7.0)] and len(stub.calls) == 2
    pred.speaker_diarization(rec, vad_segments=[(1.0, 7.5)])
    assert len(stub.calls) == 2 and seen['regions'] == [(1.0, 7.5)]                          # an explicit list wins
    pred.set_vad(None)
    with pytest.raises(NotImplementedError, match='vad'):
        pred.speaker_diarization(rec)
    with pytest.raises(NotImplementedError, match='vad'):
        pred.vad(rec)
    assert len(stub.calls) == 2
    with pytest.raises(ValueError, match='8000'):
        pred.set_vad(Stub(sample_rate=8000))
        pred.speaker_diarization(rec)
