"""Speaker diarization, the parts that need no GPU: the chunk table, the label bookkeeping of SpeakerDiarization, the pruning count of
SpectralCluster and the predictor's refusal to run without speech regions -- against tests/diarization_oracle.py and hand-derived values."""
import numpy as np
import pytest
import torch

from tests import diarization_oracle as od

SR = 16000


class _Seg:
    def __init__(self, n, sr=SR):
        self.samples, self.sample_rate = np.zeros(n, np.float32), sr


def _sd(**kw):
    from ppvector.infer_utils.speaker_diarization import SpeakerDiarization
    return SpeakerDiarization(**kw)


def test_chunk_table_matches_the_restatement_and_the_hand_derived_offsets():
    """Regions of 0.3 s (one short window), exactly 1.5 s (one window: the second would reach no further), and 4.1 s (four strided windows
    and a tail pulled back to end at the region's end; the walk stops after it)."""
    sd = _sd()
    regions = [(0.5, 0.8), (1.0, 2.5), (3.0, 7.1)]
    table = sd.segments(_Seg(8 * SR), regions)
    assert table == od.chunk_table(regions)
    offs = [(r[2], r[3]) for r in table]
    assert offs == [(8000, 12800),
                    (16000, 40000),
                    (48000, 72000), (60000, 84000), (72000, 96000), (84000, 108000), (89600, 113600)]
    for r in table:
        assert abs(r[0] - r[2] / SR) < 1e-9 and abs(r[1] - r[3] / SR) < 1e-9
    # dict regions, as AudioSegment.vad(return_seconds=True) gives them, are read the same way
    assert sd.segments(_Seg(8 * SR), [dict(start=a, end=b) for a, b in regions]) == table


def test_chunk_table_one_sample_past_a_window():
    """1.5 s plus one sample: a second window [1, 24001) pulled back to the region's end, then the stop.  (A (start_s, end_s) pair cannot
    say this: the reference rounds the times to 1 ms, so the region list is built as _chunk takes it.)"""
    sd = _sd()
    got = sd._chunk([[2.0, 2.0 + 24001 / SR, np.zeros(24001, np.float32)]])
    assert [(r[2], r[3]) for r in got] == [(32000, 56000), (32001, 56001)]
    assert got[1][0] == 1 / SR + 2.0 and got[1][1] == 24001 / SR + 2.0
    # other window / shift settings against the restatement
    sd2 = _sd(seg_duration=1.0, seg_shift=0.3)
    regions = [(0.0, 2.75), (3.001, 6.4)]
    assert sd2.segments(_Seg(7 * SR), regions) == od.chunk_table(regions, dur=1.0, shift=0.3)


def test_check_audio_list_rejects_what_the_reference_rejects():
    sd = _sd()
    with pytest.raises(AssertionError):
        sd.segments(_Seg(8 * SR), [(0.0, 4.0)])                         # 5 s of speech at least
    with pytest.raises(AssertionError):
        sd.segments(_Seg(8 * SR), [(3.0, 7.0), (1.0, 2.9)])             # regions in order
    with pytest.raises(AssertionError):
        sd.segments(_Seg(8 * SR), [(0.0, 3.0), (4.0, 9.0)])             # a region past the end of the recording


def test_correct_labels_and_merge_by_cos():
    sd = _sd()
    raw = np.array([2, 2, 0, 1, 0, 2, 1])
    assert sd._correct_labels(raw).tolist() == [0, 0, 1, 2, 1, 0, 2] == od.relabel(raw).tolist()
    # centres 0 and 2 at cosine 0.9, centre 1 orthogonal: 2 is folded into 0, nothing above it to renumber
    c = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.9, 0.0, np.sqrt(1 - 0.81)]])
    labels = np.array([0, 1, 2, 2, 1, 0])
    assert sd._merge_by_cos(labels.copy(), list(c), 0.78).tolist() == [0, 1, 0, 0, 1, 0] == od.merge_by_cos(labels, c, 0.78).tolist()
    assert sd._merge_by_cos(labels.copy(), list(c), 0.95).tolist() == labels.tolist() == od.merge_by_cos(labels, c, 0.95).tolist()
    # 0 and 1 close: 1 is folded into 0 and 2 renumbered to 1; the centres are not re-indexed, so the next round compares rows 0 and 1 again
    c = np.array([[1.0, 0.0, 0.0], [0.8, 0.6, 0.0], [0.0, 0.0, 1.0]])
    labels = np.array([2, 0, 1, 2, 1])
    assert sd._merge_by_cos(labels.copy(), list(c), 0.78).tolist() == [0, 0, 0, 0, 0] == od.merge_by_cos(labels, c, 0.78).tolist()
    c4 = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.8, 0.6, 0.0], [0.0, 0.0, 0.0, 1.0]])
    labels = np.array([0, 1, 2, 3, 2, 3])
    assert sd._merge_by_cos(labels.copy(), list(c4), 0.78).tolist() == [0, 1, 1, 1, 1, 1] == od.merge_by_cos(labels, c4, 0.78).tolist()


def test_merge_seque_and_smooth():
    sd = _sd()
    rows = [[0.0, 1.5, 0], [0.75, 2.25, 0], [1.5, 3.0, 1], [4.0, 5.5, 1], [4.75, 6.25, 1]]
    assert sd._merge_seque([list(r) for r in rows]) == [[0.0, 2.25, 0], [1.5, 3.0, 1], [4.0, 6.25, 1]] == od.join_runs(rows)
    # a short first segment takes its successor's speaker, a short last one its predecessor's
    rows = [[0.0, 0.6, 0], [0.6, 3.0, 1], [3.0, 5.0, 0], [5.0, 5.4, 1]]
    want = [[0.0, 3.0, 1], [3.0, 5.4, 0]]
    assert sd._smooth([list(r) for r in rows]) == want == od.smooth(rows)
    # a short middle segment goes to the nearer neighbour; equal gaps: the earlier one
    rows = [[0.0, 2.0, 0], [2.5, 3.0, 1], [3.2, 6.0, 2]]
    assert sd._smooth([list(r) for r in rows]) == [[0.0, 2.0, 0], [2.5, 3.0, 2], [3.2, 6.0, 2]] == od.smooth(rows)
    rows = [[0.0, 2.0, 0], [2.2, 3.0, 1], [3.2, 6.0, 2]]
    assert sd._smooth([list(r) for r in rows]) == [[0.0, 2.0, 0], [2.2, 3.0, 0], [3.2, 6.0, 2]] == od.smooth(rows)
    # times are rounded to 10 ms before the length is judged
    rows = [[0.004, 1.0, 0], [1.0, 3.0, 1]]
    assert sd._smooth([list(r) for r in rows]) == [[0.0, 1.0, 0], [1.0, 3.0, 1]] == od.smooth(rows)


def test_postprocess_hand_made_sequences():
    sd = _sd()
    # windows every 0.75 s over [0, 6.0], then a region of one short window; speaker changes inside the first region
    table = sd.segments(_Seg(10 * SR), [(0.0, 6.0), (7.0, 7.4)])
    assert len(table) == 8
    labels = np.array([0, 0, 0, 1, 1, 1, 1, 0])
    got = sd.postprocess(table, labels)
    # runs [0, 3.0] (0) and [2.25, 6.0] (1) overlap: split at 2.625 -> rounded to 10 ms by the smoothing (banker's rounding of the
    # binary value); the last window (0.4 s) is short and takes its predecessor's speaker but stays apart (it starts after its end)
    assert got == [dict(speaker=0, start=0.0, end=round(round(2.625, 2), 3)), dict(speaker=1, start=round(round(2.625, 2), 3), end=6.0),
                   dict(speaker=1, start=7.0, end=7.4)]
    assert got == od.postprocess(table, labels)
    # a short first segment: a 0.5 s region of speaker 1 in front takes its successor's speaker and stays apart from it
    table = sd.segments(_Seg(10 * SR), [(0.0, 0.5), (1.0, 7.0)])
    labels = np.array([1] + [0] * (len(table) - 1))
    got = sd.postprocess(table, labels)
    assert got == [dict(speaker=0, start=0.0, end=0.5), dict(speaker=0, start=1.0, end=7.0)] == od.postprocess(table, labels)
    # one window of another speaker in front of a long run keeps 1.12 s after the split at the overlap's midpoint: not short
    table = sd.segments(_Seg(10 * SR), [(0.0, 6.0)])
    labels = np.array([1, 0, 0, 0, 0, 0, 0])
    got = sd.postprocess(table, labels)
    assert got == [dict(speaker=1, start=0.0, end=1.12), dict(speaker=0, start=1.12, end=6.0)] == od.postprocess(table, labels)
    # alternating speakers: every run is short after the splits and the relabelling cascades in order
    labels = np.array([0, 1, 0, 1, 0, 1, 0])
    assert sd.postprocess(table, labels) == od.postprocess(table, labels)
    assert len(table) == len(labels)
    with pytest.raises(AssertionError):
        sd.postprocess(table, labels[:-1])


def test_n_elems_either_side_of_the_pval_switch():
    from ppvector.infer_utils.speaker_diarization import SpectralCluster
    sc = SpectralCluster()
    assert sc.n_elems(7) == int((1 - 6. / 7) * 7) == od.n_elems(7) and sc.n_elems(7) in (0, 1)
    assert sc.n_elems(272) == int((1 - 6. / 272) * 272) == od.n_elems(272) and sc.n_elems(272) in (265, 266)     # 272 * 0.022 < 6
    assert sc.n_elems(273) == int((1 - 0.022) * 273) == od.n_elems(273) == 266                                    # 273 * 0.022 >= 6
    assert sc.n_elems(1025) == int((1 - 0.022) * 1025) == od.n_elems(1025) == 1002
    assert SpectralCluster(pval=0.1).n_elems(100) == 90 == od.n_elems(100, 0.1)
    # under six rows the reference's count is negative and, used as a slice end, counts from the other side
    for n in (2, 3, 4, 5):
        assert sc.n_elems(n) == len(list(range(n))[0:od.n_elems(n)])
    for n in range(2, 400):
        assert 0 <= sc.n_elems(n) < n


def test_eigen_gap_rule():
    from ppvector.infer_utils.speaker_diarization import SpectralCluster
    sc = SpectralCluster()
    assert sc.get_eigen_gaps([0.0, 0.1, 0.5, 0.6]) == [0.1, 0.4, 0.09999999999999998]
    L = np.diag([0.0, 1e-9, 2e-9, 0.7, 0.8, 0.9]).astype(np.float64)
    emb, k = sc.get_spec_embs(L)
    assert k == 3 and emb.shape == (6, 3)
    emb, k = sc.get_spec_embs(L, 2)
    assert k == 2 and emb.shape == (6, 2)


def test_speaker_diarization_needs_vad_segments():
    """The reference finds the speech regions with yeaudio's model-based VAD, which is not built: without vad_segments the method
    raises and says so (before it touches the audio or the GPU)."""
    import inspect
    from ppvector.predict import PPVectorPredictor
    sig = inspect.signature(PPVectorPredictor.speaker_diarization)
    assert list(sig.parameters)[1:] == ['audio_data', 'sample_rate', 'speaker_num', 'search_audio_db', 'vad_segments']
    assert [sig.parameters[k].default for k in ('sample_rate', 'speaker_num', 'search_audio_db', 'vad_segments')] == [16000, None, False, None]
    pred = PPVectorPredictor.__new__(PPVectorPredictor)
    with pytest.raises(NotImplementedError, match='vad'):
        pred.speaker_diarization(np.zeros(16000 * 12, np.float32))


def test_engine_entries_have_no_cpu_path():
    from ppvector import _native as N
    from ppvector.infer_utils import speaker_diarization as sdm
    with pytest.raises(N.VpmiError):
        sdm.chunk_batch(torch.zeros(100), np.array([[0, 10]], np.int32), 16)
    with pytest.raises(N.VpmiError):
        sdm.affinity_prune(torch.zeros(4, 3), 1)
    with pytest.raises(N.VpmiError):
        sdm.laplacian(torch.zeros(4, 4))
