"""Speaker diarization on the MI355X: the three kernels of csrc/diarize.hip against the float64 restatements of tests/diarization_oracle.py,
the clustering end to end, and PPVectorPredictor.speaker_diarization."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import diarization_oracle as od

pytestmark = pytest.mark.gpu

AFFINITY_SHAPES = [(7, 5), (273, 192), (1025, 192), (300, 512)]      # n_elems 0 or 1 | just past the pval switch | two row blocks and a
AFFINITY_SEED = 20                                                   # 32-row tile remainder | another D


def _embeddings(n, d):
    return np.random.RandomState(AFFINITY_SEED + n).standard_normal((n, d)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(n, d):
    """float64 affinity of the f32 embeddings, the pruning count, the pruned matrix and the rows on which f32 and f64 may disagree."""
    S = od.cosine_affinity(_embeddings(n, d))
    k = od.n_elems(n)
    P = od.prune(S, k)
    if k > 0:
        srt = np.sort(S, axis=1)
        ambiguous = (srt[:, k] - srt[:, k - 1]) < 1e-5               # the k-th and (k + 1)-th smallest of the row
    else:
        ambiguous = np.zeros(n, bool)
    for a in (S, P, ambiguous):
        a.setflags(write=False)
    return S, k, P, ambiguous


@functools.lru_cache(maxsize=None)
def _gpu_pruned(n, d):
    from ppvector.infer_utils.speaker_diarization import SpectralCluster, affinity_prune
    k = SpectralCluster().n_elems(n)
    assert k == od.n_elems(n)
    P = affinity_prune(torch.from_numpy(_embeddings(n, d)).cuda(), k).cpu().numpy()
    P.setflags(write=False)
    return P


def test_chunk_batch_against_float64():
    """40 000 samples; windows: full length, one sample, one sample at the very end, ending at the last sample (full and short),
    overlapping, and empty.  1e-6 of the row's peak; pad columns exactly 0; two runs the same bits."""
    from ppvector.infer_utils.speaker_diarization import chunk_batch
    rng = np.random.RandomState(5)
    wave = (0.1 * rng.standard_normal(40000)).astype(np.float32)
    L = 24000
    table = np.array([[0, 24000], [5, 6], [39999, 40000], [16000, 40000], [30000, 40000], [12000, 36000], [12001, 36001], [777, 777]], np.int32)
    w = torch.from_numpy(wave).cuda()
    for normalize in (True, False):
        got_t = chunk_batch(w, table, L, normalize=normalize, target_db=-20.0)
        again = chunk_batch(w, table, L, normalize=normalize, target_db=-20.0)
        assert got_t.shape == (len(table), L) and torch.equal(got_t, again)
        got = got_t.cpu().numpy()
        ref = od.chunk_batch(wave, table, L, normalize=normalize, target_db=-20.0)
        for b, (a, e) in enumerate(table):
            peak = np.abs(ref[b]).max()
            err = np.abs(got[b] - ref[b]).max()
            print(f'[chunk_batch normalize={normalize}] window {a}:{e}  peak {peak:.4g}  max err {err:.3g}')
            assert err <= 1e-6 * peak, (b, err, peak)
            assert not got[b, e - a:].any()
        if normalize:                                                # every non-empty row sits at -20 dBFS over its padded length
            ms = (got[:-1].astype(np.float64) ** 2).mean(axis=1)
            assert np.abs(10 * np.log10(ms) + 20.0).max() < 1e-4
        else:
            assert np.array_equal(got[0], wave[:L]) and got[1, 0] == wave[5]
    # a silent window: mean square floored at 1e-20, the gain finite, the row zero
    z = chunk_batch(torch.zeros(30000, device='cuda'), np.array([[0, 24000]], np.int32), L).cpu().numpy()
    assert not z.any()
    # a window of tiny samples: the 1e-20 floor decides the gain (180 dB), not the samples
    tiny = np.full(24000, 1e-12, np.float32)
    g = chunk_batch(torch.from_numpy(tiny).cuda(), np.array([[0, 24000]], np.int32), L).cpu().numpy()
    r = od.chunk_batch(tiny, [[0, 24000]], L)
    assert np.abs(g - r).max() <= 1e-6 * np.abs(r).max()


@pytest.mark.parametrize('n,d', AFFINITY_SHAPES)
def test_affinity_prune_against_float64(n, d):
    """Off the ambiguous rows (reference gap at the threshold under 1e-5: f32 and f64 may order the two values differently) the set of
    surviving columns is the reference's and the surviving values agree to 2e-5, the tolerance of the cosine logits."""
    S, k, P_ref, ambiguous = _reference(n, d)
    assert ambiguous.mean() <= 0.05, ambiguous.mean()                # a condition on the seeds, met by the float64 reference alone
    P = _gpu_pruned(n, d)
    assert P.shape == (n, n)
    clear = ~ambiguous
    kept_ref, kept = P_ref != 0, P != 0
    bad = np.nonzero((kept_ref != kept).any(axis=1) & clear)[0]
    print(f'[affinity_prune N={n} D={d}] n_elems {k}  ambiguous rows {int(ambiguous.sum())}  rows with another surviving set {bad.size}')
    assert bad.size == 0, bad[:10]
    assert (kept[clear].sum(axis=1) == n - k).all()
    err = np.abs(P - S)[kept & clear[:, None]].max()
    print(f'[affinity_prune N={n} D={d}] max |cos - float64| over the survivors {err:.3g}')
    assert err <= 2e-5, err
    # on an ambiguous row exactly n_elems entries are zeroed all the same, and the survivors are cosines
    assert (kept.sum(axis=1) == n - k).all()
    assert np.abs(P - S)[kept].max() <= 2e-5


@pytest.mark.parametrize('n,d', [(2049, 16), (4097, 16), (8193, 8), (16384, 8)])
def test_affinity_prune_larger_row_blocks(n, d):
    """The sizes at which a workgroup takes fewer rows (4, 2, 1: a block's similarities stay within 64 KB of LDS) and the largest N of
    the contract, on a sample of rows (the first and last ones, block boundaries, a stride through the rest) against the float64
    reference of those rows; same rule for ambiguous rows and the same tolerances as above."""
    from ppvector.infer_utils.speaker_diarization import affinity_prune
    x = np.random.RandomState(n).standard_normal((n, d)).astype(np.float32)
    rows = np.unique(np.concatenate([np.arange(8), np.arange(n - 8, n), np.arange(0, n, max(n // 240, 1))]))
    xn = x.astype(np.float64) / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
    S = xn[rows] @ xn.T
    k = od.n_elems(n)
    srt = np.sort(S, axis=1)
    ambiguous = (srt[:, k] - srt[:, k - 1]) < 1e-5
    assert ambiguous.mean() <= 0.05, ambiguous.mean()
    P = affinity_prune(torch.from_numpy(x).cuda(), k)[torch.from_numpy(rows).cuda()].cpu().numpy()
    kept_ref, kept = od.prune(S, k) != 0, P != 0
    assert (kept.sum(axis=1) == n - k).all()
    bad = np.nonzero((kept_ref != kept).any(axis=1) & ~ambiguous)[0]
    err = np.abs(P - S)[kept].max()
    print(f'[affinity_prune N={n} D={d}] n_elems {k}  rows checked {rows.size}  ambiguous {int(ambiguous.sum())}  '
          f'rows with another surviving set {bad.size}  max |cos - float64| {err:.3g}')
    assert bad.size == 0, rows[bad[:10]]
    assert err <= 2e-5, err


def _tie_case(n, d, cols, seed):
    """Embeddings whose columns `cols` are one vector: their similarities to row 0 are the same bits."""
    x = np.random.RandomState(seed).standard_normal((n, d)).astype(np.float32)
    for c in cols[1:]:
        x[c] = x[cols[0]]
    s0 = od.cosine_affinity(x)[0]
    below = int((s0 < s0[cols[0]] - 1e-5).sum())
    near = np.abs(np.delete(s0, cols) - s0[cols[0]]).min()
    return x, below, near


@pytest.mark.parametrize('n,d,cols,n_zeroed,seed', [(12, 8, (3, 9), 1, 1), (600, 16, (70, 300, 400), 2, 2), (600, 16, (70, 300, 400), 1, 2),
                                                    (600, 16, (10, 20, 40), 2, 3)])
def test_affinity_prune_tie_lower_column_first(n, d, cols, n_zeroed, seed):
    """Identical embeddings tie at row 0's threshold; the lower columns are the ones zeroed (in one wave, across waves and across the
    256-column passes of the tie walk).  The reference's argsort leaves the choice undefined; this is the engine's rule."""
    from ppvector.infer_utils.speaker_diarization import affinity_prune
    x, below, near = _tie_case(n, d, cols, seed)
    assert near > 1e-4                                               # nothing else near the tied value: the threshold is the tie
    k = below + n_zeroed
    P = affinity_prune(torch.from_numpy(x).cuda(), k).cpu().numpy()
    S = od.cosine_affinity(x)
    assert (P[0, list(cols[:n_zeroed])] == 0).all(), P[0, list(cols)]
    assert (P[0, list(cols[n_zeroed:])] != 0).all(), P[0, list(cols)]
    assert len(set(P[0, list(cols[n_zeroed:])].tolist())) == 1
    assert ((P != 0).sum(axis=1) == n - k).all()
    ref = od.prune(S, k)                                             # stable sort: the same rule
    assert np.array_equal(P[0] != 0, ref[0] != 0)
    assert np.abs(P - S)[P != 0].max() <= 2e-5


def test_affinity_prune_rejects_what_is_outside_the_contract():
    from ppvector import _native as N
    lib, ctx = N.lib(), N.ctx()
    buf = torch.zeros(1 << 16, device='cuda')
    out = torch.zeros(1 << 16, device='cuda')
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device='cuda')

    def call(n, d, k, nbytes=ws.numel()):
        return lib.vp_affinity_prune_f32(ctx, buf.data_ptr(), n, d, k, out.data_ptr(), ws.data_ptr(), nbytes, N.stream_ptr())

    for n, d, k in ((1, 8, 0), (16385, 8, 0), (8, 0, 0), (8, 1025, 0), (8, 8, 8), (8, 8, -1)):
        assert call(n, d, k) == N.VP_EINVAL, (n, d, k)
    assert lib.vp_affinity_prune_workspace_bytes(64, 8) >= 64 * 4 + 64 * 8 * 4
    assert call(64, 8, 3, nbytes=16) == N.VP_EWORKSPACE
    assert call(8, 8, 7) == N.VP_OK
    assert lib.vp_laplacian_f32(ctx, buf.data_ptr(), 8, buf.data_ptr(), N.stream_ptr()) == N.VP_EINVAL      # in place
    assert lib.vp_laplacian_f32(ctx, buf.data_ptr(), 0, ws.data_ptr(), N.stream_ptr()) == N.VP_EINVAL
    assert lib.vp_chunk_batch_f32(ctx, buf.data_ptr(), 100, ws.data_ptr(), 0, 16, 1, C.c_float(-20.0), buf.data_ptr(),
                                  N.stream_ptr()) == N.VP_EINVAL
    torch.cuda.synchronize()


@pytest.mark.parametrize('n,d', [(7, 5), (273, 192), (1025, 192)])
def test_laplacian_of_the_engines_own_pruned_affinity(n, d):
    """The GPU's own P (downloaded) through vp_laplacian_f32 against the float64 Laplacian of that same P: no ambiguity left.
    Off-diagonal 1e-6 absolute, diagonal 1e-5 relative, L exactly symmetric.  Row sums: sum_j L_ij = sum_j (|M_ij| - M_ij), which is 0
    where no negative similarity survives the pruning -- there the row sums must stay under 1e-4 of the degree; where some do (N = 7
    keeps nearly everything) the row sums are compared, to the same 1e-4 of the degree, with that float64 figure."""
    from ppvector.infer_utils.speaker_diarization import laplacian
    P = _gpu_pruned(n, d)
    L_t = laplacian(torch.from_numpy(np.array(P)).cuda())
    assert torch.equal(L_t, laplacian(torch.from_numpy(np.array(P)).cuda()))
    L = L_t.cpu().numpy()
    ref = od.laplacian(P)
    off = ~np.eye(n, dtype=bool)
    deg = np.diag(ref)
    e_off = np.abs(L - ref)[off].max()
    e_diag = (np.abs(np.diag(L) - deg) / deg).max()
    print(f'[laplacian N={n}] off-diagonal max abs err {e_off:.3g}  diagonal max rel err {e_diag:.3g}')
    assert e_off <= 1e-6 and e_diag <= 1e-5
    assert np.array_equal(L, L.T)
    M = 0.5 * (P.astype(np.float64) + P.astype(np.float64).T)
    np.fill_diagonal(M, 0.0)
    expect = (np.abs(M) - M).sum(axis=1)
    rows = L.astype(np.float64).sum(axis=1)
    print(f'[laplacian N={n}] max |row sum - expected| / degree {(np.abs(rows - expect) / deg).max():.3g}  negative survivors {int((M < 0).sum())}')
    assert (np.abs(rows - expect) <= 1e-4 * deg).all()
    if n != 7:
        assert not (M < 0).any()
        assert (np.abs(rows) <= 1e-4 * deg).all()


def _speakers(centres, counts, seed, noise=0.3):
    """Points around unit centres with Gaussian noise of relative norm `noise`, in a shuffled order."""
    rng = np.random.RandomState(seed)
    d = centres.shape[1]
    who = rng.permutation(np.repeat(np.arange(len(counts)), counts))
    x = centres[who] + noise / np.sqrt(d) * rng.standard_normal((who.size, d))
    return x.astype(np.float32), who


def _unit_centres(k, d, seed):
    c = np.random.RandomState(seed).standard_normal((k, d))
    return c / np.linalg.norm(c, axis=1, keepdims=True)


@pytest.mark.parametrize('speaker_num', [3, None])
def test_clustering_three_separated_speakers(speaker_num):
    from ppvector.infer_utils.speaker_diarization import SpeakerDiarization
    centres = _unit_centres(3, 192, 11)
    assert np.triu(centres @ centres.T, 1).max() <= 0.2
    x, who = _speakers(centres, (40, 30, 20), 12)
    want, want_centres = od.clustering(x, speaker_num)
    assert want.max() == 2 and np.array_equal(want, od.relabel(who))          # the restatement finds the three speakers
    labels, spk_centres = SpeakerDiarization().clustering(x, speaker_num=speaker_num)
    assert np.array_equal(labels, want), (labels, want)
    assert spk_centres.shape == (3, 192) and np.abs(spk_centres - want_centres).max() < 1e-5


def test_clustering_merges_two_speakers_at_cosine_0_9():
    """Two of three centres at cosine 0.9: the spectral step tells them apart, their centres' cosine is over 0.78 and _merge_by_cos folds
    them; the third stays apart.  A point of the third speaker comes first, so the close pair is not labels (0, 1): the reference does
    not re-index the centres after a merge, and with the pair at (0, 1) its second round would compare the same two rows again and fold
    the third speaker too (tests/test_diarization_cpu.py has that case)."""
    from ppvector.infer_utils.speaker_diarization import SpeakerDiarization
    c = _unit_centres(3, 192, 21)
    u = c[1] - (c[1] @ c[0]) * c[0]
    c[1] = 0.9 * c[0] + np.sqrt(1 - 0.81) * u / np.linalg.norm(u)
    assert abs(c[0] @ c[1] - 0.9) < 1e-12 and abs(c[2] @ c[0]) <= 0.2 and abs(c[2] @ c[1]) <= 0.2
    x, who = _speakers(c, (35, 30, 25), 22)
    j = int(np.argmax(who == 2))
    x[[0, j]], who[[0, j]] = x[[j, 0]], who[[j, 0]]
    want, _ = od.clustering(x, 3)
    assert np.array_equal(want, od.relabel(np.where(who == 1, 0, who)))        # the restatement: speakers 0 and 1 as one
    labels, spk_centres = SpeakerDiarization().clustering(x, speaker_num=3)
    assert spk_centres.shape == (3, 192)                                       # the centres are those before the merge, as in the reference
    assert labels.max() == 1 and np.array_equal(labels, want)
    # with a threshold the pair does not reach nothing is merged
    labels, _ = SpeakerDiarization(merge_threshold=0.97).clustering(x, speaker_num=3)
    assert labels.max() == 2


def _cfg():
    from ppvector.utils.utils import dict_to_object
    return dict_to_object(dict(
        dataset_conf=dict(dataset=dict(min_duration=0.3, max_duration=3, sample_rate=16000, use_dB_normalization=True, target_dB=-20)),
        preprocess_conf=dict(feature_method='Fbank', method_args=dict(sr=16000, n_mels=80)),
        model_conf=dict(model='EcapaTdnn', model_args=dict(embd_dim=192, pooling_type='ASP', channels=[512, 512, 512, 512, 1536]))))


@pytest.fixture(scope='module')
def predictor():
    from oracle import models as om
    from ppvector.predict import PPVectorPredictor
    state = {'0.' + k: v for k, v in om.ecapa_params(80, seed=1000).items()}
    return PPVectorPredictor(_cfg(), model_path=state)


@pytest.fixture(scope='module')
def recording():
    from oracle import fbank as ofb
    w = ofb.synth_waves(3, 64000, seed=77, lowpass=0.9)               # 12 s: three 4 s stretches of different loudness
    return np.concatenate([w[0], 0.3 * w[1], 2.0 * w[2]]).astype(np.float32)


VAD = [(0.5, 5.0), (6.0, 11.3), (11.5, 11.9)]                         # 5 + 7 windows and one short one (6 400 samples, padded)


def test_predictor_chunk_embeddings_match_predict_batch(predictor, recording):
    """The new path (one upload, windows cut / padded / normalised on the GPU) against predict_batch over the windows cut, padded and
    normalised on the host one by one, to the engine's embedding tolerance for the active dtype."""
    import ppvector
    seg = predictor._load_audio(recording.copy(), 16000)
    table = predictor.speaker_diarize.segments(seg, VAD)
    assert table == od.chunk_table(VAD) and len(table) == 13
    L = predictor.speaker_diarize.chunk_len
    host = []
    for _, _, a, e in table:
        c = np.zeros(L, np.float32)
        c[:e - a] = seg.samples[a:e]
        host.append(c)
    ref = predictor.predict_batch(host)
    got = predictor.chunk_embeddings(seg, table, batch_size=5)
    assert got.shape == ref.shape == (13, 192)
    rel = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)
    tol = {'float32': 2e-4, 'float32x3': 2e-4, 'bfloat16': 6e-2}[ppvector.get_compute_dtype()]
    print(f'[chunk_embeddings vs predict_batch] max rel-L2 {rel.max():.3g} (tolerance {tol:g})')
    assert rel.max() < tol, rel


def test_predictor_speaker_diarization(predictor, recording, monkeypatch):
    table = od.chunk_table(VAD)
    # end to end on the engine's own embeddings: the reference's output format, times inside the speech regions, in order
    out = predictor.speaker_diarization(recording.copy(), speaker_num=2, vad_segments=VAD)
    assert out and all(set(o) == {'speaker', 'start', 'end'} for o in out)
    assert all(o['speaker'] in (0, 1) and 0.5 <= o['start'] < o['end'] <= 11.9 for o in out)
    assert all(a['end'] <= b['start'] + 1e-9 for a, b in zip(out[:-1], out[1:]))
    # with the labels fixed by hand the list is the restatement's postprocess of the same table
    hand = np.array([0, 0, 0, 1, 1] + [1, 1, 0, 0, 0, 0, 2] + [2])
    seen = {}

    def fixed(embeddings, speaker_num=None):
        seen['shape'] = np.asarray(embeddings).shape
        return hand.copy(), seen['centres']

    monkeypatch.setattr(predictor.speaker_diarize, 'clustering', fixed)
    seen['centres'] = np.eye(3, 192, dtype=np.float32)
    out = predictor.speaker_diarization(recording.copy(), vad_segments=VAD)
    assert seen['shape'] == (13, 192)
    assert out == od.postprocess(table, hand)
    assert len(out) >= 3
    # search_audio_db: a speaker whose centre is the registered user's embedding gets the name, the others 陌生人{n}
    with pytest.raises(AssertionError):
        predictor.speaker_diarization(recording.copy(), vad_segments=VAD, search_audio_db=True)      # nobody registered
    predictor.register(recording[:48000].copy(), 'alice')
    feat = predictor.predict(recording[:48000].copy())
    other = np.roll(feat, 1) * np.where(np.arange(192) % 2, 1.0, -1.0).astype(np.float32)
    assert abs(feat @ other) / (np.linalg.norm(feat) * np.linalg.norm(other)) < 0.5
    seen['centres'] = np.stack([other, feat, -feat])
    named = predictor.speaker_diarization(recording.copy(), vad_segments=VAD, search_audio_db=True)
    want = [dict(speaker={0: '陌生人0', 1: 'alice', 2: '陌生人2'}[o['speaker']], start=o['start'], end=o['end']) for o in out]
    assert named == want
    seen['centres'] = np.stack([other, -feat, -feat])                # none matching
    named = predictor.speaker_diarization(recording.copy(), vad_segments=VAD, search_audio_db=True)
    assert [o['speaker'] for o in named] == [f"陌生人{o['speaker']}" for o in out]
    assert predictor.remove_user('alice')
