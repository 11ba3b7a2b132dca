"""1:N speaker search on the GPU (csrc/gallery.hip, ppvector/infer_utils/gallery.py, PPVectorPredictor.recognition /
recognition_batch) against the float64 oracle of tests/gallery_oracle.py.  Shapes are the smallest at which the kernels can go wrong:
every edge of the 32-query tile, the 32-row wave tile, the slab (VP_GALLERY_SLAB rows) and a workgroup's range of slabs."""
import numpy as np
import pytest
import torch

from tests import gallery_oracle as og

pytestmark = pytest.mark.gpu

TOL = og.TOL


@pytest.fixture(scope='module')
def N():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: these tests must run on an MI355X (no CPU fallback exists)')
    from ppvector import _native
    return _native


def _unit_rows(rs, U, D):
    g = rs.standard_normal((U, D)).astype(np.float32)
    return (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)


def _queries(rs, gal, Q):
    """Every other query is a gallery row plus noise (scaled by a random gain: the kernel normalises), the rest are unrelated."""
    U, D = gal.shape
    q = rs.standard_normal((Q, D)).astype(np.float32)
    for i in range(0, Q, 2):
        q[i] = (gal[rs.randint(U)] + 0.05 * rs.standard_normal(D)) * rs.uniform(0.5, 20.0)
    return q.astype(np.float32)


def _topk(N, queries, cen, k, Q=None, U=None):
    """vp_gallery_topk_f32 on device tensors (or arrays); Q / U may be smaller than the buffers."""
    q = torch.as_tensor(queries).cuda().contiguous()
    c = torch.as_tensor(cen).cuda().contiguous()
    Q = q.shape[0] if Q is None else Q
    U = c.shape[0] if U is None else U
    D = q.shape[1]
    lib, ctx = N.lib(), N.ctx()
    need = lib.vp_gallery_topk_workspace_bytes(Q, U, D, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    idx = torch.full((Q, k), -7, dtype=torch.int32, device='cuda')
    score = torch.full((Q, k), float('nan'), dtype=torch.float32, device='cuda')
    N.check(lib.vp_gallery_topk_f32(ctx, q.data_ptr(), Q, c.data_ptr(), U, D, k, idx.data_ptr(), score.data_ptr(), ws.data_ptr(),
                                    ws.numel(), N.stream_ptr()), ctx)
    return idx.cpu().numpy(), score.cpu().numpy()


S = 128     # asserted against the header's constant below
CASES = [   # (D, U, Q, k): every U edge, every Q edge and every k once, k > U included
    (20, 1, 1, 1), (20, 1, 33, 5), (512, 1, 1, 32),
    (20, 31, 31, 32), (192, 31, 1, 5),
    (192, 32, 32, 32), (512, 33, 33, 1), (192, 33, 70, 5),
    (192, S - 1, 1, 1), (20, S - 1, 32, 5),
    (192, S, 32, 5), (20, S, 33, 1), (512, S, 31, 32),
    (192, S + 1, 33, 32), (512, S + 1, 1, 5),
    (192, 3 * S + 5, 70, 5), (512, 3 * S + 5, 32, 1), (20, 3 * S + 5, 70, 32),
    (192, 2500, 31, 32), (192, 2500, 70, 1), (20, 2500, 1, 1), (512, 2500, 70, 32),
    (1024, 300, 33, 32),        # the largest LDS request: D = 1024 with k = 32
    (24, 200, 5, 3),
]


@pytest.mark.parametrize('D,U,Q,k', CASES)
def test_topk_vs_float64(N, D, U, Q, k):
    assert N.VP_GALLERY_SLAB == S
    rs = np.random.RandomState(1000 * D + 7 * U + Q + k)
    gal = _unit_rows(rs, U, D)
    q = _queries(rs, gal, Q)
    idx, score = _topk(N, q, gal, k)
    worst = og.check_topk(idx, score, og.scores(q, gal), k, TOL)
    print(f'[gallery topk D={D} U={U} Q={Q} k={k}] largest |score - float64| {worst:.3e}')


def test_ties_go_to_the_lower_row(N):
    """Bit-identical rows on both sides of a slab boundary (127 | 128), in different waves (40, 100), in different workgroups' ranges
    (a workgroup walks two slabs: 255 | 256) and far apart."""
    rs = np.random.RandomState(5)
    D, U = 192, 3 * S + 5
    gal = _unit_rows(rs, U, D)
    planted = [40, 100, 127, 128, 255, 256, 380]
    gal[planted] = gal[planted[0]]
    q = np.stack([gal[planted[0]] * 3.0, gal[planted[0]] + 0.01 * rs.standard_normal(D).astype(np.float32)]).astype(np.float32)
    for k in (1, 5, 32):
        idx, score = _topk(N, q, gal, k)
        n = min(k, len(planted))
        for r in range(2):
            assert idx[r, :n].tolist() == planted[:n], (k, r, idx[r])
            assert (score[r, :n].view(np.int32) == score[r, 0].view(np.int32)).all()
        og.check_topk(idx, score, og.scores(q, gal), k, TOL)


@pytest.mark.parametrize('U,k', [(300, 32), (5, 32), (129, 1)])
def test_identical_gallery(N, U, k):
    rs = np.random.RandomState(6)
    row = _unit_rows(rs, 1, 192)
    gal = np.repeat(row, U, axis=0)
    q = rs.standard_normal((3, 192)).astype(np.float32)
    idx, score = _topk(N, q, gal, k)
    n = min(U, k)
    for r in range(3):
        assert idx[r].tolist() == list(range(n)) + [-1] * (k - n)
        assert (score[r, :n].view(np.int32) == score[r, 0].view(np.int32)).all() and np.isneginf(score[r, n:]).all()


@pytest.fixture(scope='module')
def big():
    rs = np.random.RandomState(7)
    gal = _unit_rows(rs, 2500, 192)
    return gal, _queries(rs, gal, 70)


def test_two_runs_same_bits(N, big):
    gal, q = big
    a = _topk(N, q, gal, 32)
    b = _topk(N, q, gal, 32)
    assert (a[0] == b[0]).all() and (a[1].view(np.int32) == b[1].view(np.int32)).all()


@pytest.mark.parametrize('r', [127, 128, 200, 255, 256, 2499])
def test_a_score_does_not_depend_on_the_rows_behind_it(N, big, r):
    """Row r scored in the gallery of 2500 rows and in the gallery truncated to r + 1 rows (another grid, r in another place of its
    workgroup's walk): the same bits."""
    gal, _ = big
    q = (gal[r] * 2.0 + 0.01 * np.random.RandomState(r).standard_normal(192)).astype(np.float32)[None]
    i_full, s_full = _topk(N, q, gal, 1)
    i_cut, s_cut = _topk(N, q, gal, 1, U=r + 1)
    assert i_full[0, 0] == r and i_cut[0, 0] == r
    assert s_full.view(np.int32)[0, 0] == s_cut.view(np.int32)[0, 0]


@pytest.mark.parametrize('U,Q', [(2 * S + 3, 33), (S, 1), (31, 32)])
def test_nothing_is_read_past_Q_or_U(N, U, Q):
    rs = np.random.RandomState(8)
    D, k = 192, 5
    gal = np.full((U + 50, D), np.nan, np.float32)
    gal[:U] = _unit_rows(rs, U, D)
    q = np.full((Q + 40, D), np.nan, np.float32)
    q[:Q] = _queries(rs, gal[:U], Q)
    loose = _topk(N, q, gal, k, Q=Q, U=U)
    tight = _topk(N, q[:Q].copy(), gal[:U].copy(), k)
    assert (loose[0] == tight[0]).all() and (loose[1].view(np.int32) == tight[1].view(np.int32)).all()
    og.check_topk(tight[0], tight[1], og.scores(q[:Q], gal[:U]), k, TOL)


def test_zero_rows(N):
    rs = np.random.RandomState(9)
    D, U = 20, 30                                         # k = 32 > U: every row is returned
    gal = _unit_rows(rs, U, D)
    gal[3] = 0.0
    q = _queries(rs, gal, 4)
    q[1] = 0.0
    idx, score = _topk(N, q, gal, 32)
    og.check_topk(idx, score, og.scores(q, gal), 32, TOL)
    for r in (0, 2, 3):
        assert score[r, idx[r].tolist().index(3)] == 0.0                 # a zero centroid scores exactly 0
    assert idx[1, :U].tolist() == list(range(U)) and (score[1, :U] == 0.0).all()     # a zero query: the rows in order, score 0
    idx, score = _topk(N, q, gal, 5)
    assert idx[1].tolist() == [0, 1, 2, 3, 4] and (score[1] == 0.0).all()


# ------------------------------------------------------------------------------------------------ SpeakerGallery
def _library(rs, D):
    """Users with 1, 2 and 37 utterances and one whose two utterances cancel, interleaved."""
    names = ['solo'] + ['pair'] * 2 + ['many'] * 37 + ['void'] * 2
    feats = rs.standard_normal((len(names), D)).astype(np.float32)
    feats[-1] = -feats[-2]
    order = rs.permutation(len(names))
    return [names[i] for i in order], feats[order]


@pytest.mark.parametrize('D', [192, 20, 260])
def test_centroids_vs_float64(N, D):
    from ppvector.infer_utils.gallery import SpeakerGallery
    names, feats = _library(np.random.RandomState(11), D)
    users, ref = og.centroids(feats, names)
    g = SpeakerGallery(D)
    g.rebuild(names, feats)
    assert g.names == users and len(g) == 4
    cen = g.centroids.cpu().numpy()
    err = np.abs(cen - ref).max()
    print(f'[gallery centroids D={D}] largest |centroid - float64| {err:.3e}')
    assert err <= TOL
    assert (cen[users.index('void')] == 0.0).all()
    # user by user, in the order of first enrolment: the same bits
    h = SpeakerGallery(D)
    for u in users:
        h.set_user(u, feats[[i for i, n in enumerate(names) if n == u]])
    assert h.names == users and torch.equal(h.centroids, g.centroids)
    # a user re-enrolled with one more utterance: only that row changes, and it equals the rebuild's
    extra = np.random.RandomState(12).standard_normal((1, D)).astype(np.float32)
    h.set_user('pair', np.concatenate([feats[[i for i, n in enumerate(names) if n == 'pair']], extra]))
    g.rebuild(names + ['pair'], np.concatenate([feats, extra]))
    assert torch.equal(h.centroids, g.centroids)


def test_gallery_grows_removes_and_searches(N):
    from ppvector.infer_utils.gallery import SpeakerGallery
    rs = np.random.RandomState(13)
    D, users = 192, 150                                   # past the first capacity (64) twice
    feats = rs.standard_normal((users, D)).astype(np.float32)
    names = [f'u{i}' for i in range(users)]
    g = SpeakerGallery(D)
    for n, f in zip(names[:70], feats[:70]):              # grown row by row ...
        g.set_user(n, f[None])
    h = SpeakerGallery(D)
    h.rebuild(names[:70], feats[:70])                     # ... and at once
    assert torch.equal(g.centroids, h.centroids) and g.names == h.names == names[:70]
    g.rebuild(names, feats)
    assert len(g) == users
    idx, score = g.search(feats, top_k=3)
    assert idx.shape == score.shape == (users, 3) and idx.dtype == torch.int32 and idx.is_cuda and score.is_cuda
    og.check_topk(idx.cpu().numpy(), score.cpu().numpy(), og.scores(feats, g.centroids.cpu().numpy()), 3, TOL)
    assert idx[:, 0].cpu().tolist() == list(range(users))
    # remove: the last row moves into the hole and keeps its name; the removed user is never returned
    assert g.remove('u5') and not g.remove('u5')
    assert len(g) == users - 1 and g.names[5] == f'u{users - 1}' and 'u5' not in g.names
    idx, score = g.search(feats, top_k=32)
    idx = idx.cpu().numpy()
    assert idx.max() == users - 2 and idx.min() == 0
    got = [g.names[i] for i in idx[:, 0]]
    assert got[users - 1] == f'u{users - 1}' and idx[users - 1, 0] == 5
    assert [n for j, n in enumerate(got) if j != 5] == [n for j, n in enumerate(names) if j != 5]
    assert got[5] != 'u5'
    empty = SpeakerGallery(D)
    idx, score = empty.search(feats[:2], top_k=2)
    assert (idx.cpu().numpy() == -1).all() and np.isneginf(score.cpu().numpy()).all()
    with pytest.raises(N.VpmiError):
        g.search(feats[:2], top_k=33)


# ------------------------------------------------------------------------------------------------ PPVectorPredictor
def _parent_recognition(audio_feature, users_name, feat, threshold):
    """The parent's recognition body (sorted users, per-user mean, cosine, argmax, threshold) in float64."""
    users = sorted(set(users_name))
    means = np.stack([audio_feature[[i for i, n in enumerate(users_name) if n == u]].astype(np.float64).mean(axis=0) for u in users])
    s = og.scores(feat[None], means)[0]
    i = int(np.argmax(s))
    return (users[i], s[i]) if s[i] >= threshold else (None, None)


def test_predictor_recognition(N, golden_dir, tmp_path, monkeypatch):
    import wave
    from oracle import models as om
    from ppvector.predict import PPVectorPredictor
    from ppvector.utils.checkpoint import save_pdparams
    from tests.test_gpu_models import _cfg
    pcm = np.load(f'{golden_dir}/wavs_3s.npz')['pcm']
    cuts = [(0, 0, 40000), (1, 0, 30000), (1, 9000, 48000), (2, 0, 41000), (2, 6000, 40000), (3, 0, 20000), (3, 10000, 44000)]
    paths = []
    for j, (i, a, b) in enumerate(cuts):
        p = str(tmp_path / f'u{j}.wav')
        with wave.open(p, 'wb') as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm[i, a:b].tobytes())
        paths.append(p)
    mdir = tmp_path / 'EcapaTdnn_Fbank' / 'best_model'
    mdir.mkdir(parents=True)
    save_pdparams({'0.' + k: v for k, v in om.ecapa_params(80, seed=1000).items()}, str(mdir / 'model.pdparams'))
    db = str(tmp_path / 'audio_db')
    pred = PPVectorPredictor(_cfg(), audio_db_path=db, model_path=str(mdir))
    assert pred.recognition(paths[0]) == (None, None) and pred.recognition_batch(paths[:2]) == [[], []]
    # three users with 1, 2 and 3 utterances, enrolled interleaved; paths[6] is enrolled by nobody
    for j, user in ((3, 'carol'), (0, 'alice'), (1, 'bob'), (4, 'carol'), (2, 'bob'), (5, 'carol')):
        assert pred.register(paths[j], user)[0]
    assert pred.gallery.names == ['carol', 'alice', 'bob'] and len(pred.gallery) == 3
    assert pred.audio_feature.shape == (6, 192) and len(pred.users_name) == 6

    singles = []
    for p in paths:
        name, score = pred.recognition(p, threshold=-1.0)
        ref_name, ref_score = _parent_recognition(pred.audio_feature, pred.users_name, pred.predict(p), -1.0)
        assert name == ref_name and name is not None
        assert abs(score - ref_score) <= 1e-5
        singles.append((name, score))
    assert singles[0][0] == 'alice' and singles[0][1] > 0.9999

    # the batch: predict_batch's embeddings (zero-padded waveforms) on both sides
    eb = pred.predict_batch(paths)
    batch = pred.recognition_batch(paths, threshold=-1.0)
    assert len(batch) == len(paths)
    for j, p in enumerate(paths):
        with monkeypatch.context() as m:
            m.setattr(pred, 'predict', lambda *a, _e=eb[j], **kw: _e)
            assert batch[j] == [pred.recognition(p, threshold=-1.0)]
    top3 = pred.recognition_batch(paths, threshold=-1.0, top_k=3)
    for j, row in enumerate(top3):
        assert sorted(n for n, _ in row) == ['alice', 'bob', 'carol']
        assert [s for _, s in row] == sorted((s for _, s in row), reverse=True)
        assert row[0] == batch[j][0]
    assert pred.recognition_batch(paths, threshold=1.5, top_k=3) == [[] for _ in paths]
    assert pred.recognition(paths[0], threshold=1.5) == (None, None)

    # a second predictor over the same directory loads audio_indexes.bin: the same library, the same answers
    again = PPVectorPredictor(_cfg(), audio_db_path=db, model_path=str(mdir))
    assert again.users_name == pred.users_name and np.array_equal(again.audio_feature, pred.audio_feature)
    assert again.gallery.names == pred.gallery.names and torch.equal(again.gallery.centroids, pred.gallery.centroids)
    assert [again.recognition(p, threshold=-1.0) for p in paths] == singles
    assert again.recognition_batch(paths, threshold=-1.0, top_k=3) == top3

    # a zero embedding scores 0 against everybody: nobody at any positive threshold
    with monkeypatch.context() as m:
        m.setattr(pred, 'predict', lambda *a, **kw: np.zeros(192, np.float32))
        assert pred.recognition(paths[0], threshold=1e-6) == (None, None)

    assert pred.remove_user('bob') and not pred.remove_user('bob')
    assert pred.gallery.names == ['carol', 'alice']
    for row in pred.recognition_batch(paths, threshold=-1.0, top_k=3):
        assert sorted(n for n, _ in row) == ['alice', 'carol']
    assert all(pred.recognition(p, threshold=-1.0)[0] in ('alice', 'carol') for p in paths)
    assert pred.remove_user('carol') and pred.remove_user('alice') and pred.audio_feature is None
    assert pred.recognition(paths[0]) == (None, None)
    assert pred.register(paths[0], 'alice')[0] and pred.recognition(paths[0], threshold=0.5)[0] == 'alice'
