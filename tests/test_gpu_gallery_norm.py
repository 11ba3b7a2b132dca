"""The 1:N search on normalised scores (csrc/gallery.hip: vp_gallery_topk_norm_f32), the cohort statistics with the cohort split
over workgroups (csrc/cohort_stats.hip: vp_cohort_stats_split_f32) and their way up through SpeakerGallery and PPVectorPredictor,
against tests/gallery_norm_oracle.py; docs/gallery.md ("Search on normalised scores") and docs/score_norm.md are the contract.
Shapes: every edge of the 32-query tile, the 128-row slab and the split's ranges, D with and without the tail of four, both digit
widths (D = 1024 is the largest LDS request of both kernels, at k = 32), U < k.  No case has more than 65 x 384 pairs.

Observed on an MI355X (the tests print these; docs/gallery.md has them): band family, largest |z - float64| 1.9e-06 and 4.0e-06
against a tol (the largest per-pair z_bound) of 5.4e-04 and 3.9e-04; split statistics |mean - float64| 3.0e-08 and 4.8e-09,
|std - float64| 1.5e-08 and 4.9e-09, against the derived 2e-06; at the split's plan edges at most 5.3e-08."""
import numpy as np
import pytest
import torch

from tests import gallery_norm_oracle as ogn
from tests import gallery_oracle as og
from tests import score_norm_oracle as osn
from tests import trial_ranks_oracle as ot

pytestmark = pytest.mark.gpu

TOL = ot.TOL

EXACT = [       # (Q, U, C, D, k, top_n), then lattice_case's (nspk, moved) and whether the returned rows must hold exact z ties
    (1, 1, 129, 20, 1, 20, 6, 5, False),
    (33, 129, 129, 32, 5, 20, 3, 2, True),
    (31, 128, 257, 64, 32, 128, 2, 1, True),
    (65, 257, 384, 192, 5, 300, 3, 2, True),
    (32, 129, 384, 1024, 32, 100, 12, 5, True),
    (3, 7, 129, 20, 32, 20, 6, 5, False),               # U < k: the tail
]
BAND = [        # (Q, U, C, D, k, top_n), then band_case's (nspk, seed): chosen so that every sigma64 >= 0.01 (asserted)
    (70, 300, 300, 20, 5, 50, 10, 3),
    (33, 640, 640, 192, 32, 300, 30, 3),
]


@pytest.fixture(scope='module')
def N():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: these tests must run on an MI355X (no CPU fallback exists)')
    from ppvector import _native
    return _native


@pytest.fixture(scope='module')
def SN():
    from ppvector.metric import score_norm
    return score_norm


def _gpu(a):
    return torch.as_tensor(a).cuda().contiguous()


def _same_bits(a, b):
    return all(x.shape == y.shape and (np.ascontiguousarray(x).view(np.int32) == np.ascontiguousarray(y).view(np.int32)).all()
               for x, y in zip(a, b))


_CASES = {}


def _lattice(Q, U, C, D, nspk, moved):
    """lattice_case once per shape (never modified): the first list is the queries, then the gallery; the second list is the cohort.
    A row has length 4: a quarter of it is its unit row, exactly.  -> queries, gallery unit rows, cohort, exact float32 cosines of
    queries x gallery, queries x cohort, gallery x cohort."""
    key = (Q, U, C, D, nspk, moved)
    if key not in _CASES:
        x, _, c, _ = ot.lattice_case(Q + U, C, D, nspk, moved, seed=7)
        q, g = x[:Q], x[Q:] / np.float32(4)
        s, sq, su = ot.scores64(q, g), ot.scores64(q, c), ot.scores64(g, c)
        assert all((m * 16 == np.round(m * 16)).all() for m in (s, sq, su))
        _CASES[key] = (q, g, c, s.astype(np.float32), sq.astype(np.float32), su.astype(np.float32))
    return _CASES[key]


def _band(Q, U, C, D, top_n, nspk, seed):
    """band_case once per shape: queries, gallery rows (raw), cohort, then the float64 z matrix, its per-pair bound and the float64
    statistics of the queries and of the gallery rows."""
    key = ('band', Q, U, C, D, top_n, nspk, seed)
    if key not in _CASES:
        x, _, c, _ = ot.band_case(Q + U, C, D, nspk, seed)
        _CASES[key] = (x[:Q], x[Q:], c) + ogn.z_matrix64(x[:Q], x[Q:], c, top_n)
    return _CASES[key]


def _unit(N, cohort, C):
    """vp_unit_rows_f32 over the first C rows of a (possibly larger) buffer; the rows behind them keep what they held."""
    c = _gpu(cohort)
    out = torch.full_like(c, float('nan'))
    ctx = N.ctx()
    N.check(N.lib().vp_unit_rows_f32(ctx, c.data_ptr(), C, c.shape[1], out.data_ptr(), N.stream_ptr()), ctx)
    return out


def _search(N, SN, q, g, cohort, k, top_n, Q=None, U=None, C=None, poison=False):
    """The whole query path on the entry points: the split statistics of the queries, the gallery rows' statistics from
    vp_cohort_stats_f32 (the unit rows handed in as raw rows), r, vp_gallery_topk_norm_f32.  Q / U / C may be smaller than the
    buffers; ``poison`` fills both workspaces with NaN first.  -> (query mean, std), (row mean, std), idx, z: host arrays."""
    q, g, cohort = _gpu(q), _gpu(g), _gpu(cohort)
    Q = q.shape[0] if Q is None else Q
    U = g.shape[0] if U is None else U
    C = cohort.shape[0] if C is None else C
    D = q.shape[1]
    lib, ctx = N.lib(), N.ctx()

    def scratch(need):
        assert need > 0
        return torch.full((need // 4 + 64,), float('nan') if poison else 0.0, dtype=torch.float32, device='cuda').view(torch.uint8)
    qm, qs = SN.cohort_stats_split(q, _unit(N, cohort, C), top_n, Q=Q, C=C, ws=scratch(lib.vp_cohort_stats_split_workspace_bytes(Q, C, D)))
    um, us = SN.cohort_stats(g, cohort, top_n, Q=U, C=C)
    qr, ur = SN.recip_std(qs), SN.recip_std(us)
    ws = scratch(lib.vp_gallery_topk_workspace_bytes(Q, U, D, k))
    idx = torch.full((Q, k), -7, dtype=torch.int32, device='cuda')
    z = torch.full((Q, k), float('nan'), dtype=torch.float32, device='cuda')
    N.check(lib.vp_gallery_topk_norm_f32(ctx, q.data_ptr(), Q, g.data_ptr(), U, D, k, qm.data_ptr(), qr.data_ptr(), um.data_ptr(),
                                         ur.data_ptr(), idx.data_ptr(), z.data_ptr(), ws.data_ptr(), ws.numel(), N.stream_ptr()), ctx)
    return tuple(t.cpu().numpy() for t in (qm, qs)), tuple(t.cpu().numpy() for t in (um, us)), idx.cpu().numpy(), z.cpu().numpy()


# ------------------------------------------------------------------------------------------------ exact family
@pytest.mark.parametrize('Q,U,C,D,k,top_n,nspk,moved,ties', EXACT)
def test_exact(N, SN, Q, U, C, D, k, top_n, nspk, moved, ties):
    q, g, c, s, sq, su = _lattice(Q, U, C, D, nspk, moved)
    qref, uref = osn.topn_stats32(sq, top_n), osn.topn_stats32(su, top_n)
    zref = ogn.z_matrix32(s, qref, uref)
    iref, vref = ogn.topk_z(zref, k)
    n = min(k, U)
    tied = int(sum((np.diff(vref[i, :n]) == 0).any() for i in range(Q)))
    print(f'[gallery norm exact {(Q, U, C, D, k, top_n)}] {tied} of {Q} returned rows hold an exact z tie; {len(np.unique(zref))} distinct z')
    assert tied >= 1 or not ties                        # a property of the inputs: the tie rule is exercised
    qst, ust, idx, z = _search(N, SN, q, g, c, k, top_n)
    assert _same_bits(qst, qref), (np.abs(qst[0] - qref[0]).max(), np.abs(qst[1] - qref[1]).max())
    unsplit = tuple(t.cpu().numpy() for t in SN.cohort_stats(_gpu(q), _gpu(c), top_n))
    assert _same_bits(qst, unsplit)
    assert _same_bits(ust, uref)
    assert idx.dtype == np.int32 and (idx == iref).all(), np.argwhere(idx != iref)[:4]
    assert _same_bits((z,), (vref,))
    assert (idx[:, n:] == -1).all() and np.isneginf(z[:, n:]).all()
    first = (qst, ust, idx, z)

    def same(other):
        return _same_bits(first[0] + first[1] + (first[3],), other[0] + other[1] + (other[3],)) and (first[2] == other[2]).all()
    assert same(_search(N, SN, q, g, c, k, top_n))                                              # a second run
    assert same(_search(N, SN, q, g, c[np.random.RandomState(3).permutation(C)], k, top_n))     # the cohort's order
    # NaN rows behind Q, U and C in larger buffers, NaN-filled workspaces
    big = [np.full((rows + extra, D), np.nan, np.float32) for rows, extra in ((Q, 40), (U, 50), (C, 60))]
    big[0][:Q], big[1][:U], big[2][:C] = q, g, c
    assert same(_search(N, SN, big[0], big[1], big[2], k, top_n, Q=Q, U=U, C=C, poison=True))


def test_zero_query_and_null_statistics(N, SN):
    Q, U, C, D, k, top_n, nspk, moved, _ = EXACT[1]
    q, g, c, s, sq, su = _lattice(Q, U, C, D, nspk, moved)
    q, s, sq = q.copy(), s.copy(), sq.copy()
    q[7], s[7], sq[7] = 0.0, 0.0, 0.0
    qst, ust, idx, z = _search(N, SN, q, g, c, k, top_n)
    assert qst[0][7] == 0.0 and qst[1][7] == 0.0 and float(osn.recip_std(qst[1])[7]) == float(np.float32(1) / np.float32(1e-6))
    zref = ogn.z_matrix32(s, osn.topn_stats32(sq, top_n), osn.topn_stats32(su, top_n))
    iref, vref = ogn.topk_z(zref, k)
    assert np.isfinite(z).all() and (idx == iref).all() and _same_bits((z,), (vref,))
    # a null statistics pointer, everything else in place: VP_EINVAL, nothing launched
    lib, ctx = N.lib(), N.ctx()
    t = torch.zeros(1 << 16, dtype=torch.float32, device='cuda')
    p = t.data_ptr()
    for missing in range(4):
        st = [p] * 4
        st[missing] = None
        assert lib.vp_gallery_topk_norm_f32(ctx, p, 3, p, 10, 192, 5, st[0], st[1], st[2], st[3], p, p, p, t.numel() * 4,
                                            N.stream_ptr()) == N.VP_EINVAL


# ------------------------------------------------------------------------------------------------ band family
def _gallery(q_rows, sn):
    from ppvector.infer_utils.gallery import SpeakerGallery
    g = SpeakerGallery(q_rows.shape[1])
    g.rebuild([f'u{i}' for i in range(len(q_rows))], q_rows)
    g.set_score_norm(sn)
    return g


@pytest.mark.parametrize('Q,U,C,D,k,top_n,nspk,seed', BAND)
def test_band(N, SN, Q, U, C, D, k, top_n, nspk, seed):
    """Statistics: every score is within TOL of its float64 value; order statistics, and the standard deviation of the sorted top-N
    vector, are 1-Lipschitz in the sup norm; a second TOL covers the rounding to float32 (docs/score_norm.md, "Band family").  The
    search: tests/gallery_oracle.py's check_topk on the float64 z matrix with tol = the largest per-pair z_bound, the precedent of the
    fused scorer's band test."""
    q, rows, c, z64, bound, (qm64, qs64), (um64, us64) = _band(Q, U, C, D, top_n, nspk, seed)
    assert min(qs64.min(), us64.min()) >= 0.01              # a condition on the inputs: first-order propagation is valid
    sn = SN.ScoreNorm(_gpu(c), top_n)
    qm, qr = sn.mean_r_queries(_gpu(q))
    qs = SN.cohort_stats_split(_gpu(q), sn.unit_cohort(), top_n)[1]
    em, es = np.abs(qm.cpu().numpy() - qm64).max(), np.abs(qs.cpu().numpy() - qs64).max()
    g = _gallery(rows, sn)
    um, ur = g._mean[:U].cpu().numpy(), g._r[:U].cpu().numpy()
    eu = np.abs(um - um64).max()
    idx, z = g.search(_gpu(q), k)
    assert idx.dtype == torch.int32 and z.dtype == torch.float32 and idx.is_cuda and z.is_cuda
    print(f'[gallery norm band {(Q, U, C, D, k, top_n)}] sigma64 {min(qs64.min(), us64.min()):.3f} ..; split statistics: largest '
          f'|mean - float64| {em:.3e}, |std - float64| {es:.3e} (bound {2 * TOL:.0e}); rows: |mean - float64| {eu:.3e}')
    assert em <= 2 * TOL and es <= 2 * TOL and eu <= 2 * TOL
    assert (np.abs(1.0 / ur.astype(np.float64) - us64) <= 2 * TOL + 2.0 ** -22).all()      # r = 1 / std, one more f32 rounding
    worst = og.check_topk(idx.cpu().numpy(), z.cpu().numpy(), z64, k, tol=float(bound.max()))
    print(f'[gallery norm band {(Q, U, C, D, k, top_n)}] largest |z - float64| {worst:.3e} (tol {bound.max():.3e})')
    again = g.search(_gpu(q), k)
    assert torch.equal(again[0], idx) and torch.equal(again[1].view(torch.int32), z.view(torch.int32))


# ------------------------------------------------------------------------------------------------ the split's plan
def _plan_edges(N):
    per = N.VP_COHORT_SPLIT_SLABS
    return [(1, 192), (128 * per, 192), (128 * per + 1, 192), (128 * per * 2 + 77, 192), (128 * per * 2 + 77, 1024),
            (128 * per * N.VP_COHORT_SPLIT_MAX_RANGES + 1, 20)]


@pytest.mark.parametrize('edge', range(6))
def test_split_plan_edges(N, SN, edge):
    """C = 1, C = exactly one workgroup's slabs, one row more, three ranges at both digit widths, and the first C at which a
    workgroup walks one slab more than VP_COHORT_SPLIT_SLABS.  k = 1 over a gallery of 32 rows: the plain search at k = 32 returns
    every cosine as the walk computes it, so the normalised search must return the restatement's z of those, bit for bit."""
    C, D = _plan_edges(N)[edge]
    ranges = ogn.split_ranges(C, N.VP_COHORT_SPLIT_SLABS, N.VP_COHORT_SPLIT_MAX_RANGES)[1]
    assert ranges == (1, 1, 2, 3, 3, 43)[edge]
    Q, U = 37, 32
    x, _, c, _ = ot.band_case(Q + U, C, D, 10, seed=5)
    q, rows = x[:Q], x[Q:]
    m64, s64 = osn.topn_stats(ot.scores64(q, c), 50)
    sn = SN.ScoreNorm(_gpu(c), 50)
    mean, std = (t.cpu().numpy() for t in SN.cohort_stats_split(_gpu(q), sn.unit_cohort(), 50))
    em, es = np.abs(mean - m64).max(), np.abs(std - s64).max()
    print(f'[split plan C = {C}, D = {D}, {ranges} ranges] largest |mean - float64| {em:.3e}, |std - float64| {es:.3e}')
    assert em <= 2 * TOL and es <= 2 * TOL
    again = tuple(t.cpu().numpy() for t in SN.cohort_stats_split(_gpu(q), sn.unit_cohort(), 50))
    assert _same_bits((mean, std), again)
    unsplit = tuple(t.cpu().numpy() for t in SN.cohort_stats(_gpu(q), _gpu(c), 50))
    assert np.abs(mean - unsplit[0]).max() <= 4 * TOL and np.abs(std - unsplit[1]).max() <= 4 * TOL     # each within 2 TOL of float64
    g = _gallery(rows, None)
    cos_idx, cos = (t.cpu().numpy() for t in g.search(_gpu(q), 32))
    s = np.empty((Q, U), np.float32)
    np.put_along_axis(s, cos_idx.astype(np.int64), cos, axis=1)             # the cosines by row
    g.set_score_norm(sn)
    ustats = (g._mean[:U].cpu().numpy(), g._r[:U].cpu().numpy())
    zref = osn.z32(s, ustats[0], ustats[1], mean, osn.recip_std(std))
    iref, vref = ogn.topk_z(zref, 1)
    idx, z = (t.cpu().numpy() for t in g.search(_gpu(q), 1))
    assert (idx == iref).all() and _same_bits((z,), (vref,))


def test_batch_independence(N, SN):
    """A query's statistics and its z row do not depend on the batch it came in: alone, or as row 40 of 70."""
    Q, U, C, D, k, top_n, nspk, seed = BAND[0]
    q, rows, c = _band(Q, U, C, D, top_n, nspk, seed)[:3]
    sn = SN.ScoreNorm(_gpu(c), top_n)
    g = _gallery(rows, sn)
    all_stats = [t.cpu().numpy() for t in sn.mean_r_queries(_gpu(q))]
    one_stats = [t.cpu().numpy() for t in sn.mean_r_queries(_gpu(q[40:41]))]
    assert _same_bits([t[40:41] for t in all_stats], one_stats)
    all_idx, all_z = (t.cpu().numpy() for t in g.search(_gpu(q), 32))
    one_idx, one_z = (t.cpu().numpy() for t in g.search(_gpu(q[40:41]), 32))
    assert (all_idx[40:41] == one_idx).all() and _same_bits((all_z[40:41],), (one_z,))


def test_queries_past_the_cap_go_in_chunks(N, SN):
    Q, C, D = N.VP_COHORT_SPLIT_MAX_Q + 33, 129, 20
    x, _, c, _ = ot.lattice_case(64, C, D, 6, 5, seed=7)
    q = np.tile(x, (Q // 64 + 1, 1))[:Q]
    ref = osn.topn_stats32(ot.scores64(q, c).astype(np.float32), 20)
    sn = SN.ScoreNorm(_gpu(c), 20)
    mean, r = (t.cpu().numpy() for t in sn.mean_r_queries(_gpu(q)))
    assert _same_bits((mean, r), (ref[0], osn.recip_std(ref[1])))


# ------------------------------------------------------------------------------------------------ gallery bookkeeping
def test_gallery_keeps_the_statistics_in_step(N, SN):
    from ppvector.infer_utils.gallery import SpeakerGallery
    D, users = 20, 70                                       # past the first capacity (64)
    x, _, c, _ = ot.band_case(2 * users + 9, 300, D, 10, seed=4)
    feats = {f'u{i}': x[2 * i:2 * i + 1 + i % 2] for i in range(users)}     # one or two utterances a user
    sn = SN.ScoreNorm(_gpu(c), 50)
    g = SpeakerGallery(D)
    g.set_score_norm(sn)                                    # on the empty gallery
    assert g.score_norm is sn

    def fresh():
        h = SpeakerGallery(D)
        h.rebuild([n for n in g.names for _ in feats[n]], np.concatenate([feats[n] for n in g.names]))
        h.set_score_norm(sn)
        return h

    def in_step(what):
        h, n = fresh(), len(g)
        assert h.names == g.names and torch.equal(h.centroids, g.centroids), what
        for a, b in ((g._mean, h._mean), (g._r, h._r)):
            assert torch.equal(a[:n].view(torch.int32), b[:n].view(torch.int32)), what
        assert torch.isfinite(g._mean[:n]).all() and (g._r[:n] > 0).all()
    for name in list(feats)[:40]:
        g.set_user(name, feats[name])                       # new users, one row at a time
    in_step('set_user of new users')
    feats['u7'] = x[-9:-5]
    g.set_user('u7', feats['u7'])                           # an existing user
    in_step('set_user of an existing user')
    assert g.remove('u20')                                  # a middle user: the last row moves into the hole
    feats.pop('u20')
    in_step('remove')
    for name in list(feats)[39:]:
        g.set_user(name, feats[name])                       # growth past 64 rows
    assert len(g) == users - 1 > 64
    in_step('growth')
    g.rebuild([n for n in g.names for _ in feats[n]], np.concatenate([feats[n] for n in g.names]))
    in_step('rebuild with a score norm set')
    # set_score_norm(None): the search of a gallery that never had one, bit for bit
    q = _gpu(x[-5:])
    zi, z = g.search(q, 5)
    g.set_score_norm(None)
    assert g.score_norm is None and g._mean is None and g._r is None
    never = SpeakerGallery(D)
    never.rebuild([n for n in g.names for _ in feats[n]], np.concatenate([feats[n] for n in g.names]))
    (ai, a), (bi, b) = g.search(q, 5), never.search(q, 5)
    assert torch.equal(ai, bi) and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(a, z)                            # ... which is not what it returned with one
    with pytest.raises(ValueError):
        g.set_score_norm('as-norm')
    with pytest.raises(ValueError):
        g.set_score_norm(SN.ScoreNorm(torch.ones((5, D + 4), device='cuda'), 3))


# ------------------------------------------------------------------------------------------------ PPVectorPredictor
def test_predictor_on_normalised_scores(N, SN, golden_dir, tmp_path, monkeypatch):
    import wave
    from oracle import models as om
    from ppvector.metric.metrics import cosine_score_matrix
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
    pred = PPVectorPredictor(_cfg(), threshold=-1.0, audio_db_path=str(tmp_path / 'audio_db'), model_path=str(mdir))
    for j, user in ((3, 'carol'), (0, 'alice'), (1, 'bob'), (4, 'carol'), (2, 'bob')):
        assert pred.register(paths[j], user)[0]

    def answers():
        return [pred.recognition(p) for p in paths], pred.recognition_batch(paths, top_k=3), pred.contrast(paths[0], paths[6])
    before = answers()
    assert all(name is not None for name, _ in before[0])

    # the cohort: the enrolled embeddings and noise around them (an untrained model: any cohort of the right width will do)
    rs = np.random.RandomState(11)
    cohort = np.concatenate([pred.audio_feature + 0.3 * np.abs(pred.audio_feature).mean() * rs.standard_normal(pred.audio_feature.shape)
                             for _ in range(8)]).astype(np.float32)
    sn = SN.ScoreNorm(cohort, top_n=10)
    with pytest.raises(TypeError):
        pred.set_score_norm(sn)                             # a z is not a cosine: the threshold has to be given
    assert pred.score_norm is None and pred.gallery.score_norm is None and pred.threshold == -1.0
    pred.set_score_norm(sn, threshold=-1e9)
    assert pred.gallery.score_norm is sn and pred.threshold == -1e9
    names = pred.gallery.names
    for p, (name, z) in zip(paths, [pred.recognition(p) for p in paths]):
        idx, score = pred.gallery.search(_gpu(pred.predict(p)[None]), 1)
        assert (name, z) == (names[int(idx[0, 0])], round(float(score[0, 0]), 5))
    eb = pred.predict_batch(paths)
    idx, score = (t.cpu().numpy() for t in pred.gallery.search(_gpu(eb), 3))
    assert pred.recognition_batch(paths, top_k=3) == [[(names[i], round(float(s), 5)) for i, s in zip(ri, rs_)]
                                                      for ri, rs_ in zip(idx, score)]
    zq = np.asarray([[s for _, s in row] for row in pred.recognition_batch(paths, top_k=3)])
    cq = np.asarray([[s for _, s in row] for row in before[1]])
    assert np.isfinite(zq).all() and np.abs(zq - cq).max() > 1e-3           # these are not the cosines
    a, b = _gpu(pred.predict(paths[0])[None]), _gpu(pred.predict(paths[6])[None])
    want = float(sn.normalise(cosine_score_matrix(a, b).contiguous(), a, b)[0, 0])
    assert pred.contrast(paths[0], paths[6]) == want != before[2]
    # the threshold is on z
    pred.set_score_norm(sn, threshold=1e9)
    assert pred.recognition(paths[0]) == (None, None) and pred.recognition_batch(paths[:2]) == [[], []]
    # a user enrolled while the score norm is set gets its statistics
    assert pred.register(paths[5], 'carol')[0]
    fresh = sn.mean_r(pred.gallery.centroids)
    n = len(pred.gallery)
    assert torch.equal(pred.gallery._mean[:n], fresh[0]) and torch.equal(pred.gallery._r[:n], fresh[1])
    # ... and carol as she was: her two utterances in their order give her centroid's bits again (her row is now the last one)
    assert pred.remove_user('carol') and pred.register(paths[3], 'carol')[0] and pred.register(paths[4], 'carol')[0]
    # back: the cosine search and the threshold that was in force before
    pred.set_score_norm(None)
    assert pred.score_norm is None and pred.gallery.score_norm is None and pred.threshold == -1.0
    assert answers() == before
