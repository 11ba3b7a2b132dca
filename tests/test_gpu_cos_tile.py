"""The gallery search (csrc/gallery.hip) and the trial scorer (csrc/trial_ranks.hip) walk their rows with the same code
(csrc/cos_tile.h), so they give the same BITS for the same pair.  Rows are small integers: every float64 sum of squares is then an exact
integer in any order of addition, the three normalisers (the centroid kernel, the query tile's load, unit_rows_kernel) produce identical
unit rows, and a difference can only come from the walk.

Q = Nt = 33 is two column tiles, the second with one column; U = Ne = 289 is three slabs, the last with one full wave, one wave with a
single row and two waves with none.  D = 20: two groups of eight k and the D & 4 tail; 64: exactly one batch of eight groups, no tail;
76: one batch, one remainder group and the tail."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NQ, NU, K = 33, 289, 32
DIMS = (20, 64, 76)


@pytest.fixture(scope='module')
def N():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: these tests must run on an MI355X (no CPU fallback exists)')
    from ppvector import _native
    return _native


def _int_rows(rs, n, D):
    x = rs.randint(-8, 9, size=(n, D))
    for r in np.flatnonzero(~x.any(axis=1)):
        while not x[r].any():
            x[r] = rs.randint(-8, 9, size=D)
    return x.astype(np.float32)


def _gallery_topk(rows, queries):
    from ppvector.infer_utils.gallery import SpeakerGallery
    gal = SpeakerGallery(rows.shape[1])
    gal.rebuild([f'u{i}' for i in range(len(rows))], rows)       # one feature per user: the centroid is the unit row
    idx, score = gal.search(queries, top_k=K)
    return idx.cpu().numpy(), score.cpu().numpy()


def _pair_scores(N, trials, enroll):
    """vp_trial_ranks_targets_f32 as TrialRanks.__init__ calls it, with all labels equal, trial_offsets[i] = i Ne and
    enroll_ranks[j] = j: the raw, unsorted targets are the (Nt, Ne) scores of every pair."""
    (Nt, D), Ne = trials.shape, enroll.shape[0]
    NT = Nt * Ne
    lib, ctx = N.lib(), N.ctx()
    need = lib.vp_trial_ranks_workspace_bytes(Nt, Ne, D, NT)
    assert need > 0
    t, e = torch.from_numpy(trials).cuda(), torch.from_numpy(enroll).cuda()
    tl, el = torch.zeros(Nt, dtype=torch.int32, device='cuda'), torch.zeros(Ne, dtype=torch.int32, device='cuda')
    off = torch.arange(Nt, dtype=torch.int64, device='cuda') * Ne
    rank = torch.arange(Ne, dtype=torch.int32, device='cuda')
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    raw = torch.full((NT,), float('nan'), dtype=torch.float32, device='cuda')
    N.check(lib.vp_trial_ranks_targets_f32(ctx, t.data_ptr(), tl.data_ptr(), off.data_ptr(), Nt, e.data_ptr(), el.data_ptr(),
                                           rank.data_ptr(), Ne, D, NT, raw.data_ptr(), ws.data_ptr(), ws.numel(), N.stream_ptr()), ctx)
    return raw.cpu().numpy().reshape(Nt, Ne)


def _host_topk(pairs):
    """Per trial the K best enrol rows, score descending then row ascending."""
    idx = np.stack([np.lexsort((np.arange(pairs.shape[1]), -s))[:K] for s in pairs]).astype(np.int32)
    return idx, np.take_along_axis(pairs, idx, axis=1)


_runs = {}


def _run(N, D):
    """Both units on the same rows, and on the rows shuffled by one permutation: computed once per D."""
    if D not in _runs:
        rs = np.random.RandomState(4000 + D)
        rows, queries = _int_rows(rs, NU, D), _int_rows(rs, NQ, D)
        perm = rs.permutation(NU)
        _runs[D] = dict(perm=perm, gallery=_gallery_topk(rows, queries), pairs=_pair_scores(N, queries, rows),
                        gallery_p=_gallery_topk(rows[perm], queries), pairs_p=_pair_scores(N, queries, rows[perm]))
    return _runs[D]


def _assert_same_bits(gallery, pairs):
    idx, score = gallery
    want_idx, want_score = _host_topk(pairs)
    assert not np.isnan(pairs).any()
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(score.view(np.uint32), want_score.view(np.uint32))


@pytest.mark.parametrize('D', DIMS)
def test_gallery_and_scorer_give_the_same_bits(N, D):
    r = _run(N, D)
    _assert_same_bits(r['gallery'], r['pairs'])


@pytest.mark.parametrize('D', DIMS)
def test_a_pair_keeps_its_bits_when_the_rows_move(N, D):
    """Row j of the shuffled matrix is row perm[j] of the first: the pair (i, perm[j]) has the same bits in both runs of the scorer,
    and the shuffled gallery agrees with the shuffled scorer as the first does."""
    r = _run(N, D)
    assert np.array_equal(r['pairs_p'].view(np.uint32), r['pairs'][:, r['perm']].view(np.uint32))
    _assert_same_bits(r['gallery_p'], r['pairs_p'])
