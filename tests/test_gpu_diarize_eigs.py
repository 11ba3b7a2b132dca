"""The GPU spectral solver (csrc/diarize_eigs.hip, smallest_eigenpairs) on the engine's own Laplacians of planted speakers, against the
float64 eigenpairs of the same f32 matrix (tests/eigs_oracle.py).  The yardstick of every accuracy bound is the path the solver replaces,
scipy.linalg.eigh of the f32 matrix, scored by the same measures in the same test: bound = max(8 x that, a floor)."""
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import diarization_oracle as od
from tests import eigs_oracle as oe

pytestmark = pytest.mark.gpu

K = oe.N_VALUES
CASE_IDS = [f'N{n}-spk{s}-noise{z}' for n, s, z, _ in oe.CASES]


@functools.lru_cache(maxsize=None)
def _laplacian(case):
    from ppvector.infer_utils.speaker_diarization import SpectralCluster
    n, spk, noise, seed = case
    x, who = oe.planted(n, spk, noise, seed)
    return SpectralCluster().laplacian(x), who


@functools.lru_cache(maxsize=None)
def _case(case):
    """Computed once per case: the device Laplacian, its float64 reference, the host-f32 eigenpairs and the GPU solver's."""
    import scipy.linalg
    from ppvector.infer_utils.speaker_diarization import smallest_eigenpairs
    L, who = _laplacian(case)
    L_host = L.cpu().numpy()
    ref = oe.reference(L_host)
    lam32, V32 = scipy.linalg.eigh(L_host)
    lam, V, info = smallest_eigenpairs(L, K)
    for a in (L_host, lam, V, ref['lam'], ref['V']):
        a.setflags(write=False)
    return dict(L=L, who=who, ref=ref, host=(lam32, V32), gpu=(lam, V, info))


@pytest.mark.parametrize('case', oe.CASES, ids=CASE_IDS)
def test_accuracy_against_float64_with_the_host_path_as_yardstick(case):
    c = _case(case)
    ref = c['ref']
    assert ref['well_separated'] and ref['k_s'] == case[1], (ref['largest_gap'], ref['second_gap'], ref['k_s'])   # the input, not the solver
    lam, V, info = c['gpu']
    assert lam.dtype == np.float64 and lam.shape == (K,) and V.dtype == np.float32 and V.shape == (case[0], K)
    assert info.converged and (info.residuals <= 1e-6 * info.sigma).all(), info
    assert (np.diff(lam) >= 0).all()
    host = oe.measures(*c['host'], ref)
    got = oe.measures(lam, V, ref)
    bound = oe.bounds(host)
    print(f'[eigs N={case[0]} spk={case[1]} noise={case[2]}] rounds {info.rounds} products {info.products} worst residual '
          f'{info.residuals.max() / info.sigma:.3g} sigma | eigenvalues {got[0]:.3g} eps lmax (host f32 {host[0]:.3g}, bound {bound[0]:.3g}) | '
          f'leakage {got[1]:.3g} (host {host[1]:.3g}, bound {bound[1]:.3g}) | orthogonality {got[2]:.3g} (host {host[2]:.3g}, bound {bound[2]:.3g})')
    assert got[0] <= bound[0] and got[1] <= bound[1] and got[2] <= bound[2], (got, bound)
    # the whole basis, not only the first k_s columns, is orthonormal: the contract's floor for k_s columns, scaled to 16 (at a given
    # error per entry the Frobenius norm of Q^T Q - I grows with the number of columns)
    Q = V.astype(np.float64)
    assert np.linalg.norm(Q.T @ Q - np.eye(K)) <= 1e-5 * K / ref['k_s']
    # the reported residuals are residuals: recomputed in float64 from the f32 matrix they agree to 1e-6 sigma
    L64 = c['L'].cpu().numpy().astype(np.float64)
    res = np.linalg.norm(L64 @ Q - Q * lam[None, :], axis=0)
    assert np.abs(res - info.residuals).max() <= 1e-6 * info.sigma, (res, info.residuals)


@pytest.mark.parametrize('case', oe.CASES, ids=CASE_IDS)
def test_gap_decision_is_the_float64_one(case):
    c = _case(case)
    assert c['ref']['well_separated']
    assert oe.decision(c['gpu'][0]) == oe.decision(c['ref']['lam']) == case[1]


def test_two_runs_give_the_same_bits():
    from ppvector.infer_utils.speaker_diarization import smallest_eigenpairs
    c = _case(oe.CASES[3])                                            # N = 257: a partial 32-row tile and a partial Gram block
    lam, V, info = smallest_eigenpairs(c['L'], K)
    assert np.array_equal(lam, c['gpu'][0]) and np.array_equal(V, c['gpu'][1])
    assert info.rounds == c['gpu'][2].rounds and np.array_equal(info.residuals, c['gpu'][2].residuals)


@pytest.mark.parametrize('n', [4097, 16384])
def test_larger_sizes_are_eigenpairs(n):
    """The sizes at which a product is cut into fewer slices of k (7 at 4097, with a one-row tile at the end; 2 at 16384, the largest N
    of the contract), without a float64 decomposition: the pairs are checked as eigenpairs on the GPU.  |L v - lambda v|_2 recomputed by
    an f32 matmul stays under the stopping tolerance 1e-6 sigma plus 1e-6 sigma for the f32 product and the f32 rounding of lambda and v;
    the basis is orthonormal to the contract's floor scaled to 16 columns; the eigenvalues ascend from (nearly) 0."""
    from ppvector.infer_utils.speaker_diarization import SpectralCluster, smallest_eigenpairs
    x, _ = oe.planted(n, 8, 1.0, 0)
    L = SpectralCluster().laplacian(x)
    lam, V, info = smallest_eigenpairs(L, K)
    print(f'[eigs N={n}] rounds {info.rounds} products {info.products} worst residual {info.residuals.max() / info.sigma:.3g} sigma')
    assert info.converged and V.shape == (n, K)
    Vd = torch.from_numpy(V).cuda()
    res = torch.linalg.norm(L @ Vd - Vd * torch.from_numpy(lam).float().cuda()[None, :], dim=0).cpu().numpy()
    assert res.max() <= 2e-6 * info.sigma, (res / info.sigma)
    Q = V.astype(np.float64)
    assert np.linalg.norm(Q.T @ Q - np.eye(K)) <= 1e-5 * K
    assert (np.diff(lam) >= 0).all() and abs(lam[0]) <= 1e-5 * info.sigma and lam[-1] < info.sigma


def _speakers(centres, counts, seed, noise=0.3):
    """The recipe of tests/test_gpu_diarization.py: points around unit centres with Gaussian noise of relative norm `noise`, shuffled."""
    rng = np.random.RandomState(seed)
    d = centres.shape[1]
    who = rng.permutation(np.repeat(np.arange(len(counts)), counts))
    x = centres[who] + noise / np.sqrt(d) * rng.standard_normal((who.size, d))
    return x.astype(np.float32), who


def _unit_centres(k, d, seed):
    c = np.random.RandomState(seed).standard_normal((k, d))
    return c / np.linalg.norm(c, axis=1, keepdims=True)


@pytest.fixture
def gpu_solver(monkeypatch):
    """The switch on 'gpu' for one test, every call of the solver counted, a RuntimeWarning (the fallback's) an error."""
    import ppvector
    from ppvector.infer_utils import speaker_diarization as sd
    calls = []
    real = sd.smallest_eigenpairs

    def counted(L, k, *a, **kw):
        calls.append((L.shape[0], k))
        return real(L, k, *a, **kw)

    monkeypatch.setattr(sd, 'smallest_eigenpairs', counted)
    before = ppvector.get_spectral_solver()
    ppvector.set_spectral_solver('gpu')
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('error', RuntimeWarning)
            yield calls
    finally:
        ppvector.set_spectral_solver(before)


@pytest.mark.parametrize('speaker_num', [None, 3])
def test_labels_of_three_separated_speakers(speaker_num, gpu_solver):
    from ppvector.infer_utils.speaker_diarization import SpeakerDiarization
    centres = _unit_centres(3, 192, 11)
    x, who = _speakers(centres, (40, 30, 20), 12)
    want, want_centres = od.clustering(x, speaker_num)
    assert want.max() == 2 and np.array_equal(want, od.relabel(who))
    labels, spk_centres = SpeakerDiarization().clustering(x, speaker_num=speaker_num)
    assert gpu_solver == [(90, 16 if speaker_num is None else 3)]                 # the GPU path ran, once
    assert np.array_equal(labels, want), (labels, want)
    assert spk_centres.shape == (3, 192) and np.abs(spk_centres - want_centres).max() < 1e-5


def test_labels_of_four_planted_speakers(gpu_solver):
    from ppvector.infer_utils.speaker_diarization import SpeakerDiarization
    x, who = oe.planted(257, 4, 0.8, 0)
    labels, _ = SpeakerDiarization().clustering(x)
    assert gpu_solver == [(257, 16)]
    assert np.array_equal(labels, od.relabel(who)), (labels, od.relabel(who))


def test_round_cap_falls_back_to_the_host_path(monkeypatch):
    import ppvector
    from ppvector.infer_utils import speaker_diarization as sd
    L, _ = _laplacian(oe.CASES[4])                                    # N = 1000: some ten rounds at the default caps
    _, _, info = sd.smallest_eigenpairs(L, K, max_rounds=1)
    assert not info.converged and info.rounds == 1 and info.residuals.max() > 1e-6 * info.sigma
    sc = sd.SpectralCluster()
    want_emb, want_k = sc.get_spec_embs(L)                            # the switch is on 'host'
    monkeypatch.setattr(sd, 'EIGS_MAX_ROUNDS', 1)
    before = ppvector.get_spectral_solver()
    ppvector.set_spectral_solver('gpu')
    try:
        with pytest.warns(RuntimeWarning, match='worst residual'):
            emb, k = sc.get_spec_embs(L)
    finally:
        ppvector.set_spectral_solver(before)
    assert k == want_k == 6 and np.array_equal(emb, want_emb)


def test_below_the_solvers_range_the_host_path_runs_silently(gpu_solver):
    from ppvector.infer_utils.speaker_diarization import SpectralCluster
    x, who = oe.planted(40, 2, 0.8, 0)
    labels = SpectralCluster()(x, oracle_num=2)
    assert gpu_solver == []
    assert np.array_equal(od.relabel(labels), od.relabel(who))


def test_argument_errors_launch_nothing():
    from ppvector import _native as N
    lib, ctx = N.lib(), N.ctx()
    L = torch.zeros((64, 64), device='cuda')
    out = torch.full((2 * 24 + 2,), 7.0, device='cuda')
    vecs = torch.full((64, 24), 7.0, device='cuda')
    ws = torch.zeros(lib.vp_eigs_workspace_bytes(64, 16), dtype=torch.uint8, device='cuda')
    assert ws.numel() > 4 * 64 * 32 * 4

    def call(fn, n, k, nbytes=ws.numel(), steps=()):
        return fn(ctx, L.data_ptr(), n, k, *steps, ws.data_ptr(), nbytes, out.data_ptr(), vecs.data_ptr(), out.data_ptr() + 4 * 24,
                  out.data_ptr() + 4 * 48, N.stream_ptr())

    for fn, steps in ((lib.vp_eigs_init_f32, ()), (lib.vp_eigs_iterate_f32, (4,))):
        assert call(fn, 63, 16, steps=steps) == N.VP_EUNSUP
        assert call(fn, 16385, 16, steps=steps) == N.VP_EUNSUP
        assert call(fn, 64, 0, steps=steps) == N.VP_EINVAL
        assert call(fn, 64, 25, steps=steps) == N.VP_EINVAL
        assert call(fn, 63, 25, steps=steps) == N.VP_EINVAL           # k is looked at first
        assert call(fn, 64, 16, nbytes=ws.numel() - 1, steps=steps) == N.VP_EWORKSPACE
    assert call(lib.vp_eigs_iterate_f32, 64, 16, steps=(0,)) == N.VP_EINVAL
    assert call(lib.vp_eigs_iterate_f32, 64, 16, steps=(65,)) == N.VP_EINVAL
    assert lib.vp_eigs_workspace_bytes(63, 16) == 0 and lib.vp_eigs_workspace_bytes(64, 25) == 0
    assert lib.vp_eigs_workspace_bytes(16384, 24) >= 4 * 16384 * 32 * 4
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((vecs == 7.0).all()) and not bool(ws.any())       # nothing was written


def test_zero_matrix():
    from ppvector.infer_utils.speaker_diarization import smallest_eigenpairs
    lam, V, info = smallest_eigenpairs(torch.zeros((64, 64), device='cuda'), K)
    assert info.converged and info.rounds == 0 and info.sigma == 0.0
    assert not lam.any() and not info.residuals.any()
    assert np.array_equal(V, np.eye(64, K, dtype=np.float32))
