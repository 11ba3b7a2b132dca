"""Host side of the GPU spectral solver: the switch, the binding of its entry points, the filter-degree rule and the paths that must not
reach the GPU (no device is needed for any of it)."""
import ctypes as C

import numpy as np
import pytest

from tests import diarization_oracle as od
from tests import eigs_oracle as oe


def test_the_default_solver_is_the_host():
    import ppvector
    assert ppvector.get_spectral_solver() == 'host'


def test_solver_switch():
    import ppvector
    try:
        ppvector.set_spectral_solver('gpu')
        assert ppvector.get_spectral_solver() == 'gpu'
        ppvector.set_spectral_solver('host')
        assert ppvector.get_spectral_solver() == 'host'
        for bad in ('cuda', 'GPU', '', None):
            with pytest.raises(ValueError):
                ppvector.set_spectral_solver(bad)
        assert ppvector.get_spectral_solver() == 'host'
    finally:
        ppvector.set_spectral_solver('host')


def test_entry_points_are_bound_as_the_header_declares_them():
    from ppvector import _native as N
    p, i, z = C.c_void_p, C.c_int, C.c_size_t
    assert N._PROTOS['vp_eigs_workspace_bytes'] == (z, [i, i])
    #                                          ctx L  N  k  ws ws_bytes evals evecs resid bounds stream
    assert N._PROTOS['vp_eigs_init_f32'] == (i, [p, p, i, i, p, z, p, p, p, p, p])
    #                                             ctx L  N  k steps ws ws_bytes evals evecs resid bounds stream
    assert N._PROTOS['vp_eigs_iterate_f32'] == (i, [p, p, i, i, i, p, z, p, p, p, p, p])
    lib = N.load_library()
    assert lib.vp_version() == 100
    # the workspace query is host arithmetic: four N x 32 f32 blocks and the Gram partials at least; 0 outside the supported range
    for n, k in ((64, 1), (257, 16), (16384, 24)):
        blocks = (n + 127) // 128
        assert lib.vp_eigs_workspace_bytes(n, k) >= 4 * n * 32 * 4 + blocks * (2 * 32 * 32 + 32) * 8
    for n, k in ((63, 16), (16385, 16), (64, 0), (64, 25), (-1, 1)):
        assert lib.vp_eigs_workspace_bytes(n, k) == 0


def test_filter_degree_rule():
    """m = floor(acosh(A) / acosh((sigma + a) / (sigma - a))) clamped to [2, EIGS_MAX_DEGREE]: T_m at the image of 0 stays under A."""
    import math
    from ppvector.infer_utils import speaker_diarization as sd
    A = sd.EIGS_MAX_AMPLIFICATION
    for sigma, a in ((89.4, 6.37), (22.7, 1.29), (14.2, 2.98), (100.0, 50.0), (100.0, 0.01)):
        m = sd._filter_degree(sigma, a)
        assert 2 <= m <= sd.EIGS_MAX_DEGREE
        t = math.acosh((sigma + a) / (sigma - a))
        if 2 < m:
            assert math.cosh(m * t) <= A * (1 + 1e-9)
        if m < sd.EIGS_MAX_DEGREE:
            assert math.cosh((m + 1) * t) > A
    assert sd._filter_degree(100.0, 0.01) == sd.EIGS_MAX_DEGREE
    for sigma, a in ((0.0, 0.0), (1.0, 1.0), (1.0, 2.0), (1.0, 0.0), (float('nan'), 1.0)):      # a degenerate interval: any small degree
        assert sd._filter_degree(sigma, a) == 2


def test_a_host_matrix_takes_the_host_path_whatever_the_switch(monkeypatch):
    import ppvector
    from ppvector.infer_utils import speaker_diarization as sd

    def boom(*a, **kw):
        raise AssertionError('the GPU solver was called')

    monkeypatch.setattr(sd, 'smallest_eigenpairs', boom)
    x, _ = oe.planted(96, 3, 0.8, 0)
    L = od.laplacian(od.prune(od.cosine_affinity(x), od.n_elems(96))).astype(np.float32)
    sc = sd.SpectralCluster()
    want_emb, want_k = sc.get_spec_embs(L)
    try:
        ppvector.set_spectral_solver('gpu')
        emb, k = sc.get_spec_embs(L)
        emb2, k2 = sc.get_spec_embs(L, 2)
    finally:
        ppvector.set_spectral_solver('host')
    assert k == want_k == 3 and np.array_equal(emb, want_emb)
    assert k2 == 2 and np.array_equal(emb2, want_emb[:, :2])


def test_smallest_eigenpairs_needs_a_gpu_tensor():
    import torch
    from ppvector import _native as N
    from ppvector.infer_utils.speaker_diarization import smallest_eigenpairs
    with pytest.raises(N.VpmiError):
        smallest_eigenpairs(np.zeros((64, 64), np.float32), 4)
    with pytest.raises(N.VpmiError):
        smallest_eigenpairs(torch.zeros(64, 64), 4)


def test_oracle_measures_on_a_known_case():
    """tests/eigs_oracle.py on a matrix whose eigenpairs are known: diag(0, 1, 2, 10, 11, ...) -- the largest gap after three values; a
    basis tilted out of the subspace by a known angle leaks by its sine."""
    n = 40
    lam = np.concatenate([[0.0, 1.0, 2.0], 10.0 + np.arange(n - 3)])
    ref = oe.reference(np.diag(lam).astype(np.float32))
    assert ref['k_s'] == 3 and ref['well_separated'] and ref['largest_gap'] == 8.0 and ref['second_gap'] == 1.0
    assert oe.decision(lam) == 3
    V = np.eye(n)
    assert oe.measures(lam, V, ref) == (0.0, 0.0, 0.0)
    t = 1e-3
    V2 = V.copy()
    V2[:, 0] = np.cos(t) * V[:, 0] + np.sin(t) * V[:, 7]
    e_val, leak, orth = oe.measures(lam + oe.EPS * lam[-1], V2, ref)
    assert abs(e_val - 1.0) < 1e-6 and abs(leak - np.sin(t)) < 1e-12 and orth < 1e-12
    assert oe.bounds((0.3, 1e-7, 2e-6)) == (8.0, 1e-5, 1.6e-5)
