"""Oracle (CPU, NumPy / SciPy float64): the smallest eigenpairs of a diarization Laplacian.  Test helper, not a test module.

Inputs: planted speakers -- balanced labels in a shuffled order, centres ~ N(0, I) in D dimensions, point = centre + noise * N(0, I),
rounded to f32.  Reference: scipy.linalg.eigh of the float64 image of the f32 Laplacian the engine built.  The three measures of the
accuracy contract (docs/diarize_eigs.md), each applied alike to the solver under test and to the yardstick, scipy.linalg.eigh of the same
f32 matrix:
  eigenvalues   max over the first 16 of |lambda - lambda64|, in units of eps * lambda_max (eps = 2^-23);
  leakage       |Q - Q64 (Q64^T Q)|_F for Q = the first k_s vectors, k_s = the place of the largest gap among the first 16 eigenvalues:
                the part of the computed basis outside the true invariant subspace (inside the dense bulk single vectors are ill-defined);
  orthogonality |Q^T Q - I|_F for the same Q.
"""
import numpy as np

EPS = 2.0 ** -23
N_VALUES = 16                                   # what the gap rule reads: max_num_spks + 1

# (N, speakers, noise, seed): the lower bound of the solver, one past a 32-row tile, the sizes of the issue's table (odd, not a multiple
# of 32 or 128, several Gram blocks), two noise levels at one size, and the largest N whose float64 eigh still takes about a second
CASES = [(64, 2, 0.8, 0), (65, 2, 0.8, 0), (96, 3, 0.8, 0), (257, 4, 0.8, 0), (1000, 6, 0.8, 0), (1000, 6, 2.0, 0), (2048, 8, 1.0, 0)]


def planted(n, speakers, noise, seed, d=192):
    rng = np.random.default_rng(seed)
    who = rng.permutation(np.arange(n) % speakers)
    centres = rng.standard_normal((speakers, d))
    x = centres[who] + noise * rng.standard_normal((n, d))
    return x.astype(np.float32), who


def reference(L32):
    """float64 eigenpairs of the f32 matrix, the gaps of its first 16 eigenvalues, the decision and the 2x condition on the input."""
    import scipy.linalg
    lam, V = scipy.linalg.eigh(np.asarray(L32, dtype=np.float64))
    gaps = np.diff(lam[:N_VALUES])
    srt = np.sort(gaps)
    return dict(lam=lam, V=V, k_s=int(np.argmax(gaps)) + 1, largest_gap=float(srt[-1]), second_gap=float(srt[-2]),
                well_separated=bool(srt[-1] >= 2.0 * srt[-2]))


def decision(lam):
    """The eigen-gap rule on the first 16 eigenvalues (min_num_spks = 1)."""
    lam = np.asarray(lam, dtype=np.float64)[:N_VALUES]
    return int(np.argmax(np.diff(lam))) + 1


def measures(lam, V, ref):
    """(eigenvalue error / (eps lambda_max), leakage, orthogonality) of the first 16 values / first k_s vectors against `ref`."""
    lam = np.asarray(lam, dtype=np.float64)
    k_s = ref['k_s']
    Q, Q64 = np.asarray(V, dtype=np.float64)[:, :k_s], ref['V'][:, :k_s]
    e_val = np.abs(lam[:N_VALUES] - ref['lam'][:N_VALUES]).max() / (EPS * ref['lam'][-1])
    leak = np.linalg.norm(Q - Q64 @ (Q64.T @ Q))
    orth = np.linalg.norm(Q.T @ Q - np.eye(k_s))
    return float(e_val), float(leak), float(orth)


def bounds(host):
    """The contract: the larger of 8x the host-f32 figure of the case and a floor (8 eps lambda_max; 1e-5 for the two basis measures)."""
    return max(8.0 * host[0], 8.0), max(8.0 * host[1], 1e-5), max(8.0 * host[2], 1e-5)
