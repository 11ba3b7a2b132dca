"""Speaker diarization on the MI355X engine -- ppvector/infer_utils/speaker_diarization.py of the reference.

What runs in HIP (csrc/diarize.hip): the batch of fixed-length windows (``chunk_batch``: _chunk's padding :75-77 and the per-chunk
decibel normalisation of predict.py:213-215), the pruned cosine affinity (``affinity_prune``: get_sim_mat + p_pruning, :253-273) and the
Laplacian (``laplacian``: :246, :276-282).  There is no CPU path: these raise ``VpmiError`` without a GPU.
Host arithmetic kept in Python as in the reference: the chunk table, label bookkeeping, merging and smoothing, the eigen-gap rule;
``sklearn.cluster.k_means`` runs on the host exactly as it does there.

The Laplacian's eigenpairs have two solvers (``ppvector.set_spectral_solver``).  'host', the default, is the reference's
``scipy.linalg.eigh`` of the whole matrix.  'gpu' is ``smallest_eigenpairs``: Chebyshev-filtered subspace iteration in HIP
(csrc/diarize_eigs.hip, docs/diarize_eigs.md) for the max_num_spks + 1 eigenvalues the gap rule reads (or the oracle_num vectors asked
for) on the Laplacian where it was built, without copying it to the host; it is taken for 64 <= N <= 16384 windows and at most 24 wanted
eigenvalues, and hands over to the host path (with a RuntimeWarning) when it does not converge within its caps.

The reference's voice-activity detection is NOT built: it is yeaudio's model-based ``AudioSegment.vad`` (:37).  ``segments`` takes the
speech regions from the caller instead -- who may get them from this project's own energy detector (``ppvector/infer_utils/vad.py``).
"""
import math
import warnings
from types import SimpleNamespace

import numpy as np
import torch

from ppvector import _native as N


# ------------------------------------------------------------------------------------------------ engine entry points
def chunk_batch(wave, table, chunk_len, normalize=True, target_db=-20.0):
    """wave (n,) float32 GPU tensor, table (N, 2) int32 (first sample, one past the last) -> (N, chunk_len) float32 GPU tensor:
    every window zero-padded on the right and, if ``normalize``, decibel-normalised over the padded row (vp_chunk_batch_f32)."""
    if not isinstance(wave, torch.Tensor) or not wave.is_cuda:
        raise N.VpmiError('chunk_batch needs a GPU tensor: the engine has no CPU fallback')
    wave = wave.contiguous().float()
    table = torch.as_tensor(np.ascontiguousarray(table, dtype=np.int32) if not isinstance(table, torch.Tensor) else table)
    table = table.to(device=wave.device, dtype=torch.int32).contiguous()
    if wave.dim() != 1 or table.dim() != 2 or table.shape[1] != 2:
        raise ValueError('chunk_batch: wave must be (n,), table (N, 2)')
    lib, ctx = N.lib(), N.ctx(wave.device)
    out = torch.empty((table.shape[0], int(chunk_len)), dtype=torch.float32, device=wave.device)
    N.check(lib.vp_chunk_batch_f32(ctx, N.ptr(wave), wave.shape[0], N.ptr(table), table.shape[0], int(chunk_len), int(bool(normalize)),
                                   float(target_db), N.ptr(out), N.stream_ptr()), ctx)
    return out


def affinity_prune(embeddings, n_elems):
    """(N, D) float32 GPU tensor -> (N, N) cosine affinity with the ``n_elems`` smallest entries of every row zeroed
    (vp_affinity_prune_f32; equal values at the threshold: the lower columns are zeroed first)."""
    if not isinstance(embeddings, torch.Tensor) or not embeddings.is_cuda:
        raise N.VpmiError('affinity_prune needs a GPU tensor: the engine has no CPU fallback')
    x = embeddings.contiguous().float()
    if x.dim() != 2:
        raise ValueError('affinity_prune: embeddings must be (N, D)')
    n, d = x.shape
    lib, ctx = N.lib(), N.ctx(x.device)
    out = torch.empty((n, n), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(lib.vp_affinity_prune_workspace_bytes(n, d), 256), dtype=torch.uint8, device=x.device)
    N.check(lib.vp_affinity_prune_f32(ctx, N.ptr(x), n, d, int(n_elems), N.ptr(out), N.ptr(ws), ws.numel(), N.stream_ptr()), ctx)
    return out


def laplacian(pruned):
    """(N, N) float32 GPU tensor P -> L = diag(sum_j |M_ij|) - M, M = (P + P^T) / 2 with a zero diagonal (vp_laplacian_f32)."""
    if not isinstance(pruned, torch.Tensor) or not pruned.is_cuda:
        raise N.VpmiError('laplacian needs a GPU tensor: the engine has no CPU fallback')
    p = pruned.contiguous().float()
    if p.dim() != 2 or p.shape[0] != p.shape[1]:
        raise ValueError('laplacian: P must be square')
    lib, ctx = N.lib(), N.ctx(p.device)
    out = torch.empty_like(p)
    N.check(lib.vp_laplacian_f32(ctx, N.ptr(p), p.shape[0], N.ptr(out), N.stream_ptr()), ctx)
    return out


# Defaults of smallest_eigenpairs (docs/diarize_eigs.md has the measurements behind them).  A round is one filter plus one Rayleigh-Ritz
# step; the filter's degree is chosen per round so that it amplifies the eigenvalue 0 over the block's largest Ritz value by at most
# EIGS_MAX_AMPLIFICATION: beyond that the filtered block is too ill-conditioned for one Cholesky orthonormalisation of f32 vectors.
EIGS_TOL = 1e-6                    # stop when every wanted |L v - lambda v| <= EIGS_TOL * sigma
EIGS_MAX_ROUNDS = 40
EIGS_MAX_DEGREE = 40
EIGS_MAX_AMPLIFICATION = 1e4
EIGS_MIN_N, EIGS_MAX_N, EIGS_MAX_K = 64, 16384, 24
_eigs_ws = N.Workspace()


def _filter_degree(sigma, upper):
    """Degree m with T_m((sigma + a) / (sigma - a)) <= EIGS_MAX_AMPLIFICATION, a = upper: T_m(t) = cosh(m acosh t) outside [-1, 1]."""
    if not (sigma > upper > 0.0):
        return 2
    t0 = math.acosh((sigma + upper) / (sigma - upper))
    if t0 <= 0.0:
        return EIGS_MAX_DEGREE
    return int(max(2, min(EIGS_MAX_DEGREE, math.floor(math.acosh(EIGS_MAX_AMPLIFICATION) / t0))))


def smallest_eigenpairs(L, k, tol=None, max_rounds=None):
    """The k smallest eigenpairs of the symmetric positive semi-definite (N, N) float32 GPU tensor L (``laplacian``'s output):
    -> (eigenvalues (k,) float64 ndarray ascending, eigenvectors (N, k) float32 ndarray, orthonormal, info).
    vp_eigs_init_f32 once, then rounds of vp_eigs_iterate_f32; after each the k residuals |L v - lambda v|_2 (with the eigenvalues and the
    two interval ends, one small copy) are read back and the loop stops once all are <= tol * sigma, sigma = 2 max L_ii, or after
    max_rounds rounds.  ``info``: rounds, products (block products L X spent), residuals (k,), sigma, converged."""
    if not isinstance(L, torch.Tensor) or not L.is_cuda:
        raise N.VpmiError('smallest_eigenpairs needs a GPU tensor: the engine has no CPU fallback')
    if L.dim() != 2 or L.shape[0] != L.shape[1]:
        raise ValueError('smallest_eigenpairs: L must be square')
    L = L.contiguous().float()
    n, k = L.shape[0], int(k)
    tol = EIGS_TOL if tol is None else float(tol)
    max_rounds = EIGS_MAX_ROUNDS if max_rounds is None else int(max_rounds)
    lib, ctx = N.lib(), N.ctx(L.device)
    nbytes = lib.vp_eigs_workspace_bytes(n, k)
    ws = _eigs_ws.get(nbytes, L.device)
    out = torch.empty(2 * k + 2, dtype=torch.float32, device=L.device)          # eigenvalues | residuals | sigma, largest Ritz value
    vecs = torch.empty((n, max(k, 1)), dtype=torch.float32, device=L.device)
    esz = out.element_size()
    args = (N.ptr(ws), nbytes, N.ptr(out), N.ptr(vecs), N.ptr(out) + k * esz, N.ptr(out) + 2 * k * esz, N.stream_ptr())
    N.check(lib.vp_eigs_init_f32(ctx, N.ptr(L), n, k, *args), ctx)
    rounds, products = 0, 1
    while True:
        host = out.cpu().numpy().astype(np.float64)
        sigma, upper = host[2 * k], host[2 * k + 1]
        converged = bool(np.all(host[k:2 * k] <= tol * sigma))                  # a NaN residual is not converged
        if converged or rounds >= max_rounds:
            break
        steps = _filter_degree(sigma, upper)
        N.check(lib.vp_eigs_iterate_f32(ctx, N.ptr(L), n, k, steps, *args), ctx)
        rounds += 1
        products += steps + 1
    info = SimpleNamespace(rounds=rounds, products=products, residuals=host[k:2 * k].copy(), sigma=float(sigma), converged=converged)
    return host[:k].copy(), vecs.cpu().numpy(), info


# ------------------------------------------------------------------------------------------------ the reference's classes
class SpeakerDiarization(object):

    def __init__(self, seg_duration=1.5, seg_shift=0.75, sample_rate=16000, merge_threshold=0.78):
        """说话人日志工具 (same arguments as the reference)."""
        self.seg_duration = seg_duration
        self.seg_shift = seg_shift
        self.sample_rate = sample_rate
        self.merge_threshold = merge_threshold
        self.spectral_cluster = SpectralCluster()

    @property
    def chunk_len(self):
        return int(self.seg_duration * self.sample_rate)

    def segments(self, audio_segment, vad_segments):
        """The chunk table of a recording: one row ``[start_s, end_s, first_sample, end_sample]`` per window, in the order of
        the reference's ``segments_audio`` (:26-44).  ``vad_segments``: the speech regions as (start_s, end_s) pairs -- what
        ``AudioSegment.vad(return_seconds=True)`` would have given; the windows' samples are not cut here (vp_chunk_batch_f32 does)."""
        samples = audio_segment.samples
        self.sample_rate = audio_segment.sample_rate
        regions = []
        for t in vad_segments:
            start, end = (t['start'], t['end']) if isinstance(t, dict) else (t[0], t[1])
            st, ed = round(float(start), 3), round(float(end), 3)
            regions.append([st, ed, samples[int(st * self.sample_rate):int(ed * self.sample_rate)]])
        self._check_audio_list(regions)
        return self._chunk(regions)

    def _check_audio_list(self, audio):
        total = 0
        for i, (st, ed, data) in enumerate(audio):
            assert ed >= st, '分割的时间戳错误'
            assert isinstance(data, np.ndarray), '数据的类型不正确'
            assert int(ed * self.sample_rate) - int(st * self.sample_rate) == data.shape[0], '时间长度和数据长度不匹配'
            if i > 0:
                assert st >= audio[i - 1][1], 'modelscope error: Wrong time stamps.'
            total += ed - st
        assert total > 5, f'音频时间过段，应当大于5秒，当前长度是{total}秒'

    def _chunk(self, vad_segments):
        """Windows of seg_duration every seg_shift inside each region; the last one is pulled back to end at the region's end, and
        the walk stops once a window would not reach past the previous one (:60-87).  A region shorter than a window gives one
        short window (padded later)."""
        sr = self.sample_rate
        chunk_len, chunk_shift = int(self.seg_duration * sr), int(self.seg_shift * sr)
        table = []
        for st, _, data in vad_segments:
            n = data.shape[0] if isinstance(data, np.ndarray) else int(data)
            first = int(st * sr)
            reached = 0
            for pos in range(0, n, chunk_shift):
                stop = min(pos + chunk_len, n)
                if stop <= reached:
                    break
                reached = stop
                begin = max(0, stop - chunk_len)
                table.append([begin / sr + st, stop / sr + st, first + begin, first + stop])
        return table

    def clustering(self, embeddings, speaker_num=None):
        """聚类音频特征向量 -> (labels (n,), speaker centres (n_speakers_before_merging, D)) as the reference (:89-109)."""
        embeddings = np.asarray(embeddings)
        labels = self.spectral_cluster(embeddings, oracle_num=speaker_num)
        labels = self._correct_labels(labels)
        centers = np.stack([embeddings[labels == i].mean(0) for i in range(int(labels.max()) + 1)], axis=0)
        labels = self._merge_by_cos(labels, list(centers), self.merge_threshold)
        return labels, centers

    @staticmethod
    def _merge_by_cos(labels, spk_center_emb, cos_thr):
        """Merge the closest pair of speakers while its cosine reaches cos_thr.  As in the reference the centres are NOT recomputed
        or re-indexed after a merge: row i of spk_center_emb stands for label i throughout (:112-136)."""
        assert 0 < cos_thr <= 1
        while True:
            n_spk = int(labels.max()) + 1
            if n_spk == 1:
                break
            c = np.stack([spk_center_emb[i] for i in range(n_spk)], axis=0)
            c = c / np.linalg.norm(c, axis=1, keepdims=True)
            aff = np.triu(c @ c.T, 1)
            a, b = np.unravel_index(np.argmax(aff), aff.shape)
            if aff[a, b] < cos_thr:
                break
            for i in range(len(labels)):
                if labels[i] == b:
                    labels[i] = a
                elif labels[i] > b:
                    labels[i] -= 1
        return labels

    def postprocess(self, segments, labels):
        """Chunk labels -> [dict(speaker, start, end)]: runs of one speaker joined, overlaps split at their midpoint, short
        segments given to a neighbour (:138-174)."""
        assert len(segments) == len(labels)
        res = self._merge_seque([[segments[i][0], segments[i][1], labels[i]] for i in range(len(segments))])
        for i in range(1, len(res)):
            if res[i - 1][1] > res[i][0] + 1e-4:
                mid = (res[i][0] + res[i - 1][1]) / 2
                res[i][0] = mid
                res[i - 1][1] = mid
        res = self._smooth(res)
        return [dict(speaker=r[2], start=round(r[0], 3), end=round(r[1], 3)) for r in res]

    @staticmethod
    def _correct_labels(labels):
        """Relabel in order of first appearance."""
        seen = {}
        return np.array([seen.setdefault(int(l), len(seen)) for l in labels])

    @staticmethod
    def _merge_seque(distribute_res):
        res = [distribute_res[0]]
        for cur in distribute_res[1:]:
            if cur[2] != res[-1][2] or cur[0] > res[-1][1]:
                res.append(cur)
            else:
                res[-1][1] = cur[1]
        return res

    def _smooth(self, res, min_duration=1):
        last = len(res) - 1
        for i in range(len(res)):
            res[i][0] = round(res[i][0], 2)
            res[i][1] = round(res[i][1], 2)
            if res[i][1] - res[i][0] < min_duration:
                if i == 0:
                    res[i][2] = res[i + 1][2]
                elif i == last:
                    res[i][2] = res[i - 1][2]
                elif res[i][0] - res[i - 1][1] <= res[i + 1][0] - res[i][1]:
                    res[i][2] = res[i - 1][2]
                else:
                    res[i][2] = res[i + 1][2]
        return self._merge_seque(res)


class SpectralCluster:
    def __init__(self, min_num_spks=1, max_num_spks=15, pval=0.022):
        """Spectral clustering on the unnormalised Laplacian of the pruned cosine affinity (same arguments as the reference)."""
        self.min_num_spks = min_num_spks
        self.max_num_spks = max_num_spks
        self.pval = pval

    def n_elems(self, n):
        """How many of a row's n similarities p_pruning zeroes (:261-265), in double precision as there.  The reference uses the
        number as a slice end, so a negative one (n < 6) counts from the other end."""
        pval = 6. / n if n * self.pval < 6 else self.pval
        k = int((1 - pval) * n)
        return max(n + k, 0) if k < 0 else k

    def laplacian(self, X):
        """Embeddings (n, D), ndarray or tensor -> the Laplacian on the GPU (two engine calls)."""
        x = torch.as_tensor(np.asarray(X, dtype=np.float32)) if not isinstance(X, torch.Tensor) else X
        if not x.is_cuda:
            x = x.to(N.default_device())
        return laplacian(affinity_prune(x, self.n_elems(x.shape[0])))

    def __call__(self, X, oracle_num=None):
        emb, num_of_spk = self.get_spec_embs(self.laplacian(X), oracle_num)
        return self.cluster_embs(emb, num_of_spk)

    def _gpu_eigenpairs(self, L, k_oracle):
        """The wanted eigenpairs from the GPU solver, or None where the host path has to run: the switch is on 'host', L is not on
        the GPU, the size or the count is outside the solver's range, or it did not converge (the only case that warns)."""
        import ppvector
        if ppvector.get_spectral_solver() != 'gpu' or not isinstance(L, torch.Tensor) or not L.is_cuda:
            return None
        wanted = self.max_num_spks + 1 if k_oracle is None else int(k_oracle)
        if not (EIGS_MIN_N <= L.shape[0] <= EIGS_MAX_N and 1 <= wanted <= EIGS_MAX_K):
            return None
        lambdas, eig_vecs, info = smallest_eigenpairs(L, wanted)
        if not info.converged:
            warnings.warn(f'spectral solver: worst residual {np.max(info.residuals) / max(info.sigma, 1e-300):.3g} sigma after '
                          f'{info.rounds} rounds (tolerance {EIGS_TOL:g}); running scipy.linalg.eigh on the host', RuntimeWarning)
            return None
        return lambdas, eig_vecs

    def get_spec_embs(self, L, k_oracle=None):
        pairs = self._gpu_eigenpairs(L, k_oracle)
        if pairs is None:
            import scipy.linalg
            pairs = scipy.linalg.eigh(L.cpu().numpy() if isinstance(L, torch.Tensor) else L)
        lambdas, eig_vecs = pairs
        if k_oracle is not None:
            num_of_spk = k_oracle
        else:
            gaps = self.get_eigen_gaps(lambdas[self.min_num_spks - 1:self.max_num_spks + 1])
            num_of_spk = int(np.argmax(gaps)) + self.min_num_spks
        return eig_vecs[:, :num_of_spk], num_of_spk

    @staticmethod
    def cluster_embs(emb, k):
        from sklearn.cluster import k_means
        _, labels, _ = k_means(emb, k, n_init="auto")
        return labels

    @staticmethod
    def get_eigen_gaps(eig_vals):
        return [float(eig_vals[i + 1]) - float(eig_vals[i]) for i in range(len(eig_vals) - 1)]
