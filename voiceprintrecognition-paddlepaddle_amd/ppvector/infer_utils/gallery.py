"""The voice-print library of PPVectorPredictor as a matrix that stays on the GPU.

This file has no counterpart in the reference: there the library is ``audio_feature_mean`` (ppvector/predict.py:154-164, one mean
embedding per user, recomputed on the host) and the search is ``__retrieval`` (:173-187, sklearn ``cosine_similarity`` over the whole
library + ``argmax``).  Here one unit centroid per user lives in a device matrix (csrc/gallery.hip: vp_gallery_centroids_f32) and a
search is one fused score-and-select pass over it (vp_gallery_topk_f32): nothing of the library's size is computed, uploaded or
written per query.  docs/gallery.md states the contract and the tie rule (equal scores: the user enrolled first).

``set_score_norm(ScoreNorm)`` switches the search to adaptive score normalisation (docs/score_norm.md): the gallery then keeps every
row's (mean, r) beside the centroids and ``search`` selects on z inside the score kernel (vp_gallery_topk_norm_f32).  Opt-in: without
it every path is the one that ran before.
"""
import numpy as np
import torch

from ppvector import _native as N


class SpeakerGallery:
    """One unit centroid row per user; row order = order of first enrolment (``remove`` moves the last row into the hole)."""

    def __init__(self, dim, device=None):
        self.dim = int(dim)
        self.device = torch.device(device) if device is not None else N.default_device()
        if self.device.type != 'cuda':
            raise N.VpmiError('SpeakerGallery needs a GPU: the engine has no CPU fallback')
        self._cen = torch.zeros((64, self.dim), dtype=torch.float32, device=self.device)    # rows past len(self) are never read
        self._names = []
        self._row = {}
        self._ws = N.Workspace()
        self._norm = None                                           # a ScoreNorm: search on z
        self._mean = self._r = None                                 # then: per row the mean of its top cohort cosines and r, as _cen

    def __len__(self):
        return len(self._names)

    @property
    def names(self):
        """User names by row."""
        return list(self._names)

    @property
    def centroids(self):
        """The (len, dim) unit centroids (a view of the device matrix)."""
        return self._cen[:len(self._names)]

    def _features(self, features):
        f = torch.as_tensor(np.asarray(features) if not isinstance(features, torch.Tensor) else features)
        f = f.to(self.device, torch.float32).reshape(-1, self.dim).contiguous()
        return f

    def _reserve(self, rows, keep):
        """Capacity for ``rows`` rows, by doubling; the first ``keep`` rows survive the move."""
        cap = self._cen.shape[0]
        if rows <= cap:
            return
        while cap < rows:
            cap *= 2
        grown = torch.zeros((cap, self.dim), dtype=torch.float32, device=self.device)
        grown[:keep] = self._cen[:keep]
        self._cen = grown
        if self._norm is not None:
            for name in ('_mean', '_r'):
                vec = torch.zeros(cap, dtype=torch.float32, device=self.device)
                vec[:keep] = getattr(self, name)[:keep]
                setattr(self, name, vec)

    @property
    def score_norm(self):
        return self._norm

    def set_score_norm(self, score_norm):
        """A ``ScoreNorm``: ``search`` returns and orders by z; the rows' statistics are computed now and kept in step with the
        centroids.  ``None``: the cosine search, the statistics are dropped."""
        from ppvector.metric.score_norm import ScoreNorm
        if score_norm is not None and not isinstance(score_norm, ScoreNorm):
            raise ValueError(f'set_score_norm: a ScoreNorm or None, got {type(score_norm).__name__}')
        if score_norm is not None and score_norm.cohort.shape[1] != self.dim:
            raise ValueError(f'set_score_norm: the cohort has D = {score_norm.cohort.shape[1]}, the gallery D = {self.dim}')
        self._norm = score_norm
        self._mean = self._r = None
        if score_norm is not None:
            self._mean = torch.zeros(self._cen.shape[0], dtype=torch.float32, device=self.device)
            self._r = torch.zeros(self._cen.shape[0], dtype=torch.float32, device=self.device)
            self._norm_rows(0, len(self._names))

    def _norm_rows(self, first, end):
        """(mean, r) of the rows first .. end - 1 from the stored unit centroids, handed to ``cohort_stats`` as raw rows.  That kernel's
        sums do not depend on how many rows it is given: one row or all give a row the same bits."""
        if self._norm is None or end <= first:
            return
        mean, r = self._norm.mean_r(self._cen[first:end])
        self._mean[first:end] = mean
        self._r[first:end] = r

    def _write(self, emb, offsets, dst_rows):
        off = torch.as_tensor(np.asarray(offsets, dtype=np.int32)).to(self.device)
        dst = torch.as_tensor(np.asarray(dst_rows, dtype=np.int32)).to(self.device)
        ctx = N.ctx(self.device)
        with torch.cuda.device(self.device):
            N.check(N.lib().vp_gallery_centroids_f32(ctx, emb.data_ptr(), off.data_ptr(), dst.data_ptr(), len(dst_rows), self.dim,
                                                     self._cen.data_ptr(), N.stream_ptr()), ctx)

    def set_user(self, name, features):
        """``features`` (m, dim): ALL of this user's utterance embeddings; recomputes the user's one row (a new user is appended)."""
        emb = self._features(features)
        if emb.shape[0] == 0:
            raise ValueError(f'set_user({name!r}): no embeddings')
        row = self._row.get(name)
        if row is None:
            row = len(self._names)
            self._reserve(row + 1, keep=row)
            self._names.append(name)
            self._row[name] = row
        self._write(emb, [0, emb.shape[0]], [row])
        self._norm_rows(row, row + 1)

    def remove(self, name):
        """Drops the user; the last row moves into its place.  False when the name is unknown."""
        row = self._row.pop(name, None)
        if row is None:
            return False
        last = len(self._names) - 1
        if row != last:
            self._cen[row].copy_(self._cen[last])
            if self._norm is not None:
                self._mean[row].copy_(self._mean[last])
                self._r[row].copy_(self._r[last])
            self._names[row] = self._names[last]
            self._row[self._names[row]] = row
        self._names.pop()
        return True

    def rebuild(self, names, features):
        """From scratch: ``names[i]`` is the user of row i of ``features`` (M, dim); users take rows in order of first appearance."""
        emb = self._features(features)
        names = list(names)
        if emb.shape[0] != len(names):
            raise ValueError(f'rebuild: {len(names)} names for {emb.shape[0]} embeddings')
        self._names, self._row = [], {}
        for n in names:
            if n not in self._row:
                self._row[n] = len(self._names)
                self._names.append(n)
        if not names:
            return
        rows = np.asarray([self._row[n] for n in names], dtype=np.int64)
        order = np.argsort(rows, kind='stable')                      # a user's utterances stay in their own order
        counts = np.bincount(rows, minlength=len(self._names))
        offsets = np.concatenate(([0], np.cumsum(counts)))
        self._reserve(len(self._names), keep=0)
        emb = emb[torch.as_tensor(order).to(self.device)].contiguous()
        self._write(emb, offsets, np.arange(len(self._names)))
        self._norm_rows(0, len(self._names))

    def search(self, features, top_k=1):
        """(Q, dim) raw embeddings -> (idx int32, score f32), device tensors (Q, top_k): the best users of each query by cosine, score
        descending then row ascending; ``idx`` indexes ``names``; past ``len(self)`` matches the tail is -1 / -inf.  With a score norm
        set the score is z (the row as enrolment, the query as trial) and the selection is on z."""
        q = self._features(features)
        Q, U, k = q.shape[0], len(self._names), int(top_k)
        idx = torch.empty((Q, max(k, 0)), dtype=torch.int32, device=self.device)
        score = torch.empty((Q, max(k, 0)), dtype=torch.float32, device=self.device)
        if Q == 0 or (U == 0 and 1 <= k <= 32):                     # an empty library: every entry is the "no match" tail
            return idx.fill_(-1), score.fill_(float('-inf'))
        lib, ctx = N.lib(), N.ctx(self.device)
        with torch.cuda.device(self.device):
            ws = self._ws.get(lib.vp_gallery_topk_workspace_bytes(Q, U, self.dim, k), self.device)
            if self._norm is not None:
                qmean, qr = self._norm.mean_r_queries(q)
                N.check(lib.vp_gallery_topk_norm_f32(ctx, q.data_ptr(), Q, self._cen.data_ptr(), U, self.dim, k, qmean.data_ptr(),
                                                     qr.data_ptr(), self._mean.data_ptr(), self._r.data_ptr(), idx.data_ptr(),
                                                     score.data_ptr(), ws.data_ptr(), ws.numel(), N.stream_ptr()), ctx)
                return idx, score
            N.check(lib.vp_gallery_topk_f32(ctx, q.data_ptr(), Q, self._cen.data_ptr(), U, self.dim, k, idx.data_ptr(), score.data_ptr(),
                                            ws.data_ptr(), ws.numel(), N.stream_ptr()), ctx)
        return idx, score
