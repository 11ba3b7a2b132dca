"""Adaptive score normalisation (AS-norm) on the engine: per embedding the mean and standard deviation of its top-N cohort cosines
(csrc/cohort_stats.hip), and the normalised score z of a trial against an enrolment (csrc/score_norm.h).  The reference has no score
normalisation: this is an opt-in extension (ppvector.set_score_norm, docs/score_norm.md).  GPU tensors only.
"""


def _device_rows(x, what, device=None):
    import torch
    from ppvector import _native as N
    x = torch.as_tensor(x)
    if not x.is_cuda:
        raise N.VpmiError(f'{what} needs GPU tensors: the engine has no CPU fallback')
    if x.dim() != 2:
        raise ValueError(f'{what}: expected (rows, D), got {tuple(x.shape)}')
    return (x if device is None else x.to(device)).contiguous().float()


def cohort_stats(embeddings, cohort, top_n=300, Q=None, C=None, ws=None):
    """(Q, D) embeddings and a (C, D) cohort, GPU tensors of raw rows -> (mean, std), float32 device tensors of shape (Q,): the mean
    and the population standard deviation of each embedding's min(top_n, C) largest cosines against the cohort.  ``Q`` / ``C`` may be
    smaller than the buffers; ``ws`` is a caller's workspace (uint8, device)."""
    import torch
    from ppvector import _native as N
    x = _device_rows(embeddings, 'cohort_stats')
    cohort = _device_rows(cohort, 'cohort_stats', x.device)
    Q = x.shape[0] if Q is None else int(Q)
    C = cohort.shape[0] if C is None else int(C)
    D, top_n = x.shape[1], int(top_n)
    if cohort.shape[1] != D:
        raise ValueError(f'cohort_stats: embeddings have D = {D}, the cohort has D = {cohort.shape[1]}')
    lib, ctx = N.lib(), N.ctx(x.device)
    need = lib.vp_cohort_stats_workspace_bytes(Q, C, D)
    if need == 0 or top_n < 1:
        raise N.VpmiError(f'cohort_stats: unsupported shape Q={Q} C={C} D={D} top_n={top_n} (Q, C, top_n >= 1, D % 4 == 0, D <= 1024)')
    ws = torch.empty(need, dtype=torch.uint8, device=x.device) if ws is None else ws
    mean = torch.empty(Q, dtype=torch.float32, device=x.device)
    std = torch.empty(Q, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        N.check(lib.vp_cohort_stats_f32(ctx, x.data_ptr(), Q, cohort.data_ptr(), C, D, top_n, mean.data_ptr(), std.data_ptr(),
                                        ws.data_ptr(), ws.numel(), N.stream_ptr()), ctx)
    return mean, std


def unit_rows(x):
    """(rows, D) raw rows, a GPU tensor -> their unit rows as the kernels form them (length in float64, one rounding per element)."""
    import torch
    from ppvector import _native as N
    x = _device_rows(x, 'unit_rows')
    y = torch.empty_like(x)
    ctx = N.ctx(x.device)
    with torch.cuda.device(x.device):
        N.check(N.lib().vp_unit_rows_f32(ctx, x.data_ptr(), x.shape[0], x.shape[1], y.data_ptr(), N.stream_ptr()), ctx)
    return y


def cohort_stats_split(embeddings, cohort_unit, top_n=300, Q=None, C=None, ws=None):
    """``cohort_stats`` for few rows (a search's queries), the cohort split over workgroups (vp_cohort_stats_split_f32).
    ``cohort_unit`` is the cohort ALREADY as unit rows (``unit_rows``, ``ScoreNorm.unit_cohort``).  More rows than
    VP_COHORT_SPLIT_MAX_Q go in chunks: a row's statistics do not depend on its chunk.  ``ws``: a caller's workspace (uint8, device)
    for a call of one chunk."""
    import torch
    from ppvector import _native as N
    x = _device_rows(embeddings, 'cohort_stats_split')
    cu = _device_rows(cohort_unit, 'cohort_stats_split', x.device)
    Q = x.shape[0] if Q is None else int(Q)
    C = cu.shape[0] if C is None else int(C)
    D, top_n = x.shape[1], int(top_n)
    if cu.shape[1] != D:
        raise ValueError(f'cohort_stats_split: embeddings have D = {D}, the cohort has D = {cu.shape[1]}')
    lib, ctx = N.lib(), N.ctx(x.device)
    cap = N.VP_COHORT_SPLIT_MAX_Q
    if Q < 1 or top_n < 1 or lib.vp_cohort_stats_split_workspace_bytes(min(Q, cap), C, D) == 0:
        raise N.VpmiError(f'cohort_stats_split: unsupported shape Q={Q} C={C} D={D} top_n={top_n} '
                          f'(Q, C, top_n >= 1, D % 4 == 0, D <= 1024)')
    mean = torch.empty(Q, dtype=torch.float32, device=x.device)
    std = torch.empty(Q, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        for first in range(0, Q, cap):
            n = min(cap, Q - first)
            need = lib.vp_cohort_stats_split_workspace_bytes(n, C, D)
            if ws is None or ws.numel() < need:
                ws = torch.empty(need, dtype=torch.uint8, device=x.device)
            N.check(lib.vp_cohort_stats_split_f32(ctx, x[first:].data_ptr(), n, cu.data_ptr(), C, D, top_n, mean[first:].data_ptr(),
                                                  std[first:].data_ptr(), ws.data_ptr(), ws.numel(), N.stream_ptr()), ctx)
    return mean, std


def recip_std(std):
    """r = 1 / max(std, 1e-6) in float32, on the device."""
    import torch
    from ppvector import _native as N
    r = torch.empty_like(std)
    ctx = N.ctx(std.device)
    with torch.cuda.device(std.device):
        N.check(N.lib().vp_score_norm_recip_f32(ctx, std.data_ptr(), std.numel(), r.data_ptr(), N.stream_ptr()), ctx)
    return r


class ScoreNorm:
    """A cohort kept on the device and the top_n of its statistics."""

    def __init__(self, cohort, top_n=300):
        import torch
        from ppvector import _native as N
        if int(top_n) < 1:
            raise ValueError(f'ScoreNorm: top_n = {top_n}')
        cohort = torch.as_tensor(cohort)
        if not cohort.is_cuda:                                  # a host array (a loaded .npy) is uploaded once
            cohort = cohort.to(N.default_device())
        self.cohort = _device_rows(cohort, 'ScoreNorm')
        self.top_n = int(top_n)
        self._unit = None
        self._query_ws = None

    def unit_cohort(self):
        """The cohort as unit rows, made once: what the split statistics of a search's queries read."""
        if self._unit is None:
            self._unit = unit_rows(self.cohort)
        return self._unit

    def mean_r_queries(self, emb, n=None):
        """``mean_r`` for the queries of a search: the cohort split over workgroups (csrc/cohort_stats.hip), chunked past the entry
        point's largest Q.  Where the float64 sums are exact these are ``mean_r``'s bits; elsewhere both are within 2e-6 of float64."""
        import torch
        from ppvector import _native as N
        x = _device_rows(emb, 'ScoreNorm.mean_r_queries', self.cohort.device)
        n = x.shape[0] if n is None else int(n)
        need = N.lib().vp_cohort_stats_split_workspace_bytes(min(n, N.VP_COHORT_SPLIT_MAX_Q), self.cohort.shape[0], x.shape[1])
        if self._query_ws is None or self._query_ws.numel() < need:
            self._query_ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        mean, std = cohort_stats_split(x, self.unit_cohort(), self.top_n, Q=n, ws=self._query_ws)
        return mean, recip_std(std)

    def stats(self, emb, n=None):
        """(mean, std) of the first n (default: all) rows of emb."""
        return cohort_stats(emb, self.cohort, self.top_n, Q=n)

    def mean_r(self, emb, n=None):
        """(mean, 1 / max(std, 1e-6)): what the normalised kernels read."""
        mean, std = self.stats(emb, n)
        return mean, recip_std(std)

    def normalise(self, scores, trial_emb, enroll_emb):
        """(Nt, Ne) cosines of trial_emb against enroll_emb (a contiguous float32 GPU tensor) -> z, in place; returns it."""
        import torch
        from ppvector import _native as N
        if not scores.is_cuda or scores.dtype != torch.float32 or not scores.is_contiguous():
            raise N.VpmiError('ScoreNorm.normalise needs a contiguous float32 GPU tensor: the engine has no CPU fallback')
        tm, tr = self.mean_r(trial_emb)
        em, er = self.mean_r(enroll_emb)
        if scores.shape != (tm.shape[0], em.shape[0]):
            raise ValueError(f'ScoreNorm.normalise: scores {tuple(scores.shape)} for {tm.shape[0]} trials and {em.shape[0]} enrolments')
        ctx = N.ctx(scores.device)
        with torch.cuda.device(scores.device):
            N.check(N.lib().vp_score_norm_apply_f32(ctx, scores.data_ptr(), scores.shape[0], scores.shape[1], tm.data_ptr(),
                                                    tr.data_ptr(), em.data_ptr(), er.data_ptr(), N.stream_ptr()), ctx)
        return scores
