"""EER / minDCF on the host (NumPy), semantics of ppvector/metric/metrics.py:4-37, plus the GPU
trial scorer that replaces the per-trial sklearn loop of trainer.py:416-423: by default one cosine GEMM and the reference's
arithmetic over all pairs; with ppvector.set_trial_scorer('fused') the same numbers from the sorted target scores and the counts of
non-target scores between them, without the (Nt, Ne) matrix (csrc/trial_ranks.hip, docs/trial_ranks.md).  Both scorers take an
optional ``score_norm`` (ppvector.metric.score_norm.ScoreNorm, docs/score_norm.md; the reference has none): every cosine is then
replaced by its adaptively normalised score z before anything is ranked.
"""
import numpy as np


def compute_fnr_fpr(scores, labels, weights=None):
    """False-negative / false-positive rates at every score threshold (ascending)."""
    order = np.argsort(scores)
    thresholds = scores[order]
    labels = labels[order]
    weights = np.ones(labels.shape, dtype='f8') if weights is None else weights[order]
    tgt = weights * (labels == 1).astype('f8')
    imp = weights * (labels == 0).astype('f8')
    fnr = np.cumsum(tgt) / np.sum(tgt)
    fpr = 1 - np.cumsum(imp) / np.sum(imp)
    return fnr, fpr, thresholds


def compute_eer(fnr, fpr, scores=None):
    """Equal error rate by linear interpolation between the two points around fnr == fpr."""
    gap = fnr - fpr
    hi = np.flatnonzero(gap >= 0)[0]
    lo = np.flatnonzero(gap < 0)[-1]
    a = (fnr[hi] - fpr[hi]) / (fpr[lo] - fpr[hi] - (fnr[lo] - fnr[hi]))
    rate = fnr[hi] + a * (fnr[lo] - fnr[hi])
    if scores is not None:
        return rate, np.sort(scores)[hi]
    return rate


def compute_dcf(fnr, fpr, p_target=0.01, c_miss=1, c_fa=1):
    """Minimum normalised detection cost."""
    c_det = min(c_miss * fnr * p_target + c_fa * fpr * (1 - p_target))
    c_def = min(c_miss * p_target, c_fa * (1 - p_target))
    return c_det / c_def


def cosine_score_matrix(trials, enroll):
    """(Nt, D), (Ne, D) GPU tensors -> (Nt, Ne) cosine scores on the engine (csrc/head.hip)."""
    import torch
    from ppvector import _native as N
    if not trials.is_cuda:
        raise N.VpmiError('cosine_score_matrix needs GPU tensors: the engine has no CPU fallback')
    a = trials.contiguous().float()
    b = enroll.to(a.device).contiguous().float()
    lib, ctx = N.lib(), N.ctx(a.device)
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    ws = torch.empty(max(lib.vp_cosine_scores_workspace_bytes(a.shape[0], b.shape[0], a.shape[1]), 256),
                     dtype=torch.uint8, device=a.device)
    N.check(lib.vp_cosine_scores_f32(ctx, a.data_ptr(), b.data_ptr(), a.shape[0], b.shape[0], a.shape[1],
                                     out.data_ptr(), ws.data_ptr(), ws.numel(), N.stream_ptr()), ctx)
    return out


def evaluate_trials(enroll_features, enroll_labels, trials_features, trials_labels, score_norm=None):
    """The scoring half of PPVectorTrainer.evaluate (ppvector/trainer.py:412-431): every trial embedding against every enrolled
    one (one cosine GEMM on the GPU instead of a Python loop of sklearn calls), target / non-target labels in the same
    trial-major order, then the reference's fnr/fpr -> EER / minDCF arithmetic on the host.  Returns (eer, min_dcf, threshold).
    ``score_norm``: a ScoreNorm, or None for ppvector.get_score_norm() (None by default: raw cosines, as the reference)."""
    import numpy as np
    import torch
    import ppvector
    if score_norm is None:
        score_norm = ppvector.get_score_norm()
    if ppvector.get_trial_scorer() == 'fused':
        return evaluate_trials_fused(enroll_features, enroll_labels, trials_features, trials_labels, score_norm=score_norm)
    scores = cosine_score_matrix(torch.as_tensor(trials_features), torch.as_tensor(enroll_features))
    if score_norm is not None:
        scores = score_norm.normalise(scores, torch.as_tensor(trials_features), torch.as_tensor(enroll_features))
    scores = scores.cpu().numpy()
    el = np.asarray(enroll_labels).astype(np.int32)
    tl = np.asarray(trials_labels).astype(np.int32)
    all_score = scores.astype(np.float32).reshape(-1)
    all_labels = (el[None, :] == tl[:, None]).astype(np.int32).reshape(-1)
    fnr, fpr, thresholds = compute_fnr_fpr(all_score, all_labels)
    eer, threshold = compute_eer(fnr, fpr, all_score)
    min_dcf = compute_dcf(fnr, fpr)
    return float(eer), float(min_dcf), float(threshold)


# ------------------------------------------------------------------------------------------------ the same numbers without the matrix
# EER, minDCF and the EER threshold need the sorted TARGET scores t[0] <= ... <= t[NT-1] and, per gap, the NUMBER of non-target
# scores in it: hist[b], b = 0 .. NT, counts the non-targets s with b = #{j : t[j] < s} (docs/trial_ranks.md).  With
# C[j] = hist[0] + ... + hist[j], target j stands at sorted position j + C[j] with fnr = (j + 1) / NT, fpr = 1 - C[j] / NN, and the
# k-th non-target of bin j (k = 1 .. hist[j]) has fnr = j / NT, fpr = 1 - (C[j-1] + k) / NN: the float64 values that
# np.cumsum(...) / np.sum(...) of compute_fnr_fpr holds at those positions.  Tie rule: a non-target equal to a target sorts before it.
def _label_plan(trial_labels, enroll_labels):
    """Labels of any integer kind -> (trial ids, enrol ids) int32 in one dense numbering, per trial the first place of its targets
    (int64), per enrol row its rank among the rows of its label (int32), and NT.  O(Nt + Ne) beside one sort of the labels."""
    tl = np.asarray(trial_labels).reshape(-1)
    el = np.asarray(enroll_labels).reshape(-1)
    _, ids = np.unique(np.concatenate([el, tl]), return_inverse=True)
    ids = ids.reshape(-1)
    e_id, t_id = ids[:len(el)], ids[len(el):]
    per_label = np.bincount(e_id, minlength=int(ids.max()) + 1 if len(ids) else 0)
    order = np.argsort(e_id, kind='stable')
    first = np.concatenate(([0], np.cumsum(per_label)[:-1]))
    rank = np.empty(len(el), np.int64)
    rank[order] = np.arange(len(el)) - first[e_id[order]]
    per_trial = per_label[t_id].astype(np.int64)
    offsets = np.concatenate(([0], np.cumsum(per_trial)[:-1])).astype(np.int64) if len(tl) else np.zeros(0, np.int64)
    return t_id.astype(np.int32), e_id.astype(np.int32), offsets, rank.astype(np.int32), int(per_trial.sum())


def _host_labels(labels):
    return labels.detach().cpu().numpy() if hasattr(labels, 'detach') else np.asarray(labels)


class TrialRanks:
    """The device side of the fused scorer (csrc/trial_ranks.hip): ``targets`` (NT,) float32 ascending and ``hist`` (NT + 1,) int64
    as device tensors, and the k-th smallest non-target of a bin on request.  ``Nt`` / ``Ne`` may be smaller than the buffers; ``ws``
    is a caller's workspace (uint8, device).  ``score_norm`` (a ScoreNorm): every score, in all three passes, is z instead of the
    cosine; the statistics are kept as ``stats`` = (trial mean, trial r, enrol mean, enrol r), device tensors."""
    DIGITS = ((21, 2048), (10, 2048), (0, 1024))         # shift and size of the three digits of vp_trial_ranks_select_f32

    def __init__(self, trials, trial_labels, enroll, enroll_labels, Nt=None, Ne=None, ws=None, score_norm=None):
        import torch
        from ppvector import _native as N
        trials, enroll = torch.as_tensor(trials), torch.as_tensor(enroll)
        if not trials.is_cuda or not enroll.is_cuda:
            raise N.VpmiError('trial_ranks needs GPU tensors: the engine has no CPU fallback')
        dev = trials.device
        self._t = trials.contiguous().float()
        self._e = enroll.to(dev).contiguous().float()
        self.Nt = self._t.shape[0] if Nt is None else int(Nt)
        self.Ne = self._e.shape[0] if Ne is None else int(Ne)
        self.D = self._t.shape[1]
        tl, el, off, rank, self.NT = _label_plan(_host_labels(trial_labels)[:self.Nt], _host_labels(enroll_labels)[:self.Ne])
        self._lib, self._ctx, self._dev = N.lib(), N.ctx(dev), dev
        need = self._lib.vp_trial_ranks_workspace_bytes(self.Nt, self.Ne, self.D, self.NT)
        if need == 0:
            raise N.VpmiError(f'trial_ranks: unsupported shape Nt={self.Nt} Ne={self.Ne} D={self.D} NT={self.NT} '
                              '(Nt, Ne >= 1, D % 4 == 0, D <= 1024, 1 <= NT <= 2^24)')
        self._ws = torch.empty(need, dtype=torch.uint8, device=dev) if ws is None else ws
        self._tl, self._el = torch.from_numpy(tl).to(dev), torch.from_numpy(el).to(dev)
        off, rank = torch.from_numpy(off).to(dev), torch.from_numpy(rank).to(dev)
        raw = torch.empty(self.NT, dtype=torch.float32, device=dev)
        lib, ctx = self._lib, self._ctx
        self.stats = None if score_norm is None else score_norm.mean_r(self._t, self.Nt) + score_norm.mean_r(self._e, self.Ne)
        stats = () if self.stats is None else tuple(t.data_ptr() for t in self.stats)
        targets_pass = lib.vp_trial_ranks_targets_f32 if self.stats is None else lib.vp_trial_ranks_targets_norm_f32
        counts_pass = lib.vp_trial_ranks_counts_f32 if self.stats is None else lib.vp_trial_ranks_counts_norm_f32
        with torch.cuda.device(dev):
            N.check(targets_pass(ctx, self._t.data_ptr(), self._tl.data_ptr(), off.data_ptr(), self.Nt,
                                 self._e.data_ptr(), self._el.data_ptr(), rank.data_ptr(), self.Ne, self.D, self.NT,
                                 raw.data_ptr(), *stats, self._ws.data_ptr(), self._ws.numel(), N.stream_ptr()), ctx)
            self.targets = torch.sort(raw).values
            self.hist = torch.empty(self.NT + 1, dtype=torch.int64, device=dev)
            N.check(counts_pass(ctx, self._tl.data_ptr(), self.Nt, self._el.data_ptr(), self.Ne, self.D,
                                self.targets.data_ptr(), self.NT, self.hist.data_ptr(), *stats, self._ws.data_ptr(),
                                self._ws.numel(), N.stream_ptr()), ctx)

    def kth_nontarget(self, b, k):
        """The k-th smallest (k = 1 .. hist[b]) of the non-target scores of bin b, by three digit-counting passes."""
        import torch
        from ppvector import _native as N
        b, k = int(b), int(k)
        if not (0 <= b <= self.NT and 1 <= k <= int(self.hist[b])):
            raise ValueError(f'kth_nontarget: bin {b} has no {k}-th score')
        lo = float(self.targets[b - 1]) if b > 0 else float('-inf')
        hi = float(self.targets[b]) if b < self.NT else float('inf')
        digits = torch.empty(2048, dtype=torch.int64, device=self._dev)
        key = 0
        stats = () if self.stats is None else tuple(t.data_ptr() for t in self.stats)
        select_pass = self._lib.vp_trial_ranks_select_f32 if self.stats is None else self._lib.vp_trial_ranks_select_norm_f32
        for level, (shift, size) in enumerate(self.DIGITS):
            with torch.cuda.device(self._dev):
                N.check(select_pass(self._ctx, self._tl.data_ptr(), self.Nt, self._el.data_ptr(), self.Ne,
                                    self.D, self.NT, lo, hi, level, key, digits.data_ptr(), *stats,
                                    self._ws.data_ptr(), self._ws.numel(), N.stream_ptr()), self._ctx)
            upto = np.cumsum(digits[:size].cpu().numpy())
            d = int(np.searchsorted(upto, k, side='left'))
            if d >= size:
                raise RuntimeError(f'kth_nontarget: {int(upto[-1])} scores at level {level}, {k} wanted')
            k -= int(upto[d - 1]) if d else 0
            key |= d << shift
        bits = key ^ 0x80000000 if key >> 31 else key ^ 0xffffffff
        return float(np.asarray([bits], np.uint32).view(np.float32)[0])

    def calib_sums(self, a, b):
        """The twelve float64 sums of the calibration objective at llr + tau = a s + b over all pairs (csrc/calibrate.hip,
        docs/calibration.md) -> ndarray (2, 6) float64, targets first: sum of softplus(u), sigma(u), sigma(u) s, w, w s, w s^2.
        One pass over the unit rows this object's workspace holds and one 96-byte read-back; s is z when a score norm was given."""
        import ctypes
        import torch
        from ppvector import _native as N
        if getattr(self, '_calib_partials', None) is None:
            need = self._lib.vp_trial_calib_partials_bytes(self.Nt, self.Ne, self.D)
            self._calib_partials = torch.empty(need, dtype=torch.uint8, device=self._dev)
            self._calib_out = torch.empty(12, dtype=torch.float64, device=self._dev)
        ab = (ctypes.c_double * 2)(float(a), float(b))
        stats = () if self.stats is None else tuple(t.data_ptr() for t in self.stats)
        sums_pass = self._lib.vp_trial_calib_sums_f32 if self.stats is None else self._lib.vp_trial_calib_sums_norm_f32
        with torch.cuda.device(self._dev):
            N.check(sums_pass(self._ctx, self._tl.data_ptr(), self.Nt, self._el.data_ptr(), self.Ne, self.D,
                              ctypes.addressof(ab), self._calib_out.data_ptr(), self._calib_partials.data_ptr(),
                              self._calib_partials.numel(), *stats, self._ws.data_ptr(), self._ws.numel(), N.stream_ptr()), self._ctx)
        return self._calib_out.cpu().numpy().reshape(2, 6)


def trial_ranks(trials, trial_labels, enroll, enroll_labels):
    """(Nt, D), (Ne, D) GPU tensors and their labels -> (targets float32 (NT,) ascending, hist int64 (NT + 1,)), NumPy arrays: the
    scores of the pairs with equal labels, and per b the number of other pairs whose score s has b = #{j : targets[j] < s}."""
    r = TrialRanks(trials, trial_labels, enroll, enroll_labels)
    return r.targets.cpu().numpy(), r.hist.cpu().numpy()


def eer_dcf_from_ranks(targets, hist, p_target=0.01, c_miss=1, c_fa=1):
    """compute_fnr_fpr / compute_eer / compute_dcf on (targets, hist) instead of the sorted list of all scores: the same float64
    expressions at the same positions, so the same bits.  Returns (eer, min_dcf, where); ``where`` says which score stands at
    compute_eer's position ``hi``: ('t', j) = targets[j], ('n', b, k) = the k-th smallest (from 1) non-target of bin b.  ValueError
    where the reference divides by zero or indexes an empty array: no target, no non-target, hi == 0."""
    hist = np.asarray(hist, dtype=np.int64).reshape(-1)
    NT = hist.shape[0] - 1
    if NT != np.asarray(targets).reshape(-1).shape[0]:
        raise ValueError(f'eer_dcf_from_ranks: {hist.shape[0]} bins for {np.asarray(targets).size} targets')
    NN = int(hist.sum())
    if NT == 0 or NN == 0:
        raise ValueError('eer_dcf_from_ranks: no target or no non-target pairs')
    nt, nn = np.float64(NT), np.float64(NN)
    C = np.cumsum(hist)                                  # C[j]: the non-targets at or before target j
    j = np.arange(NT)
    fnr_t = (j + 1).astype('f8') / nt                    # at target j
    fnr_b = j.astype('f8') / nt                          # inside bin j
    fpr_t = 1 - C[:NT].astype('f8') / nn                 # at target j and at the last non-target of bin j

    def at(where):
        if where[0] == 't':
            return fnr_t[where[1]], fpr_t[where[1]]
        b, k = where[1], where[2]
        return fnr_b[b], 1 - np.float64((int(C[b - 1]) if b else 0) + k) / nn

    # fnr - fpr never decreases along the sorted order: the first target at which it is >= 0, then the first such score of its bin
    js = int(np.flatnonzero(fnr_t - fpr_t >= 0)[0])
    lo_k, hi_k = 1, int(hist[js]) + 1                    # the smallest k in [1, hist[js]] with gap >= 0; hist[js] + 1: none
    while lo_k < hi_k:
        mid = (lo_k + hi_k) // 2
        f, p = at(('n', js, mid))
        if f - p >= 0:
            hi_k = mid
        else:
            lo_k = mid + 1
    hi = ('n', js, lo_k) if lo_k <= int(hist[js]) else ('t', js)
    if hi[0] == 'n':
        lo = ('n', js, hi[2] - 1) if hi[2] > 1 else (('t', js - 1) if js > 0 else None)
    else:
        lo = ('n', js, int(hist[js])) if hist[js] > 0 else (('t', js - 1) if js > 0 else None)
    if lo is None:
        raise ValueError('eer_dcf_from_ranks: fnr >= fpr at the lowest score already (hi == 0)')
    fnr_hi, fpr_hi = at(hi)
    fnr_lo, fpr_lo = at(lo)
    a = (fnr_hi - fpr_hi) / (fpr_lo - fpr_hi - (fnr_lo - fnr_hi))
    eer = fnr_hi + a * (fnr_lo - fnr_hi)

    # c_det falls inside a run of non-targets (fpr falls, fnr stands) and rises at a target: its minimum is at the last position before
    # a target, at a target that opens the list, or at the very last position
    cost_t = c_miss * fnr_t * p_target + c_fa * fpr_t * (1 - p_target)
    cost_b = c_miss * fnr_b * p_target + c_fa * fpr_t * (1 - p_target)
    if hist[0] == 0:
        cost_b = cost_b[1:]                              # nothing stands before target 0
    fpr_end = 1 - np.float64(NN) / nn
    cost_end = c_miss * (nt / nt) * p_target + c_fa * fpr_end * (1 - p_target)
    c_det = min(float(cost_t.min()), float(cost_b.min()) if cost_b.size else float('inf'), float(cost_end))
    c_def = min(c_miss * p_target, c_fa * (1 - p_target))
    return float(eer), c_det / c_def, hi


def evaluate_trials_fused(enroll_features, enroll_labels, trials_features, trials_labels, score_norm=None):
    """evaluate_trials without the (Nt, Ne) matrix: nothing on the device or the host grows with Nt * Ne.  Returns
    (eer, min_dcf, threshold).  ``score_norm``: a ScoreNorm, or None for raw cosines."""
    r = TrialRanks(trials_features, trials_labels, enroll_features, enroll_labels, score_norm=score_norm)
    targets = r.targets.cpu().numpy()
    eer, min_dcf, where = eer_dcf_from_ranks(targets, r.hist.cpu().numpy())
    threshold = float(targets[where[1]]) if where[0] == 't' else r.kth_nontarget(where[1], where[2])
    return float(eer), float(min_dcf), float(threshold)
