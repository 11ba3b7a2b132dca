"""Oracle (CPU, NumPy float64): speaker diarization.  Test helper, not a test module.

A restatement, from its behaviour, of the reference's ppvector/infer_utils/speaker_diarization.py:
  chunk table   inside every speech region windows of `dur` seconds start every `shift` seconds; a window that would run past the region
                is pulled back to end at its end; the walk stops at the first window that reaches no further than the one before.
  chunk batch   each window zero-padded on the right to the window length, then scaled to `target_db` dBFS RMS (the RMS over the PADDED row,
                floored at 1e-20 mean square, the gain capped at 300 dB) -- what the predictor's _load_audio does to every ndarray it is given.
  clustering    cosine affinity -> the n_elems smallest entries of each row zeroed (n_elems = int((1 - p) n), p = max-style floor 6 / n when
                n * pval < 6) -> M = (P + P^T) / 2, zero diagonal -> L = diag(sum |M|) - M -> eigenvectors of the smallest eigenvalues (their
                number given, or the place of the largest gap among the first max_spk + 1 eigenvalues) -> k-means -> labels renumbered in
                order of first appearance -> speakers whose centres' cosine reaches the merge threshold merged (centres never recomputed).
  postprocess   runs of one speaker joined; overlapping neighbours split at the midpoint of the overlap; times rounded to 10 ms; segments
                shorter than 1 s given to the nearer neighbour (the only neighbour at either end); runs joined again.
Ties in the pruning are broken by the lower column being zeroed first (a stable sort), the engine's documented rule.
"""
import numpy as np


def chunk_table(regions, sr=16000, dur=1.5, shift=0.75):
    """regions: (start_s, end_s) pairs -> rows [start_s, end_s, first_sample, end_sample]."""
    win, hop = int(dur * sr), int(shift * sr)
    rows = []
    for start, end in regions:
        s0, s1 = round(float(start), 3), round(float(end), 3)
        base = int(s0 * sr)
        n = int(s1 * sr) - base
        pos, prev_stop = 0, 0
        while pos < n:
            stop = pos + win if pos + win < n else n
            if stop <= prev_stop:
                break
            begin = stop - win if stop > win else 0
            rows.append([begin / sr + s0, stop / sr + s0, base + begin, base + stop])
            prev_stop = stop
            pos += hop
    return rows


def chunk_batch(wave, table, chunk_len, normalize=True, target_db=-20.0):
    wave = np.asarray(wave, dtype=np.float64)
    out = np.zeros((len(table), chunk_len), dtype=np.float64)
    for b, (a, e) in enumerate(table):
        a, e = int(a), int(e)
        row = wave[a:e][:chunk_len]
        out[b, :row.shape[0]] = row
        if normalize:
            mean_sq = max(float(np.mean(out[b] ** 2)), 1e-20)
            gain_db = min(target_db - 10.0 * np.log10(mean_sq), 300.0)
            out[b] *= 10.0 ** (gain_db / 20.0)
    return out


def n_elems(n, pval=0.022):
    p = 6.0 / n if n * pval < 6 else pval
    return int((1 - p) * n)


def cosine_affinity(X):
    X = np.asarray(X, dtype=np.float64)
    Xn = X / np.linalg.norm(X, axis=1, keepdims=True)
    return Xn @ Xn.T


def prune(S, k):
    """Zero the k smallest entries of every row; equal values: lower column first."""
    P = np.array(S, dtype=np.float64, copy=True)
    if k > 0:
        order = np.argsort(P, axis=1, kind='stable')[:, :k]
        np.put_along_axis(P, order, 0.0, axis=1)
    return P


def laplacian(P):
    P = np.asarray(P, dtype=np.float64)
    M = 0.5 * (P + P.T)
    np.fill_diagonal(M, 0.0)
    return np.diag(np.abs(M).sum(axis=1)) - M


def relabel(labels):
    first = {}
    for l in labels:
        first.setdefault(int(l), len(first))
    return np.array([first[int(l)] for l in labels])


def spectral_labels(X, num=None, min_spk=1, max_spk=15, pval=0.022):
    import scipy.linalg
    from sklearn.cluster import k_means
    X = np.asarray(X, dtype=np.float64)
    L = laplacian(prune(cosine_affinity(X), n_elems(X.shape[0], pval)))
    vals, vecs = scipy.linalg.eigh(L)
    if num is None:
        head = vals[min_spk - 1:max_spk + 1]
        num = int(np.argmax(np.diff(head))) + min_spk
    return k_means(vecs[:, :num], num, n_init='auto')[1]


def merge_by_cos(labels, centers, thr):
    labels = np.array(labels, copy=True)
    centers = np.asarray(centers, dtype=np.float64)
    while labels.max() > 0:
        c = centers[:labels.max() + 1]
        c = c / np.linalg.norm(c, axis=1, keepdims=True)
        aff = np.triu(c @ c.T, 1)
        a, b = divmod(int(np.argmax(aff)), aff.shape[1])
        if aff[a, b] < thr:
            break
        labels = np.where(labels == b, a, np.where(labels > b, labels - 1, labels))
    return labels


def clustering(X, speaker_num=None, merge_threshold=0.78):
    X = np.asarray(X, dtype=np.float64)
    labels = relabel(spectral_labels(X, speaker_num))
    centers = np.stack([X[labels == i].mean(axis=0) for i in range(labels.max() + 1)])
    return merge_by_cos(labels, centers, merge_threshold), centers


def join_runs(rows):
    out = []
    for st, ed, spk in rows:
        if out and out[-1][2] == spk and st <= out[-1][1]:
            out[-1][1] = ed
        else:
            out.append([st, ed, spk])
    return out


def smooth(rows, min_duration=1):
    rows = [list(r) for r in rows]
    n = len(rows)
    for i in range(n):                                   # in place and in order: a relabelled segment is what its successor sees
        rows[i][0], rows[i][1] = round(rows[i][0], 2), round(rows[i][1], 2)
        if rows[i][1] - rows[i][0] >= min_duration:
            continue
        if i == 0:
            src = 1
        elif i == n - 1:
            src = i - 1
        else:                                            # rows[i + 1] is not rounded yet at this point, as in the reference
            src = i - 1 if rows[i][0] - rows[i - 1][1] <= rows[i + 1][0] - rows[i][1] else i + 1
        rows[i][2] = rows[src][2]
    return join_runs(rows)


def postprocess(table, labels):
    rows = join_runs([[table[i][0], table[i][1], labels[i]] for i in range(len(table))])
    for prev, cur in zip(rows[:-1], rows[1:]):
        if prev[1] > cur[0] + 1e-4:
            prev[1] = cur[0] = (cur[0] + prev[1]) / 2
    return [dict(speaker=spk, start=round(st, 3), end=round(ed, 3)) for st, ed, spk in smooth(rows)]
