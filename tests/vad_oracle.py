"""NumPy restatement of the energy voice-activity detector (csrc/vad.hip, docs/vad.md), from the contract in include/vpmi.h alone.

Stage A (``frame_db``) in float64 is the reference; the same arithmetic in float32 (``dtype=np.float32``) is there only to MEASURE what
f32 rounding costs on an input, which is where the GPU tests take their bound from.  Stage B (``regions``) does the threshold
arithmetic in np.float32 exactly as rule 3 states it and everything else in integers and plain loops, so on given f32 energies the
comparison with the kernel is bit-exact."""
import numpy as np


def num_frames(n, win, hop):
    return 0 if n < win else 1 + (n - win) // hop


def frame_db(x, win, hop, preemph, dtype=np.float64, block=4096):
    """Frame energies in dB of one recording: per frame the mean removed, pre-emphasis with y[0] = f[0] - c f[0], p = mean y^2,
    e = 10 log10(max(p, 1e-10)).  Every operation in ``dtype``."""
    x = np.asarray(x, dtype=dtype)
    F = num_frames(x.shape[0], win, hop)
    c = dtype(preemph)
    out = np.empty(F, dtype=dtype)
    for f0 in range(0, F, block):
        f1 = min(F, f0 + block)
        idx = (np.arange(f0, f1) * hop)[:, None] + np.arange(win)[None, :]
        fr = x[idx]
        d = fr - fr.mean(axis=1, dtype=dtype, keepdims=True)
        prev = np.concatenate([d[:, :1], d[:, :-1]], axis=1)
        y = d - c * prev
        p = (y * y).mean(axis=1, dtype=dtype)
        out[f0:f1] = dtype(10) * np.log10(np.maximum(p, dtype(1e-10)))
    return out


def rank(pct, F):
    """floor((double)pct (F - 1)), pct an f32 argument."""
    return int(np.floor(np.float64(np.float32(pct)) * np.float64(F - 1)))


def thresholds(e, floor_pct, peak_pct, margin_db, onset, offset):
    """(fl, pk, on, off) as np.float32, rules 2 and 3."""
    e = np.asarray(e, dtype=np.float32)
    srt = np.sort(e)
    fl, pk = srt[rank(floor_pct, e.size)], srt[rank(peak_pct, e.size)]
    with np.errstate(over='ignore', invalid='ignore'):               # energies the size of FLT_MAX: inf, as in the kernel
        r = np.float32(pk - fl)
        m = np.float32(margin_db)
        on = np.float32(fl + max(m, np.float32(np.float32(onset) * r)))
        off = np.float32(fl + max(m, np.float32(np.float32(offset) * r)))
    return fl, pk, on, off


def hysteresis(e, on, off):
    """Rule 4: the state of the latest decisive frame, silence before the first."""
    state, out = False, []
    for v in np.asarray(e):
        if v >= on:
            state = True
        elif v < off:
            state = False
        out.append(state)
    return out


def runs(states):
    """The maximal runs of True as [a, b) pairs."""
    out, start = [], None
    for t, s in enumerate(list(states) + [False]):
        if s and start is None:
            start = t
        elif not s and start is not None:
            out.append([start, t])
            start = None
    return out


def clean(states, min_gap, min_speech, pad):
    """Rules 5 - 7 on the frame states -> the regions [a, b) in frames."""
    F = len(states)
    rs = runs(states)
    filled = []
    for a, b in rs:                                                  # 5: a silence run between two speech frames, shorter than min_gap
        if filled and a - filled[-1][1] < min_gap:
            filled[-1][1] = b
        else:
            filled.append([a, b])
    kept = [r for r in filled if r[1] - r[0] >= min_speech]          # 6
    out = []
    for a, b in kept:                                                # 7: padded, then merged where they overlap or touch
        a, b = max(0, a - pad), min(F, b + pad)
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [tuple(r) for r in out]


def regions(e, floor_pct=0.10, peak_pct=0.95, margin_db=6.0, onset=0.35, offset=0.25, min_gap=30, min_speech=25, pad=10):
    """One recording's f32 energies -> ((fl, pk, on, off) f32, [(a, b)]); F = 0: zeros and nothing."""
    e = np.asarray(e, dtype=np.float32)
    if e.size == 0:
        z = np.float32(0)
        return (z, z, z, z), []
    thr = thresholds(e, floor_pct, peak_pct, margin_db, onset, offset)
    return thr, clean(hysteresis(e, thr[2], thr[3]), min_gap, min_speech, pad)


def to_seconds(a, b, n, win, hop, sr):
    """start = a hop / sr; end = min((b - 1) hop + win, n) / sr, and n / sr when b is the recording's last frame + 1."""
    end = n if b == num_frames(n, win, hop) else min((b - 1) * hop + win, n)
    return a * hop / sr, end / sr
