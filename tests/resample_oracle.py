"""Float64 restatement of the sample-rate conversion (csrc/resample.hip, ppvector/data_utils/wave_batch.py resample_waves): the closed
form of scipy.signal.resample_poly(x, up, down) with its defaults (window ('kaiser', 5.0), padtype 'constant'), written on the output
index so that any stretch of outputs can be computed on its own:

    half = 10 max(up, down),   h = up firwin(2 half + 1, 1 / max(up, down), window=('kaiser', 5.0)),   M = ceil(n up / down)
    y[m] = sum_i x[i] h[m down + half - i up]      over the i with 0 <= i < n and 0 <= index <= 2 half

Nothing here is shared with the code under test: the filter is designed here, the sums are numpy's over float64."""
from math import gcd

import numpy as np
from scipy.signal import firwin

PAIRS = ((2, 1), (1, 2), (1, 3), (2, 3), (160, 441), (320, 441), (640, 441), (147, 160))     # (up, down) of the GPU cases
RATES_TO_16K = (8000, 11025, 22050, 24000, 32000, 44100, 48000)


def ratio(src_rate, dst_rate):
    g = gcd(int(dst_rate), int(src_rate))
    return int(dst_rate) // g, int(src_rate) // g


def out_len(n, up, down):
    return -(-int(n) * up // down)


def taps_per_phase(up, down):
    return -(-(20 * max(up, down) + 1) // up)


def design(up, down):
    half = 10 * max(up, down)
    return up * firwin(2 * half + 1, 1.0 / max(up, down), window=('kaiser', 5.0)), half


def closed_form(x, up, down, m_lo=0, m_hi=None):
    """y[m_lo:m_hi] of the closed form, float64; x is taken as float64.  Memory (m_hi - m_lo) x taps, so cut long rows into stretches."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    h, half = design(up, down)
    m_hi = out_len(n, up, down) if m_hi is None else m_hi
    m = np.arange(m_lo, m_hi, dtype=np.int64)
    c = m * down + half
    i_hi = c // up                                       # the largest i with index >= 0
    J = taps_per_phase(up, down)
    i = i_hi[:, None] - np.arange(J, dtype=np.int64)[None, :]
    k = c[:, None] - i * up
    ok = (i >= 0) & (i < n) & (k >= 0) & (k <= 2 * half)
    return np.sum(np.where(ok, x[np.clip(i, 0, max(n - 1, 0))] * h[np.clip(k, 0, 2 * half)], 0.0), axis=1)


def n_with_out_len(target, up, down, at_least=True):
    """An input length whose output length is the closest to `target` from above (at_least) or from below: every M is reachable when
    up <= down, only multiples' neighbours when up > down."""
    n = max(1, target * down // up)
    if at_least:
        while out_len(n, up, down) < target:
            n += 1
        while n > 1 and out_len(n - 1, up, down) >= target:
            n -= 1
    else:
        while n > 1 and out_len(n, up, down) > target:
            n -= 1
        while out_len(n + 1, up, down) <= target:
            n += 1
    return n


def edge_lengths(up, down, tile):
    """n = 1, n = 2, n with M one under / at / one over the tile (the nearest reachable), and a row spanning three tiles."""
    return sorted({1, 2, n_with_out_len(tile - 1, up, down, at_least=False), n_with_out_len(tile, up, down),
                   n_with_out_len(tile + 1, up, down), n_with_out_len(2 * tile + 77, up, down)})
