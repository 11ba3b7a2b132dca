"""Float64 NumPy reference of the two waveform augmentations that run on the GPU (csrc/augment.hip noise_mix_kernel,
csrc/reverb.hip), in the spirit of tests/conv2d_oracle.py.  TEST INFRASTRUCTURE ONLY.

PARITY UNPINNED [3P-memory]: the reference calls yeaudio's NoisePerturbAugmentor / ReverbPerturbAugmentor
(ppvector/data_utils/reader.py:159-162); yeaudio is third party, not vendored and not installed, so these restate its
published behaviour (AudioSegment.add_noise / AudioSegment.reverb), exactly as ppvector/data_utils/wave_batch.py documents it.
"""
import numpy as np


def rms_db(v):
    """AudioSegment.rms_db: 10 log10(max(mean v^2, 1e-20))."""
    v = np.asarray(v, np.float64)
    return 10.0 * np.log10(max(float(np.mean(v * v)), 1e-20))


def effective_noise(noise, n, start):
    """e[i] = noise[(start + i) mod Ln], i < n: the wrap-padded file when it is shorter than the utterance (start 0), else the
    segment [start, start + n)."""
    noise = np.asarray(noise, np.float64)
    return noise[(int(start) + np.arange(n)) % len(noise)]


def noise_gain_db(x, noise, snr_dB):
    """min(rms_dB(x) - rms_dB(noise) - snr_dB, 300); the noise level over the wrap-padded n samples when Ln < n, over the whole
    file otherwise (yeaudio measures it before it takes the subsegment)."""
    n = len(x)
    level = rms_db(effective_noise(noise, n, 0)) if len(noise) < n else rms_db(noise)
    return min(rms_db(x) - level - float(snr_dB), 300.0)


def add_noise(x, noise, snr_dB, start):
    """x (n,) + 10^(gain_dB / 20) * e, float64, not clipped."""
    x = np.asarray(x, np.float64)
    g = 10.0 ** (noise_gain_db(x, noise, snr_dB) / 20.0)
    return x + g * effective_noise(noise, len(x), start)


def unit_energy(rir):
    """h = rir / sqrt(sum rir^2) in float64; None for an all-zero response."""
    rir = np.asarray(rir, np.float64)
    e = float(np.sum(rir * rir))
    return rir / np.sqrt(e) if e > 0.0 else None


def convolve_cut(x, h):
    """convolve(x, h, 'full')[:n] in float64 with h taken as it is -- what the GPU kernel computes from an already scaled h."""
    x = np.asarray(x, np.float64)
    return np.convolve(x, np.asarray(h, np.float64), 'full')[:len(x)]


def reverb(x, rir):
    """convolve(x, rir / sqrt(sum rir^2), 'full')[:n] in float64; an all-zero response leaves x untouched."""
    h = unit_energy(rir)
    return np.asarray(x, np.float64).copy() if h is None else convolve_cut(x, h)
