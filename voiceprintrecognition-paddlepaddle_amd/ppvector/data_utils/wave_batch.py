"""Waveform batch assembly on the GPU -- the work PPVectorDataset.__getitem__ does per utterance on CPU workers in front
of the featurizer (ppvector/data_utils/reader.py:97-101: decibel normalisation, crop to max_duration) plus the zero
padding of predict_batch (ppvector/predict.py:246-254), as one launch over the whole batch (csrc/augment.hip
wave_batch_kernel).  Decoding stays on the host; this takes the decoded utterances already on the device.  Sample-rate conversion
stays on the host too unless ppvector.set_resampler('gpu') is in force: then resample_waves (csrc/resample.hip, docs/resample.md)
converts the uploaded native-rate utterances here, in front of everything else."""
import threading
from math import gcd

import numpy as np
import torch

from ppvector import _native as N


def assemble_waves(waves, max_len=None, starts=None, use_dB_normalization=True, target_dB=-20.0, gains_dB=None, with_valid=False):
    """waves: list of 1-D float GPU tensors (ragged).  Returns (batch (B, L) f32, input_lens_ratio (B,) f32) -- what
    AudioFeaturizer.forward(waveforms, input_lens_ratio) takes.  L = max_len or the longest utterance after its crop start.
    starts: per-utterance crop start in samples (the training-mode random crop; None = 0).  gains_dB: per-utterance gain when
    normalisation is off (the volume perturbation's draw).  with_valid adds the kept sample counts (B,) int32."""
    waves = [torch.as_tensor(w) for w in waves]
    if not waves or not all(w.is_cuda for w in waves):
        raise N.VpmiError('assemble_waves packs GPU waveforms: the engine has no CPU fallback')
    waves = [w.reshape(-1).contiguous().float() for w in waves]
    dev = waves[0].device
    B = len(waves)
    lens = [int(w.numel()) for w in waves]
    st = [0] * B if starts is None else [min(max(int(s), 0), n) for s, n in zip(starts, lens)]
    L = int(max_len) if max_len else max(n - s for n, s in zip(lens, st))
    if L <= 0:
        raise ValueError('assemble_waves: empty batch row length')
    out = torch.empty((B, L), dtype=torch.float32, device=dev)
    meta = torch.tensor([[w.data_ptr() for w in waves], lens, st], dtype=torch.int64)
    ptrs = meta[0].to(dev)
    lens_d, st_d = meta[1].to(torch.int32).to(dev), meta[2].to(torch.int32).to(dev)
    nv = torch.empty((B,), dtype=torch.int32, device=dev)
    g = None if gains_dB is None else torch.as_tensor(gains_dB, dtype=torch.float32).to(dev).contiguous()
    ctx = N.ctx(dev)
    N.check(N.lib().vp_wave_batch_f32(ctx, ptrs.data_ptr(), lens_d.data_ptr(), st_d.data_ptr(), B, L, int(bool(use_dB_normalization)),
                                      float(target_dB), None if g is None else g.data_ptr(), out.data_ptr(), nv.data_ptr(),
                                      N.stream_ptr()), ctx)
    ratio = nv.float() / float(L)
    return (out, ratio, nv) if with_valid else (out, ratio)


SPEEDS = (1.0, 0.9, 1.1)          # yeaudio SpeedPerturbAugmentor's rates; index = the class offset of speed_perturb_3_class


def speed_perturb(waves, rates):
    """Speed perturbation of a ragged batch on the GPU (SpeedPerturbAugmentor / AudioSegment.change_speed, reader.py:155-156):
    utterance b is resampled by linear interpolation to int(len / rates[b]) samples; rate 1.0 passes through untouched.
    waves: list of 1-D float GPU tensors.  Returns a list of the same length."""
    waves = [torch.as_tensor(w) for w in waves]
    if not waves or not all(w.is_cuda for w in waves):
        raise N.VpmiError('speed_perturb takes GPU waveforms: the engine has no CPU fallback')
    idx = [b for b, r in enumerate(rates) if float(r) != 1.0]
    out = list(waves)
    if not idx:
        return out
    src = [waves[b].reshape(-1).contiguous().float() for b in idx]
    lens = [int(w.numel()) for w in src]
    new_lens = [int(n / float(rates[b])) for n, b in zip(lens, idx)]
    if min(new_lens) <= 0:
        raise ValueError('speed_perturb: an utterance would become empty')
    dev = src[0].device
    dst = [torch.empty(m, dtype=torch.float32, device=dev) for m in new_lens]
    meta = torch.tensor([[w.data_ptr() for w in src], [w.data_ptr() for w in dst], lens, new_lens], dtype=torch.int64)
    sp, dp = meta[0].to(dev), meta[1].to(dev)
    ld, nd = meta[2].to(torch.int32).to(dev), meta[3].to(torch.int32).to(dev)
    ctx = N.ctx(dev)
    N.check(N.lib().vp_speed_perturb_f32(ctx, sp.data_ptr(), ld.data_ptr(), nd.data_ptr(), dp.data_ptr(), len(idx), max(new_lens),
                                         N.stream_ptr()), ctx)
    for b, w in zip(idx, dst):
        out[b] = w
    return out


def _selected(name, waves, others):
    """Shared front of noise_perturb / reverb_perturb: GPU checks, the selected rows, their flattened f32 sources and partners."""
    waves = [torch.as_tensor(w) for w in waves]
    if not waves or not all(w.is_cuda for w in waves):
        raise N.VpmiError(f'{name} takes GPU waveforms: the engine has no CPU fallback')
    if len(others) != len(waves):
        raise ValueError(f'{name}: {len(others)} entries for {len(waves)} utterances')
    idx = [b for b, o in enumerate(others) if o is not None]
    oth = [torch.as_tensor(others[b]) for b in idx]
    if not all(o.is_cuda for o in oth):
        raise N.VpmiError(f'{name} takes GPU noise / impulse-response tensors: the engine has no CPU fallback')
    src = [waves[b].reshape(-1).contiguous().float() for b in idx]
    oth = [o.reshape(-1).contiguous().float() for o in oth]
    if any(w.numel() == 0 for w in src) or any(o.numel() == 0 for o in oth):
        raise ValueError(f'{name}: empty utterance or empty partner signal')
    return waves, idx, src, oth


def _ragged_empty(lens, dev):
    """New f32 rows of the given lengths as views of ONE allocation (16-byte aligned starts), like the trainer's upload."""
    offs = np.concatenate(([0], np.cumsum([(n + 3) // 4 * 4 for n in lens]))).tolist()
    buf = torch.empty(max(offs[-1], 1), dtype=torch.float32, device=dev)
    return [buf[o:o + n] for o, n in zip(offs[:-1], lens)]


def _device_tables(dev, ptr_rows, int_rows, float_rows=()):
    """The launch's per-utterance tables -- rows of device pointers, of int32 and of float32, k entries each -- through ONE
    host-to-device copy.  Returns (buffer to keep alive until the launch, [device address of each row, in the order given])."""
    k = len(ptr_rows[0])
    host = np.empty((2 * len(ptr_rows) + len(int_rows) + len(float_rows)) * k, dtype=np.int32)
    a, b = 2 * len(ptr_rows) * k, (2 * len(ptr_rows) + len(int_rows)) * k
    host[:a].view(np.int64)[:] = np.asarray(ptr_rows, dtype=np.int64).ravel()
    host[a:b] = np.asarray(int_rows, dtype=np.int32).ravel()
    if float_rows:
        host[b:].view(np.float32)[:] = np.asarray(float_rows, dtype=np.float32).ravel()
    d = torch.from_numpy(host).to(dev)
    base = d.data_ptr()
    return d, [base + 8 * k * r for r in range(len(ptr_rows))] + [base + 4 * a + 4 * k * r for r in range(len(int_rows) + len(float_rows))]


def noise_perturb(waves, noises, snrs_dB, noise_starts):
    """Noise perturbation of a ragged batch on the GPU (NoisePerturbAugmentor -> AudioSegment.add_noise, reader.py:159-160).  yeaudio
    is third party and not installed: restated from its published behaviour [3P-memory], PARITY UNPINNED.  For utterance x (n
    samples, after the speed change) and the decoded noise file (Ln samples, first channel, at the dataset's rate):
        Ln <  n: the noise is wrap-padded to n samples and used whole (start 0), its level measured over those n samples;
        Ln >= n: the segment [start, start + n) is used, its level measured over the WHOLE file (yeaudio measures before it cuts);
        e[i] = noise[(start + i) mod Ln];  rms_dB(v) = 10 log10(max(mean v^2, 1e-20));
        out[i] = x[i] + 10^(min(rms_dB(x) - rms_dB(noise) - snr_dB, 300) / 20) * e[i], not clipped.
    waves: list of 1-D float GPU tensors; noises[b]: 1-D float GPU tensor, or None = not selected (snrs_dB[b] / noise_starts[b] are then
    ignored).  Returns a list: an unselected row is the SAME tensor object, a selected one a new tensor of the same length."""
    waves, idx, src, nz = _selected('noise_perturb', waves, noises)
    out = list(waves)
    if not idx:
        return out
    dev = src[0].device
    lens, nlens = [int(w.numel()) for w in src], [int(z.numel()) for z in nz]
    dst = _ragged_empty(lens, dev)
    keep, (sp, zp, dp, ld, zd, sd, snr) = _device_tables(
        dev, [[w.data_ptr() for w in src], [z.data_ptr() for z in nz], [w.data_ptr() for w in dst]],
        [lens, nlens, [int(noise_starts[b]) for b in idx]], [[float(snrs_dB[b]) for b in idx]])
    ctx = N.ctx(dev)
    N.check(N.lib().vp_noise_mix_f32(ctx, sp, ld, zp, zd, sd, snr, dp, len(idx), N.stream_ptr()), ctx)
    for b, w in zip(idx, dst):
        out[b] = w
    return out


_reverb_ws = N.Workspace()


def reverb_perturb(waves, rirs):
    """Reverberation of a ragged batch on the GPU (ReverbPerturbAugmentor -> AudioSegment.reverb, reader.py:161-162).  yeaudio is third
    party and not installed: restated from its published behaviour [3P-memory], PARITY UNPINNED: out = convolve(x, h, 'full')[:n] with
    h = rir / sqrt(sum rir^2).  rirs[b] is h ALREADY scaled to unit energy (the reader does it in float64 when it decodes the file;
    an all-zero file is never selected), or None = not selected.  csrc/reverb.hip: partitioned overlap-save FFT convolution.
    waves: list of 1-D float GPU tensors.  Returns a list: an unselected row is the SAME tensor object, a selected one a new tensor
    of the same length."""
    waves, idx, src, hs = _selected('reverb_perturb', waves, rirs)
    out = list(waves)
    if not idx:
        return out
    dev = src[0].device
    lens, hlens = [int(w.numel()) for w in src], [int(h.numel()) for h in hs]
    dst = _ragged_empty(lens, dev)
    keep, (sp, hp, dp, ld, hd) = _device_tables(dev, [[w.data_ptr() for w in src], [h.data_ptr() for h in hs], [w.data_ptr() for w in dst]],
                                                [lens, hlens])
    need = int(N.lib().vp_reverb_workspace_bytes(len(idx), max(lens), max(hlens)))
    ws = _reverb_ws.get(need, dev)
    ctx = N.ctx(dev)
    N.check(N.lib().vp_reverb_f32(ctx, sp, ld, hp, hd, dp, len(idx), max(lens), max(hlens), ws.data_ptr(), ws.numel(), N.stream_ptr()), ctx)
    for b, w in zip(idx, dst):
        out[b] = w
    return out


# ------------------------------------------------------------------------------------------------------------- sample rate
MAX_RESAMPLE_RATE = 1024          # of max(up, down): csrc/resample.hip; a pair past it goes through the host function


def resample_ratio(src_rate, dst_rate):
    """(up, down) of scipy.signal.resample_poly for src_rate -> dst_rate, as AudioSegment.resample forms them."""
    g = gcd(int(dst_rate), int(src_rate))
    return int(dst_rate) // g, int(src_rate) // g


def resample_len(n, up, down):
    """resample_poly's output length for n samples: ceil(n up / down)."""
    return -(-int(n) * int(up) // int(down))


def resample_filter(up, down):
    """(h float64 (2 half + 1,), half): resample_poly's default filter, up * firwin(2 half + 1, 1 / max(up, down), ('kaiser', 5.0))."""
    from scipy.signal import firwin
    half = 10 * max(int(up), int(down))
    return int(up) * firwin(2 * half + 1, 1.0 / max(int(up), int(down)), window=('kaiser', 5.0)), half


def phase_table(up, down):
    """The kernel's coefficient table, float32 (up, J): P[p][j] = h[p + j up], zero past the filter's end, J = ceil((2 half + 1) / up).
    Designed in float64, rounded once."""
    h, half = resample_filter(up, down)
    J = -(-(2 * half + 1) // int(up))
    flat = np.zeros(J * int(up), dtype=np.float64)
    flat[:h.shape[0]] = h
    return np.ascontiguousarray(flat.reshape(J, int(up)).T, dtype=np.float32)


_phase_tables, _phase_lock = {}, threading.Lock()


def _phase_table_on(up, down, dev):
    """phase_table(up, down) on the device, kept per (up, down, device)."""
    key = (int(up), int(down), str(dev))
    with _phase_lock:
        if key not in _phase_tables:
            _phase_tables[key] = torch.from_numpy(phase_table(up, down)).to(dev)
        return _phase_tables[key]


def resample_waves(waves, src_rates, dst_rate):
    """Sample-rate conversion of a ragged batch on the GPU: row b goes from src_rates[b] to dst_rate as AudioSegment.resample does on
    the host (scipy.signal.resample_poly(x, up, down) with its defaults; csrc/resample.hip, docs/resample.md) -- one launch per source
    rate in the batch.  waves: list of 1-D float GPU tensors.  Returns a list: a row already at dst_rate is the SAME tensor object, a
    converted one a new tensor of ceil(n up / down) samples.  A pair with max(up, down) > 1024 is outside the kernel's range: that
    row takes the host function and is uploaded again."""
    waves = [torch.as_tensor(w) for w in waves]
    if not waves or not all(w.is_cuda for w in waves):
        raise N.VpmiError('resample_waves takes GPU waveforms: the engine has no CPU fallback')
    if len(src_rates) != len(waves):
        raise ValueError(f'resample_waves: {len(src_rates)} rates for {len(waves)} utterances')
    out = list(waves)
    groups = {}
    for b, r in enumerate(src_rates):
        if int(r) != int(dst_rate):
            groups.setdefault(resample_ratio(r, dst_rate), []).append(b)
    for ud in [ud for ud in groups if max(ud) > MAX_RESAMPLE_RATE]:
        from ppvector.predict import AudioSegment
        for b in groups.pop(ud):
            seg = AudioSegment(waves[b].reshape(-1).float().cpu().numpy(), int(src_rates[b]))
            seg.resample(dst_rate)
            out[b] = torch.from_numpy(seg.samples).to(waves[b].device)
    if not groups:
        return out
    idx = [b for rows in groups.values() for b in rows]            # group by group: a launch's rows are neighbours in the tables
    src = [waves[b].reshape(-1).contiguous().float() for b in idx]
    dev = src[0].device
    lens = [int(w.numel()) for w in src]
    new_lens = [resample_len(n, *ud) for n, ud in zip(lens, [ud for ud, rows in groups.items() for _ in rows])]
    dst = _ragged_empty(new_lens, dev)
    keep, (sp, dp, ld, nd) = _device_tables(dev, [[w.data_ptr() for w in src], [w.data_ptr() for w in dst]], [lens, new_lens])
    ctx = N.ctx(dev)
    k0 = 0
    for (up, down), rows in groups.items():
        k, longest = len(rows), max(new_lens[k0:k0 + len(rows)])
        if longest > 0:
            table = _phase_table_on(up, down, dev)
            N.check(N.lib().vp_resample_poly_f32(ctx, sp + 8 * k0, ld + 4 * k0, nd + 4 * k0, dp + 8 * k0, k, longest, up, down,
                                                 table.data_ptr(), int(table.shape[1]), N.stream_ptr()), ctx)
        k0 += k
    for b, w in zip(idx, dst):
        out[b] = w
    return out
