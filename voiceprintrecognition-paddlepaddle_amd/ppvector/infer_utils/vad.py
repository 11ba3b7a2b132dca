"""Energy voice-activity detection on the MI355X engine: the speech regions ``SpeakerDiarization.segments`` reads, from the recording alone.

This file has no counterpart in the reference.  There the regions come from yeaudio's model-based ``AudioSegment.vad``
(infer_utils/speaker_diarization.py:37), whose model has no weights here.  ``EnergyVad`` is a deterministic detector of this project's
own, opt-in (``PPVectorPredictor.set_vad``), and does NOT reproduce that model's regions: frame energies in dB, a noise floor and a
speech level taken from the recording's own distribution, two thresholds with hysteresis, run-length clean-up (docs/vad.md has the
method, the contract and the known failure modes).

What runs in HIP (csrc/vad.hip): everything between the waveform on the device and the list of regions -- ``vp_vad_frame_db_f32`` and
``vp_vad_regions_f32``, two launches for a whole ragged batch.  What comes back to the host is B counts, B x 4 thresholds and the
regions; nothing of the size of the audio.  There is no CPU path: the calls raise ``VpmiError`` without a GPU.
"""
from collections import namedtuple

import numpy as np
import torch

from ppvector import _native as N

Thresholds = namedtuple('Thresholds', 'floor peak on off')          # dB: the two order statistics and the two thresholds

MAX_WIN = 4096                                                       # csrc/vad.hip


class EnergyVad:
    def __init__(self, sample_rate=16000, frame_ms=25, hop_ms=10, preemph=0.97, floor_pct=0.10, peak_pct=0.95, margin_db=6.0,
                 onset=0.35, offset=0.25, min_silence=0.30, min_speech=0.25, pad=0.10):
        """``floor_pct`` / ``peak_pct``: the ranks (as fractions of F - 1) of the frame energies taken as noise floor and speech level.
        A frame turns speech on at floor + max(margin_db, onset (peak - floor)) and off under floor + max(margin_db, offset (peak -
        floor)).  ``min_silence`` (a shorter pause inside speech is filled), ``min_speech`` (a shorter burst is dropped) and ``pad``
        (added on both sides of what is left) are in seconds and become frames by ``round(x / hop_s)``."""
        self.sample_rate = int(sample_rate)
        if self.sample_rate < 1:
            raise ValueError(f'EnergyVad: sample_rate >= 1, got {sample_rate}')
        self.win = int(round(self.sample_rate * frame_ms / 1000.0))
        self.hop = int(round(self.sample_rate * hop_ms / 1000.0))
        if not 1 <= self.hop <= self.win <= MAX_WIN:
            raise ValueError(f'EnergyVad: 1 <= hop <= win <= {MAX_WIN} samples, got hop {self.hop}, win {self.win}')
        if not 0.0 <= preemph < 1.0:
            raise ValueError(f'EnergyVad: 0 <= preemph < 1, got {preemph}')
        if not 0.0 <= floor_pct <= peak_pct <= 1.0:
            raise ValueError(f'EnergyVad: 0 <= floor_pct <= peak_pct <= 1, got {floor_pct}, {peak_pct}')
        if not 0.0 <= offset <= onset <= 1.0:
            raise ValueError(f'EnergyVad: 0 <= offset <= onset <= 1, got {offset}, {onset}')
        if not margin_db >= 0.0:
            raise ValueError(f'EnergyVad: margin_db >= 0, got {margin_db}')
        if not (min_silence >= 0.0 and min_speech >= 0.0 and pad >= 0.0):
            raise ValueError(f'EnergyVad: min_silence, min_speech, pad >= 0 s, got {min_silence}, {min_speech}, {pad}')
        self.preemph, self.floor_pct, self.peak_pct = float(preemph), float(floor_pct), float(peak_pct)
        self.margin_db, self.onset, self.offset = float(margin_db), float(onset), float(offset)
        hop_s = self.hop / self.sample_rate
        self.min_gap = max(int(round(min_silence / hop_s)), 1)       # frames; 1 = nothing is filled / dropped
        self.min_run = max(int(round(min_speech / hop_s)), 1)
        self.pad = int(round(pad / hop_s))
        self._ws = N.Workspace()

    # ------------------------------------------------------------------ host arithmetic
    def num_frames(self, n):
        """Snip-edges: 0 under one window, else 1 + (n - win) // hop (vp_vad_num_frames)."""
        return 0 if n < self.win else 1 + (int(n) - self.win) // self.hop

    def to_seconds(self, a, b, n):
        """Frames [a, b) of a recording of n samples -> (start_s, end_s): the region ends with its last frame's window, and the last
        frame's region with the recording, so the tail no frame covers is not cut off."""
        end = n if b == self.num_frames(n) else min((b - 1) * self.hop + self.win, n)
        return a * self.hop / self.sample_rate, end / self.sample_rate

    # ------------------------------------------------------------------ engine calls
    def _pack(self, waves):
        """One 1-D array or tensor, or a list of them -> (the recordings back to back as one f32 device tensor, their lengths, single)."""
        single = not isinstance(waves, (list, tuple))
        device = N.default_device()
        parts = []
        for w in ([waves] if single else waves):
            if not isinstance(w, torch.Tensor):
                w = np.ascontiguousarray(w, dtype=np.float32)
                w = torch.from_numpy(w if w.flags.writeable else w.copy())      # torch refuses to wrap a read-only array quietly
            t = w
            if t.dim() != 1:
                raise ValueError(f'EnergyVad: a recording is a 1-D array, got shape {tuple(t.shape)}')
            parts.append(t.to(device=device if not t.is_cuda else t.device, dtype=torch.float32).contiguous())
        if not parts:
            raise ValueError('EnergyVad: an empty list of recordings')
        lengths = [int(p.shape[0]) for p in parts]
        if sum(lengths) >= 2 ** 31:
            raise ValueError('EnergyVad: the batch has 2^31 samples or more (the offsets are int32)')
        return (parts[0] if len(parts) == 1 else torch.cat(parts)), lengths, single

    def _frame_db(self, wave, lengths):
        frames = [self.num_frames(n) for n in lengths]
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)).to(wave.device)
        frame_offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(frames)]).astype(np.int32)).to(wave.device)
        e = torch.empty(max(sum(frames), 1), dtype=torch.float32, device=wave.device)
        lib, ctx = N.lib(), N.ctx(wave.device)
        N.check(lib.vp_vad_frame_db_f32(ctx, N.ptr(wave), N.ptr(offsets), N.ptr(frame_offsets), len(lengths), self.win, self.hop,
                                        self.preemph, N.ptr(e), N.stream_ptr()), ctx)
        return e[:sum(frames)], frames, frame_offsets

    def frame_db(self, waves):
        """The frame energies in dB, a device tensor (F,) per recording (vp_vad_frame_db_f32)."""
        wave, lengths, single = self._pack(waves)
        e, frames, _ = self._frame_db(wave, lengths)
        out = list(torch.split(e, frames))
        return out[0] if single else out

    def regions_of_db(self, e, frame_offsets, frames, cap=None):
        """vp_vad_regions_f32 on energies that are already on the device -> host (counts (B,), regions (B, k, 2), thr (B, 4)), k the
        largest count (at most ``cap``).  ``cap`` defaults to ceil(F_max / 2), which no recording can exceed."""
        B = len(frames)
        cap = (max(frames) + 1) // 2 if cap is None else int(cap)
        lib, ctx = N.lib(), N.ctx(e.device)
        thr = torch.empty((B, 4), dtype=torch.float32, device=e.device)
        counts = torch.empty(B, dtype=torch.int32, device=e.device)
        regions = torch.empty((B, max(cap, 1), 2), dtype=torch.int32, device=e.device)
        nbytes = lib.vp_vad_workspace_bytes(sum(frames), B)
        ws = self._ws.get(nbytes, e.device)
        N.check(lib.vp_vad_regions_f32(ctx, N.ptr(e), N.ptr(frame_offsets), B, self.floor_pct, self.peak_pct, self.margin_db,
                                       self.onset, self.offset, self.min_gap, self.min_run, self.pad, N.ptr(thr), N.ptr(counts),
                                       N.ptr(regions), cap, N.ptr(ws), ws.numel(), N.stream_ptr()), ctx)
        counts = counts.cpu().numpy()
        most = min(int(counts.max()), cap)                           # only the rows that were written come to the host
        return counts, regions[:, :most].cpu().numpy(), thr.cpu().numpy()

    def frame_regions(self, waves):
        """Per recording ``(regions, Thresholds)`` with the regions in frames, an int array (k, 2) of (first, one past the last)."""
        wave, lengths, single = self._pack(waves)
        e, frames, frame_offsets = self._frame_db(wave, lengths)
        counts, regions, thr = self.regions_of_db(e, frame_offsets, frames)
        out = [(regions[b, :counts[b]].astype(np.int64), Thresholds(*(float(v) for v in thr[b]))) for b in range(len(lengths))]
        return out[0] if single else out

    def regions(self, waves):
        """Per recording ``(regions, Thresholds)`` with the regions as a list of (start_s, end_s).  ``waves``: one 1-D array or tensor
        (host or device), or a list of them -- a list goes through one ragged call and returns a list."""
        wave, lengths, single = self._pack(waves)
        e, frames, frame_offsets = self._frame_db(wave, lengths)
        counts, regions, thr = self.regions_of_db(e, frame_offsets, frames)
        out = []
        for b, n in enumerate(lengths):
            secs = [self.to_seconds(int(a), int(z), n) for a, z in regions[b, :counts[b]]]
            out.append((secs, Thresholds(*(float(v) for v in thr[b]))))
        return out[0] if single else out
