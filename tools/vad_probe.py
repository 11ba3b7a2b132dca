"""The energy voice-activity detector on one MI355X against the host (reported, not gated; timings only).

GPU: ``EnergyVad.regions`` on a recording that is ALREADY on the device (the upload is timed on its own), for --minutes long recordings
at 16 kHz: the host clock around the whole call -- two launches, the two small offset read-backs, and the copy of counts, thresholds and
regions to the host -- the median of --iters calls after a warm-up, with the spread; ``frame_db`` alone likewise (with a synchronise).
Host, same machine: the float32 restatement of tests/vad_oracle.py (NumPy frame energies, np.sort for the two order statistics, plain
loops for the hysteresis and the clean-up) under --threads threads, the median of --host-iters runs.  The regions of the two are
compared on the way (they may differ where a frame's f32 energy falls on the other side of a threshold; the count is printed).
Then ``PPVectorPredictor.speaker_diarization`` end to end on the 12.5 s recording of tests/test_gpu_vad.py with the detector set,
against the same call given the regions.  The clocks are printed with the numbers.

Usage: python tools/vad_probe.py [--minutes 10 60] [--iters 20] [--warmup 3] [--host-iters 3] [--threads 16]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'voiceprintrecognition-paddlepaddle_amd')):
    sys.path.insert(0, p)


def clocks():
    try:
        return subprocess.run(['amd-smi', 'metric', '--clock'], capture_output=True, text=True, timeout=30).stdout.strip()
    except Exception as e:      # the tool is optional on the machine
        return f'(amd-smi unavailable: {e})'


def recording(minutes, sr=16000, seed=0):
    """Noise at -55 dB with stretches of 0.2 .. 6 s at -20 .. -32 dB separated by pauses of 0.1 .. 3 s, on a small DC."""
    import numpy as np
    rng = np.random.RandomState(seed)
    n = int(minutes * 60 * sr)
    level = np.full(n, 10 ** (-55 / 20), np.float32)
    t = 0
    while t < n:
        t += int(rng.uniform(0.1, 3.0) * sr)
        d = int(rng.uniform(0.2, 6.0) * sr)
        level[t:t + d] = 10 ** (rng.uniform(-32, -20) / 20)
        t += d
    return (0.01 + level * rng.standard_normal(n).astype(np.float32)).astype(np.float32)


def spread(ts):
    return f'median {statistics.median(ts):9.3f} ms   (min {min(ts):.3f}, max {max(ts):.3f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--minutes', type=float, nargs='+', default=[10, 60])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-iters', type=int, default=3)
    ap.add_argument('--threads', type=int, default=16)
    a = ap.parse_args()
    for v in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):
        os.environ[v] = str(a.threads)
    import numpy as np
    import torch
    from tests import vad_oracle as ov
    from ppvector.infer_utils.vad import EnergyVad
    torch.set_num_threads(a.threads)
    assert torch.cuda.is_available(), 'needs an MI355X: the engine has no CPU fallback'
    vad = EnergyVad()
    print(clocks(), flush=True)

    def host_clock(fn, iters, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    for minutes in a.minutes:
        x = recording(minutes)
        F = vad.num_frames(x.size)
        print(f'--- {minutes:g} min at 16 kHz: {x.size} samples, {F} frames ({a.iters} calls after {a.warmup} warm-up, host clock, the result on the host)')
        up = host_clock(lambda: torch.from_numpy(x).cuda(), 5, 1)
        xd = torch.from_numpy(x).cuda()
        print(f'upload (pageable host memory)      {spread(up)}')
        print(f'gpu  EnergyVad.regions             {spread(host_clock(lambda: vad.regions(xd), a.iters, a.warmup))}', flush=True)
        print(f'gpu  EnergyVad.frame_db alone      {spread(host_clock(lambda: vad.frame_db(xd), a.iters, a.warmup))}', flush=True)
        e_dev = vad.frame_db(xd)
        fo = torch.tensor([0, F], dtype=torch.int32, device='cuda')
        print(f'gpu  regions of the energies alone {spread(host_clock(lambda: vad.regions_of_db(e_dev, fo, [F]), a.iters, a.warmup))}', flush=True)

        hs, hs_a = [], []
        for i in range(a.host_iters + 1):
            t0 = time.perf_counter()
            e = ov.frame_db(x, vad.win, vad.hop, vad.preemph, dtype=np.float32)
            t1 = time.perf_counter()
            thr, reg = ov.regions(e, vad.floor_pct, vad.peak_pct, vad.margin_db, vad.onset, vad.offset, vad.min_gap, vad.min_run, vad.pad)
            t2 = time.perf_counter()
            if i:                                                    # the first run is the warm-up
                hs.append((t2 - t0) * 1e3)
                hs_a.append((t1 - t0) * 1e3)
        print(f'host float32 restatement, {a.threads} threads  {spread(hs)}   of which frame energies {spread(hs_a)}', flush=True)
        got, gthr = vad.frame_regions(xd)
        same = [tuple(r) for r in got.tolist()] == reg
        print(f'check: {len(reg)} regions on the host, {len(got)} on the GPU, identical: {same};  thresholds host {[float(v) for v in thr]} '
              f'gpu {list(gthr)};  max |e_gpu - e_host_f32| {np.abs(e_dev.cpu().numpy() - e).max():.3g} dB')
        del xd, e_dev

    # end to end on the test recording
    from oracle import fbank as ofb
    from oracle import models as om
    from ppvector.predict import PPVectorPredictor
    from ppvector.utils.utils import dict_to_object
    cfg = dict_to_object(dict(
        dataset_conf=dict(dataset=dict(min_duration=0.3, max_duration=3, sample_rate=16000, use_dB_normalization=True, target_dB=-20)),
        preprocess_conf=dict(feature_method='Fbank', method_args=dict(sr=16000, n_mels=80)),
        model_conf=dict(model='EcapaTdnn', model_args=dict(embd_dim=192, pooling_type='ASP', channels=[512, 512, 512, 512, 1536]))))
    pred = PPVectorPredictor(cfg, model_path={'0.' + k: v for k, v in om.ecapa_params(80, seed=1000).items()})
    w = ofb.synth_waves(3, 64000, seed=77, lowpass=0.9)
    hush = lambda n, seed: (1e-4 * np.random.RandomState(seed).standard_normal(n)).astype(np.float32)
    rec = np.concatenate([hush(8000, 1), w[0], hush(16000, 2), 0.3 * w[1], hush(8000, 3), 2.0 * w[2][:32000], hush(8000, 4)]).astype(np.float32)
    pred.set_vad(vad)
    regions = pred.vad(rec.copy())
    with_vad = host_clock(lambda: pred.speaker_diarization(rec.copy(), speaker_num=2), a.iters, a.warmup)
    given = host_clock(lambda: pred.speaker_diarization(rec.copy(), speaker_num=2, vad_segments=regions), a.iters, a.warmup)
    print(f'--- speaker_diarization, {rec.size / 16000:g} s, {len(regions)} regions, speaker_num=2 ({a.iters} calls after {a.warmup} warm-up, host clock)')
    print(f'with the detector                  {spread(with_vad)}')
    print(f'given the regions                  {spread(given)}')
    print(clocks(), flush=True)


if __name__ == '__main__':
    main()
