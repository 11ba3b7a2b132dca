"""Cost of the sample-rate conversion on the GPU (ppvector/data_utils/wave_batch.py resample_waves, csrc/resample.hip) beside the host
function it replaces and the training step it feeds.  B = 64 utterances of 6 s at 8 kHz, 44.1 kHz and 48 kHz, and one 30-minute 48 kHz
recording, all to 16 kHz; HIP events around the whole Python call (pointer tables and output allocation included: what the trainer
pays; the phase table is cached after the first call), 5 warm-up calls, median of 30.  Host: wall time of
scipy.signal.resample_poly on the same float32 inputs, one after the other on 1 thread and through a pool of 16 threads (the loader's
workers), median of 5.  The training step (TDNN and ECAPA-TDNN, f32 engine, 3 s features, forward + backward + Adam: code this
change does not touch) is timed as tools/augment_probe.py times it.  Usage: python tools/resample_probe.py [B]"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'voiceprintrecognition-paddlepaddle_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy.signal import resample_poly  # noqa: E402
from oracle import models as om  # noqa: E402
from ppvector.data_utils.wave_batch import resample_ratio, resample_waves  # noqa: E402
from ppvector.models.ecapa_tdnn import EcapaTdnn  # noqa: E402
from ppvector.models.tdnn import TDNN  # noqa: E402
from tools.augment_probe import step_time, timed  # noqa: E402

SR = 16000


def wall(fn, reps=5):
    """Median wall milliseconds of fn()."""
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t))
    return sorted(ms)[len(ms) // 2]


def case(B, rate, seconds, seed=7, gpu_reps=30, host_reps=5):
    rng = np.random.RandomState(seed)
    xs = [(0.1 * rng.standard_normal(int(seconds * rate))).astype(np.float32) for _ in range(B)]
    waves = [torch.from_numpy(x).cuda() for x in xs]
    up, down = resample_ratio(rate, SR)
    t_gpu = timed(lambda: resample_waves(waves, [rate] * B, SR), reps=gpu_reps)
    t_1 = wall(lambda: [resample_poly(x, up, down) for x in xs], host_reps)
    with ThreadPoolExecutor(max_workers=16) as pool:
        t_16 = wall(lambda: list(pool.map(lambda x: resample_poly(x, up, down), xs)), host_reps)
    return t_gpu, t_1, t_16


if __name__ == '__main__':
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    batch_ms = {}
    for rate in (8000, 44100, 48000):
        g, h1, h16 = case(B, rate, 6.0)
        batch_ms[rate] = g
        print(f'B={B} utterances 6 s at {rate} Hz -> {SR} Hz (up, down) = {resample_ratio(rate, SR)}: resample_waves {g:.3f} ms   '
              f'host resample_poly {h1:.1f} ms on 1 thread, {h16:.1f} ms on 16 threads', flush=True)
    g, h1, h16 = case(1, 48000, 1800.0, gpu_reps=10, host_reps=3)
    print(f'one 30-minute recording at 48000 Hz -> {SR} Hz: resample_waves {g:.3f} ms   host resample_poly {h1:.1f} ms on 1 thread '
          f'({h16:.1f} ms through the pool: one recording is one task)', flush=True)
    for name, cls, params in (('TDNN', TDNN, om.tdnn_params(80)), ('EcapaTdnn', EcapaTdnn, om.ecapa_params(80))):
        ms = step_time(cls, params, B)
        print(f'{name} training step f32 B={B}: {ms:.2f} ms; resample_waves of the batch is ' +
              ', '.join(f'{100 * batch_ms[r] / ms:.1f} % ({r} Hz)' for r in batch_ms) + ' of it', flush=True)
