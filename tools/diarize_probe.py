"""Clustering front half of the diarization on one MI355X against the host (reported, not gated).

GPU: vp_affinity_prune_f32 + vp_laplacian_f32 at N x D (default 4096 x 192: about 50 minutes of speech in 1.5 s windows every 0.75 s),
each call timed with HIP events after a warm-up, the median of --iters calls; the two kernels also one by one.
Host, same machine: the float64 restatement of tests/diarization_oracle.py (cosine affinity, per-row pruning, symmetrisation,
Laplacian) under --threads BLAS / OpenMP threads, the median of --host-iters runs by the host clock.  The per-row selection there is a
NumPy sort, as the reference's is an argsort; the reference itself (sklearn + a Python loop over the rows) is not in this tree.
The GPU result is compared with the restatement on the way (rows whose threshold gap is under 1e-5 set aside).  The clocks are printed
with the numbers.

Usage: python tools/diarize_probe.py [--N 4096] [--D 192] [--iters 30] [--warmup 5] [--host-iters 5] [--threads 16]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--N', type=int, default=4096)
    ap.add_argument('--D', type=int, default=192)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--host-iters', type=int, default=5)
    ap.add_argument('--threads', type=int, default=16)
    a = ap.parse_args()
    for v in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):
        os.environ[v] = str(a.threads)
    import numpy as np
    import torch
    from tests import diarization_oracle as od
    from ppvector.infer_utils.speaker_diarization import SpectralCluster, affinity_prune, laplacian
    torch.set_num_threads(a.threads)
    assert torch.cuda.is_available(), 'needs an MI355X: the engine has no CPU fallback'
    x = np.random.RandomState(0).standard_normal((a.N, a.D)).astype(np.float32)
    k = SpectralCluster().n_elems(a.N)
    xd = torch.from_numpy(x).cuda()
    print(clocks(), flush=True)

    def gpu_median(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            ts.append(s.elapsed_time(e))
        return statistics.median(ts), min(ts), max(ts)

    P = affinity_prune(xd, k)
    both = gpu_median(lambda: laplacian(affinity_prune(xd, k)))
    aff = gpu_median(lambda: affinity_prune(xd, k))
    lap = gpu_median(lambda: laplacian(P))
    print(f'N={a.N} D={a.D} n_elems={k}  ({a.iters} calls after {a.warmup} warm-up, HIP events, output and workspace allocation included)')
    for name, (med, lo, hi) in (('affinity_prune + laplacian', both), ('affinity_prune', aff), ('laplacian', lap)):
        print(f'gpu  {name:28s} median {med:8.3f} ms   (min {lo:.3f}, max {hi:.3f})', flush=True)

    def host():
        return od.laplacian(od.prune(od.cosine_affinity(x), k))

    host()
    hs = []
    for _ in range(a.host_iters):
        t0 = time.perf_counter()
        Lh = host()
        hs.append((time.perf_counter() - t0) * 1e3)
    print(f'host float64 restatement, {a.threads} threads: median {statistics.median(hs):8.1f} ms   (min {min(hs):.1f}, max {max(hs):.1f}; '
          f'{a.host_iters} runs after 1 warm-up, host clock)', flush=True)
    print(clocks(), flush=True)

    S = od.cosine_affinity(x)
    srt = np.sort(S, axis=1)
    clear = (srt[:, k] - srt[:, k - 1]) >= 1e-5 if k > 0 else np.ones(a.N, bool)
    Pg = P.cpu().numpy()
    same = ((Pg != 0) == (od.prune(S, k) != 0)).all(axis=1)
    Lg = laplacian(P).cpu().numpy()
    print(f'check: rows off the 1e-5 threshold gap {int(clear.sum())} / {a.N}, of them with the restatement\'s surviving set '
          f'{int((same & clear).sum())};  max |L - float64 L of the same P| {np.abs(Lg - od.laplacian(Pg)).max():.3g}')
    del Lh


if __name__ == '__main__':
    main()
