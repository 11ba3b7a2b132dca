"""The diarization's eigen step on one MI355X: the GPU spectral solver against the two things it could have been (reported, not gated).

For every N of --sizes (default 1024 4096 8192): planted speakers at D = 192 (tests/eigs_oracle.py: --speakers centres ~ N(0, I), point =
centre + --noise * N(0, I)), the Laplacian from the engine (SpectralCluster().laplacian), then in this one process:
  gpu solver         smallest_eigenpairs(L, 16) at its defaults: HIP events around the whole call -- init, every round, the read-back of
                     the residuals after each round and the download of the 16 vectors -- the median of --iters calls after --warmup;
                     rounds and block products L X spent;
  scipy f32, host    scipy.linalg.eigh of the f32 Laplacian under --threads threads: what SpectralCluster.get_spec_embs runs by default
                     (the download of L not included); host clock, the median of --host-iters runs (one run from --host-once-from up);
  torch eigh, gpu    torch.linalg.eigh of the same device tensor, vectors included, HIP events, the same --iters / --warmup: the
                     plumbing alternative.
The solver's 16 eigenvalues are compared with scipy's on the way.  The clocks are printed with the numbers.

Usage: python tools/eigs_probe.py [--sizes 1024 4096 8192] [--iters 10] [--warmup 2] [--host-iters 3] [--threads 16] [--log FILE]
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
    ap.add_argument('--sizes', type=int, nargs='+', default=[1024, 4096, 8192])
    ap.add_argument('--speakers', type=int, default=8)
    ap.add_argument('--noise', type=float, default=1.0)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--host-iters', type=int, default=3)
    ap.add_argument('--host-once-from', type=int, default=8192)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--log', default=None)
    a = ap.parse_args()
    for v in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):
        os.environ[v] = str(a.threads)
    import numpy as np
    import scipy.linalg
    import torch
    from tests import eigs_oracle as oe
    from ppvector.infer_utils.speaker_diarization import SpectralCluster, smallest_eigenpairs
    torch.set_num_threads(a.threads)
    assert torch.cuda.is_available(), 'needs an MI355X: the engine has no CPU fallback'
    log = open(a.log, 'w') if a.log else None

    def say(text=''):
        print(text, flush=True)
        if log:
            log.write(text + '\n')
            log.flush()

    def gpu_median(fn, iters, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            ts.append(s.elapsed_time(e))
        return statistics.median(ts), min(ts), max(ts)

    say(f'python tools/eigs_probe.py {" ".join(sys.argv[1:])}')
    say(torch.cuda.get_device_name(0))
    say(clocks())
    for n in a.sizes:
        x, _ = oe.planted(n, a.speakers, a.noise, 0)
        L = SpectralCluster().laplacian(x)
        lam, _, info = smallest_eigenpairs(L, 16)
        say(f'\nN={n} D=192 speakers={a.speakers} noise={a.noise}: solver rounds {info.rounds}, block products {info.products}, converged '
            f'{info.converged}, worst residual {info.residuals.max() / info.sigma:.3g} sigma')
        med, lo, hi = gpu_median(lambda: smallest_eigenpairs(L, 16), a.iters, a.warmup)
        say(f'  gpu solver (k=16, read-backs and vector download included)  median {med:10.3f} ms   (min {lo:.3f}, max {hi:.3f}; '
            f'{a.iters} calls after {a.warmup}, HIP events)')
        tmed, tlo, thi = gpu_median(lambda: torch.linalg.eigh(L), max(1, a.iters // 2), 1)
        say(f'  torch.linalg.eigh on the GPU, f32                            median {tmed:10.3f} ms   (min {tlo:.3f}, max {thi:.3f}; '
            f'{max(1, a.iters // 2)} calls after 1, HIP events)')
        Lh = L.cpu().numpy()
        runs = 1 if n >= a.host_once_from else a.host_iters
        hs = []
        for i in range(runs + (0 if runs == 1 else 1)):                # one warm-up where there is more than one run
            t0 = time.perf_counter()
            lam32 = scipy.linalg.eigh(Lh)[0]
            hs.append((time.perf_counter() - t0) * 1e3)
        hs = hs[-runs:]
        say(f'  scipy.linalg.eigh on the host, f32, {a.threads} threads                median {statistics.median(hs):10.1f} ms   '
            f'(min {min(hs):.1f}, max {max(hs):.1f}; {runs} run(s), host clock)')
        say(f'  solver / scipy-host {statistics.median(hs) / med:.1f}x   solver / torch-gpu {tmed / med:.1f}x   '
            f'max |lambda - scipy f32 lambda| over the 16: {np.abs(lam - lam32[:16]).max() / (oe.EPS * lam32[-1]):.3g} eps lambda_max')
    say()
    say(clocks())


if __name__ == '__main__':
    main()
