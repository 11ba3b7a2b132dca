"""Score calibration on one MI355X (docs/calibration.md has the table): per shape (D = 192, Nt = Ne = N, synthetic embeddings of N / 16
speakers), after warming every path,
  sums pass      vp_trial_calib_sums_f32, HIP events around the call (its two kernels; no read-back);
  counts pass    vp_trial_ranks_counts_f32 on the same lists, the same way: the nearest kernel over the same walk -- context, no target;
  fit            a whole fit_calibration (the ranks, every evaluation with its 96-byte read-back, minCllr), by the host clock;
  host path      up to --host-max: cosine_score_matrix + the copy of the matrix to the host + the Newton fit of
                 tests/calibration_oracle.py with NumPy sums, by the host clock: what a user has without this module.
Every number is a median with (min, max) of --iters calls (the host path: --host-iters).

Usage: python tools/calibration_probe.py [--sizes 4096,16384] [--iters 20] [--warmup 3] [--host-max 4096] [--host-iters 3]
"""
import argparse
import ctypes
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


def mmm(ts):
    return f'{statistics.median(ts):10.3f} ({min(ts):.3f}, {max(ts):.3f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='4096,16384')
    ap.add_argument('--D', type=int, default=192)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-max', type=int, default=4096)
    ap.add_argument('--host-iters', type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    from ppvector import _native as N
    from ppvector.metric.calibration import fit_calibration
    from ppvector.metric.metrics import TrialRanks, cosine_score_matrix
    from tests import calibration_oracle as oc
    assert torch.cuda.is_available(), 'needs an MI355X'
    print(clocks())
    lib = N.lib()
    for n in [int(s) for s in a.sizes.split(',')]:
        g = torch.Generator(device='cuda').manual_seed(n)
        nspk = max(n // 16, 2)
        cen = torch.nn.functional.normalize(torch.randn((nspk, a.D), generator=g, device='cuda'), dim=1)
        tl = torch.randint(0, nspk, (n,), generator=g, device='cuda')
        el = torch.randint(0, nspk, (n,), generator=g, device='cuda')
        trials = 1.8 * a.D ** -0.25 * cen[tl] + torch.randn((n, a.D), generator=g, device='cuda') / a.D ** 0.5
        enroll = 1.8 * a.D ** -0.25 * cen[el] + torch.randn((n, a.D), generator=g, device='cuda') / a.D ** 0.5
        tl_h, el_h = tl.cpu().numpy(), el.cpu().numpy()
        r = TrialRanks(trials, tl_h, enroll, el_h)
        r.calib_sums(1.0, 0.0)
        ab = (ctypes.c_double * 2)(9.3, -3.5)

        def sums_pass():
            N.check(lib.vp_trial_calib_sums_f32(r._ctx, r._tl.data_ptr(), r.Nt, r._el.data_ptr(), r.Ne, r.D, ctypes.addressof(ab),
                                                r._calib_out.data_ptr(), r._calib_partials.data_ptr(), r._calib_partials.numel(),
                                                r._ws.data_ptr(), r._ws.numel(), N.stream_ptr()), r._ctx)

        def counts_pass():
            N.check(lib.vp_trial_ranks_counts_f32(r._ctx, r._tl.data_ptr(), r.Nt, r._el.data_ptr(), r.Ne, r.D, r.targets.data_ptr(),
                                                  r.NT, r.hist.data_ptr(), r._ws.data_ptr(), r._ws.numel(), N.stream_ptr()), r._ctx)

        def events(f):
            ts = []
            for i in range(a.warmup + a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    ts.append(e0.elapsed_time(e1))
            return ts

        def host(f, iters, warmup):
            ts, out = [], None
            for i in range(warmup + iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = f()
                torch.cuda.synchronize()
                if i >= warmup:
                    ts.append((time.perf_counter() - t0) * 1e3)
            return ts, out

        t_sums, t_counts = events(sums_pass), events(counts_pass)
        t_fit, (cal, info) = host(lambda: fit_calibration(enroll, el_h, trials, tl_h), a.iters, a.warmup)
        print(f'N = {n}: NT {info["NT"]} NN {info["NN"]}; ms, median (min, max)')
        print(f'  sums pass   {mmm(t_sums)}   {n * n / statistics.median(t_sums) / 1e6:.2f} G pairs / s')
        print(f'  counts pass {mmm(t_counts)}   sums / counts = {statistics.median(t_sums) / statistics.median(t_counts):.2f}')
        print(f'  fit         {mmm(t_fit)}   {info["iterations"]} steps, {info["evaluations"]} evaluations; a {cal.a:.6f} b {cal.b:.6f} '
              f'Cllr {info["cllr"]:.6f} min {info["min_cllr"]:.6f} raw {info["cllr_raw"]:.6f}')
        if n <= a.host_max:
            target = tl_h[:, None] == el_h[None, :]

            def host_path():
                s = cosine_score_matrix(trials, enroll).cpu().numpy()
                return oc.fit(s, target, exact=False)

            t_host, got = host(host_path, a.host_iters, 1)
            print(f'  host path   {mmm(t_host)}   a {got[0]:.6f} b {got[1]:.6f} in {got[2]} steps; host / fit = '
                  f'{statistics.median(t_host) / statistics.median(t_fit):.1f}')
    print(clocks())


if __name__ == '__main__':
    main()
