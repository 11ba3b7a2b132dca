"""evaluate_trials on one MI355X: the 'matrix' scorer (the (Nt, Ne) cosine matrix + the reference's host arithmetic over all pairs)
against the 'fused' one (csrc/trial_ranks.hip: sorted targets + counts, no matrix), on the same embeddings in the same process,
alternating call by call (reported, not gated).

Data: seeded; Ne / 3 speakers with 3 enrolments each, every trial from a uniformly drawn enrolled speaker; an embedding is
1.8 D^(-1/4) x (unit Gaussian centroid) + N(0, 1/D) noise.  A call is evaluate_trials from device embeddings to three Python floats,
timed on the host clock between two synchronisations.  Sizes given with --fused-only run the fused scorer alone.

Usage: python tools/trial_ranks_probe.py [--sizes 17777x196,20000x5000] [--fused-only 100000x10000] [--iters 10] [--fused-iters 5]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'voiceprintrecognition-paddlepaddle_amd')):
    sys.path.insert(0, p)


def mmm(ts):
    return f'{statistics.median(ts):10.2f} ({min(ts):.2f}, {max(ts):.2f})'


def sizes(text):
    return [tuple(int(v) for v in s.split('x')) for s in text.split(',') if s]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='17777x196,20000x5000')
    ap.add_argument('--fused-only', default='100000x10000')
    ap.add_argument('--D', type=int, default=192)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--fused-iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    import torch
    import ppvector
    from ppvector.metric import metrics as M
    assert torch.cuda.is_available(), 'needs an MI355X: the engine has no CPU fallback'
    dev = torch.device('cuda', 0)
    D = a.D

    def data(Nt, Ne):
        gen = torch.Generator(device=dev).manual_seed(Nt * 31 + Ne)
        nspk = max(Ne // 3, 1)
        cen = torch.randn(nspk, D, generator=gen, device=dev)
        cen /= cen.norm(dim=1, keepdim=True)
        el = torch.arange(Ne, device=dev) % nspk
        tl = torch.randint(0, nspk, (Nt,), generator=gen, device=dev)
        emb = lambda lab: 1.8 * D ** -0.25 * cen[lab] + torch.randn(len(lab), D, generator=gen, device=dev) / D ** 0.5
        return emb(el), el.cpu().numpy(), emb(tl), tl.cpu().numpy()

    def call(scorer, args):
        ppvector.set_trial_scorer(scorer)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = M.evaluate_trials(*args)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, r
        finally:
            ppvector.set_trial_scorer('matrix')

    print(f'D={D}; ms per evaluate_trials call, median (min, max), after {a.warmup} warm-up calls of each scorer', flush=True)
    for (Nt, Ne), scorers, iters in [(s, ('matrix', 'fused'), a.iters) for s in sizes(a.sizes)] + \
                                    [(s, ('fused',), a.fused_iters) for s in sizes(a.fused_only)]:
        args = data(Nt, Ne)
        times = {s: [] for s in scorers}
        last = {}
        for i in range(a.warmup + iters):
            for s in scorers:                               # the scorers alternate call by call
                t, last[s] = call(s, args)
                if i >= a.warmup:
                    times[s].append(t)
                print(f'  {Nt}x{Ne} call {i} {s} {t:.1f} ms', flush=True)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() / 2 ** 20
        for s in scorers:
            eer, dcf, thr = last[s]
            print(f'Nt={Nt} Ne={Ne} pairs={Nt * Ne:.3g} {s:6s} {mmm(times[s])} ms  ({iters} calls)  EER {eer!r} minDCF {dcf!r} '
                  f'threshold {thr!r}', flush=True)
        if len(scorers) == 2:
            m, f = last['matrix'], last['fused']
            print(f'  fused - matrix: EER {f[0] - m[0]:+.3e} minDCF {f[1] - m[1]:+.3e} threshold {f[2] - m[2]:+.3e}; '
                  f'speed-up {statistics.median(times["matrix"]) / statistics.median(times["fused"]):.1f}x', flush=True)
        print(f'  peak device memory allocated so far {peak:.0f} MiB', flush=True)
        del args
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
