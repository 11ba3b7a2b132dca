"""Top-N cohort statistics on one MI355X: cohort_stats (csrc/cohort_stats.hip: selection by digit counting, no (Q, C) matrix) against
what a user has without it, cosine_score_matrix + torch.topk + mean / std on the device, on the same embeddings in the same process,
alternating call by call (reported, not gated).

Data: the recipe of tools/trial_ranks_probe.py, seeded; the cohort is C embeddings of C / 3 speakers, the Q embeddings are drawn from
the same speakers; an embedding is 1.8 D^(-1/4) x (unit Gaussian centroid) + N(0, 1/D) noise.  A call goes from device embeddings to
the two device vectors (mean, std), timed on the host clock between two synchronisations.  Sizes given with --fused-only run
cohort_stats alone.

Usage: python tools/score_norm_probe.py [--sizes 17777x5994,20000x10000] [--fused-only 100000x10000] [--iters 10] [--fused-iters 5]
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
    ap.add_argument('--sizes', default='17777x5994,20000x10000')
    ap.add_argument('--fused-only', default='100000x10000')
    ap.add_argument('--D', type=int, default=192)
    ap.add_argument('--top-n', type=int, default=300)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--fused-iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    import torch
    from ppvector.metric import metrics as M
    from ppvector.metric.score_norm import cohort_stats
    assert torch.cuda.is_available(), 'needs an MI355X: the engine has no CPU fallback'
    dev = torch.device('cuda', 0)
    D, top_n = a.D, a.top_n

    def data(Q, C):
        gen = torch.Generator(device=dev).manual_seed(Q * 31 + C)
        nspk = max(C // 3, 1)
        cen = torch.randn(nspk, D, generator=gen, device=dev)
        cen /= cen.norm(dim=1, keepdim=True)
        emb = lambda lab: 1.8 * D ** -0.25 * cen[lab] + torch.randn(len(lab), D, generator=gen, device=dev) / D ** 0.5
        return emb(torch.randint(0, nspk, (Q,), generator=gen, device=dev)), emb(torch.arange(C, device=dev) % nspk)

    def topk(x, cohort):                                    # the alternative: the (Q, C) matrix, a partial sort per row
        top = torch.topk(M.cosine_score_matrix(x, cohort), min(top_n, cohort.shape[0]), dim=1).values.double()
        mean = top.mean(dim=1)
        return mean.float(), ((top * top).mean(dim=1) - mean * mean).clamp_min(0).sqrt().float()

    methods = {'topk': topk, 'cohort_stats': lambda x, cohort: cohort_stats(x, cohort, top_n)}

    def call(name, args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = methods[name](*args)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    print(f'D={D} top_n={top_n}; ms per call, median (min, max), after {a.warmup} warm-up calls of each method', flush=True)
    for (Q, C), names, iters in [(s, ('topk', 'cohort_stats'), a.iters) for s in sizes(a.sizes)] + \
                                [(s, ('cohort_stats',), a.fused_iters) for s in sizes(a.fused_only)]:
        args = data(Q, C)
        times = {n: [] for n in names}
        last = {}
        for i in range(a.warmup + iters):
            for n in names:                                 # the methods alternate call by call
                t, last[n] = call(n, args)
                if i >= a.warmup:
                    times[n].append(t)
                print(f'  {Q}x{C} call {i} {n} {t:.2f} ms', flush=True)
        for n in names:
            print(f'Q={Q} C={C} pairs={Q * C:.3g} {n:12s} {mmm(times[n])} ms  ({iters} calls)', flush=True)
        if len(names) == 2:
            dm = (last['topk'][0] - last['cohort_stats'][0]).abs().max().item()
            ds = (last['topk'][1] - last['cohort_stats'][1]).abs().max().item()
            print(f'  largest |difference| of the two methods: mean {dm:.3e} std {ds:.3e}; speed-up '
                  f'{statistics.median(times["topk"]) / statistics.median(times["cohort_stats"]):.2f}x', flush=True)
        print(f'  peak device memory allocated so far {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB', flush=True)
        del args, last
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
