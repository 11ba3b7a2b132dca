"""1:N speaker search on one MI355X: the resident gallery (SpeakerGallery.search = vp_gallery_topk_f32) against the path it replaced,
on the same data in the same process, alternating (reported, not gated).

Per shape (D = 192; U users with one utterance each; Q queries; k results), after warming both sides:
  search         SpeakerGallery.search, HIP events around the call (its two kernels; the output tensors are allocated inside);
  search + read  the same plus the copy of (idx, score) to the host, by the host clock: what PPVectorPredictor.recognition waits for;
  gemm path      the parent's kernel path on PREPARED means: vp_cosine_scores_f32 (Q, U) + the copy of the score matrix to the host +
                 np.argmax, by the host clock (k does not enter: it only ever gave the single best);
  parent body    the parent's whole recognition body -- sorted(set(names)), the per-user mean rebuild in Python, the upload of the means,
                 the gemm path -- by the host clock, in full up to --body-max-users users; above that the mean rebuild is timed for
                 --body-sample users and scaled by U / sample (it is a loop of U independent list scans), and marked "extrapolated".
For Q <= 32 the search's U D 4 bytes over its event time are given as a share of the HBM peak, for Q = 256 its 2 Q U D flop as a share
of the f32 matrix-core peak (docs: MI355X 8 TB/s, 157.3 TFLOP/s), with the larger share named as the bound that applies.
Every number is a median with (min, max) of --iters calls.

Usage: python tools/gallery_probe.py [--users 1000,100000,1000000] [--queries 1,32,256] [--k 1,10] [--iters 20] [--warmup 3]
       python tools/gallery_probe.py --norm [--users 1000,100000] [--queries 1,32,256] [--k 1] [--cohort 6000] [--top-n 300]
       (the search on normalised scores: norm_probe's docstring)
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

HBM_PEAK = 8.0e12          # bytes / s
MFMA_F32_PEAK = 157.3e12   # flop / s


def clocks():
    try:
        return subprocess.run(['amd-smi', 'metric', '--clock'], capture_output=True, text=True, timeout=30).stdout.strip()
    except Exception as e:      # the tool is optional on the machine
        return f'(amd-smi unavailable: {e})'


def mmm(ts):
    return f'{statistics.median(ts):9.3f} ({min(ts):.3f}, {max(ts):.3f})'


def norm_probe(a):
    """--norm: the search on normalised scores (docs/gallery.md).  Per (U, Q), k = --k's first value, C = --cohort rows, top_n = --top-n,
    five sides alternating call by call in one process, each timed by HIP events and by the host clock between two synchronisations:
      split      SpeakerGallery.search with a score norm set: query statistics from vp_cohort_stats_split_f32 + r + the normalised search;
      unsplit    (a) the same path with the query statistics from vp_cohort_stats_f32 (ScoreNorm.mean_r);
      matrix     (b) what there was before: cosine_score_matrix (Q, U) + vp_score_norm_apply_f32 + torch.topk, with the query statistics
                 from ScoreNorm.mean_r and the rows' statistics PREPARED (ScoreNorm.normalise itself recomputes them at every call);
      z search   vp_gallery_topk_norm_f32 alone on prepared statistics;
      cos search vp_gallery_topk_f32 alone (SpeakerGallery.search without a score norm): the z epilogue is the difference of the two."""
    import torch
    from ppvector import _native as N
    from ppvector.infer_utils.gallery import SpeakerGallery
    from ppvector.metric.metrics import cosine_score_matrix
    from ppvector.metric.score_norm import ScoreNorm, recip_std
    dev = torch.device('cuda', 0)
    D, k = a.D, int(a.k.split(',')[0])
    print(clocks(), flush=True)
    print(f'D={D} C={a.cohort} top_n={a.top_n} k={k}; ms, median (min, max) of {a.iters} calls after {a.warmup} warm-up calls of every '
          f'side; the sides alternate call by call; "ev" HIP events, "host" the host clock between two synchronisations')
    gen = torch.Generator(device=dev).manual_seed(7)
    spk = torch.randn(a.cohort // 3 + 1, D, generator=gen, device=dev)             # three cohort rows a speaker
    cohort = spk.repeat_interleave(3, 0)[:a.cohort] * 1.8 * D ** -0.25 + torch.randn(a.cohort, D, generator=gen, device=dev)
    sn = ScoreNorm(cohort, a.top_n)
    lib, ctx = N.lib(), N.ctx(dev)
    for U in [int(u) for u in a.users.split(',')]:
        feats = spk[torch.randint(0, spk.shape[0], (U,), generator=gen, device=dev)] * 1.8 * D ** -0.25 + torch.randn(U, D, generator=gen, device=dev)
        names = [f'u{i}' for i in range(U)]
        gal, plain = SpeakerGallery(D, dev), SpeakerGallery(D, dev)
        gal.rebuild(names, feats)
        plain.rebuild(names, feats)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gal.set_score_norm(sn)
        torch.cuda.synchronize()
        print(f'\nU={U}: set_score_norm (the rows\' statistics, vp_cohort_stats_f32 over {U} x {a.cohort}) {(time.perf_counter() - t0) * 1e3:.1f} ms', flush=True)
        cen, um, ur = gal.centroids, gal._mean, gal._r
        for Q in [int(q) for q in a.queries.split(',')]:
            q = (feats[torch.randint(0, U, (Q,), generator=gen, device=dev)] + 0.3 * torch.randn(Q, D, generator=gen, device=dev)).contiguous()
            ws = torch.empty(lib.vp_gallery_topk_workspace_bytes(Q, U, D, k), dtype=torch.uint8, device=dev)

            def z_search(qm, qr):
                idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
                z = torch.empty((Q, k), dtype=torch.float32, device=dev)
                N.check(lib.vp_gallery_topk_norm_f32(ctx, q.data_ptr(), Q, cen.data_ptr(), U, D, k, qm.data_ptr(), qr.data_ptr(),
                                                     um.data_ptr(), ur.data_ptr(), idx.data_ptr(), z.data_ptr(), ws.data_ptr(), ws.numel(),
                                                     N.stream_ptr()), ctx)
                return idx, z

            def matrix():
                s = cosine_score_matrix(q, cen).contiguous()
                qm, qr = sn.mean_r(q)
                N.check(lib.vp_score_norm_apply_f32(ctx, s.data_ptr(), Q, U, qm.data_ptr(), qr.data_ptr(), um.data_ptr(), ur.data_ptr(),
                                                    N.stream_ptr()), ctx)
                z, idx = torch.topk(s, k, dim=1)
                return idx, z

            prepared = sn.mean_r_queries(q)
            sides = {'split': lambda: gal.search(q, k), 'unsplit': lambda: z_search(*sn.mean_r(q)), 'matrix': matrix,
                     'z search': lambda: z_search(*prepared), 'cos search': lambda: plain.search(q, k)}
            for _ in range(a.warmup):
                for fn in sides.values():
                    fn()
            ev, host, last = {n: [] for n in sides}, {n: [] for n in sides}, {}
            iters = a.iters if Q * U <= 32 * 1000000 else max(5, a.iters // 2)
            for _ in range(iters):
                for name, fn in sides.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    last[name] = fn()
                    e1.record()
                    torch.cuda.synchronize()
                    host[name].append((time.perf_counter() - t0) * 1e3)
                    ev[name].append(e0.elapsed_time(e1))
            same = {n: int((last[n][0][:, 0].long() == last['split'][0][:, 0].long()).sum()) for n in ('unsplit', 'matrix', 'z search')}
            dz = float((last['unsplit'][1] - last['split'][1]).abs().max())
            for name in sides:
                print(f'U={U:8d} Q={Q:4d} {name:10s} ev {mmm(ev[name])}   host {mmm(host[name])}', flush=True)
            for clock, t in (('ev', ev), ('host', host)):
                gain = statistics.median(t['unsplit']) - statistics.median(t['split'])
                width = max(t['unsplit']) - min(t['unsplit'])
                print(f'U={U:8d} Q={Q:4d} [{clock}] unsplit - split medians {gain:+.3f} ms against the unsplit side\'s own (min, max) width '
                      f'{width:.3f} ms: split {"below by more than the width" if gain > width else "NOT below by more than the width"}')
            print(f'U={U:8d} Q={Q:4d} same best row as split: {same} of {Q}; largest |z unsplit - z split| {dz:.3e}  ({iters} calls)', flush=True)
        del gal, plain, feats
    print(clocks(), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--norm', action='store_true', help='the search on normalised scores instead of the cosine search')
    ap.add_argument('--cohort', type=int, default=6000)
    ap.add_argument('--top-n', type=int, default=300)
    ap.add_argument('--users', default='1000,100000,1000000')
    ap.add_argument('--queries', default='1,32,256')
    ap.add_argument('--k', default='1,10')
    ap.add_argument('--D', type=int, default=192)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--body-max-users', type=int, default=2000)
    ap.add_argument('--body-sample', type=int, default=200)
    ap.add_argument('--body-users', default='1000,100000')
    a = ap.parse_args()
    import numpy as np
    import torch
    if a.norm:
        assert torch.cuda.is_available(), 'needs an MI355X: the engine has no CPU fallback'
        return norm_probe(a)
    from ppvector.infer_utils.gallery import SpeakerGallery
    from ppvector.metric.metrics import cosine_score_matrix
    assert torch.cuda.is_available(), 'needs an MI355X: the engine has no CPU fallback'
    dev = torch.device('cuda', 0)
    D = a.D
    print(clocks(), flush=True)
    print(f'D={D}; ms, median (min, max) of {a.iters} calls after {a.warmup} warm-up calls of every shape; the two sides alternate call by call')

    def sync_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    for U in [int(u) for u in a.users.split(',')]:
        gen = torch.Generator(device=dev).manual_seed(U)
        feats = torch.randn(U, D, generator=gen, device=dev)
        names = [f'u{i}' for i in range(U)]
        gal = SpeakerGallery(D, dev)
        t, _ = sync_ms(lambda: gal.rebuild(names, feats))
        print(f'\nU={U}: rebuild of the gallery (host name map + one kernel) {t:.1f} ms', flush=True)
        for Q in [int(q) for q in a.queries.split(',')]:
            pick = torch.randint(0, U, (Q,), generator=gen, device=dev)
            q = feats[pick] + 0.3 * torch.randn(Q, D, generator=gen, device=dev)

            def gemm_path():
                s = cosine_score_matrix(q, feats).cpu().numpy()
                return np.argmax(s, axis=1)

            iters = a.iters if Q * U <= 32 * 1000000 else max(3, a.iters // 4)
            for k in [int(x) for x in a.k.split(',')]:
                def search():
                    return gal.search(q, k)

                def search_read():
                    i, s = gal.search(q, k)
                    return i.cpu().numpy(), s.cpu().numpy()

                for _ in range(a.warmup):
                    search_read()
                    gemm_path()
                ev, host, old = [], [], []
                agree = None
                for _ in range(iters):
                    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    s0.record()
                    search()
                    s1.record()
                    torch.cuda.synchronize()
                    ev.append(s0.elapsed_time(s1))
                    t, (idx, _) = sync_ms(search_read)
                    host.append(t)
                    t, best = sync_ms(gemm_path)
                    old.append(t)
                    agree = int((idx[:, 0] == best).sum())
                med = statistics.median(ev) * 1e-3
                if Q <= 32:
                    share = f'{U * D * 4 / med / HBM_PEAK * 100:5.1f}% of HBM peak ({U * D * 4 / med / 1e12:.2f} TB/s)'
                else:
                    bw, fl = U * D * 4 / med / HBM_PEAK, 2.0 * Q * U * D / med / MFMA_F32_PEAK
                    share = (f'{fl * 100:5.1f}% of f32 MFMA peak, {bw * 100:5.1f}% of HBM peak counting ONE read of the gallery '
                             f'-> nearer the {"matrix-core" if fl > bw else "memory"} bound')
                print(f'U={U:8d} Q={Q:4d} k={k:3d}  search {mmm(ev)}   search + read {mmm(host)}   gemm path {mmm(old)}   '
                      f'[{share}]  same best user {agree}/{Q}  ({iters} calls)', flush=True)
        del gal, feats

    # the query as a user of the parent saw it: the whole recognition body, one query
    print('\nparent recognition body (host clock, one query), against search + read at the same U:')
    for U in [int(u) for u in a.body_users.split(',')]:
        rs = np.random.RandomState(U)
        audio_feature = rs.standard_normal((U, D)).astype(np.float32)
        users_name = [f'u{i}' for i in range(U)]
        feat = (audio_feature[rs.randint(U)] + 0.3 * rs.standard_normal(D)).astype(np.float32)
        gal = SpeakerGallery(D, dev)
        gal.rebuild(users_name, audio_feature)
        full = U <= a.body_max_users
        n_mean = U if full else a.body_sample

        def body():
            t0 = time.perf_counter()
            users = sorted(set(users_name))
            t1 = time.perf_counter()
            means = np.stack([audio_feature[[i for i, n in enumerate(users_name) if n == u]].mean(axis=0) for u in users[:n_mean]])
            t2 = time.perf_counter()
            if not full:
                means = audio_feature            # the same values (one utterance per user): what the rest of the body works on
            s = cosine_score_matrix(torch.from_numpy(feat[None]).to(dev), torch.from_numpy(means.astype(np.float32)).to(dev)).cpu().numpy()[0]
            i = int(np.argmax(s))
            t3 = time.perf_counter()
            return (t1 - t0) * 1e3, (t2 - t1) * 1e3 * (U / n_mean), (t3 - t2) * 1e3, i

        def new():
            i, s = gal.search(torch.from_numpy(feat[None]).to(dev), 1)
            return int(i.cpu()[0, 0]), float(s.cpu()[0, 0])

        body()
        new()
        parts, news = [], []
        for _ in range(5 if full else 3):
            parts.append(body())
            t, _ = sync_ms(new)
            news.append(t)
        tot = [p[0] + p[1] + p[2] for p in parts]
        print(f'U={U:8d}  parent body {mmm(tot)} ms = sort {statistics.median(p[0] for p in parts):.2f} + mean rebuild '
              f'{statistics.median(p[1] for p in parts):.1f}{"" if full else f" (EXTRAPOLATED from {n_mean} of {U} users)"} + upload, gemm, '
              f'copy, argmax {statistics.median(p[2] for p in parts):.2f};   gallery search + read {mmm(news)} ms', flush=True)
    print(clocks(), flush=True)


if __name__ == '__main__':
    main()
