"""Pooling-statistics kernels (csrc/pooling_stats.hip) timed alone, two builds of libvpmi against each other: the attentive forward and
backward at the ECAPA training shape (B = 256, C = 1536; T = 150, 300, 333: one per dispatch bucket; f32 and bf16 logits), the time
statistics forward + backward there, and the many-frames forward on a ResNetSE layer-1 feature map (B = 32, 298 x 80 positions, C = 64).
Device events; half a second of GPU work first, then per call ten warm-up calls and the median of five batches of 20.  The driver
starts one process per library and round, A and B alternating (VPMI_LIB selects the build), and prints per call the median of each and A's own round-to-round spread: B's median belongs inside it.
Usage: python tools/pooling_probe.py LIB_A LIB_B [rounds = 7]        (python tools/pooling_probe.py --child: one round, one JSON line)"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(reps=20):
    sys.path.insert(0, os.path.join(ROOT, 'voiceprintrecognition-paddlepaddle_amd'))
    import torch
    from ppvector import _native as N
    lib, ctx, st = N.lib(), N.ctx(0), N.stream_ptr()
    bf = torch.bfloat16

    def timed(fn):
        """Median of five batches of `reps` calls behind ten warm-up calls.  (One 4 ms batch behind three calls, in a process that had
        just started, read the SAME kernel 8 % apart in two libraries that differ in which code object holds it; timed late in a
        process the two agree to 0.5 %.)"""
        for _ in range(10):
            N.check(fn(), ctx)
        batches = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            batches.append(a.elapsed_time(b) / reps * 1e3)
        return statistics.median(batches)

    busy = torch.randn(4096, 4096, device='cuda')          # half a second of work before the first timed call
    t0 = time.time()
    while time.time() - t0 < 0.5:
        for _ in range(20):
            busy @ busy
        torch.cuda.synchronize()

    out = {}
    g = torch.Generator(device='cuda').manual_seed(1)
    B, C = 256, 1536
    for T in (150, 300, 333):
        x = torch.randn(B * T, C, device='cuda', generator=g)
        e = torch.randn(B * T, C, device='cuda', generator=g)
        dp = torch.randn(B, 2 * C, device='cuda', generator=g)
        pooled, de, dx = torch.empty(B, 2 * C, device='cuda'), torch.empty(B * T, C, device='cuda'), torch.empty(B * T, C, device='cuda')
        p = [t.data_ptr() for t in (e, x, pooled, dp, de, dx)]
        out[f'asp fwd f32 T{T}'] = timed(lambda: lib.vp_asp_softmax_stats(ctx, N.VP_F32, p[0], p[1], C, 0, B, T, C, 1e-12, p[2], st))
        out[f'asp bwd f32 T{T}'] = timed(lambda: lib.vp_attn_stats_bwd_f32(ctx, p[0], p[1], C, p[2], p[3], B, T, C, 1e-12, p[4], p[5], C, st))
        if T <= 320:
            e16, de16 = e.to(bf), torch.empty(B * T, C, device='cuda', dtype=bf)
            q = (e16.data_ptr(), de16.data_ptr())
            out[f'asp fwd l16 T{T}'] = timed(lambda: lib.vp_asp_softmax_stats_l16(ctx, q[0], p[1], N.VP_F32, C, 0, B, T, C, 1e-12, p[2], st))
            out[f'asp bwd e16 T{T}'] = timed(lambda: lib.vp_attn_stats_bwd_e16(ctx, q[0], p[1], N.VP_F32, C, p[2], p[3], B, T, C, 1e-12, q[1], p[5], C, st))
        if T == 300:
            out['time_stats_f32 T300'] = timed(lambda: lib.vp_time_stats_f32(ctx, p[1], C, B, T, C, 1e-12, 0, p[2], st))
            out['time_stats_bwd_add_f32 T300'] = timed(lambda: lib.vp_time_stats_bwd_add_f32(ctx, p[1], C, p[2], p[3], B, T, C, 1e-12, 0, p[0], C, p[5], C, st))
        del x, e, dp, pooled, de, dx
    B, T, C = 32, 298 * 80, 64
    x, stats = torch.randn(B * T, C, device='cuda', generator=g), torch.empty(B, 2 * C, device='cuda')
    ws = torch.zeros(lib.vp_time_stats_workspace_bytes(B, T, C), dtype=torch.uint8, device='cuda')
    out['time_stats_ws_f32 ResNetSE'] = timed(lambda: lib.vp_time_stats_ws_f32(ctx, x.data_ptr(), C, B, T, C, 1e-8, 1, stats.data_ptr(), ws.data_ptr(),
                                                                                ws.numel(), st))
    print(json.dumps(out), flush=True)


def main(lib_a, lib_b, rounds=7):
    runs = {lib_a: [], lib_b: []}
    for r in range(rounds):
        for lib in (lib_a, lib_b):
            res = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=dict(os.environ, VPMI_LIB=lib), stdout=subprocess.PIPE,
                                 text=True, timeout=300, check=True)
            runs[lib].append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(f'round {r} {lib}: done', flush=True)
    print(f'A = {lib_a}\nB = {lib_b}\n| call | A median us | A min .. max | B median us | B min .. max | B median inside A\'s spread |\n|---|---|---|---|---|---|')
    outside = 0
    for k in runs[lib_a][0]:
        a, b = [r[k] for r in runs[lib_a]], [r[k] for r in runs[lib_b]]
        inside = min(a) <= statistics.median(b) <= max(a)
        outside += not inside
        print(f'| {k} | {statistics.median(a):.1f} | {min(a):.1f} .. {max(a):.1f} | {statistics.median(b):.1f} | {min(b):.1f} .. {max(b):.1f} | '
              f'{"yes" if inside else "NO"} |')
    print(f'{outside} of {len(runs[lib_a][0])} calls outside')
    return outside


if __name__ == '__main__':
    if sys.argv[1:2] == ['--child']:
        child()
    else:
        sys.exit(1 if main(sys.argv[1], sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 7) else 0)
