"""Res2Net eval throughput on one MI355X (reported, not gated).

For each engine: utterances per second at B x T frames (default 256 x 298 = 3 s at 80 Fbank bins, the shipped res2net.yml shape),
timed with HIP events over --iters forwards after --warmup (eager, and replayed from a captured HIP graph: the difference is
the host launch overhead), and the fraction of HBM bandwidth that the activation traffic of the
launch graph implies (every tensor a kernel writes is read back at least once: 2 x the bytes written, counted from the layer shapes).
The GPU clocks are printed with the numbers.  For the per-kernel picture run it under `rocprofv3 --kernel-trace --stats -- python
tools/res2net_probe.py --iters 5`.

Usage: python tools/res2net_probe.py [--B 256] [--T 298] [--iters 30] [--warmup 5] [--hbm-tbs 8.0]
"""
import argparse
import os
import subprocess
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'voiceprintrecognition-paddlepaddle_amd')):
    sys.path.insert(0, p)


def activation_bytes(m, B, T, es):
    """Bytes the launch graph writes to HBM per forward (stem output, every block's conv1 / concat / chain / residual / output), x 2."""
    from ppvector.models.res2net import stem_out
    t, f = stem_out(T), stem_out(m.input_size)
    n = B * t * f * m.m_channels
    for layer in (m.layer1, m.layer2, m.layer3, m.layer4):
        for b in layer:
            s = b.stride
            to, fo = (t - 1) // s + 1, (f - 1) // s + 1
            cc = b.conv1.weight.shape[0]
            n += B * t * f * cc                                    # conv1
            n += B * to * fo * cc                                  # concat (split convs + pooled / passed chunk)
            if b.stype != 'stage':
                n += B * t * f * b.width * max(b.nums - 1, 0)      # chained inputs
            cout = b.conv3.weight.shape[0]
            if b.downsample is not None:
                n += B * to * fo * cout
            n += B * to * fo * cout                                # block output
            t, f = to, fo
    return 2 * n * es


def clocks():
    try:
        return subprocess.run(['amd-smi', 'metric', '--clock'], capture_output=True, text=True, timeout=30).stdout.strip()
    except Exception as e:      # the tool is optional on the machine
        return f'(amd-smi unavailable: {e})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=256)
    ap.add_argument('--T', type=int, default=298)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--hbm-tbs', type=float, default=8.0, help='peak HBM bandwidth in TB/s for the fraction')
    a = ap.parse_args()
    from ppvector.models.res2net import Res2Net
    torch.manual_seed(0)
    m = Res2Net(80).cuda().eval()
    x = torch.randn(a.B, a.T, 80, device='cuda') * 3.0
    print(clocks())
    for dtype in ('float32', 'float32x3', 'bfloat16'):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            eng = m.engine(dtype)
        xin = x.bfloat16() if dtype == 'bfloat16' else x
        for _ in range(a.warmup):
            eng.forward(xin)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            eng.forward(xin)
        e.record()
        torch.cuda.synchronize()
        ms = s.elapsed_time(e) / a.iters
        from ppvector.models.engine import _graph_forward           # the same launch sequence replayed from a captured HIP graph
        for _ in range(2):
            _graph_forward(eng, xin)
        torch.cuda.synchronize()
        s.record()
        for _ in range(a.iters):
            _graph_forward(eng, xin)
        e.record()
        torch.cuda.synchronize()
        ms_g = s.elapsed_time(e) / a.iters
        print(f'res2net {dtype:10s} graph replay: {ms_g:.3f} ms/forward (eager {ms:.3f}: launch overhead {ms - ms_g:+.3f} ms)', flush=True)
        nb = activation_bytes(m, a.B, a.T, 2 if dtype == 'bfloat16' else 4)
        print(f'res2net {dtype:10s} B={a.B} T={a.T}: {ms:.3f} ms/forward  {a.B / ms * 1e3:,.0f} utt/s  activation traffic '
              f'{nb / 1e9:.2f} GB -> {nb / (ms * 1e-3) / 1e12:.2f} TB/s ({nb / (ms * 1e-3) / (a.hbm_tbs * 1e12):.0%} of {a.hbm_tbs} TB/s)',
              flush=True)


if __name__ == '__main__':
    main()
