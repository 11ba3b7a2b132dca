"""Bit-identity instrument for changes that must not move a single output bit of the eval forwards (host-side refactors of the launch
layer): writes the embeddings of every backbone x engine at a small and a BASELINE-sized batch to .npy, from seeded weights and a seeded
batch.  Run it on two checkouts (each with its own build), then compare the two directories.

    python tools/engine_bits.py --out DIR            # 36 arrays (+ EcapaTdnn float32x3 says which path ran; VPMI_X3_GENERIC=1 pins the generic one)
    python tools/engine_bits.py --compare DIR_A DIR_B
    python tools/engine_bits.py --time-b1            # 200 B = 1 forwards of ECAPA and ResNetSE per engine, GPU events (host launch overhead)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'voiceprintrecognition-paddlepaddle_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

# (model, BASELINE-sized per-GPU batch of 3 s utterances)
MODELS = (('EcapaTdnn', 256), ('TDNN', 256), ('CAMPPlus', 256), ('ResNetSE', 32), ('ERes2Net', 32), ('Res2Net', 256))
DTYPES = ('float32', 'float32x3', 'bfloat16')
SMALL = (2, 200)


def _model(name):
    import torch
    from ppvector.models import _BUILT
    torch.manual_seed(1234)
    return _BUILT[name](input_size=80).cuda().eval()


def _batch(B, T):
    import torch
    g = torch.Generator().manual_seed(100 * B + T)
    return torch.randn(B, T, 80, generator=g).cuda()


def dump(out, only=None, suffix=''):
    import warnings
    import torch
    warnings.simplefilter('ignore', RuntimeWarning)
    os.makedirs(out, exist_ok=True)
    for name, big in MODELS:
        if only and name not in only:
            continue
        m = _model(name)
        for dt in DTYPES:
            eng = m.engine(dt)
            for B, T in (SMALL, (big, 298)):
                with torch.no_grad():
                    e = eng.forward(_batch(B, T))
                torch.cuda.synchronize()
                path = ''
                if name == 'EcapaTdnn' and dt == 'float32x3':
                    path = ' fast-path' if eng.x3_fast_path(B, T) else ' generic-path'
                f = f'{name}_{dt}_B{B}_T{T}{suffix}.npy'
                np.save(os.path.join(out, f), e.cpu().numpy())
                print(f'{f}{path} finite={bool(torch.isfinite(e).all())}', flush=True)


def compare(a, b):
    names = sorted(f for f in os.listdir(a) if f.endswith('.npy'))
    assert names == sorted(f for f in os.listdir(b) if f.endswith('.npy')), 'the two directories hold different arrays'
    bad = 0
    for f in names:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        eq = x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))
        bad += not eq
        print(f'{f}: {"equal" if eq else "DIFFERENT"}')
    print(f'{len(names) - bad} of {len(names)} equal')
    return bad


def time_b1(n=200):
    import warnings
    import torch
    warnings.simplefilter('ignore', RuntimeWarning)
    for name in ('EcapaTdnn', 'ResNetSE'):
        m = _model(name)
        x = _batch(1, 298)
        for dt in DTYPES:
            eng = m.engine(dt)
            xin = eng.feats_in(x)
            for _ in range(20):
                eng.forward(xin)
            torch.cuda.synchronize()
            reps = []
            for _ in range(3):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(n):
                    eng.forward(xin)
                t1.record()
                torch.cuda.synchronize()
                reps.append(t0.elapsed_time(t1) / n * 1e3)
            print(f'b1 {name} {dt}: ' + ' '.join(f'{r:.1f}' for r in reps) + f' us/forward ({n} forwards per repeat)', flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--only', nargs='*')
    ap.add_argument('--suffix', default='')
    ap.add_argument('--compare', nargs=2)
    ap.add_argument('--time-b1', action='store_true')
    a = ap.parse_args()
    if a.compare:
        sys.exit(1 if compare(*a.compare) else 0)
    if a.time_b1:
        time_b1()
    if a.out:
        dump(a.out, a.only, a.suffix)
