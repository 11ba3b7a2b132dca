"""Generate / verify tests/golden/res2net_ref_small.npz from the reference's own Res2Net.  Run by hand; nothing in the test suite runs it.

It executes the reference's unmodified ppvector/models/res2net.py (with its pooling / utils modules) through oracle/paddle_shim,
after registering the two layers the shim lacks -- MaxPool2D and AvgPool2D(exclusive=...) -- in the shim's ``paddle.nn`` namespace
of THIS process only.  Weights come from tests/res2net_oracle.res2net_params(seed); for every configuration it

  1. checks that the helper oracle (tests/res2net_oracle.py) reproduces the reference graph's embeddings, and
  2. stores the input, the reference embedding, the parameter seed and the model kwargs (the fixture stays small: the parameters
     are regenerated from the seed).

Usage:  python tools/gen_res2net_golden.py            # check + (re)write the fixture
        python tools/gen_res2net_golden.py --check    # check the oracle against the reference and against the stored fixture
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'res2net_ref_small.npz')

# name -> (model kwargs, input (B, T), parameter seed)
CONFIGS = {
    'shipped80': (dict(input_size=80, m_channels=32, layers=[3, 4, 6, 3], base_width=32, scale=2, embd_dim=192), (2, 66), 1000),
    'small80': (dict(input_size=80, m_channels=8, layers=[1, 1, 1, 1], base_width=32, scale=4, embd_dim=192), (2, 70), 1001),
    # two blocks in the first two layers: 'normal' blocks with nums = 3, i.e. the sp + spx[i] chain (and widths 4 / 8, zero-padded)
    'chain80': (dict(input_size=80, m_channels=8, layers=[2, 2, 1, 1], base_width=32, scale=4, embd_dim=192), (2, 60), 1003),
    'shipped64': (dict(input_size=64, m_channels=32, layers=[3, 4, 6, 3], base_width=32, scale=2, embd_dim=192), (2, 50), 1002),
}


def install_pools(shim):
    """MaxPool2D / AvgPool2D as Paddle defines them (padding excluded from the max; exclusive=True by default for the average)."""
    import torch.nn.functional as TF

    class MaxPool2D(shim.Layer):
        def __init__(self, kernel_size, stride=None, padding=0, ceil_mode=False, return_mask=False, data_format='NCHW', name=None):
            super().__init__()
            assert not return_mask and data_format == 'NCHW'
            self.k, self.s, self.p, self.ceil = kernel_size, stride or kernel_size, padding, ceil_mode

        def forward(self, x):
            return TF.max_pool2d(x, self.k, self.s, self.p, ceil_mode=self.ceil)

    class AvgPool2D(shim.Layer):
        def __init__(self, kernel_size, stride=None, padding=0, ceil_mode=False, exclusive=True, divisor_override=None,
                     data_format='NCHW', name=None):
            super().__init__()
            assert divisor_override is None and data_format == 'NCHW'
            self.k, self.s, self.p, self.ceil, self.exclusive = kernel_size, stride or kernel_size, padding, ceil_mode, exclusive

        def forward(self, x):
            return TF.avg_pool2d(x, self.k, self.s, self.p, ceil_mode=self.ceil, count_include_pad=not self.exclusive)

    shim.nn.MaxPool2D = MaxPool2D
    shim.nn.AvgPool2D = AvgPool2D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--check', action='store_true')
    args = ap.parse_args()
    from oracle import paddle_shim
    paddle_shim.install()
    ref_dir = sys.modules['ppvector.models'].__path__[0]
    if not os.path.exists(os.path.join(ref_dir, 'res2net.py')):
        print(f'the reference model source is not present ({ref_dir}); nothing to do')
        return 0
    install_pools(paddle_shim)
    ref = importlib.import_module('ppvector.models.res2net')
    import res2net_oracle as o2

    torch.manual_seed(0)
    out = {'configs': np.array(json.dumps(list(CONFIGS)))}
    stored = np.load(GOLD) if args.check and os.path.exists(GOLD) else None
    worst = 0.0
    for name, (kw, (B, T), seed) in CONFIGS.items():
        okw = {k: v for k, v in kw.items() if k != 'input_size' and k != 'embd_dim'}
        p = o2.res2net_params(input_size=kw['input_size'], embd_dim=kw['embd_dim'], seed=seed, **okw)
        m = ref.Res2Net(pooling_type='ASP', **kw)
        sd = m.state_dict()
        assert set(sd.keys()) == set(p.keys()), sorted(set(sd.keys()) ^ set(p.keys()))[:10]
        for k in sd:
            assert tuple(sd[k].shape) == tuple(p[k].shape), k
        m.load_state_dict(p)
        m.eval()
        rng = np.random.RandomState(seed)
        x = (rng.standard_normal((B, T, kw['input_size'])) * 3.0).astype(np.float32)
        with torch.no_grad():
            e_ref = torch.as_tensor(m(paddle_shim.to_tensor(x))).detach().double()
            p64 = {k: v.double() for k, v in p.items()}
            e_or = o2.res2net_forward(p64, torch.from_numpy(x).double(), **okw)
        rel = float((e_or - e_ref).norm() / e_ref.norm())
        worst = max(worst, rel)
        nparam = sum(v.numel() for k, v in p.items() if not k.endswith(('_mean', '_variance')))
        print(f'{name}: {nparam} parameters, oracle vs reference rel-L2 {rel:.2e}')
        assert rel < 2e-5, (name, rel)
        if stored is not None:
            srel = float(np.linalg.norm(stored[f'emb_eval__{name}'] - e_ref.numpy()) / np.linalg.norm(e_ref.numpy()))
            print(f'{name}: stored fixture vs reference rel-L2 {srel:.2e}')
            assert np.array_equal(stored[f'x__{name}'], x) and srel < 2e-5, (name, srel)
        out[f'x__{name}'] = x
        out[f'emb_eval__{name}'] = e_ref.float().numpy()
        out[f'param_seed__{name}'] = np.int64(seed)
        out[f'config__{name}'] = np.array(json.dumps(kw))
    print(f'worst oracle vs reference rel-L2 {worst:.2e}')
    if not args.check:
        np.savez_compressed(GOLD, **out)
        print('wrote', GOLD, os.path.getsize(GOLD), 'bytes')
    return 0


if __name__ == '__main__':
    sys.exit(main())
