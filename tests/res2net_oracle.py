"""Oracle (CPU, PyTorch at any float dtype): Res2Net forward.  Test helper, not a test module.

Functional restatement over the reference's Paddle parameter names of ppvector/models/res2net.py:
  Bottle2neck   1x1 (inplanes -> width*scale) + BN + ReLU -> split into `scale` chunks -> for i < nums (= max(scale - 1, 1)):
                sp = spx[i] (i == 0 or 'stage') | sp + spx[i]; sp = ReLU(BN(conv3x3 stride s (sp))) -> concat with the last chunk
                ('normal': as it is; 'stage': AvgPool2D(3, s, 1) with Paddle's exclusive=True) -> 1x1 + BN -> + residual -> ReLU
  Res2Net       conv 7x7 stride 3 pad 1 (1 -> m) + BN + ReLU -> MaxPool2D(3, 2, 1) -> layers [3, 4, 6, 3] (strides 1, 2, 2, 2, the first
                block of each layer 'stage') -> reshape (B, C*F', T') -> ASP -> BN -> Linear -> BN
Paddle Linear weights are [in, out]; every conv has a bias.  Paddle's MaxPool2D excludes the padding and routes the gradient to the
first maximum of a window, as torch's max_pool2d on the CPU does.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.campplus import _bn, _conv
from oracle.models import _bn_keys, asp, batchnorm

LAYERS = [3, 4, 6, 3]
EXPANSION = 4


def width_of(planes, base_width):
    return int(math.floor(planes * (base_width / 64.0)))


def avg_pool_exclusive(x, stride):
    """AvgPool2D(kernel_size=3, stride, padding=1), Paddle's default exclusive=True: the divisor counts only elements inside the map."""
    return F.avg_pool2d(x, 3, stride=stride, padding=1, count_include_pad=False)


def max_pool(x):
    """MaxPool2D(kernel_size=3, stride=2, padding=1), padding excluded, ceil_mode=False."""
    return F.max_pool2d(x, 3, stride=2, padding=1)


def _block(x, p, pre, stride, stage, scale, width, training=False):
    out = F.relu(_bn(F.conv2d(x, p[pre + 'conv1.weight'], p[pre + 'conv1.bias']), p, pre + 'bn1.', training))
    spx = torch.split(out, width, dim=1)
    nums = 1 if scale == 1 else scale - 1
    outs = []
    sp = None
    for i in range(nums):
        sp = spx[i] if (i == 0 or stage) else sp + spx[i]
        sp = F.conv2d(sp, p[f'{pre}convs.{i}.weight'], p[f'{pre}convs.{i}.bias'], stride=stride, padding=1)
        sp = F.relu(_bn(sp, p, f'{pre}bns.{i}.', training))
        outs.append(sp)
    if scale != 1:
        outs.append(avg_pool_exclusive(spx[nums], stride) if stage else spx[nums])
    out = torch.cat(outs, dim=1)
    out = _bn(F.conv2d(out, p[pre + 'conv3.weight'], p[pre + 'conv3.bias']), p, pre + 'bn3.', training)
    if (pre + 'downsample.0.weight') in p:
        res = _bn(F.conv2d(x, p[pre + 'downsample.0.weight'], p[pre + 'downsample.0.bias'], stride=stride), p, pre + 'downsample.1.',
                  training)
    else:
        res = x
    return F.relu(out + res)


def res2net_forward(p, x, m_channels=32, layers=LAYERS, base_width=32, scale=2, training=False, taps=None):
    """Res2Net.forward, pooling_type ASP.  x (B, T, F) -> (B, embd).  Runs at the dtype of p / x."""
    x = x.transpose(1, 2).unsqueeze(1)
    x = F.relu(_bn(F.conv2d(x, p['conv1.weight'], p['conv1.bias'], stride=3, padding=1), p, 'bn1.', training))
    x = max_pool(x)
    if taps is not None:
        taps['stem'] = x
    for li, n in enumerate(layers, start=1):
        planes = m_channels * 2 ** (li - 1)
        w = width_of(planes, base_width)
        for bi in range(n):
            stride = 2 if (li > 1 and bi == 0) else 1
            x = _block(x, p, f'layer{li}.{bi}.', stride, bi == 0, scale, w, training)
    if taps is not None:
        taps['layer4'] = x
    x = x.reshape(x.shape[0], -1, x.shape[-1])
    x = asp(x, p, 'pooling.', True, training)
    x = batchnorm(x, p, 'bn2.norm.', training)
    x = x @ p['linear.weight'] + p['linear.bias']
    return batchnorm(x, p, 'bn3.norm.', training)


def res2net_params(input_size=80, m_channels=32, layers=LAYERS, base_width=32, scale=2, embd_dim=192, seed=1000, randomize_stats=True,
                   dtype=torch.float32):
    """Random parameters keyed with the reference's names (BatchNorm statistics randomised unless told otherwise)."""
    rng = np.random.RandomState(seed)
    p = {}
    p.update(_conv('conv1.', (m_channels, 1, 7, 7), rng)); p.update(_bn_keys('bn1.', m_channels, rng, randomize_stats))
    inpl = m_channels
    for li, n in enumerate(layers, start=1):
        planes = m_channels * 2 ** (li - 1)
        w = width_of(planes, base_width)
        nums = 1 if scale == 1 else scale - 1
        for bi in range(n):
            pre = f'layer{li}.{bi}.'
            stride = 2 if (li > 1 and bi == 0) else 1
            p.update(_conv(pre + 'conv1.', (w * scale, inpl, 1, 1), rng)); p.update(_bn_keys(pre + 'bn1.', w * scale, rng, randomize_stats))
            for i in range(nums):
                p.update(_conv(f'{pre}convs.{i}.', (w, w, 3, 3), rng)); p.update(_bn_keys(f'{pre}bns.{i}.', w, rng, randomize_stats))
            p.update(_conv(pre + 'conv3.', (planes * EXPANSION, w * scale, 1, 1), rng))
            p.update(_bn_keys(pre + 'bn3.', planes * EXPANSION, rng, randomize_stats))
            if bi == 0 and (stride != 1 or inpl != planes * EXPANSION):
                p.update(_conv(pre + 'downsample.0.', (planes * EXPANSION, inpl, 1, 1), rng))
                p.update(_bn_keys(pre + 'downsample.1.', planes * EXPANSION, rng, randomize_stats))
            inpl = planes * EXPANSION
    C = m_channels * 8 * EXPANSION * (input_size // base_width)
    bound = 1.0 / math.sqrt(3 * C)
    p['pooling.tdnn.conv.conv.weight'] = rng.uniform(-bound, bound, (128, 3 * C, 1)) * math.sqrt(3.0)
    p['pooling.tdnn.conv.conv.bias'] = rng.uniform(-bound, bound, 128)
    p.update(_bn_keys('pooling.tdnn.norm.norm.', 128, rng, randomize_stats))
    b2 = 1.0 / math.sqrt(128)
    p['pooling.conv.conv.weight'] = rng.uniform(-b2, b2, (C, 128, 1)) * math.sqrt(3.0)
    p['pooling.conv.conv.bias'] = rng.uniform(-b2, b2, C)
    p.update(_bn_keys('bn2.norm.', 2 * C, rng, randomize_stats))
    b3 = 1.0 / math.sqrt(2 * C)
    p['linear.weight'] = rng.uniform(-b3, b3, (2 * C, embd_dim)) * math.sqrt(3.0)
    p['linear.bias'] = rng.uniform(-b3, b3, embd_dim)
    p.update(_bn_keys('bn3.norm.', embd_dim, rng, randomize_stats))
    return {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in p.items()}


def config_kwargs(cfg):
    """The model kwargs stored in a golden file's `config` entry (a JSON string)."""
    import json
    return json.loads(str(cfg))
