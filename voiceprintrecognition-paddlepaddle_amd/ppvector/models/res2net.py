"""Res2Net backbone on the MI355X engine.

Same constructor surface, ``embd_dim`` attribute and state-dict keys as ppvector/models/res2net.py (Bottle2neck, Res2Net):
``conv1``/``bn1`` (7x7 stride 3), ``layer{1..4}.{j}.conv1`` / ``bn1`` / ``convs.{i}`` / ``bns.{i}`` / ``conv3`` / ``bn3`` /
``downsample.{0,1}``, ``pooling.*``, ``bn2.norm``, ``linear`` (Paddle Linear, weight [in, out]), ``bn3.norm``.  The modules are
parameter containers; ``forward`` runs the whole graph through libvpmi (csrc/res2net.hip: vp_res2net_fwd).
"""
import math

from torch import nn

from ppvector.models.campplus import _ConvNd
from ppvector.models.engine import EngineMixin, Res2NetEngine
from ppvector.models.pooling import AttentiveStatisticsPooling
from ppvector.models.resnet_se import _LinearParams
from ppvector.models.utils import BatchNorm1d, _BNParams


def stem_out(v):
    """Conv2D(k=7, stride=3, padding=1) then MaxPool2D(k=3, stride=2, padding=1) along one axis."""
    c = (v + 2 - 7) // 3 + 1
    return (c - 1) // 2 + 1 if c >= 1 else 0


def feature_bins(input_size):
    """F' of layer4's output: the stem, then three stride-2 stages."""
    f = stem_out(input_size)
    for _ in range(3):
        f = (f - 1) // 2 + 1 if f >= 1 else 0
    return f


class Bottle2neck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, baseWidth=26, scale=4, stype='normal'):
        super().__init__()
        width = int(math.floor(planes * (baseWidth / 64.0)))
        self.conv1 = _ConvNd(inplanes, width * scale, 1, 1)
        self.bn1 = _BNParams(width * scale)
        self.nums = 1 if scale == 1 else scale - 1
        self.convs = nn.ModuleList([_ConvNd(width, width, 3, 3) for _ in range(self.nums)])
        self.bns = nn.ModuleList([_BNParams(width) for _ in range(self.nums)])
        self.conv3 = _ConvNd(width * scale, planes * self.expansion, 1, 1)
        self.bn3 = _BNParams(planes * self.expansion)
        self.relu = nn.ReLU()
        self.downsample = downsample
        self.stype = stype
        self.scale = scale
        self.width = width
        self.stride = stride


class Res2Net(EngineMixin, nn.Module):
    # quoted by engine('bfloat16') / engine('float32x3')'s warnings (models/engine.py; tests/test_gpu_res2net_train.py, docs/res2net.md)
    _bf16_trained_score_err = '6.6e-2'
    _x3_trained_score_err = '1.1e-4'
    _engine_cls = Res2NetEngine

    def __init__(self, input_size, m_channels=32, layers=[3, 4, 6, 3], base_width=32, scale=2, embd_dim=192,
                 pooling_type="ASP"):
        super().__init__()
        self.input_size = input_size
        self.inplanes = m_channels
        self.m_channels = m_channels
        self.base_width = base_width
        self.scale = scale
        self.embd_dim = embd_dim
        cat_channels = m_channels * 8 * Bottle2neck.expansion * (input_size // base_width)
        if pooling_type in ("SAP", "TAP", "TSP"):
            raise NotImplementedError(f'pooling_type {pooling_type} is not built on the HIP engine (ASP is); the reference hands '
                                      'its (B, C, 1) output to a Linear and fails there')
        if pooling_type != "ASP":
            raise Exception(f'没有{pooling_type}池化层！')
        fq = feature_bins(input_size)
        if fq < 1 or fq != input_size // base_width:
            raise ValueError(f'Res2Net: input_size {input_size} leaves {fq} frequency bins after layer4, but the reference sizes its '
                             f'pooling for input_size // base_width = {input_size // base_width} (its forward fails on this shape)')
        self.conv1 = _ConvNd(1, m_channels, 7, 7)
        self.bn1 = _BNParams(m_channels)
        self.relu = nn.ReLU()
        self.layer1 = self._make_layer(Bottle2neck, m_channels, layers[0])
        self.layer2 = self._make_layer(Bottle2neck, m_channels * 2, layers[1], stride=2)
        self.layer3 = self._make_layer(Bottle2neck, m_channels * 4, layers[2], stride=2)
        self.layer4 = self._make_layer(Bottle2neck, m_channels * 8, layers[3], stride=2)
        self.pooling = AttentiveStatisticsPooling(cat_channels, attention_channels=128)
        self.bn2 = BatchNorm1d(cat_channels * 2)
        self.linear = _LinearParams(cat_channels * 2, embd_dim)
        self.bn3 = BatchNorm1d(embd_dim)

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(_ConvNd(self.inplanes, planes * block.expansion, 1, 1),
                                       _BNParams(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample=downsample, stype='stage', baseWidth=self.base_width,
                        scale=self.scale)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, baseWidth=self.base_width, scale=self.scale))
        return nn.Sequential(*layers)

    def _train_forward(self, x):
        """Training mode: batch-statistics BatchNorm, autograd through libvpmi's backward entry points (train/res2net_train.py)."""
        from ppvector import _native as N
        from ppvector.train.res2net_train import res2net_forward_train
        if not x.is_cuda:
            raise N.VpmiError('model input must be a GPU tensor: the engine has no CPU fallback')
        return res2net_forward_train(self, x.float().contiguous())
