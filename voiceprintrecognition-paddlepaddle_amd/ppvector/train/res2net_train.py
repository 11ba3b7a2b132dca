"""Training-mode forward of Res2Net (ppvector/models/res2net.py: Res2Net.forward, Bottle2neck.forward) through the autograd functions
of functions.py plus the two pooling functions below.
Activations are (B*T*F, C) position-major.  Chunk splitting / concatenation, the `sp + spx[i]` hand-off and the residual add are tensor
slicing, torch.cat and `+`; every conv / BatchNorm / activation / pooling runs in libvpmi (the pools on the kernels of csrc/res2net.hip:
the max pool's backward routes each gradient to the first maximum of its window, both backward kernels gather, no atomics).  The reference's
reshape (B, C*F', T') before the pooling is a permute + reshape of a small tensor.  Input (B, T, F) f32 on the GPU -> embeddings (B, embd)."""
import torch

from ppvector import _native as N
from ppvector.train.functions import Act, BNRows, Conv2dBlock, ConvBlock, _chk, _f32c
from ppvector.train.segments import cut
from ppvector.train.tdnn_train import asp_forward


class MaxPool2d(torch.autograd.Function):
    """MaxPool2D(kernel_size=3, stride=2, padding=1) over (B*T*F, C) rows (res2net.py stem); padding excluded."""

    @staticmethod
    def forward(ctx, x, B, T, F):
        lib, hctx = N.lib(), N.ctx(x.device)
        x = _f32c(x)
        Cc = x.shape[1]
        To, Fo = (T - 1) // 2 + 1, (F - 1) // 2 + 1
        y = torch.empty((B * To * Fo, Cc), dtype=torch.float32, device=x.device)
        _chk(lib.vp_maxpool3x3_fwd_f32(hctx, x.data_ptr(), y.data_ptr(), B, T, F, Cc, N.stream_ptr()), hctx)
        ctx.save_for_backward(x)
        ctx.geom = (B, T, F)
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        B, T, F = ctx.geom
        lib, hctx = N.lib(), N.ctx(x.device)
        g = _f32c(g)
        dx = torch.empty_like(x)
        _chk(lib.vp_maxpool3x3_bwd_f32(hctx, x.data_ptr(), g.data_ptr(), dx.data_ptr(), B, T, F, x.shape[1], N.stream_ptr()), hctx)
        return dx, None, None, None


class AvgPool2d(torch.autograd.Function):
    """AvgPool2D(kernel_size=3, stride, padding=1) with Paddle's default exclusive=True (the divisor counts only elements inside the
    map) over (B*T*F, C) rows: the last chunk of a 'stage' Bottle2neck."""

    @staticmethod
    def forward(ctx, x, B, T, F, stride):
        lib, hctx = N.lib(), N.ctx(x.device)
        x = _f32c(x)
        Cc = x.shape[1]
        To, Fo = (T - 1) // stride + 1, (F - 1) // stride + 1
        y = torch.empty((B * To * Fo, Cc), dtype=torch.float32, device=x.device)
        _chk(lib.vp_avgpool3x3_fwd(hctx, N.VP_F32, x.data_ptr(), Cc, 0, y.data_ptr(), Cc, 0, B, T, F, Cc, stride, N.stream_ptr()), hctx)
        ctx.geom = (B, T, F, Cc, stride)
        return y

    @staticmethod
    def backward(ctx, g):
        B, T, F, Cc, stride = ctx.geom
        lib, hctx = N.lib(), N.ctx(g.device)
        g = _f32c(g)
        dx = torch.empty((B * T * F, Cc), dtype=torch.float32, device=g.device)
        _chk(lib.vp_avgpool3x3_bwd_f32(hctx, g.data_ptr(), Cc, 0, dx.data_ptr(), Cc, 0, B, T, F, Cc, stride, N.stream_ptr()), hctx)
        return dx, None, None, None, None


def _bn(p):
    return p.weight, p.bias, p._mean, p._variance


def _cb(x, conv, bn, B, T, F, relu=False, stride=1, **kw):
    return Conv2dBlock.apply(x, conv.weight, conv.bias, *_bn(bn),
                             dict(B=B, T=T, F=F, relu=relu, stride=stride, momentum=bn.momentum, eps=bn.eps, **kw))


def bottle2neck(b, x, B, T, F):
    """Bottle2neck.forward: 1x1 -> chunks -> 3x3 convs (stride; sp + spx[i] in 'normal' blocks) -> concat with the last chunk (as it is,
    or the exclusive 3x3 average pool in a 'stage' block) -> 1x1 + BN -> + residual -> ReLU."""
    s, w, stage = b.stride, b.width, b.stype == 'stage'
    out = _cb(x, b.conv1, b.bn1, B, T, F, relu=True)
    To, Fo = (T - 1) // s + 1, (F - 1) // s + 1
    spx = torch.split(out, w, dim=1)
    outs, sp = [], None
    for i in range(b.nums):
        sp = spx[i] if (i == 0 or stage) else sp + spx[i]
        sp = _cb(sp, b.convs[i], b.bns[i], B, T, F, relu=True, stride=s)
        outs.append(sp)
    if b.scale != 1:
        outs.append(AvgPool2d.apply(spx[b.nums], B, T, F, s) if stage else spx[b.nums])
    out = _cb(torch.cat(outs, dim=1) if len(outs) > 1 else outs[0], b.conv3, b.bn3, B, To, Fo)
    res = x
    if b.downsample is not None:
        res = _cb(x, b.downsample[0], b.downsample[1], B, T, F, stride=s)
    return Act.apply(out + res, 'relu'), To, Fo


def res2net_forward_train(m, feats):
    B, T, F = feats.shape
    for layer in (m.layer1, m.layer2, m.layer3, m.layer4):
        for b in layer:
            if b.width % 4:
                raise NotImplementedError(f'Res2Net training needs chunk widths that are multiples of 4 (got {b.width})')
    # stem: conv 7x7 stride 3 pad 1 (1 -> m) -> BN -> ReLU, the single input channel zero-padded to 4 (16-byte channel chunks)
    x = torch.zeros((B * T * F, 4), dtype=torch.float32, device=feats.device)
    x[:, 0] = feats.reshape(-1)
    wt = m.conv1.weight
    w4 = torch.cat([wt, torch.zeros((wt.shape[0], 3, 7, 7), dtype=wt.dtype, device=wt.device)], dim=1)
    x = Conv2dBlock.apply(x, w4, m.conv1.bias, *_bn(m.bn1),
                          dict(B=B, T=T, F=F, relu=True, stride=3, pad=1, momentum=m.bn1.momentum, eps=m.bn1.eps))
    T, F = (T + 2 - 7) // 3 + 1, (F + 2 - 7) // 3 + 1
    x = MaxPool2d.apply(x, B, T, F)
    T, F = (T - 1) // 2 + 1, (F - 1) // 2 + 1
    for li, layer in enumerate((m.layer1, m.layer2, m.layer3, m.layer4)):
        for b in layer:
            x, T, F = bottle2neck(b, x, B, T, F)
        if li < 3:
            (x,) = cut(x)          # backward stage boundary (train/segments.py): a plain chain, one live tensor
    Cc = x.shape[1]
    # (B, T', F', C) -> the reference's (B, C*F', T') channel order c*F' + f, frame-major for the pooling: (B*T', C*F')
    x = x.reshape(B, T, F, Cc).permute(0, 1, 3, 2).reshape(B * T, Cc * F)
    p = asp_forward(m.pooling, x, B, T)
    n2, n3 = m.bn2.norm, m.bn3.norm
    p = BNRows.apply(p, n2.weight, n2.bias, n2._mean, n2._variance, n2.momentum, n2.eps)
    y = ConvBlock.apply(p, m.linear.weight.t().unsqueeze(2), m.linear.bias, None, None, None, None, None, dict(B=B, T=1))
    return BNRows.apply(y, n3.weight, n3.bias, n3._mean, n3._variance, n3.momentum, n3.eps)
