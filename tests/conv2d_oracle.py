"""Oracle (CPU, PyTorch float64): the 2-D convolution of the conv GEMM -- forward, data gradient, weight gradient -- and the
Conv2D -> BatchNorm2D(batch statistics) -> ReLU / Hardtanh(0, 20) training unit, with the conv's OPERANDS rounded the way each engine
precision rounds them.  Test helper, not a test module; imports nothing of the engine.

The engine sums products of operand pairs in f32; what differs between its precisions is which pairs (`terms`):
  'f32'   the operands as they are                                      (vp_conv1d_desc.mfma_bf16 = 0)
  'amp'   both operands rounded to bf16                                 (mfma_bf16 = 1, ppvector.set_train_amp, bf16 tensors)
  'x3'    hi*hi + hi*lo + lo*hi, hi = bf16(v), lo = bf16(v - hi)        (mfma_bf16 = 2 / 3, ppvector.set_train_x3; pack_hl32's split)
Everything else -- the sums, the bias, BatchNorm, the clamp -- is exact here (float64); the engine keeps it in f32 in every mode.

Tensors are in the reference's (B, C, F, T) layout, weights (Cout, Cin, kF, kT); `rows` / `unrows` convert to and from the engine's
(B*T*F, C) rows.  A geometry is the keyword set of F.conv2d: stride (sf, st), padding (pad_f, pad_t), dilation (1, dil).
"""
import torch
import torch.nn.functional as F

MODES = ('f32', 'amp', 'x3')

# id -> (B, T, F, Cin, Cout, k, stride_t, stride_f, dil, pad); pad None = (k - 1) / 2 per axis (dil * (k - 1) / 2 along time).
# Each shape crosses one edge of the kernels' tiling (tests/test_gpu_conv2d.py says which).
CASES = {
    'A': (2, 9, 10, 64, 64, 3, 1, 1, 1, None),
    'B': (2, 11, 7, 48, 160, 3, 1, 1, 1, None),
    'C': (3, 13, 9, 16, 96, 3, 2, 2, 1, None),
    'D1': (2, 12, 10, 32, 64, 3, 2, 1, 1, None),
    'D2': (2, 12, 10, 32, 64, 3, 1, 2, 1, None),
    'E': (2, 17, 8, 24, 32, 3, 1, 1, 2, None),
    'F': (2, 33, 33, 32, 32, 3, 1, 1, 1, None),
    'G': (3, 8, 9, 64, 256, 1, 2, 2, 1, None),
    'H': (2, 20, 16, 8, 32, 7, 3, 3, 1, 1),
    'I': (1, 2, 1, 16, 16, 3, 1, 1, 1, None),
    'W': (4, 64, 65, 32, 32, 3, 1, 1, 1, None),
}

# The BatchNorm + clamp units of the GPU tests: case id -> (activation, seed).  The seed is one of 0..39 at which no pre-activation of
# the 'f32', the 'amp' or the 'x3' reference lies within 1e-4 of a clamp edge (tests/test_conv2d_oracle_cpu.py checks it): a mask
# element that flips between engine and reference moves a gradient by ~1 / sqrt(active elements), and the test would measure flips,
# not kernels.
# Of seeds 0..39, 9 (A), 15 (C), 17 (D1) and 23 (B) qualify; these are the ones with the widest margin (3.2e-4 ... 1.4e-3).
UNIT_CASES = {'A': ('relu', 7), 'C': ('relu', 11), 'D1': ('relu', 24), 'B': ('hardtanh', 35)}
EDGE_MARGIN = 1e-4


def dims(case):
    """(B, T, F, Cin, Cout, k, st, sf, dil, pad_t, pad_f, T_out, F_out) of a CASES entry."""
    B, T, Fq, Cin, Cout, k, st, sf, dil, pad = CASES[case] if isinstance(case, str) else case
    pad_t = dil * (k - 1) // 2 if pad is None else pad
    pad_f = (k - 1) // 2 if pad is None else pad
    To = (T + 2 * pad_t - dil * (k - 1) - 1) // st + 1
    Fo = (Fq + 2 * pad_f - (k - 1) - 1) // sf + 1
    return B, T, Fq, Cin, Cout, k, st, sf, dil, pad_t, pad_f, To, Fo


def geom_of(case):
    B, T, Fq, Cin, Cout, k, st, sf, dil, pad_t, pad_f, To, Fo = dims(case)
    return dict(stride=(sf, st), padding=(pad_f, pad_t), dilation=(1, dil))


def bf(t):
    """Round to bf16 (nearest even), back in float64."""
    return t.float().to(torch.bfloat16).double()


def terms(a, b, mode):
    """The operand pairs whose products the engine sums in `mode`."""
    if mode == 'f32':
        return [(a, b)]
    ah, bh = bf(a), bf(b)
    if mode == 'amp':
        return [(ah, bh)]
    if mode == 'x3':
        al, bl = bf(a - ah), bf(b - bh)
        return [(ah, bh), (ah, bl), (al, bh)]
    raise ValueError(mode)


def conv2d_fwd(x, w, geom, mode):
    return sum(F.conv2d(a, b, None, **geom) for a, b in terms(x, w, mode))


def conv2d_dgrad(dz, w, x_shape, geom, mode):
    return sum(torch.nn.grad.conv2d_input(x_shape, b, a, **geom) for a, b in terms(dz, w, mode))


def conv2d_wgrad(x, dz, w_shape, geom, mode):
    return sum(torch.nn.grad.conv2d_weight(a, w_shape, b, **geom) for a, b in terms(x, dz, mode))


class Conv2dMode(torch.autograd.Function):
    """conv2d whose three GEMMs round their operands per mode (each from the float64 tensors it is handed)."""

    @staticmethod
    def forward(ctx, x, w, geom, mode):
        ctx.save_for_backward(x, w)
        ctx.geom, ctx.mode = geom, mode
        return conv2d_fwd(x, w, geom, mode)

    @staticmethod
    def backward(ctx, dz):
        x, w = ctx.saved_tensors
        return conv2d_dgrad(dz, w, x.shape, ctx.geom, ctx.mode), conv2d_wgrad(x, dz, w.shape, ctx.geom, ctx.mode), None, None


def rows(t):
    """(B, C, F, T) -> the engine's (B*T*F, C) rows."""
    return t.permute(0, 3, 2, 1).reshape(-1, t.shape[1])


def unrows(t, B, T, Fq):
    return t.reshape(B, T, Fq, -1).permute(0, 3, 2, 1)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-30)).item()


def conv_inputs(case, seed):
    """x (B, Cin, F, T), w (Cout, Cin, k, k) / sqrt(fan-in), dz (B, Cout, F_out, T_out): float64 holding f32-representable values."""
    B, T, Fq, Cin, Cout, k, st, sf, dil, pad_t, pad_f, To, Fo = dims(case)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, Fq, T, generator=g).double()
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).double()
    dz = torch.randn(B, Cout, Fo, To, generator=g).double()
    return x, w, dz


def unit_inputs(case, seed, act=None, bn=True):
    """conv_inputs plus bias, gamma, beta (None without BatchNorm) and the upstream gradient dy.  For Hardtanh gamma is x 14 and beta
    x 3 + 6, so that both clamps are active (as tests/test_gpu_train.py::test_conv2d_block_hardtanh_folded_vs_autograd)."""
    Cout = dims(case)[4]
    x, w, dy = conv_inputs(case, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    bias = torch.randn(Cout, generator=g).double()
    gamma = beta = None
    if bn:
        h = act == 'hardtanh'
        gamma = ((torch.rand(Cout, generator=g) + 0.5) * (14.0 if h else 1.0)).double()
        beta = (torch.randn(Cout, generator=g) * (3.0 if h else 1.0) + (6.0 if h else 0.0)).double()
    return dict(x=x, w=w, bias=bias, gamma=gamma, beta=beta, dy=dy)


def unit_forward(x, w, bias, gamma, beta, geom, mode, act, eps=1e-5, conv=None):
    """y and the pre-activation of conv (+ bias) [-> BatchNorm over (B, F, T) with batch statistics] [-> clamp]."""
    z = (conv or Conv2dMode.apply)(x, w, geom, mode) + bias[None, :, None, None]
    if gamma is not None:
        mean, var = z.mean(dim=(0, 2, 3)), z.var(dim=(0, 2, 3), unbiased=False)
        z = (z - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + eps) * gamma[None, :, None, None] + beta[None, :, None, None]
    y = {None: z, 'relu': F.relu(z), 'hardtanh': F.hardtanh(z, 0.0, 20.0)}[act]
    return y, z


_UNIT_CACHE = {}


def unit_reference(case, mode, seed, act=None, bn=True):
    """The unit differentiated in float64 with the conv's operands rounded per mode: dict of y, dx (both (B, C, F, T)), dW, dbias, dgamma,
    dbeta, edge_margin (smallest distance of a pre-activation from a clamp edge: 0, and 20 for hardtanh; inf without a clamp) and
    lo / hi (fractions of elements clamped at 0 / 20).  Computed once per argument set; callers must not modify the tensors."""
    key = (case if isinstance(case, str) else tuple(case), mode, seed, act, bn)
    if key in _UNIT_CACHE:
        return _UNIT_CACHE[key]
    inp = unit_inputs(case, seed, act, bn)
    leaves = {k: v.clone().requires_grad_() for k, v in inp.items() if v is not None and k != 'dy'}
    y, pre = unit_forward(leaves['x'], leaves['w'], leaves['bias'], leaves.get('gamma'), leaves.get('beta'), geom_of(case), mode, act)
    y.backward(inp['dy'])
    p = pre.detach()
    margin, lo, hi = float('inf'), 0.0, 0.0
    if act in ('relu', 'hardtanh'):
        margin, lo = p.abs().min().item(), (p <= 0).double().mean().item()
        if act == 'hardtanh':
            margin, hi = min(margin, (p - 20.0).abs().min().item()), (p >= 20).double().mean().item()
    out = dict(y=y.detach(), dx=leaves['x'].grad, dW=leaves['w'].grad, dbias=leaves['bias'].grad,
               dgamma=leaves['gamma'].grad if bn else None, dbeta=leaves['beta'].grad if bn else None, edge_margin=margin, lo=lo, hi=hi)
    _UNIT_CACHE[key] = out
    return out
