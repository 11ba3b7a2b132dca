"""GPU tests of the conv weight gradient, one per kernel family of csrc/wgrad.hip, at the smallest shapes that reach each kernel's edges
(docs/wgrad.md).  Every case asks vp_conv1d_wgrad_plan first and asserts the family it is about -- a case that silently ran another
kernel fails there -- then launches with a workspace of exactly the queried size filled with 0xFF and dW prefilled with NaN, and
compares with the float64 gradient F.conv1d's autograd gives.  The 256-tile family needs about 229 000 rows (its flop gate) and stays
with tests/test_gpu_train.py::test_wgrad_of_bf16_operands_vs_float64.  Run with -m gpu on an MI355X.

Shapes (B, T, Cin, Cout, k, dilation, padding):
  A   2, 77, 64, 64, 3, 2, reflect    M = 154: ragged row chunks of 32 and of 64; reflected taps at both ends; one 64-tile, K = 192
  B   3, 50, 80, 96, 5, 1, none       T_out = 46, M = 138; Cin = 80: a 64-column tile straddles taps; Cout = 96, K = 400: ragged tiles
  P   1, 200, 320, 192, 1             bf16 operands inside a wider buffer (ldx 384, xoff 64): 1.5 x 2.5 tiles of 128
  N1  2, 40, 64, 64, 3, 2, reflect    the narrow kernel: K = 192, one 256-column tile, partly empty
  N2  2, 40, 64, 32, 5, 1, reflect    N < 64; K = 320: two column tiles, the second partly empty"""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CASES = {'A': (2, 77, 64, 64, 3, 2, 'reflect'), 'B': (3, 50, 80, 96, 5, 1, 'none'),
         'N1': (2, 40, 64, 64, 3, 2, 'reflect'), 'N2': (2, 40, 64, 32, 5, 1, 'reflect')}


@pytest.fixture(scope='module')
def N():
    from ppvector import _native as N
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: these tests must run on an MI355X (no CPU fallback exists)')
    N.ctx(0)
    return N


def t_out(case):
    B, T, Cin, Cout, kw, dil, pad = CASES[case]
    return T if pad != 'none' else T - dil * (kw - 1)


@functools.lru_cache(maxsize=None)
def operands(case, nconv=1):
    """x (nconv, B, T, Cin) and dz (nconv, B, T_out, Cout), f32, seeded by the case"""
    B, T, Cin, Cout, kw, dil, pad = CASES[case]
    g = torch.Generator().manual_seed(sum(CASES[case][:6]) + nconv)
    return torch.randn(nconv, B, T, Cin, generator=g), torch.randn(nconv, B, t_out(case), Cout, generator=g)


def conv_grad(case, x, dz):
    """float64 weight gradient (Cout, Cin, kw) of one conv from x (B, T, Cin) and dz (B, T_out, Cout), by autograd"""
    B, T, Cin, Cout, kw, dil, pad = CASES[case]
    xt = x.double().transpose(1, 2)
    if pad == 'reflect' and kw > 1:
        xt = F.pad(xt, (dil * (kw - 1) // 2,) * 2, mode='reflect')
    w = torch.zeros(Cout, Cin, kw, dtype=torch.float64, requires_grad=True)
    (F.conv1d(xt, w, None, dilation=dil).transpose(1, 2) * dz.double()).sum().backward()
    return w.grad


@functools.lru_cache(maxsize=None)
def reference(case, rounding, nconv=1):
    """per conv: (the float64 gradient of the operands as `rounding` leaves them, the same sum over |dz| |x|)"""
    x, dz = operands(case, nconv)
    if rounding == 'bf16':
        x, dz = x.bfloat16().float(), dz.bfloat16().float()
    return [(conv_grad(case, x[c], dz[c]), conv_grad(case, x[c].abs(), dz[c].abs())) for c in range(nconv)]


def descriptor(N, case, dtype, mode, x):
    B, T, Cin, Cout, kw, dil, pad = CASES[case]
    d = N.Conv1dDesc()
    d.dtype_in = d.dtype_out = dtype
    d.B, d.T_in, d.T_out, d.Cin, d.Cout, d.KW, d.dilation, d.stride = B, T, t_out(case), Cin, Cout, kw, dil, 1
    d.pad_mode = {'none': N.VP_PAD_NONE, 'reflect': N.VP_PAD_REFLECT}[pad]
    d.pad_left = 0 if pad == 'none' else dil * (kw - 1) // 2
    d.x, d.ldx, d.mfma_bf16 = x.data_ptr(), Cin, mode
    return d


def planned_family(N, d, dz, lddz, nbatch=1):
    fam = C.c_int(-1)
    N.check(N.lib().vp_conv1d_wgrad_plan(C.byref(d), dz.data_ptr(), lddz, nbatch, 0, C.byref(fam), None, None, None, None), N.ctx(0))
    return fam.value


def exact_workspace(N, d, nbatch=1):
    """exactly the queried bytes, every one 0xFF (NaN partials)"""
    return torch.full((int(N.lib().vp_conv1d_wgrad_workspace_bytes(C.byref(d))) * nbatch,), 0xFF, dtype=torch.uint8, device='cuda')


def rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def run_f32_operands(N, case, mode, family):
    lib, ctx = N.lib(), N.ctx(0)
    x, dz = operands(case)
    B, T, Cin, Cout, kw, dil, pad = CASES[case]
    xd, dzd = x[0].cuda().contiguous(), dz[0].cuda().contiguous()
    d = descriptor(N, case, N.VP_F32, mode, xd)
    assert planned_family(N, d, dzd, Cout) == family
    ws = exact_workspace(N, d)
    dW = torch.full((Cout, Cin, kw), float('nan'), device='cuda')
    N.check(lib.vp_conv1d_wgrad_oik_f32(ctx, C.byref(d), dzd.data_ptr(), Cout, dW.data_ptr(), ws.data_ptr(), ws.numel(), N.stream_ptr()), ctx)
    torch.cuda.synchronize()
    assert torch.isfinite(dW).all(), (case, mode)
    return dW.double().cpu()


@pytest.mark.parametrize('case', ['A', 'B'])
def test_wgrad_f32_family_vs_float64(N, case):
    """VP_WGRAD_F32 (conv_wgrad_kernel, mode 0): rel-L2 < 3e-5 against the float64 gradient, the bound test_conv2d_wgrad_vs_float64
    holds mode 0 to."""
    e = rel(run_f32_operands(N, case, 0, N.VP_WGRAD_F32), reference(case, 'f32')[0][0])
    print(f'[wgrad F32 {case}] rel-L2 {e:.2e}')
    assert e < 3e-5, e


@pytest.mark.parametrize('case', ['A', 'B'])
def test_wgrad_amp_family_f32_operands_vs_float64(N, case):
    """VP_WGRAD_AMP over f32 operands (conv_wgrad_amp_kernel<false>, mode 1; case A is NOT on the narrow kernel, which takes bf16
    operands only): rel-L2 < 3e-5 against the float64 gradient of the bf16-rounded operands -- products of bf16 values are exact in
    f32, the accumulation order is all that is left (test_conv2d_wgrad_vs_float64's mode-1 bound)."""
    e = rel(run_f32_operands(N, case, 1, N.VP_WGRAD_AMP), reference(case, 'bf16')[0][0])
    print(f'[wgrad AMP f32 operands {case}] rel-L2 vs the rounded operands {e:.2e}')
    assert e < 3e-5, e


def test_wgrad_x3_family_vs_float64(N):
    """VP_WGRAD_X3 (conv_wgrad_amp_kernel<false, true>, mode 2) on case A: rel-L2 < 2e-5 against the float64 gradient of the unrounded
    operands, the bound test_wgrad_split_precision_vs_float64 holds mode 2 to."""
    e = rel(run_f32_operands(N, 'A', 2, N.VP_WGRAD_X3), reference('A', 'f32')[0][0])
    print(f'[wgrad X3 A] rel-L2 {e:.2e}')
    assert e < 2e-5, e


def test_wgrad_amp_family_bf16_operands_vs_float64(N):
    """VP_WGRAD_AMP over bf16 operands (conv_wgrad_amp_kernel<true>): 200 rows of a 320 -> 192 1x1 layer whose input is columns 64 .. 383
    of a 384-wide buffer; Cout = 192 keeps it off the 256-tile kernel.  Max error <= 1e-5 max sum |dz| |x|, the bound of
    test_wgrad_of_bf16_operands_vs_float64: bf16 products are exact in f32."""
    lib, ctx = N.lib(), N.ctx(0)
    M, Cin, Cout, ldx, xoff = 200, 320, 192, 384, 64
    g = torch.Generator().manual_seed(M + Cout)
    x = torch.randn(M, ldx, generator=g).to(torch.bfloat16)
    dz = (torch.randn(M, Cout, generator=g) * 0.1).to(torch.bfloat16)
    xd, dzd = x.cuda(), dz.cuda()
    d = N.Conv1dDesc()
    d.dtype_in, d.dtype_out = N.VP_BF16, N.VP_F32
    d.B, d.T_in, d.T_out, d.Cin, d.Cout, d.KW, d.dilation, d.stride = 1, M, M, Cin, Cout, 1, 1, 1
    d.pad_mode, d.pad_left = N.VP_PAD_NONE, 0
    d.x, d.ldx, d.xoff, d.mfma_bf16 = xd.data_ptr(), ldx, xoff, 1
    assert planned_family(N, d, dzd, Cout) == N.VP_WGRAD_AMP
    ws = exact_workspace(N, d)
    dW = torch.full((Cout, Cin), float('nan'), device='cuda')
    N.check(lib.vp_conv1d_wgrad_bf16_oik(ctx, C.byref(d), dzd.data_ptr(), Cout, dW.data_ptr(), ws.data_ptr(), ws.numel(), N.stream_ptr()), ctx)
    torch.cuda.synchronize()
    xs = x[:, xoff:xoff + Cin].double()
    want, scale = dz.double().t() @ xs, (dz.double().abs().t() @ xs.abs()).max().item()
    err = (dW.double().cpu() - want).abs().max().item()
    print(f'[wgrad AMP bf16 operands] max err {err:.3e} against sum |dz||x| {scale:.3e}')
    assert err <= 1e-5 * scale, (err, scale)


@pytest.mark.parametrize('nbatch', [1, 3])
@pytest.mark.parametrize('case', ['N1', 'N2'])
def test_wgrad_n64_family_vs_float64(N, case, nbatch):
    """VP_WGRAD_N64 (conv_wgrad_n64_kernel) on bf16 operands, one conv and three of one geometry in one launch: conv c reads
    x + c M 64 and dz + c M Cout and writes dW[c].  Every conv of the batch: max error <= 1e-5 max sum |dz| |x| (bf16 products are
    exact in f32)."""
    lib, ctx = N.lib(), N.ctx(0)
    B, T, Cin, Cout, kw, dil, pad = CASES[case]
    M = B * T
    x, dz = operands(case, nbatch)
    xd, dzd = x.bfloat16().cuda().contiguous(), dz.bfloat16().cuda().contiguous()
    d = descriptor(N, case, N.VP_BF16, 1, xd)
    assert planned_family(N, d, dzd, Cout, nbatch) == N.VP_WGRAD_N64
    ws = exact_workspace(N, d, nbatch)
    dW = torch.full((nbatch, Cout, Cin, kw), float('nan'), device='cuda')
    if nbatch == 1:
        rc = lib.vp_conv1d_wgrad_bf16_oik(ctx, C.byref(d), dzd.data_ptr(), Cout, dW.data_ptr(), ws.data_ptr(), ws.numel(), N.stream_ptr())
    else:
        rc = lib.vp_conv1d_wgrad_bf16_oik_batched(ctx, C.byref(d), dzd.data_ptr(), Cout, dW.data_ptr(), nbatch, M * Cin, M * Cout, ws.data_ptr(),
                                                  ws.numel(), N.stream_ptr())
    N.check(rc, ctx)
    torch.cuda.synchronize()
    got = dW.double().cpu()
    for c, (want, mag) in enumerate(reference(case, 'bf16', nbatch)):
        err, scale = (got[c] - want).abs().max().item(), mag.max().item()
        print(f'[wgrad N64 {case} conv {c} of {nbatch}] max err {err:.3e} against sum |dz||x| {scale:.3e}')
        assert err <= 1e-5 * scale, (c, err, scale)


@pytest.mark.parametrize('entry', ['vp_conv1d_wgrad_f32', 'vp_conv1d_wgrad_oik_f32', 'vp_conv1d_wgrad_bf16_oik', 'vp_conv1d_wgrad_bf16_oik_batched'])
def test_wgrad_workspace_contract(N, entry):
    """Every launch entry point: a workspace one byte short of the query (nbatch x it for the batched one) is VP_EWORKSPACE, and
    nothing was launched: the NaN-filled dW is untouched.  The batched entry point refuses f32 operands with VP_EINVAL -- the only
    one that takes a count -- and a batch of two through the shared launch path is refused the same way for f32 operands
    (tests/test_wgrad_plan_cpu.py holds that on the plan)."""
    lib, ctx = N.lib(), N.ctx(0)
    case = 'N1'
    B, T, Cin, Cout, kw, dil, pad = CASES[case]
    M, bf = B * T, 'bf16' in entry
    nbatch = 2 if entry.endswith('batched') else 1
    x, dz = operands(case, nbatch)
    xd, dzd = (x.bfloat16() if bf else x).cuda().contiguous(), (dz.bfloat16() if bf else dz).cuda().contiguous()
    d = descriptor(N, case, N.VP_BF16 if bf else N.VP_F32, 1 if bf else 0, xd)
    need = int(lib.vp_conv1d_wgrad_workspace_bytes(C.byref(d))) * nbatch
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device='cuda')
    dW = torch.full((nbatch, Cout, Cin, kw), float('nan'), device='cuda')

    def launch(desc, nb, ws_bytes):
        if entry.endswith('batched'):
            return getattr(lib, entry)(ctx, C.byref(desc), dzd.data_ptr(), Cout, dW.data_ptr(), nb, M * Cin, M * Cout, ws.data_ptr(), ws_bytes,
                                       N.stream_ptr())
        return getattr(lib, entry)(ctx, C.byref(desc), dzd.data_ptr(), Cout, dW.data_ptr(), ws.data_ptr(), ws_bytes, N.stream_ptr())

    assert launch(d, nbatch, need - 1) == N.VP_EWORKSPACE
    if nbatch > 1:
        f = descriptor(N, case, N.VP_F32, 0, xd)
        assert launch(f, 2, need) == N.VP_EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(dW).all()
    assert launch(d, nbatch, need) == N.VP_OK
    torch.cuda.synchronize()
    assert torch.isfinite(dW).all()
