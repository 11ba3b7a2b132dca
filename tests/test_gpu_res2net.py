"""Res2Net on the MI355X (csrc/res2net.hip): the kernel doors against float64 / PyTorch-CPU autograd, the eval forward of all three
engines against the reference-generated golden and the float64 oracle, and the engine's behaviour (bf16 warning, forward_streams)."""
import ctypes as C
import json
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import res2net_oracle as o2

pytestmark = pytest.mark.gpu

TOL = {'float32': 3e-4, 'float32x3': 6e-4, 'bfloat16': 8e-2}        # the ResNetSE golden test's bounds


def _N():
    from ppvector import _native as N
    return N


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def _to_btfc(x):                      # (B, C, F, T) -> (B, T, F, C)
    return x.permute(0, 3, 2, 1).contiguous()


def _from_btfc(x):                    # (B, T, F, C) -> (B, C, F, T)
    return x.permute(0, 3, 2, 1).contiguous()


@pytest.mark.parametrize('T,Fd,Cm', [(28, 64, 32), (98, 64, 32), (298, 64, 32), (2000, 64, 32), (28, 80, 32), (98, 80, 32),
                                     (298, 80, 32), (2000, 80, 32), (298, 80, 128), (98, 80, 256)])
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_stem_door_matches_float64(T, Fd, Cm, dtype):
    """Cm 128 / 256: more channels than one LDS tile holds at F = 80 -- the channels are split over workgroups."""
    N = _N()
    B = 3
    rng = np.random.RandomState(T + Fd)
    x = torch.from_numpy(rng.standard_normal((B, T, Fd)) * 3.0)
    w = torch.from_numpy(rng.uniform(-0.3, 0.3, (Cm, 1, 7, 7)))
    bias = torch.from_numpy(rng.uniform(-0.2, 0.2, Cm))
    scale = torch.from_numpy(rng.uniform(0.5, 1.5, Cm))
    shift = torch.from_numpy(rng.uniform(-0.3, 0.3, Cm))
    td = torch.float32 if dtype == 'float32' else torch.bfloat16
    xd = x.to(td)
    with torch.no_grad():
        xin = xd.double().transpose(1, 2).unsqueeze(1)
        ref = F.relu((F.conv2d(xin, w, bias, stride=3, padding=1)) * scale[None, :, None, None] + shift[None, :, None, None])
        ref = _to_btfc(o2.max_pool(ref))
    out = torch.empty(ref.shape, dtype=td, device='cuda')
    wp = w[:, 0].permute(0, 2, 1).reshape(Cm, 49).float().cuda()            # tap = kt * 7 + kf
    args = [t.float().cuda() for t in (bias, scale, shift)]
    ctx = N.ctx()
    N.check(N.lib().vp_res2net_stem_fwd(ctx, N.VP_F32 if dtype == 'float32' else N.VP_BF16, xd.cuda().data_ptr(), out.data_ptr(),
                                        wp.data_ptr(), args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), B, T, Fd, Cm,
                                        N.stream_ptr()), ctx)
    got = out.double().cpu()
    rel = _rel(got.numpy(), ref.numpy())
    assert rel < (2e-6 if dtype == 'float32' else 6e-3), rel


def _slice_case(rng, B, T, Fd, Cs, ld, off):
    base = torch.from_numpy(rng.standard_normal((B * T * Fd, ld))).float()
    x = base[:, off:off + Cs].reshape(B, T, Fd, Cs)
    return base, x


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('shape', [(2, 13, 7), (3, 25, 13), (1, 5, 3)])
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_avgpool_door_matches_exclusive_average(stride, shape, dtype):
    N = _N()
    B, T, Fd = shape
    Cs, ldx, xoff, ldy, yoff = 16, 48, 8, 40, 24
    rng = np.random.RandomState(T * 7 + stride)
    base, x = _slice_case(rng, B, T, Fd, Cs, ldx, xoff)
    td = torch.float32 if dtype == 'float32' else torch.bfloat16
    xb = base.to(td).cuda()
    To, Fo = (T - 1) // stride + 1, (Fd - 1) // stride + 1
    y = torch.full((B * To * Fo, ldy), 7.0, dtype=td, device='cuda')
    ctx = N.ctx()
    N.check(N.lib().vp_avgpool3x3_fwd(ctx, N.VP_F32 if dtype == 'float32' else N.VP_BF16, xb.data_ptr(), ldx, xoff, y.data_ptr(),
                                      ldy, yoff, B, T, Fd, Cs, stride, N.stream_ptr()), ctx)
    ref = _to_btfc(F.avg_pool2d(_from_btfc(x.to(td).double()), 3, stride=stride, padding=1, count_include_pad=False))
    got = y.double().cpu()
    assert torch.all(got[:, :yoff] == 7.0) and torch.all(got[:, yoff + Cs:] == 7.0)        # only the slice is written
    rel = _rel(got[:, yoff:yoff + Cs].reshape(ref.shape).numpy(), ref.numpy())
    assert rel < (1e-6 if dtype == 'float32' else 6e-3), rel


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('shape', [(2, 13, 7), (3, 26, 14), (1, 5, 3)])
def test_avgpool_backward_matches_autograd(stride, shape):
    N = _N()
    B, T, Fd = shape
    Cs, ldg, goff, ldd, doff = 12, 20, 4, 32, 16
    rng = np.random.RandomState(T + 31 * stride)
    x = torch.from_numpy(rng.standard_normal((B, Cs, Fd, T))).requires_grad_(True)
    y = F.avg_pool2d(x, 3, stride=stride, padding=1, count_include_pad=False)
    gy = torch.from_numpy(rng.standard_normal(y.shape))
    y.backward(gy)
    To, Fo = y.shape[3], y.shape[2]
    gbase = torch.zeros(B * To * Fo, ldg)
    gbase[:, goff:goff + Cs] = _to_btfc(gy).reshape(-1, Cs).float()
    gd = gbase.cuda()
    dx = torch.full((B * T * Fd, ldd), 5.0, device='cuda')
    ctx = N.ctx()
    N.check(N.lib().vp_avgpool3x3_bwd_f32(ctx, gd.data_ptr(), ldg, goff, dx.data_ptr(), ldd, doff, B, T, Fd, Cs, stride, N.stream_ptr()),
            ctx)
    got = dx.cpu()
    assert torch.all(got[:, :doff] == 5.0)
    ref = _to_btfc(x.grad).reshape(-1, Cs).numpy()
    assert _rel(got[:, doff:doff + Cs].numpy(), ref) < 1e-6


@pytest.mark.parametrize('shape', [(2, 26, 13), (3, 9, 8), (1, 5, 3)])
@pytest.mark.parametrize('ties', [False, True])
def test_maxpool_forward_backward_match_autograd(shape, ties):
    """Forward and the first-maximum backward, including post-ReLU maps with all-zero (tied) windows."""
    N = _N()
    B, T, Fd = shape
    Cm = 8
    rng = np.random.RandomState(T * 3 + int(ties))
    v = rng.standard_normal((B, Cm, Fd, T))
    if ties:
        v = np.maximum(v - 1.0, 0.0)                 # mostly zeros: many windows hold only tied zeros
        v[0, 0] = 0.0
    x = torch.from_numpy(v).float().double().requires_grad_(True)
    y = o2.max_pool(x)
    gy = torch.from_numpy(rng.standard_normal(y.shape))
    y.backward(gy)
    xd = _to_btfc(x.detach()).float().cuda()
    yd = torch.empty(_to_btfc(y.detach()).shape, device='cuda')
    ctx = N.ctx()
    N.check(N.lib().vp_maxpool3x3_fwd_f32(ctx, xd.data_ptr(), yd.data_ptr(), B, T, Fd, Cm, N.stream_ptr()), ctx)
    assert torch.equal(yd.cpu().double(), _to_btfc(y.detach()))
    gd = _to_btfc(gy).float().cuda()
    dx = torch.empty_like(xd)
    N.check(N.lib().vp_maxpool3x3_bwd_f32(ctx, xd.data_ptr(), gd.data_ptr(), dx.data_ptr(), B, T, Fd, Cm, N.stream_ptr()), ctx)
    assert _rel(dx.cpu().numpy(), _to_btfc(x.grad).numpy()) < 1e-6
    dx2 = torch.empty_like(xd)
    N.check(N.lib().vp_maxpool3x3_bwd_f32(ctx, xd.data_ptr(), gd.data_ptr(), dx2.data_ptr(), B, T, Fd, Cm, N.stream_ptr()), ctx)
    assert torch.equal(dx, dx2)                       # gather, no atomics: deterministic


def _model(kw, seed):
    from ppvector.models.res2net import Res2Net
    okw = {k: v for k, v in kw.items() if k not in ('input_size', 'embd_dim')}
    p = o2.res2net_params(input_size=kw['input_size'], embd_dim=kw.get('embd_dim', 192), seed=seed, **okw)
    m = Res2Net(**kw)
    m.load_state_dict(p)
    return m.cuda().eval(), p, okw


def test_res2net_matches_reference_golden(golden_dir):
    """Every configuration of the reference-generated golden on the three engines: the shipped one at F = 80 and F = 64, a scale-4 one
    of 'stage' blocks only, and a scale-4 one with two blocks in layers 1-2 ('normal' blocks: the sp + spx[i] chain through the conv
    epilogue's aux output; chunk widths 4 / 8, zero-padded to 8)."""
    g = np.load(f'{golden_dir}/res2net_ref_small.npz')
    for n in json.loads(str(g['configs'])):
        kw = json.loads(str(g[f'config__{n}']))
        m, _, _ = _model(kw, int(g[f'param_seed__{n}']))
        x = torch.from_numpy(g[f'x__{n}']).cuda()
        ref = g[f'emb_eval__{n}']
        for dtype, tol in TOL.items():
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                emb = m.engine(dtype).forward(x).cpu().numpy()
            rel = _rel(emb, ref)
            print(f'[res2net golden {n} {dtype}] rel-L2 {rel:.3e}')
            assert rel < tol, (n, dtype, rel)


@pytest.mark.parametrize('T', [28, 298, 2000])
def test_res2net_matches_float64_oracle(T):
    """The shipped configuration at B = 4 against the float64 oracle, on the three engines."""
    kw = dict(input_size=80, m_channels=32, embd_dim=192)
    m, p, okw = _model(kw, 1000 + T)
    rng = np.random.RandomState(T)
    x = (rng.standard_normal((4, T, 80)) * 3.0).astype(np.float32)
    with torch.no_grad():
        ref = o2.res2net_forward({k: v.double() for k, v in p.items()}, torch.from_numpy(x).double(), **okw).numpy()
    xd = torch.from_numpy(x).cuda()
    for dtype, tol in TOL.items():
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            emb = m.engine(dtype).forward(xd).cpu().numpy()
        rel = _rel(emb, ref)
        print(f'[res2net T={T} {dtype}] rel-L2 {rel:.3e}')
        assert rel < tol, (T, dtype, rel)


def test_res2net_model_forward_and_warnings():
    """model(x) in eval mode runs the engine; the f32 engine is silent, the bf16 engine warns as for the other backbones, and so does the
    split-precision engine: on this backbone it misses the 1e-4 score bar at trained weights (tests/test_gpu_res2net_train.py)."""
    import ppvector
    kw = dict(input_size=80)
    m, _, _ = _model(kw, 7)
    x = torch.randn(2, 120, 80, device='cuda')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        e32 = m.engine('float32').forward(x)
        e = m(x)
    assert ppvector.get_compute_dtype() != 'float32' or torch.equal(e, e32)
    with pytest.warns(RuntimeWarning, match='bf16 engine') as rec:
        m.engine('bfloat16')
    assert "The 'float32' engine (the default) meets it" in str(rec[0].message)
    with pytest.warns(RuntimeWarning, match="split-precision 'float32x3' engine is outside"):
        m.engine('float32x3').forward(x)


@pytest.mark.parametrize('dtype', ['float32', 'float32x3', 'bfloat16'])
def test_forward_streams_bit_identical(dtype):
    kw = dict(input_size=80)
    m, _, _ = _model(kw, 11)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        eng = m.engine(dtype)
    x = torch.randn(12, 150, 80, device='cuda') * 3.0
    for S in (2, 4):
        bounds = [(12 * i) // S for i in range(S + 1)]
        seq = torch.cat([eng.forward(x[bounds[i]:bounds[i + 1]]) for i in range(S)])
        par = eng.forward_streams(x, S)
        torch.cuda.synchronize()
        assert torch.equal(seq, par), (dtype, S)


def test_wide_stem_model_matches_oracle():
    """m_channels 128 (the stem's channels split over workgroups) through the whole forward, f32 engine."""
    kw = dict(input_size=80, m_channels=128, layers=[1, 1, 1, 1], scale=2, embd_dim=192)
    m, p, okw = _model(kw, 21)
    x = (np.random.RandomState(5).standard_normal((2, 120, 80)) * 3.0).astype(np.float32)
    with torch.no_grad():
        ref = o2.res2net_forward({k: v.double() for k, v in p.items()}, torch.from_numpy(x).double(), **okw).numpy()
    emb = m.engine('float32').forward(torch.from_numpy(x).cuda()).cpu().numpy()
    assert _rel(emb, ref) < TOL['float32']


def test_workspace_and_refusals():
    N = _N()
    m, _, _ = _model(dict(input_size=80), 3)
    eng = m.engine('float32')
    assert N.lib().vp_res2net_workspace_bytes(C.byref(eng.W), 4, 298) > 0
    with pytest.raises(N.VpmiError):
        eng.forward(torch.randn(2, 4, 80, device='cuda'))       # fewer frames than the 7x7 stride-3 stem needs
