"""GPU parity tests of the 2-D path of the conv GEMM (MODE_2D of csrc/conv_gemm_impl.h through vp_conv1d_fwd, the zero-insert data
gradient and the 2-D taps of vp_conv1d_wgrad_oik_f32), per precision, against the float64 reference of tests/conv2d_oracle.py that
rounds the conv's operands the way each precision does.  Run with -m gpu on an MI355X.

Shapes (conv2d_oracle.CASES; B, T, F, Cin, Cout, k, stride_t, stride_f, dil) -- each is the smallest that crosses one edge:
  A   2, 9, 10, 64, 64, 3      BN = 64 tile; M = 180 (ragged second M-tile); Cout K = 36 864 >= 32 768: the wide partial-sum reduction
                               of the weight gradient with the 2-D tap permutation
  B   2, 11, 7, 48, 160, 3     BN = 128, two N-tiles, the second ragged; Cin = 48: a 32-element K-stage straddles taps; K = 432: the
                               split-plane weight rows of mode 3 are padded to 448
  C   3, 13, 9, 16, 96, 3 s2   stride on both axes, odd T and F (zero-insert data gradient); one ragged 128-column tile
  D1 / D2  2, 12, 10, 32, 64, 3, stride (2, 1) / (1, 2): stride_t != stride_f, both orders
  E   2, 17, 8, 24, 32, 3 d2   time dilation 2 (pad_t = 2)
  F   2, 33, 33, 32, 32, 3     M = 2178: 18 M-tiles > group_m = 16, the last group of the tile order is ragged
  G   3, 8, 9, 64, 256, 1 s2   strided 1x1 in MODE_2D, two full N-tiles
  H   2, 20, 16, 8, 32, 7 s3 pad 1   the 7x7 stride-3 pad-1 stem; data-gradient padding k - 1 - pad = 5
  I   1, 2, 1, 16, 16, 3       F = 1, T = 2: every tap but the centre column is padding; M = 2
  W   4, 64, 65, 32, 32, 3     M = 16 640 >= 256 x 64: the weight gradient's split count at its cap, trimmed to whole rounds of
                               workgroups under amp; ragged last split
"""
import contextlib
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import conv2d_oracle as co

pytestmark = pytest.mark.gpu

SEED = 3                                   # plain-conv inputs (the seed tests/test_conv2d_oracle_cpu.py pins the gaps at)
LINEAR_SEED = 5                            # Conv2dBlock without BatchNorm
WGRAD_CASES = ['A', 'B', 'C', 'D1', 'E', 'H', 'I', 'W']
LINEAR_CASES = ['A', 'B', 'C', 'D1', 'D2', 'E', 'G', 'H', 'W']
NAN = float('nan')


@pytest.fixture(scope='module')
def N():
    from ppvector import _native as N
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: these tests must run on an MI355X (no CPU fallback exists)')
    N.ctx(0)
    return N


@contextlib.contextmanager
def train_precision(mode):
    """The training engine's precision switch for the body; the previous setting comes back afterwards."""
    import ppvector
    amp0 = ppvector.get_train_amp()
    ppvector.set_train_amp(False)
    x30 = ppvector.get_train_x3()
    try:
        ppvector.set_train_amp(mode == 'amp')
        ppvector.set_train_x3(mode == 'x3')
        yield
    finally:
        ppvector.set_train_x3(x30)
        ppvector.set_train_amp(amp0)


def panel(w):
    """(Cout, Cin, kF, kT) -> the forward kernel's weight panel [Cout][(kt, kf, c)]."""
    return w.permute(0, 3, 2, 1).reshape(w.shape[0], -1)


def geometry(N, case, d=None):
    """The 2-D geometry fields of a vp_conv1d_desc for a case (f32 tensors unless the caller changes them)."""
    B, T, Fq, Cin, Cout, k, st, sf, dil, pad_t, pad_f, To, Fo = co.dims(case)
    d = d or N.Conv1dDesc()
    d.dtype_in = d.dtype_out = N.VP_F32
    d.B, d.T_in, d.T_out, d.Cin, d.Cout, d.KW, d.dilation, d.stride = B, T, To, Cin, Cout, k * k, dil, st
    d.KF, d.F_in, d.F_out, d.stride_f = k, Fq, Fo, sf
    d.pad_mode, d.pad_left, d.pad_f = N.VP_PAD_ZERO, pad_t, pad_f
    d.ldx, d.ldy = Cin, Cout
    return d


# ------------------------------------------------------------------------------------------- (a) forward kernel
_FWD_REF = {}


def fwd_reference(case, epilogue):
    """Inputs and the float64 forward in each mode, (B*T'*F', Cout) rows, computed once per (case, epilogue).  With the epilogue:
    relu((conv + bias) * bn_scale + bn_shift + res), as test_conv2d_resblock_epilogue builds it; `res` enters as the caller's output
    dtype stores it, so the reference is a function of it."""
    key = (case, epilogue)
    if key not in _FWD_REF:
        x, w, _ = co.conv_inputs(case, SEED)
        geom = co.geom_of(case)
        Cout = w.shape[0]
        conv = {m: co.rows(co.conv2d_fwd(x, w, geom, m)) for m in co.MODES}
        epi = None
        if epilogue:
            g = torch.Generator().manual_seed(SEED + 77)
            epi = dict(bias=torch.randn(Cout, generator=g).double(), sc=(torch.rand(Cout, generator=g) + 0.5).double(),
                       sh=torch.randn(Cout, generator=g).double(), res=torch.randn(conv['f32'].shape, generator=g).double())
        _FWD_REF[key] = (x, w, conv, epi)
    x, w, conv, epi = _FWD_REF[key]

    def ref(mode, res_bf16=False):
        if epi is None:
            return conv[mode]
        res = co.bf(epi['res']) if res_bf16 else epi['res']
        return torch.relu((conv[mode] + epi['bias']) * epi['sc'] + epi['sh'] + res)
    return x, w, epi, ref


def run_fwd(N, case, kind, x, w, epi):
    """One vp_conv1d_fwd launch.  kind: 'f32' / 'amp' / 'x3' / 'x3w' = f32 tensors with mfma_bf16 0 / 1 / 2 / 3 (3: the weights as split
    planes, rows zero-padded to 32), 'bf16' = bf16 tensors, 'bf16_f32' = bf16 operands, f32 output.  The output starts as NaN."""
    from ppvector.models.utils import pack_hl32
    lib, ctx = N.lib(), N.ctx(0)
    tin = torch.bfloat16 if kind.startswith('bf16') else torch.float32
    tout = torch.bfloat16 if kind == 'bf16' else torch.float32
    d = geometry(N, case)
    d.dtype_in, d.dtype_out = N.dtype_id(tin), N.dtype_id(tout)
    d.mfma_bf16 = {'amp': 1, 'x3': 2, 'x3w': 3}.get(kind, 0)
    xd = co.rows(x).to(tin).cuda().contiguous()
    wp = panel(w)
    if kind == 'x3w':
        K = wp.shape[1]
        wd = pack_hl32(F.pad(wp.float(), (0, (K + 31) // 32 * 32 - K))).cuda()
    else:
        wd = wp.to(tin).cuda().contiguous()
    y = torch.full((d.B * d.T_out * d.F_out, d.Cout), NAN, dtype=tout, device='cuda')
    d.x, d.w, d.y = xd.data_ptr(), wd.data_ptr(), y.data_ptr()
    keep = [xd, wd]
    if epi is not None:
        bd, sc, sh = (epi[k].float().cuda() for k in ('bias', 'sc', 'sh'))
        rd = epi['res'].to(tout).cuda().contiguous()
        keep += [bd, sc, sh, rd]
        d.bias, d.bn_scale, d.bn_shift, d.act2 = bd.data_ptr(), sc.data_ptr(), sh.data_ptr(), N.VP_ACT_RELU
        d.res, d.ld_res = rd.data_ptr(), d.Cout
    N.check(lib.vp_conv1d_fwd(ctx, C.byref(d), N.stream_ptr()), ctx)
    torch.cuda.synchronize()
    assert not torch.isnan(y).any(), (case, kind, 'output elements never written')
    return y.double().cpu()


@pytest.mark.parametrize('case,epilogue', [(c, False) for c in co.CASES] + [(c, True) for c in ('A', 'B', 'C')],
                         ids=list(co.CASES) + [c + '-epilogue' for c in ('A', 'B', 'C')])
def test_conv2d_fwd_vs_float64(N, case, epilogue):
    """vp_conv1d_fwd on a 2-D descriptor, every operand type dispatch_conv instantiates MODE_2D for, max abs error against the float64
    conv with the operands rounded as that type rounds them (outputs are O(1), |y| <= 5; constants as test_conv1d_plain /
    _mixed_precision / _split_precision / test_conv2d_resblock_epilogue hold the same kernel template to):
      f32 tensors, mode 0       vs 'f32'  < 2e-4
      mode 1                    vs 'amp'  < 2e-4 (same rounded operands, only f32 accumulation differs); and > 1e-3 from 'f32'
      modes 2, 3                vs 'f32'  < 5e-5; the single bf16 pass is >= 40x further off; and vs 'x3' (the same three operand
                                pairs, only f32 accumulation differs, as for mode 1 vs 'amp') < 2e-4
      bf16 -> bf16              vs 'amp'  < 2e-4 + 2^-8 max|ref| (the output's own rounding); bf16 -> f32 vs 'amp' < 2e-4
    bf16 tensors need Cin % 8 == 0 (every case here)."""
    x, w, epi, ref = fwd_reference(case, epilogue)
    Cin = w.shape[1]
    err = lambda y, r: (y - r).abs().max().item()
    y = {k: run_fwd(N, case, k, x, w, epi) for k in ('f32', 'amp', 'x3', 'x3w')}
    e0 = err(y['f32'], ref('f32'))
    e1, e1x = err(y['amp'], ref('amp')), err(y['amp'], ref('f32'))
    e2, e3 = err(y['x3'], ref('f32')), err(y['x3w'], ref('f32'))
    e2r, e3r = err(y['x3'], ref('x3')), err(y['x3w'], ref('x3'))
    tag = f'[conv2d fwd {case}{" + epilogue" if epilogue else ""}]'
    print(f'{tag} max abs err: mode 0 {e0:.2e} | mode 1 vs amp {e1:.2e}, vs f32 {e1x:.2e} | '
          f'mode 2 {e2:.2e}, mode 3 {e3:.2e}, vs x3 {e2r:.2e} / {e3r:.2e} (largest mode 2 - mode 3 difference {err(y["x3"], y["x3w"]):.2e})')
    assert e0 < 2e-4, e0
    assert e1 < 2e-4 and e1x > 1e-3, (e1, e1x)
    assert e2 < 5e-5 and e3 < 5e-5, (e2, e3)
    assert e2r < 2e-4 and e3r < 2e-4, (e2r, e3r)
    assert e1x >= 40 * e2 and e1x >= 40 * e3, (e1x, e2, e3)
    assert Cin % 8 == 0
    r16 = ref('amp', res_bf16=True)
    eb = err(run_fwd(N, case, 'bf16', x, w, epi), r16)
    ebf = err(run_fwd(N, case, 'bf16_f32', x, w, epi), ref('amp'))
    tol = 2e-4 + 2.0 ** -8 * r16.abs().max().item()
    print(f'{tag} bf16 -> bf16 {eb:.2e} (bound {tol:.2e}), bf16 -> f32 {ebf:.2e}')
    assert eb < tol, (eb, tol)
    assert ebf < 2e-4, ebf


# ------------------------------------------------------------------------------------------- (b) weight gradient
@pytest.mark.parametrize('case', WGRAD_CASES)
def test_conv2d_wgrad_vs_float64(N, case):
    """vp_conv1d_wgrad_oik_f32 with 2-D taps, dW in the model's (Cout, Cin, kF, kT) layout, rel-L2 (the bounds of
    test_wgrad_split_precision_vs_float64): mode 0 < 3e-5 vs 'f32'; mode 1 < 3e-5 vs 'amp' and > 1e-3 from 'f32'; mode 2 < 2e-5 vs
    'f32' with mode 1 >= 30x further off, and < 3e-5 vs 'x3' (same operand pairs, f32 accumulation alone: mode 0's bound).  dW starts as 7.0 and the partial-sum workspace as NaN."""
    lib, ctx = N.lib(), N.ctx(0)
    x, w, dz = co.conv_inputs(case, SEED)
    geom = co.geom_of(case)
    ref = {m: co.conv2d_wgrad(x, dz, w.shape, geom, m) for m in co.MODES}
    xd, dzd = co.rows(x).float().cuda().contiguous(), co.rows(dz).float().cuda().contiguous()
    out = {}
    for mode in (0, 1, 2):
        d = geometry(N, case)
        d.x, d.mfma_bf16 = xd.data_ptr(), mode
        dW = torch.full(tuple(w.shape), 7.0, device='cuda')
        ws = torch.full((int(lib.vp_conv1d_wgrad_workspace_bytes(C.byref(d))),), 0xFF, dtype=torch.uint8, device='cuda')
        N.check(lib.vp_conv1d_wgrad_oik_f32(ctx, C.byref(d), dzd.data_ptr(), d.Cout, dW.data_ptr(), ws.data_ptr(), ws.numel(),
                                            N.stream_ptr()), ctx)
        torch.cuda.synchronize()
        assert torch.isfinite(dW).all() and not (dW == 7.0).any(), (case, mode)
        out[mode] = dW.double().cpu()
    e0, e1, e1x, e2 = co.rel(out[0], ref['f32']), co.rel(out[1], ref['amp']), co.rel(out[1], ref['f32']), co.rel(out[2], ref['f32'])
    e2r = co.rel(out[2], ref['x3'])
    print(f'[conv2d wgrad {case}] rel-L2: mode 0 {e0:.2e} | mode 1 vs amp {e1:.2e}, vs f32 {e1x:.2e} | mode 2 {e2:.2e}, vs x3 {e2r:.2e}')
    assert e0 < 3e-5, e0
    assert e1 < 3e-5 and e1x > 1e-3, (e1, e1x)
    assert e2 < 2e-5 and e1x >= 30 * e2, (e2, e1x)
    assert e2r < 3e-5, e2r


# ------------------------------------------------------------------------------------------- (c), (d) the training unit
def run_unit(case, mode, inp, act, bn):
    """Conv2dBlock forward + backward under one training precision; y, dx (rows), dW, dbias, dgamma, dbeta."""
    from ppvector.train.functions import Conv2dBlock
    B, T, Fq, Cin, Cout, k, st, sf, dil, pad_t, pad_f, To, Fo = co.dims(case)
    cfg = dict(B=B, T=T, F=Fq, stride_t=st, stride_f=sf, dilation=dil)
    if co.CASES[case][9] is not None:
        cfg['pad'] = co.CASES[case][9]
    if act is not None:
        cfg['act'] = act
    leaf = lambda t: t.float().cuda().contiguous().requires_grad_()
    xd, wd, bd = leaf(co.rows(inp['x'])), leaf(inp['w']), leaf(inp['bias'])
    gd = hd = rm = rv = None
    if bn:
        gd, hd = leaf(inp['gamma']), leaf(inp['beta'])
        rm, rv = torch.zeros(Cout, device='cuda'), torch.ones(Cout, device='cuda')
    with train_precision(mode):
        out = Conv2dBlock.apply(xd, wd, bd, gd, hd, rm, rv, cfg)
        out.backward(co.rows(inp['dy']).float().cuda().contiguous())
        torch.cuda.synchronize()
    assert out.shape == (B * To * Fo, Cout)
    got = dict(y=out.detach(), dx=xd.grad, dW=wd.grad, dbias=bd.grad, dgamma=gd.grad if bn else None, dbeta=hd.grad if bn else None)
    for k_, v in got.items():
        assert v is None or torch.isfinite(v).all(), (case, mode, k_)
    return got


def unit_errors(got, ref, keys):
    return {k: co.rel(got[k], co.rows(ref[k]) if k in ('y', 'dx') else ref[k]) for k in keys}


@pytest.mark.parametrize('case', LINEAR_CASES)
def test_conv2d_block_linear_vs_float64(N, case):
    """Conv2dBlock without BatchNorm or activation (conv + bias): the unit's own plumbing -- weight layouts, cfg's stride_t / stride_f /
    dilation / pad, zero insertion, data-gradient padding -- through autograd under f32, set_train_amp and set_train_x3.  All of it is
    linear (no masks), every GEMM sees the same operands as the reference, rel-L2 against the reference of the active mode:
    f32 y < 2e-6, dx / dW < 3e-5; amp the same against 'amp'; x3 y < 2e-5, dx / dW < 3e-5 against 'f32'.  amp is > 1e-3 from 'f32' on
    all three and >= 30x further from it than x3; x3 against its own reference 'x3' (same operand pairs) meets the f32 bounds.  dbias (column sums of dy, no GEMM) < 3e-5 in every mode."""
    inp = co.unit_inputs(case, LINEAR_SEED, None, bn=False)
    ref = {m: co.unit_reference(case, m, LINEAR_SEED, None, bn=False) for m in co.MODES}
    keys = ('y', 'dx', 'dW', 'dbias')
    got = {m: run_unit(case, m, inp, None, False) for m in co.MODES}
    e = {'f32': unit_errors(got['f32'], ref['f32'], keys), 'amp': unit_errors(got['amp'], ref['amp'], keys),
         'x3': unit_errors(got['x3'], ref['f32'], keys), 'x3_vs_x3': unit_errors(got['x3'], ref['x3'], keys),
         'amp_vs_f32': unit_errors(got['amp'], ref['f32'], keys)}
    for m, v in e.items():
        print(f'[conv2d block linear {case}] {m:10s} ' + '  '.join(f'{k} {v[k]:.2e}' for k in keys))
    for m, ybound in (('f32', 2e-6), ('amp', 2e-6), ('x3', 2e-5), ('x3_vs_x3', 2e-6)):
        assert e[m]['y'] < ybound, (m, e[m])
        assert e[m]['dx'] < 3e-5 and e[m]['dW'] < 3e-5 and e[m]['dbias'] < 3e-5, (m, e[m])
    for k in ('y', 'dx', 'dW'):
        assert e['amp_vs_f32'][k] > 1e-3 and e['amp_vs_f32'][k] >= 30 * e['x3'][k], (k, e['amp_vs_f32'][k], e['x3'][k])


@pytest.mark.parametrize('case', list(co.UNIT_CASES))
def test_conv2d_block_bn_clamp_vs_float64(N, case):
    """Conv2D -> BatchNorm2D(batch statistics) -> ReLU (A, C, D1) / Hardtanh(0, 20) with both clamps active (B) in all three training
    precisions, at seeds whose pre-activations keep 1e-4 clear of the clamp edges (conv2d_oracle.UNIT_CASES), rel-L2:
      f32   y < 2e-6, gradients < 3e-5 vs 'f32' (the bounds of test_conv2d_block_grads_vs_autograd)
      x3    y < 2e-5, gradients < 3e-5 vs 'f32'; and the f32 bounds vs 'x3', whose conv sums the same three operand pairs
      amp   vs the amp reference, bound = max(the f32 bound, gap / 10) per tensor, gap = rel(ref 'amp', ref 'f32') from the two float64
            references alone: a tenth of the gap separates 'the right operands rounded' from 'wrong or no operand rounded' by 10x; the
            f32 floor covers f32 accumulation.  (dz reaches the backward GEMMs through BatchNorm's backward in f32 here and in float64
            there, so a few of its elements may round to the other bf16 neighbour: measured <= 6e-7 in all, gap / 10 >= 1.5e-4.)"""
    act, seed = co.UNIT_CASES[case]
    inp = co.unit_inputs(case, seed, act)
    ref = {m: co.unit_reference(case, m, seed, act) for m in co.MODES}
    assert min(r['edge_margin'] for r in ref.values()) >= co.EDGE_MARGIN
    if act == 'hardtanh':
        assert ref['f32']['lo'] > 0.05 and ref['f32']['hi'] > 0.05, (ref['f32']['lo'], ref['f32']['hi'])
    keys = ('y', 'dx', 'dW', 'dgamma', 'dbeta')
    floor = dict(y=2e-6, dx=3e-5, dW=3e-5, dgamma=3e-5, dbeta=3e-5)
    bounds = {'f32': floor, 'x3': dict(floor, y=2e-5), 'x3 vs x3': floor}
    gap = {k: co.rel(ref['amp'][k], ref['f32'][k]) for k in keys}
    bounds['amp'] = {k: max(floor[k], gap[k] / 10) for k in keys}
    failed = []
    for mode in co.MODES:
        got = run_unit(case, mode, inp, act, True)
        checks = [(mode, unit_errors(got, ref['amp' if mode == 'amp' else 'f32'], keys))]
        if mode == 'x3':
            checks.append(('x3 vs x3', unit_errors(got, ref['x3'], keys)))
        for name, e in checks:
            for k in keys:
                print(f'[conv2d block {act} {case}] {name:8s} {k:6s} err {e[k]:.2e}  bound {bounds[name][k]:.2e}' +
                      (f'  (amp gap {gap[k]:.2e})' if mode == 'amp' else ''))
                if not e[k] < bounds[name][k]:
                    failed.append((name, k, e[k], bounds[name][k]))
        assert got['dbias'].abs().max().item() < 1e-5                # a bias in front of BatchNorm has zero gradient
    assert not failed, failed


# ------------------------------------------------------------------------------------------- (e) refusals
def test_conv2d_refusals(N):
    """What the 2-D path does not build is an error before any launch: per-utterance epilogue terms (rowbias, psum, gate) and hl32
    tensors are VP_EUNSUP; reflect / no padding and a tap count that is no multiple of KF are VP_EINVAL, in the forward and in the
    weight gradient.  The output keeps its sentinel every time, and the same descriptor without the offending field runs."""
    lib, ctx = N.lib(), N.ctx(0)
    case = (2, 5, 6, 32, 32, 3, 1, 1, 1, None)
    B, T, Fq, Cin, Cout, k, st, sf, dil, pad_t, pad_f, To, Fo = co.dims(case)
    M = B * To * Fo
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B * T * Fq, Cin, generator=g).cuda()
    w = (torch.randn(Cout, k * k * Cin, generator=g) / (k * k * Cin) ** 0.5).cuda()
    dz = torch.randn(M, Cout, generator=g).cuda()
    side = torch.ones(4 * M * Cout, device='cuda')                    # any of rowbias / psum / gate (large enough for each)
    y = torch.full((M, Cout), 7.0, device='cuda')
    dW = torch.full((Cout, Cin, k, k), 7.0, device='cuda')

    def desc(**fields):
        d = geometry(N, case)
        d.x, d.w, d.y = x.data_ptr(), w.data_ptr(), y.data_ptr()
        for name, v in fields.items():
            setattr(d, name, v)
        return d

    def fwd(want, text, **fields):
        rc = lib.vp_conv1d_fwd(ctx, C.byref(desc(**fields)), N.stream_ptr())
        assert rc == want and text in lib.vp_last_error(ctx), (fields, rc, lib.vp_last_error(ctx))

    def wgrad(want, text, **fields):
        d = desc(**fields)
        ws = torch.empty(int(lib.vp_conv1d_wgrad_workspace_bytes(C.byref(geometry(N, case)))), dtype=torch.uint8, device='cuda')
        rc = lib.vp_conv1d_wgrad_oik_f32(ctx, C.byref(d), dz.data_ptr(), Cout, dW.data_ptr(), ws.data_ptr(), ws.numel(), N.stream_ptr())
        assert rc == want and text in lib.vp_last_error(ctx), (fields, rc, lib.vp_last_error(ctx))

    fwd(N.VP_EUNSUP, b'1-D only', rowbias=side.data_ptr())
    fwd(N.VP_EUNSUP, b'1-D only', psum=side.data_ptr(), psumsq=side.data_ptr())
    fwd(N.VP_EUNSUP, b'1-D only', gate=side.data_ptr(), gate_len=T, gate_nseg=1)
    for tin, tout in ((N.VP_HL32, N.VP_HL32), (N.VP_F32, N.VP_HL32), (N.VP_HL32, N.VP_F32)):
        fwd(N.VP_EUNSUP, b'hl32 is built for 1-D', dtype_in=tin, dtype_out=tout, mfma_bf16=2)
    for call, text in ((fwd, b'conv2d: bad geometry'), (wgrad, b'bad 2-D geometry')):
        call(N.VP_EINVAL, text, pad_mode=N.VP_PAD_REFLECT)
        call(N.VP_EINVAL, text, pad_mode=N.VP_PAD_NONE, pad_left=0, pad_f=0, T_out=T - 2, F_out=Fq - 2)
        call(N.VP_EINVAL, text, KF=2)                                 # KW = 9 taps
    torch.cuda.synchronize()
    assert torch.all(y == 7.0) and torch.all(dW == 7.0)               # nothing launched
    fwd(N.VP_OK, b'')
    wgrad(N.VP_OK, b'')
    torch.cuda.synchronize()
    assert not (y == 7.0).any() and not (dW == 7.0).any()
