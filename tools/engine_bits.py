"""Bit-identity instrument for changes that must not move a single output bit of the eval forwards (host-side refactors of the launch
layer): writes the embeddings of every backbone x engine at a small and a BASELINE-sized batch to .npy, from seeded weights and a seeded
batch.  Run it on two checkouts (each with its own build), then compare the two directories.

    python tools/engine_bits.py --out DIR            # 36 arrays (+ EcapaTdnn float32x3 says which path ran; VPMI_X3_GENERIC=1 pins the generic one)
    python tools/engine_bits.py --compare DIR_A DIR_B
    python tools/engine_bits.py --heads --out DIR    # instead: every output of the head / loss entry points (csrc/head.hip, head_tiled.hip, losses.hip)
    python tools/engine_bits.py --pooling --out DIR  # instead: every output of the pooling-statistics entry points (csrc/pooling_stats.hip)
    python tools/engine_bits.py --bn --out DIR       # instead: every output of the BatchNorm training unit (csrc/bn_train.hip), its Functions, one training step per backbone
    python tools/engine_bits.py --time-b1           # 200 B = 1 forwards of ECAPA and ResNetSE per engine, GPU events (host launch overhead)
"""
import argparse
import itertools
import math
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


# --heads: (tag, B, D, C).  Every entry point that takes the shape runs on it: the logits-tensor ones always, the class-tiled forward
# where D % 4 == 0 and D <= 256, the class-tiled backward where B <= 128 and D == 192.
HEAD_SHAPES = (('B5_D20_C67', 5, 20, 67), ('B48_D192_C2796', 48, 192, 2796), ('B200_D192_C2560', 200, 192, 2560), ('B33_D100_C65', 33, 100, 65))
LOGIT_SHAPES = ((5, 67), (37, 67))                   # (B, C) of the logits-level family; SubCenter runs K = 3 on them
HEAD_M, HEAD_TABLE_M, HEAD_SCALE = 0.2, 0.35, 32.0   # launch scalar; the margin the table holds when one is set
# the one output whose bits may move between builds that reduce the row losses differently (sum / n against sum * (1 / n)): <= 1 ulp
ULP1 = ('vp_margin_ce_fwd.loss', 'vp_margin_ce_bwd.loss', 'vp_sphereface2.loss')


def _planted_cosines(m):
    """Target cosines on both sides of th = cos(pi - m) and of 0 (the first five: the smallest batch holds them), then the rest of the range."""
    th = math.cos(math.pi - m)
    return (th - 0.003, th + 0.003, -0.003, 0.003, 0.6, -0.99, -0.2, 0.3, 0.9)


def dump_heads(out):
    """Planted-cosine inputs of tests/head_oracle.py x hard / easy margin x label smoothing 0 / 0.1 x margin table unset / set."""
    import torch
    from ppvector import _native as N
    from tests import head_oracle as ho
    os.makedirs(out, exist_ok=True)
    lib, ctx, st = N.lib(), N.ctx(0), N.stream_ptr()
    table = torch.tensor([HEAD_TABLE_M, math.cos(HEAD_TABLE_M), math.sin(HEAD_TABLE_M), math.cos(math.pi - HEAD_TABLE_M),
                          1.0 + math.cos(math.pi - HEAD_TABLE_M)], dtype=torch.float64).to(torch.float32).cuda()
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device='cuda')       # noqa: E731
    ws = lambda n: torch.zeros(max(1, n), dtype=torch.uint8, device='cuda')                      # noqa: E731
    count = blank = 0

    def save(tag, **arrays):
        nonlocal count, blank
        torch.cuda.synchronize()
        for k, v in arrays.items():
            np.save(os.path.join(out, f'heads_{tag}.{k}.npy'), v.cpu().numpy())
            count += 1
            blank += not (bool(torch.isfinite(v).all()) and bool(v.any()))       # an output nobody wrote (zeros) or a NaN says nothing

    for easy, ls, tab in itertools.product((0, 1), (0.0, 0.1), (False, True)):
        cs = _planted_cosines(HEAD_TABLE_M if tab else HEAD_M)
        cfg = f'easy{easy}_ls{ls}_{"table" if tab else "scalar"}'
        m, sc = HEAD_M, HEAD_SCALE
        N.check(lib.vp_set_margin_table(ctx, table.data_ptr() if tab else None), ctx)
        try:
            for name, B, D, C in HEAD_SHAPES:
                emb, W, y = (t.cuda() for t in ho.plant(B, D, C, cs, 7 * B + C))
                e, w, yp = emb.data_ptr(), W.data_ptr(), y.data_ptr()
                loss, row, lg = z(1), z(B), z(B, C)
                s = ws(lib.vp_cosine_aam_workspace_bytes(B, D, C))
                N.check(lib.vp_cosine_aam_ce_fwd(ctx, e, w, yp, B, D, C, m, sc, ls, easy, loss.data_ptr(), lg.data_ptr(), row.data_ptr(),
                                                 s.data_ptr(), s.numel(), st), ctx)
                save(f'{name}_{cfg}_vp_cosine_aam_ce_fwd', loss=loss, row_loss=row, logits=lg)
                loss, row = z(1), z(B)
                N.check(lib.vp_aam_ce_fwd(ctx, lg.data_ptr(), yp, B, C, m, sc, ls, easy, loss.data_ptr(), row.data_ptr(), st), ctx)
                save(f'{name}_{cfg}_vp_aam_ce_fwd', loss=loss, row_loss=row)
                loss, row, dl = z(1), z(B), z(B, C)
                N.check(lib.vp_aam_ce_bwd(ctx, lg.data_ptr(), yp, B, C, m, sc, ls, easy, 1.0, dl.data_ptr(), loss.data_ptr(), row.data_ptr(), st), ctx)
                save(f'{name}_{cfg}_vp_aam_ce_bwd', loss=loss, row_loss=row, dlogits=dl)
                de, dw = z(B, D), z(D, C)
                s = ws(lib.vp_cosine_logits_bwd_workspace_bytes(B, D, C))
                N.check(lib.vp_cosine_logits_bwd(ctx, e, w, dl.data_ptr(), B, D, C, de.data_ptr(), dw.data_ptr(), s.data_ptr(), s.numel(), st), ctx)
                save(f'{name}_{cfg}_vp_cosine_logits_bwd', demb=de, dW=dw)
                loss, de, dw = z(1), z(B, D), z(D, C)
                s = ws(lib.vp_cosine_aam_ce_bwd_workspace_bytes(B, D, C))
                N.check(lib.vp_cosine_aam_ce_bwd(ctx, e, w, yp, B, D, C, m, sc, ls, easy, 1.0, de.data_ptr(), dw.data_ptr(), loss.data_ptr(),
                                                 s.data_ptr(), s.numel(), st), ctx)
                save(f'{name}_{cfg}_vp_cosine_aam_ce_bwd', loss=loss, demb=de, dW=dw)
                if D % 4 == 0 and D <= 256:
                    loss, row, lse, cinv, pred = z(1), z(B), z(B), z(C), z(B, dtype=torch.int32)
                    s = ws(lib.vp_cosine_aam_tiled_workspace_bytes(B, D, C))
                    N.check(lib.vp_cosine_aam_tiled_fwd(ctx, e, w, yp, B, D, C, m, sc, ls, easy, loss.data_ptr(), row.data_ptr(), lse.data_ptr(),
                                                        cinv.data_ptr(), pred.data_ptr(), s.data_ptr(), s.numel(), st), ctx)
                    save(f'{name}_{cfg}_vp_cosine_aam_tiled_fwd', loss=loss, row_loss=row, lse=lse, cinv=cinv, pred=pred)
                if B <= 128 and D == 192:
                    loss, de, dw, pred = z(1), z(B, D), z(D, C), z(B, dtype=torch.int32)
                    s = ws(lib.vp_cosine_aam_tiled_bwd_workspace_bytes(B, D, C))
                    N.check(lib.vp_cosine_aam_tiled_bwd(ctx, e, w, yp, B, D, C, m, sc, ls, easy, 1.0, de.data_ptr(), dw.data_ptr(), loss.data_ptr(),
                                                        pred.data_ptr(), s.data_ptr(), s.numel(), st), ctx)
                    save(f'{name}_{cfg}_vp_cosine_aam_tiled_bwd', loss=loss, pred=pred, demb=de, dW=dw)
            for B, C in LOGIT_SHAPES:
                kinds = [('AAM', N.VP_LOSS_AAM, 1), ('SUBCENTER', N.VP_LOSS_SUBCENTER, 3), ('AM', N.VP_LOSS_AM, 1), ('ARM', N.VP_LOSS_ARM, 1),
                         ('CE', N.VP_LOSS_CE, 1)]
                for kname, kind, K in kinds:
                    lg, y, _ = ho.plant_logits(B, C, K, cs, 11 * B + K)
                    lg, y = lg.cuda(), y.cuda()
                    tag = f'B{B}_C{C}_K{K}_{kname}_{cfg}'
                    loss, row = z(1), z(B)
                    N.check(lib.vp_margin_ce_fwd(ctx, lg.data_ptr(), y.data_ptr(), B, C, K, kind, m, sc, ls, easy, loss.data_ptr(), row.data_ptr(),
                                                 st), ctx)
                    save(f'{tag}_vp_margin_ce_fwd', loss=loss, row_loss=row)
                    loss, row, dl = z(1), z(B), z(B, C * K)
                    N.check(lib.vp_margin_ce_bwd(ctx, lg.data_ptr(), y.data_ptr(), B, C, K, kind, m, sc, ls, easy, 1.0, dl.data_ptr(),
                                                 loss.data_ptr(), row.data_ptr(), st), ctx)
                    save(f'{tag}_vp_margin_ce_bwd', loss=loss, row_loss=row, dlogits=dl)
                if easy or ls:                       # SphereFace2 has neither setting
                    continue
                lg, y, _ = ho.plant_logits(B, C, 1, cs, 13 * B, (-0.98, 0.98))
                lg, y, bias = lg.cuda(), y.cuda(), torch.full((1,), 0.3, device='cuda')
                for type_a in (1, 0):
                    loss, row, dl, db, rdb = z(1), z(B), z(B, C), z(1), z(B)
                    N.check(lib.vp_sphereface2(ctx, lg.data_ptr(), y.data_ptr(), bias.data_ptr(), B, C, m, sc, 0.7, 3, type_a, 1.0, loss.data_ptr(),
                                               row.data_ptr(), dl.data_ptr(), db.data_ptr(), rdb.data_ptr(), st), ctx)
                    save(f'B{B}_C{C}_type{"A" if type_a else "C"}_{cfg}_vp_sphereface2', loss=loss, row_loss=row, dlogits=dl, dbias=db, row_dbias=rdb)
        finally:
            lib.vp_set_margin_table(ctx, None)
        print(f'{cfg}: {count} arrays so far, {blank} of them all-zero or not finite', flush=True)


# --pooling: the frame counts of tests/pooling_oracle.py's sweep (both sides of every dispatch edge of csrc/pooling_stats.hip)
POOL_T = (1, 2, 7, 8, 9, 47, 159, 160, 161, 319, 320, 321, 333)
POOL_SENTINEL = -768.0        # every output starts as this: an element nobody wrote, or a refused call that wrote, shows in the dump


def dump_pooling(out):
    """Every output array of the sixteen pooling-statistics entry points on seeded inputs (channel 0 constant over time: the clamp holds
    there).  Low-precision outputs are saved as their bit patterns."""
    import torch
    from ppvector import _native as N
    os.makedirs(out, exist_ok=True)
    lib, ctx, st = N.lib(), N.ctx(0), N.stream_ptr()
    bf = torch.bfloat16
    count = blank = 0

    def rand(seed, *shape, dtype=torch.float32, flat0=False):
        t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
        if flat0:
            t[..., 0] = 1.25
        return t.to(dtype).cuda()

    def buf(*shape, dtype=torch.float32):
        return torch.full(shape, POOL_SENTINEL, dtype=dtype, device='cuda')

    def save(tag, **arrays):
        nonlocal count, blank
        torch.cuda.synchronize()
        for k, v in arrays.items():
            np.save(os.path.join(out, f'pooling_{tag}.{k}.npy'), (v.view(torch.int16) if v.dtype == bf else v).cpu().numpy())
            count += 1
            blank += not bool(torch.isfinite(v.float()).all()) or bool((v == POOL_SENTINEL).all())

    def ok(rc, refused=False):
        if refused:
            assert rc == N.VP_EUNSUP, rc
        else:
            N.check(rc, ctx)

    B = 3
    for l16, x16 in itertools.product((False, True), (False, True)):
        for C, T, sliced in itertools.product((64, 96 if x16 else 100), POOL_T, (False, True)):
            # sliced: x is columns [xoff, xoff + C) of a (B*T, ldx) buffer; d x goes to rows lddx apart
            ldx, xoff, lddx = (C + 32, 16, C + 8) if sliced else (C, 0, C)
            tag = f'l{16 if l16 else 32}_x{16 if x16 else 32}_C{C}_T{T}' + ('_slice' if sliced else '')
            e = rand(1000 * T + C, B * T, C, dtype=bf if l16 else torch.float32)
            x = rand(2000 * T + C, B * T, ldx, dtype=bf if x16 else torch.float32)
            x[:, xoff] = 1.25
            xdt, refused = N.VP_BF16 if x16 else N.VP_F32, l16 and T > 320
            pooled = buf(B, 2 * C)
            if l16:
                ok(lib.vp_asp_softmax_stats_l16(ctx, e.data_ptr(), x.data_ptr(), xdt, ldx, xoff, B, T, C, 1e-12, pooled.data_ptr(), st), refused)
            else:
                ok(lib.vp_asp_softmax_stats(ctx, xdt, e.data_ptr(), x.data_ptr(), ldx, xoff, B, T, C, 1e-12, pooled.data_ptr(), st))
            save(f'{tag}_fwd', pooled=pooled)
            if x16 and not l16:
                continue                            # (no backward reads bf16 x beside f32 logits)
            dp, xp = rand(3000 * T + C, B, 2 * C), x.data_ptr() + xoff * x.element_size()
            for name in ('vp_attn_stats_bwd_e16',) if l16 else ('vp_attn_stats_bwd_f32', 'vp_attn_stats_bwd_de16'):
                de, dx = buf(B * T, C, dtype=torch.float32 if name.endswith('f32') else bf), buf(B * T, lddx)
                if l16:
                    ok(lib.vp_attn_stats_bwd_e16(ctx, e.data_ptr(), xp, xdt, ldx, pooled.data_ptr(), dp.data_ptr(), B, T, C, 1e-12, de.data_ptr(),
                                                 dx.data_ptr(), lddx, st), refused)
                else:
                    ok(getattr(lib, name)(ctx, e.data_ptr(), xp, ldx, pooled.data_ptr(), dp.data_ptr(), B, T, C, 1e-12, de.data_ptr(), dx.data_ptr(),
                                          lddx, st))
                save(f'{tag}_{name}', de=de, dx=dx)
        print(f'attentive, logits {"bf16" if l16 else "f32"}, x {"bf16" if x16 else "f32"}: {count} arrays so far', flush=True)

    for C, T, unbiased in itertools.product((64, 98), (1, 7, 33, 100), (0, 1)):
        tag, eps = f'C{C}_T{T}_u{unbiased}', 1e-8 if unbiased else 1e-12
        x, ds = rand(7000 * T + C, B * T, C, flat0=True), rand(8000 * T + C, B, 2 * C)
        stats, ab = buf(B, 2 * C), buf(2, B, C)
        ok(lib.vp_time_stats_f32(ctx, x.data_ptr(), C, B, T, C, eps, unbiased, stats.data_ptr(), st))
        ok(lib.vp_time_stats_bwd_coeffs(ctx, stats.data_ptr(), ds.data_ptr(), B, T, C, eps, ab.data_ptr(), st))
        save(f'time_{tag}', stats=stats, ab=ab)
        if C % 4:
            continue                                # (the backward passes are four channels wide)
        add, x16 = rand(9000 * T + C, B * T, C), x.to(bf)
        dx, dxa, dxb = buf(B * T, C), buf(B * T, C), buf(B * T, C)
        ok(lib.vp_time_stats_bwd_f32(ctx, x.data_ptr(), C, stats.data_ptr(), ds.data_ptr(), B, T, C, eps, unbiased, dx.data_ptr(), C, st))
        ok(lib.vp_time_stats_bwd_add_f32(ctx, x.data_ptr(), C, stats.data_ptr(), ds.data_ptr(), B, T, C, eps, unbiased, add.data_ptr(), C,
                                         dxa.data_ptr(), C, st))
        ok(lib.vp_time_stats_bwd_add_x16(ctx, x16.data_ptr(), C, stats.data_ptr(), ds.data_ptr(), B, T, C, eps, unbiased, add.data_ptr(), C,
                                         dxb.data_ptr(), C, st))
        save(f'time_{tag}_bwd', dx=dx, dx_add=dxa, dx_add_x16=dxb)
    Bw, Tw, Cw = 2, 4000, 64                        # 63 chunks
    x = rand(11, Bw * Tw, Cw, flat0=True)
    ws = torch.zeros(lib.vp_time_stats_workspace_bytes(Bw, Tw, Cw), dtype=torch.uint8, device='cuda')
    for unbiased in (0, 1):
        stats = buf(Bw, 2 * Cw)
        ok(lib.vp_time_stats_ws_f32(ctx, x.data_ptr(), Cw, Bw, Tw, Cw, 1e-8 if unbiased else 1e-12, unbiased, stats.data_ptr(), ws.data_ptr(),
                                    ws.numel(), st))
        save(f'time_ws_u{unbiased}', stats=stats)
    for C in (64, 100):
        a, s32, s16 = rand(13 + C, B * 47, C), buf(B, C), buf(B, C)
        a16 = a.to(bf)
        ok(lib.vp_utt_sums_f32(ctx, a.data_ptr(), C, B, 47, C, s32.data_ptr(), st))
        ok(lib.vp_utt_sums_b16(ctx, a16.data_ptr(), C, B, 47, C, s16.data_ptr(), st))
        save(f'utt_sums_C{C}', f32=s32, b16=s16)
    print(f'{count} arrays, {blank} of them untouched or not finite (the refused bf16-logit calls at T > 320 leave theirs untouched)', flush=True)


# --bn: the BatchNorm training unit (csrc/bn_train.hip, docs/bn_train.md)
BN_C, BN_M, BN_UTT = (60, 132, 260), (1, 17, 257, 4097), ((9, 7), (65, 64))


def dump_bn(out):
    """(a) every entry point of the unit through ctypes, on the operands, pitches (contiguous; ld = C + 8 at column 4) and sentinel-framed
    outputs of tests/test_gpu_bn_train.py, whose runners make the calls (VPMI_LIB picks the library); (b) one forward and backward of
    BNRows / ConvBlock / Conv2dBlock / CamDenseBlockFn and one training step of every backbone: loss, parameter gradients, running
    statistics (the Python side differs between two checkouts: run it from each).  bf16 outputs are saved as their bit patterns."""
    import warnings
    import torch
    import ppvector
    from ppvector import _native as N
    from ppvector.models import _BUILT
    from ppvector.models.campplus import CAMDenseTDNNBlock
    from ppvector.train.campplus_train import dense_block
    from ppvector.train.functions import BNRows, Conv2dBlock, ConvBlock, HeadLoss
    from tests import bn_oracle as bo
    from tests import test_gpu_bn_train as tb
    warnings.simplefilter('ignore', RuntimeWarning)
    os.makedirs(out, exist_ok=True)
    lib, ctx = N.lib(), N.ctx(0)
    count = blank = 0

    def save(tag, bf16=(), **arrays):
        nonlocal count, blank
        torch.cuda.synchronize()
        for k, v in arrays.items():
            v = torch.as_tensor(v).detach().cpu()
            blank += not bool(torch.isfinite(v.double()).all()) or bool((v == tb.SENTINEL).all())
            # (the runners hand every output back as float64, exactly: a bf16 output goes back to its 16 bits)
            v = v.to(torch.bfloat16).view(torch.int16) if k in bf16 else (v.float() if v.dtype == torch.float64 else v)
            np.save(os.path.join(out, f'bn_{tag}.{k}.npy'), v.numpy())
            count += 1

    # ---- (a) entry points
    for C, M, wide in itertools.product(BN_C, BN_M, (False, True)):
        c, tag = tb.case(M, C), f'C{C}_M{M}' + ('_pitched' if wide else '')
        save(f'{tag}_col_sums', f32=tb.run_col_sums(N, c, 'f32', wide), f32_one=tb.run_col_sums(N, c, 'f32', wide, two=False),
             masked_hi0=tb.run_col_sums(N, c, 'masked', wide, mask_hi=0.0), masked_hi20=tb.run_col_sums(N, c, 'masked', wide, mask_hi=20.0),
             b16=tb.run_col_sums(N, c, 'b16', wide))
        for entry, relu_mask, use_gamma in itertools.product(('f32', 'bf16out', 'b16'), (0, 1), (False, True)):
            dz, db = tb.run_dbias(N, c, entry, wide, relu_mask, use_gamma)[:2]
            save(f'{tag}_dbias_{entry}_relu{relu_mask}_gamma{int(use_gamma)}', bf16=('dz',) if entry != 'f32' else (), dz=dz, dbias=db)
        for relu_mask, use_gamma in itertools.product((0, 1), (False, True)):
            save(f'{tag}_bwd_relu{relu_mask}_gamma{int(use_gamma)}', dz=tb.run_bwd(N, c, wide, False, relu_mask=relu_mask, use_gamma=use_gamma)[0])
        for mask_hi, acc in itertools.product((0.0, 20.0), (0, 1)):
            save(f'{tag}_bwd_masked_hi{int(mask_hi)}_acc{acc}', dz=tb.run_bwd(N, c, wide, True, mask_hi=mask_hi, accumulate=acc)[0])
        for entry, relu in itertools.product(('f32', 'b16_f32', 'b16_b16', 'f32_b16'), (0, 1, 2)):
            save(f'{tag}_affine_{entry}_relu{relu}', bf16=('y',) if entry.endswith('b16') else (), y=tb.run_affine(N, c, entry, wide, relu)[0])
        sc, sh = tb.vec(c.ms), tb.vec(c.mh)
        for with_add in (False, True):
            zd, y, add, aux = tb.In(c.z, wide), tb.Out(M, C, True), tb.In(c.old, wide), tb.Out(M, C, wide)
            N.check(lib.vp_affine_rows_aux_f32(ctx, zd.ptr, zd.ld, sc.data_ptr(), sh.data_ptr(), M, C, y.ptr, y.ld, add.ptr if with_add else None,
                                               add.ld if with_add else 0, aux.ptr if with_add else None, aux.ld if with_add else 0,
                                               N.stream_ptr()), ctx)
            save(f'{tag}_affine_aux_add{int(with_add)}', y=y.get(), **({'aux': aux.get()} if with_add else {}))
    for C, (B, T), wide in itertools.product(BN_C, BN_UTT, (False, True)):
        c, tag = tb.case(B * T, C, T), f'C{C}_B{B}_T{T}' + ('_pitched' if wide else '')
        save(f'{tag}_col_sums', utt=tb.run_col_sums(N, c, 'utt', wide), ctx=tb.run_col_sums(N, c, 'ctx', wide))
        for entry, relu_mask, use_gamma in itertools.product(('utt', 'ctx'), (0, 1), (False, True)):
            dz, db = tb.run_dbias(N, c, entry, wide, relu_mask, use_gamma)[:2]
            save(f'{tag}_dbias_{entry}_relu{relu_mask}_gamma{int(use_gamma)}', bf16=('dz',), dz=dz, dbias=db)
    for M in BN_M:                                     # C % 4 != 0: the one-channel col_sums_kernel
        save(f'C6_M{M}_col_sums', f32=tb.run_col_sums(N, tb.case(M, 6), 'f32', False))
    for C, nparts, i in itertools.product((6, 64, 260), (1, 17, 65, 1200), (0, 1)):
        g = np.random.default_rng(31 * nparts + C)
        ps = (g.standard_normal((nparts, C)) * 30 + 40).astype(np.float32)
        pq = (g.uniform(0.5, 1.5, (nparts, C)) * (1000 / nparts) * 40 + (ps.astype(np.float64).sum(0) / 1000) ** 2 * 1000 / nparts).astype(np.float32)
        gamma, beta, rm, rv = bo.affine_params(C, nparts)
        if i:                                          # gamma / beta and the running pointers NULL
            gamma = beta = rm = rv = None
        names = ('mean', 'invstd', 'scale', 'shift', 'run_mean', 'run_var')
        res = tb.run_finalize(N, ps, pq, 1000, C, gamma, beta, rm, rv, bo.MOM, bo.EPS)
        save(f'C{C}_parts{nparts}_finalize_{"null" if i else "set"}', **{k: v for k, v in zip(names, res) if v is not None})
    print(f'entry points: {count} arrays, {blank} of them untouched or not finite', flush=True)

    # ---- (b) the Functions and the backbones' training steps
    def fwd_bwd(tag, fn, inputs, seed):
        """inputs: name -> f32 array that takes a gradient; fn(tensors) -> output"""
        ts = {k: tb.vec(v).requires_grad_() for k, v in inputs.items()}
        y = fn(ts)
        dy = torch.from_numpy(np.random.default_rng(seed).standard_normal(tuple(y.shape)).astype(np.float32)).cuda()
        y.backward(dy)
        save(tag, y=y, **{f'd_{k}': t.grad for k, t in ts.items() if t.grad is not None})

    for (M, C), relu in itertools.product(((17, 8), (48, 3072)), (False, True)):
        gamma, beta, rm0, rv0 = bo.affine_params(C, M)
        rm, rv = tb.vec(rm0), tb.vec(rv0)
        fwd_bwd(f'BNRows_M{M}_C{C}_relu{int(relu)}', lambda t: BNRows.apply(t['x'], t['gamma'], t['beta'], rm, rv, 0.9, 1e-5, relu),
                dict(x=bo.conditioned(M, C, 10), gamma=gamma, beta=beta), M + C)
        save(f'BNRows_M{M}_C{C}_relu{int(relu)}', run_mean=rm, run_var=rv)
    for T_out in (18, 19, 200):                        # 18: the separate column-sum pass; 19, 200: the conv's fused sums
        B, Cin, Cout, kw = 4, 64, 64, 3
        g = np.random.default_rng(T_out)
        x = g.standard_normal((B * (T_out + kw - 1), Cin)).astype(np.float32)
        w, bias = (g.standard_normal((Cout, Cin, kw)) / np.sqrt(Cin * kw)).astype(np.float32), g.standard_normal(Cout).astype(np.float32)
        gamma, beta, rm0, rv0 = bo.affine_params(Cout, T_out)
        rm, rv = tb.vec(rm0), tb.vec(rv0)
        fwd_bwd(f'ConvBlock_T{T_out}', lambda t: ConvBlock.apply(t['x'], t['w'], t['bias'], None, t['gamma'], t['beta'], rm, rv,
                                                                 dict(B=B, T=T_out + kw - 1, relu=True)),
                dict(x=x, w=w, bias=bias, gamma=gamma, beta=beta), T_out)
        save(f'ConvBlock_T{T_out}', run_mean=rm, run_var=rv)
    for act in ('relu', 'hardtanh'):
        B, T, Fq, Cin, Cout = 2, 9, 10, 8, 32
        g = np.random.default_rng(len(act))
        x, w = g.standard_normal((B * T * Fq, Cin)).astype(np.float32), (g.standard_normal((Cout, Cin, 3, 3)) * 2 / np.sqrt(Cin * 9)).astype(np.float32)
        gamma, beta, rm0, rv0 = bo.affine_params(Cout, 3)
        rm, rv = tb.vec(rm0), tb.vec(rv0)
        fwd_bwd(f'Conv2dBlock_{act}', lambda t: Conv2dBlock.apply(t['x'], t['w'], t['bias'], t['gamma'], t['beta'], rm, rv, dict(B=B, T=T, F=Fq, act=act)),
                dict(x=x, w=w, bias=g.standard_normal(Cout).astype(np.float32), gamma=gamma * 8, beta=beta + 6), 7)
        save(f'Conv2dBlock_{act}', run_mean=rm, run_var=rv)
    torch.manual_seed(77)
    B, T = 3, 150
    blk = CAMDenseTDNNBlock(num_layers=2, in_channels=128, out_channels=32, bn_channels=128, kernel_size=3).cuda().train()
    x = torch.randn(B * T, 128, generator=torch.Generator().manual_seed(78)).cuda().requires_grad_()
    y = dense_block([blk.tdnnd1, blk.tdnnd2], x, B, T)
    y.backward(torch.randn(y.shape, generator=torch.Generator().manual_seed(79)).cuda())
    save('CamDenseBlockFn', y=y, d_x=x.grad, **{'d_' + k: p.grad for k, p in blk.named_parameters()}, **dict(blk.named_buffers()))

    def train_step(name, Bs, Ts, amp):
        ppvector.set_train_amp(amp)
        try:
            torch.manual_seed(1234)
            m = _BUILT[name](input_size=80).cuda().train()
            g = torch.Generator().manual_seed(100 * Bs + Ts)
            x, labels = torch.randn(Bs, Ts, 80, generator=g).cuda(), torch.randint(0, 67, (Bs,), generator=g).cuda()
            emb = m(x)
            W = (torch.randn(emb.shape[1], 67, generator=g) * 0.1).cuda().requires_grad_()
            loss = HeadLoss.apply(emb, W, labels, 0.2, 32.0, 0.0, False)[0]
            loss.backward()
            save(f'step_{name}_{"amp" if amp else "f32"}_B{Bs}_T{Ts}', loss=loss, emb=emb, d_head=W.grad,
                 **{'d_' + k: p.grad for k, p in m.named_parameters() if p.grad is not None}, **dict(m.named_buffers()))
        finally:
            ppvector.set_train_amp(False)

    for name, _ in MODELS:
        train_step(name, 4, 100, False)
    train_step('EcapaTdnn', 16, 298, True)             # the wide bf16 layers (the b16 / utt / ctx forms) need M >= 4096
    print(f'{count} arrays, {blank} of them untouched or not finite', flush=True)


def _ulps(x, y):
    """Largest distance of two f32 arrays in units in the last place (inf where a NaN or the shapes differ)."""
    if x.shape != y.shape or x.dtype != np.float32 or np.isnan(x).any() or np.isnan(y).any():
        return float('inf')
    i, j = (np.where(v < 0, np.int64(-2 ** 31) - v, v) for v in (x.view(np.int32).astype(np.int64), y.view(np.int32).astype(np.int64)))
    return int(np.abs(i - j).max()) if i.size else 0


def compare(a, b):
    names = sorted(f for f in os.listdir(a) if f.endswith('.npy'))
    assert names == sorted(f for f in os.listdir(b) if f.endswith('.npy')), 'the two directories hold different arrays'
    bad = ulp1 = 0
    for f in names:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        eq = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        word = 'equal' if eq else 'DIFFERENT'
        if not eq and f.endswith(tuple(u + '.npy' for u in ULP1)) and _ulps(x, y) <= 1:
            word = '1 ulp (allowed: the mean of the row losses)'
            ulp1 += 1
        bad += word == 'DIFFERENT'
        print(f'{f}: {word}')
    print(f'{len(names) - bad - ulp1} of {len(names)} equal' + (f', {ulp1} within the allowed 1 ulp' if ulp1 else '') + (f', {bad} DIFFERENT' if bad else ''))
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
    ap.add_argument('--heads', action='store_true')
    ap.add_argument('--pooling', action='store_true')
    ap.add_argument('--bn', action='store_true')
    a = ap.parse_args()
    if a.compare:
        sys.exit(1 if compare(*a.compare) else 0)
    if a.time_b1:
        time_b1()
    if a.out and a.heads:
        dump_heads(a.out)
    elif a.out and a.pooling:
        dump_pooling(a.out)
    elif a.out and a.bn:
        dump_bn(a.out)
    elif a.out:
        dump(a.out, a.only, a.suffix)
