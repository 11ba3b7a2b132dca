"""The float64 oracle of the training step's small kernels (tests/train_ops_oracle.py) checked on the CPU, so that it cannot be wrong
unnoticed: every closed-form backward against float64 torch.autograd of the forward formula, the reflect fold against the autograd of
F.pad(mode='reflect'), zero insertion against the autograd of a strided slice, the weight layouts against plain permutes -- and the
exact family's precondition for every planted case: float32 in two summation orders is bit-identical to float64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_ops_oracle as O

F64 = torch.float64


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=F64, requires_grad=grad)


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.max(np.abs(a - b)) <= tol * max(1.0, float(np.max(np.abs(b)))), float(np.max(np.abs(a - b)))


# ------------------------------------------------------------------------------------------------ the exactness precondition
_CASES = O.exact_cases()


@pytest.mark.parametrize('name,fn,rounded', _CASES, ids=[c[0] for c in _CASES])
def test_exact_family_is_order_independent_in_float32(name, fn, rounded):
    """float32 first-to-last == float32 last-to-first == float64, bit for bit, for every output of every planted exact case: the
    products and every partial sum are representable, so a kernel that differs from float64 on these inputs dropped or doubled a term.
    (`rounded`: the formula ends in ONE rounding of an exact value; float32 must then be float64 rounded to nearest even.)"""
    fwd, bwd, ref = fn(np.float32, False), fn(np.float32, True), fn(np.float64, False)
    for a, b, r in zip(fwd, bwd, ref):
        assert a.dtype == np.float32 and r.dtype == np.float64
        assert np.array_equal(a, b), name
        assert np.array_equal(a, r.astype(np.float32)) if rounded else np.array_equal(a.astype(np.float64), r), name
        assert np.all(np.isfinite(r))


def test_exact_cases_cover_every_shape_list():
    names = [c[0] for c in _CASES]
    assert len(set(names)) == len(names)
    for prefix, count in (('fold-', len(O.FOLD_TP) * len(O.FOLD_C)), ('utt_dot_z16-', len(O.UTT_T) * len(O.UTT_C)),
                          ('scale_rows_bwd-', len(O.SRB_SIMPLE_C) * len(O.SRB_SIMPLE_T) + 4 * len(O.SRB_CHUNK_C)),
                          ('se_bwd-', len(O.SE_SHAPES) * len(O.SE_B) * 2), ('se_fwd-', len(O.SE_SHAPES) * len(O.SE_B) * 2),
                          ('adam-moments-', 2 * len(O.OPT_SIZES)), ('momentum-', 4 * len(O.OPT_SIZES)), ('act_bwd-', 2),
                          ('seg_ctx_bwd_sum-', sum(len(O.seg_T(s)) for s in O.SEG_LENS) * (len(O.SEG_C) + 1))):
        assert sum(n.startswith(prefix) for n in names) == count, prefix


def test_chunked_scale_rows_shapes_reach_their_branches():
    """srb_chunk_T against the geometry: one row; the four-row trip exactly; one row of tail; a last chunk shorter than the row groups."""
    for C in O.SRB_CHUNK_C:
        RG, _, _ = O.srb_geometry(O.SRB_B, 1, C)
        assert RG == {4: 256, 12: 64, 40: 16, 1024: 1}[C]
        T = O.srb_chunk_T(O.SRB_B, C)
        assert T[:3] == [1, 8 * RG, 8 * RG + 1]
        _, rpc, chunks = O.srb_geometry(O.SRB_B, T[3], C)
        last = T[3] - (chunks - 1) * rpc
        assert (chunks == 3 and 0 < last == RG - 1) or (RG == 1 and chunks == 2 and last == rpc)    # one row group: two full chunks


# ------------------------------------------------------------------------------------------------ layouts and data movement
@pytest.mark.parametrize('Cout,Cin,KW', O.LAYOUT_SHAPES)
def test_weight_layouts_1d_are_permutes(Cout, Cin, KW):
    w = O.gauss(O.rng(Cout, Cin, KW), (Cout, Cin, KW))
    wp, w2 = O.weight_layouts(w)
    assert np.array_equal(wp, w.transpose(0, 2, 1).reshape(Cout, KW * Cin))
    assert np.array_equal(w2, w[:, :, ::-1].transpose(1, 2, 0).reshape(Cin, KW * Cout))


@pytest.mark.parametrize('KF,KT', O.LAYOUT_2D)
def test_weight_layouts_2d_are_permutes(KF, KT):
    """wp is (Cout, KT, KF, Cin), w2 (Cin, KT, KF, Cout) with both tap axes reversed (include/vpmi.h)."""
    Cout, Cin = 5, 3
    w = O.gauss(O.rng(KF, KT), (Cout, Cin, KF, KT))
    wp, w2 = O.weight_layouts(w)
    assert np.array_equal(wp, w.transpose(0, 3, 2, 1).reshape(Cout, -1))
    assert np.array_equal(w2, w[:, :, ::-1, ::-1].transpose(1, 3, 2, 0).reshape(Cin, -1))


def test_prep_entries_reach_every_branch():
    E = O.PREP_ENTRIES
    assert len(E) == 25
    assert all(0 < nc and c0 + nc <= ld for _, ld, c0, nc, _, _ in E)
    assert any(ld > nc for _, ld, _, nc, _, _ in E) and any(a and not b for *_, a, b in E) and any(b and not a for *_, a, b in E)
    assert {(65, 1), (1, 65), (130, 70)} <= {(r, nc) for r, _, _, nc, _, _ in E}


def test_pack_segments_oracle():
    dst = np.full(12, -7.0, np.float32)
    out = O.pack_segments(dst, [np.arange(3, dtype=np.float32), None, np.ones(5, np.float32)], [1, 5, 9], [3, 2, 0])
    assert out.tolist() == [-7, 0, 1, 2, -7, 0, 0, -7, -7, -7, -7, -7]


@pytest.mark.parametrize('T,pad', O.FOLD_TP)
def test_reflect_fold_is_the_adjoint_of_reflect_pad(T, pad):
    B, C = 2, 4
    dxp = O.gauss(O.rng(T, pad), (B, T + 2 * pad, C))
    add = O.gauss(O.rng(T, pad, 1), (B, T, C))
    x = torch.zeros(B, C, T, dtype=F64, requires_grad=True)
    xp = F.pad(x, (pad, pad), mode='reflect') if pad else x
    xp.backward(t64(dxp).transpose(1, 2))
    dx, sm = O.reflect_fold(dxp, T, pad, add)
    close(dx, x.grad.transpose(1, 2).numpy())
    close(sm, dx + add)
    close(O.reflect_fold(dxp, T, pad, rev=True), dx)


@pytest.mark.parametrize('st,sf', O.ZI_STRIDES)
@pytest.mark.parametrize('n_in,n_out', O.ZI_IN_OUT)
def test_zero_insert_is_the_adjoint_of_a_strided_slice(st, sf, n_in, n_out):
    B, C = 2, 4
    for T_in, T_out, F_in, F_out in ((n_in, n_out, 5, 3), (5, 3, n_in, n_out)):
        dz = O.gauss(O.rng(st, sf, n_in, n_out), (B, T_out, F_out, C))
        x = torch.zeros(B, T_in, F_in, C, dtype=F64, requires_grad=True)
        y = x[:, ::st, ::sf][:, :T_out, :F_out]
        g = t64(dz)[:, :y.shape[1], :y.shape[2]]
        y.backward(g)
        assert np.array_equal(O.zero_insert(dz, T_in, F_in, st, sf), x.grad.numpy().astype(np.float32))
    up = O.zero_insert(np.ones((1, 3, 1, 4), np.float32), 7, 1, 2, 1)
    assert up[0, :, 0, 0].tolist() == [1, 0, 1, 0, 1, 0, 0]                     # (7, 3): frame 6 = 2 * 3 is out of range -> zero


# ------------------------------------------------------------------------------------------------ closed-form backwards vs autograd
def test_scale_rows_and_utt_dot_vs_autograd():
    B, T, C = 2, 9, 5
    dy, x = O.btc(B, T, C, 'gauss', 1, 2)
    s = O.gates(B, C, 'gauss', 1)
    xt, st = t64(x, True), t64(s, True)
    (xt * st[:, None, :]).backward(t64(dy))
    dx, ds = O.scale_rows_bwd(dy, x, s)
    close(dx, xt.grad.numpy())
    close(ds, st.grad.numpy())
    close(O.utt_dot(dy, x), st.grad.numpy())
    close(O.scale_rows_bwd(dy, x, s, rev=True)[1], ds)


def test_scale_shift_rows_vs_autograd():
    """dx of out = x * s[b] + (a function of mean_t x): dy * s + dm / T (dm = the gradient that reached the mean); 1/T enters as float32."""
    B, T, C = 2, 7, 4
    dy, x = O.btc(B, T, C, 'gauss', 2, 2)
    s, dm = O.gates(B, C, 'gauss', 2), O.gates(B, C, 'gauss', 3)
    xt = t64(x, True)
    ((xt * t64(s)[:, None, :] * t64(dy)).sum() + (xt.mean(1) * t64(dm)).sum()).backward()
    close(O.scale_shift_rows(dy, s, dm, T), xt.grad.numpy(), 2.0 ** -23)


def test_utt_dot_z16_rounds_where_the_kernel_does():
    """x = bf16(float32(z * scale + shift)): on the planted family the fma is exact and the bf16 rounding plain round-to-nearest-even."""
    z = np.asarray([[[3.0, 255.0, -129.0, 256.0]]], np.float32)
    sc, sh = np.asarray([0.75, 1.0, 2.0, 0.25], np.float32), np.asarray([1.0, 2.0, -1.0, 0.0], np.float32)
    dy = np.ones((1, 1, 4), np.float32)
    assert O.utt_dot(dy, z, sc, sh)[0].tolist() == [3.25, 256.0, -260.0, 64.0]    # ties to even: 257 -> 256, -259 -> -260


@pytest.mark.parametrize('kind', list(O.ACTS))
def test_activation_backwards_vs_autograd(kind):
    x = O.act_inputs(4096, 3).astype(np.float64)
    x = x[(np.abs(x) > 1e-30) & (np.abs(x - 20.0) > 1e-3)]                        # the kinks are pinned below, not differentiated
    dy = O.gauss(O.rng(5), x.shape).astype(np.float64)
    xt = t64(x, True)
    y = {'tanh': torch.tanh, 'sigmoid': lambda v: 1 / (1 + torch.exp(-v)), 'relu': torch.relu,
         'hardtanh20': lambda v: torch.clamp(v, 0.0, 20.0), 'silu': lambda v: v / (1 + torch.exp(-v))}[kind](xt)
    y.backward(t64(dy))
    close(O.act(kind, x), y.detach().numpy())
    got = O.act_bwd(kind, dy, x if kind == 'silu' else O.act(kind, x))
    close(got, xt.grad.numpy(), 1e-9)


def test_activation_conventions_and_overflow():
    """ReLU'(0) = 0; hardtanh20' = 0 at an output of exactly 0 or 20 and 1 one ulp inside; nothing overflows at |x| = 100."""
    one = np.ones(1)
    assert O.act_bwd('relu', one, np.zeros(1))[0] == 0 and O.act_bwd('relu', one, np.asarray([2.0 ** -126]))[0] == 1
    for y, d in ((0.0, 0), (2.0 ** -126, 1), (20.0 - 2.0 ** -19, 1), (20.0, 0)):
        assert O.act_bwd('hardtanh20', one, np.asarray([y]))[0] == d
    assert O.act('hardtanh20', np.asarray([20.0 + 2.0 ** -19]))[0] == 20.0
    for kind in O.ACTS:
        y = O.act(kind, O.PLANTED_X)
        assert np.all(np.isfinite(y)) and np.all(np.isfinite(O.act_f32(kind, O.PLANTED_X)))
        assert np.all(np.isfinite(O.act_bwd(kind, np.ones_like(y), O.PLANTED_X.astype(np.float64) if kind == 'silu' else y)))
    assert np.all(np.isfinite(O.silu_bwd_f32(np.ones(12, np.float32), O.PLANTED_X)))


def test_activation_bounds_come_from_float32_itself():
    """The bound of the transcendental activations: 4 x the worst relative error of the float32 CPU restatement (docs/train_ops.md
    quotes the figures).  It must be a float32-sized number, neither zero nor loose."""
    x = O.act_inputs(4093, 1)                                    # the block the GPU test repeats
    for kind in ('tanh', 'sigmoid', 'silu'):
        m, b = O.act_bound(kind, x)
        print(f'[act bound] {kind}: measured {m:.3e} bound {b:.3e}')
        assert 2.0 ** -26 < m < 2.0 ** -21 and b == 4 * m


def test_aff_combine_bwd_vs_autograd():
    rows, C = 37, 68
    g, t, x, y = (O.gauss(O.rng(rows, i), (rows, C)) for i in range(4))
    tt, xt, yt = t64(t, True), t64(x, True), t64(y, True)
    o = xt * (1 + tt) + yt * (1 - tt)
    o.backward(t64(g))
    close(O.aff_combine(t, x, y), o.detach().numpy())
    for a, b in zip(O.aff_combine_bwd(g, t, x, y), (xt.grad, yt.grad, tt.grad)):
        close(a, b.numpy())


@pytest.mark.parametrize('seg', O.SEG_LENS)
def test_segment_ops_vs_autograd(seg):
    B, C = 2, 5
    for T in O.seg_T(seg):
        nseg = -(-T // seg)
        x, g, y = O.btc(B, T, C, 'gauss', seg, 3)
        dctx, m = O.gates(B, C, 'gauss', T, nseg), O.gates(B, C, 'gauss', T + 1, nseg)
        xt = t64(x, True)
        segs = [xt[:, a:a + seg].mean(1) for a in range(0, T, seg)]               # the last one over its valid frames only
        ctx = torch.stack(segs, 1) + xt.mean(1, keepdim=True)
        close(O.seg_ctx(x, seg), ctx.detach().numpy())
        ctx.backward(t64(dctx))
        close(O.seg_ctx_bwd(dctx, T, seg), xt.grad.numpy())
        yt, mt = t64(y, True), t64(m, True)
        out = yt * mt.repeat_interleave(seg, 1)[:, :T]
        close(O.seg_scale(y, m, seg), out.detach().numpy())
        out.backward(t64(g))
        dy, dm = O.seg_scale_bwd(g, y, m, seg)
        close(dy, yt.grad.numpy())
        close(dm, mt.grad.numpy())


@pytest.mark.parametrize('C,H', [(4, 4), (64, 12), (80, 1000)])
def test_se_dense_bwd_vs_autograd(C, H):
    B = 5
    mean, w1, b1, w2, b2 = O.se_fwd_inputs(B, C, H, 'gauss')
    ds = O.gauss(O.rng(C, H, 3), (B, C))
    mt, w1t, b1t, w2t, b2t = (t64(v, True) for v in (mean, w1, b1, w2, b2))
    a = torch.relu(mt @ w1t.t() + b1t)
    s = torch.sigmoid(a @ w2t.t() + b2t)
    s.backward(t64(ds))
    ao, _, so = O.se_dense_fwd(mean, w1, b1, w2, b2)
    close(ao, a.detach().numpy())
    close(so, s.detach().numpy())
    for got, ref in zip(O.se_dense_bwd(ds, mean, ao, so, w1, w2), (mt.grad, w1t.grad, b1t.grad, w2t.grad, b2t.grad)):
        close(got, ref.numpy(), 1e-11)
    for got, ref in zip(O.se_dense_bwd(ds, mean, ao, so, w1, w2, rev=True), (mt.grad, w1t.grad, b1t.grad, w2t.grad, b2t.grad)):
        close(got, ref.numpy(), 1e-11)


# ------------------------------------------------------------------------------------------------ optimisers
@pytest.mark.parametrize('step', O.OPT_STEPS)
def test_adam_oracle_vs_torch(step):
    """The coupled-L2 Adam and AdamW of torch.optim, float64, state planted at `step - 1` -- up to the float32 values the oracle takes
    for beta^t (relative 2^-24 beta^t / (1 - beta^t) in 1 - beta^t) and for AdamW's 1 - lr wd."""
    p, g, m, v = O.opt_inputs(255, 'gauss')
    kw = {k: float(np.float32(x)) for k, x in dict(O.GAUSS_OPT, gscale=1.0, wd=0.01).items()}     # torch sees the float32 values too
    wd = kw.pop('wd')
    for decoupled, cls in ((False, torch.optim.Adam), (True, torch.optim.AdamW)):
        pt = t64(p, True)
        opt = cls([pt], lr=kw['lr'], betas=(kw['b1'], kw['b2']), eps=kw['eps'], weight_decay=wd)
        pt.grad = t64(g)
        opt.state[pt] = dict(step=torch.tensor(float(step - 1)), exp_avg=t64(m), exp_avg_sq=t64(v))
        opt.step()
        upd, mn, vn = O.adam(p, g, m, v, wd=wd, step=step, decoupled=decoupled, **kw)
        close(mn, opt.state[pt]['exp_avg'].numpy(), 1e-7)
        close(vn, opt.state[pt]['exp_avg_sq'].numpy(), 1e-7)
        ref = pt.detach().numpy() - p.astype(np.float64)
        # float32 costs the oracle (as it costs the entry point) half an ulp of beta^t, amplified by the cancellation in 1 - beta^t, and
        # half an ulp of AdamW's keep factor 1 - lr wd on p itself
        rel = O.U * sum(b ** step / (1 - b ** step) for b in (kw['b1'], kw['b2'])) + 1e-9
        assert np.all(np.abs(upd - ref) <= rel * np.abs(ref) + (O.U * np.abs(p) if decoupled else 0.0))
        eu, em, ev = O.adam_bounds(p, g, m, v, wd=wd, step=step, decoupled=decoupled, **kw)
        assert np.all(eu > 0) and np.all(eu < 1e-5 * (np.abs(p) + np.abs(ref)) + 1e-12)


@pytest.mark.parametrize('nesterov', [0, 1])
def test_momentum_oracle_vs_torch(nesterov):
    p, g, vel, _ = O.opt_inputs(255, 'gauss')
    for mu in (0.9, 0.0):
        if nesterov and mu == 0.0:
            continue
        pt = t64(p, True)
        opt = torch.optim.SGD([pt], lr=0.05, momentum=mu, weight_decay=0.01, nesterov=bool(nesterov))
        pt.grad = t64(g)
        if mu:
            opt.state[pt] = dict(momentum_buffer=t64(vel))
        opt.step()
        upd, vn = O.momentum(p, g, vel, 0.05, mu, 0.01, nesterov, 1.0)
        close(upd, pt.detach().numpy() - p.astype(np.float64), 1e-6)
        if mu:
            close(vn, opt.state[pt]['momentum_buffer'].numpy(), 1e-6)


def test_float32_evaluation_stays_within_the_gauss_bounds():
    """The Gaussian family's bounds hold for the oracle's own float32 evaluations (both orders): they are bounds on float32, not on a kernel."""
    B, T, C = 2, 57, 132
    dy, x = O.btc(B, T, C, 'gauss', 6, 2)
    ref, ab = O.utt_dot(dy, x), O.utt_dot(np.abs(dy), np.abs(x))
    for rev in (False, True):
        assert np.all(np.abs(O.utt_dot(dy, x, dt=np.float32, rev=rev) - ref) <= (T + 1) * O.U * ab)
    bi = O.se_bwd_inputs(5, 80, 1000, 'gauss')
    refs, bounds = O.se_dense_bwd(*bi), O.se_bwd_bounds(*bi)
    for rev in (False, True):
        for got, r, b in zip(O.se_dense_bwd(*bi, dt=np.float32, rev=rev), refs, bounds):
            assert np.all(np.abs(got - r) <= b)
    # round_bf16: the float32 evaluation rounds ITS inexact dz2, dz1 and a to bf16, so a rounding may fall the other way
    refs, bounds = O.se_dense_bwd(*bi, rnd=1), O.se_bwd_bounds(*bi, rnd=1)
    fi = O.se_fwd_inputs(5, 80, 1000, 'gauss')
    (ra, rz, _), (ea, ez) = O.se_dense_fwd(*fi, rnd=1), O.se_fwd_bounds(*fi, rnd=1)
    for rev in (False, True):
        for got, r, b in zip(O.se_dense_bwd(*bi, rnd=1, dt=np.float32, rev=rev), refs, bounds):
            assert np.all(np.abs(got - r) <= b)
        a32, z32, _ = O.se_dense_fwd(*fi, rnd=1, dt=np.float32, rev=rev)
        assert np.all(np.abs(a32 - ra) <= ea) and np.all(np.abs(z32 - rz) <= ez)
    p, g, m, v = O.opt_inputs(4093, 'gauss')
    for step in O.OPT_STEPS:
        kw = dict(O.GAUSS_OPT, wd=1e-2, step=step)
        for a, r, b in zip(O.adam(p, g, m, v, dt=np.float32, **kw), O.adam(p, g, m, v, **kw), O.adam_bounds(p, g, m, v, **kw)):
            assert np.all(np.abs(a - r) <= b)
    # the exact family's update: 5 ulps of the step and 1 of p_new hold for the float32 evaluation (its p_new - p is a seventh rounding
    # that the GPU test, which subtracts in float64, does not have: half an ulp of the update more)
    pe = O.opt_inputs(4093, 'exact')
    for step in O.OPT_STEPS:
        for wd in (0.0, 0.25):
            for dec in (False, True):
                kw = dict(O.EXACT_OPT, wd=wd, step=step, decoupled=dec)
                u32, u64 = O.adam(*pe, dt=np.float32, **kw)[0], O.adam(*pe, **kw)[0]
                assert np.all(np.abs(u32 - u64) <= O.adam_bounds(*pe, exact_moments=True, **kw)[0] + O.U * np.abs(u64))
    x = O.act_inputs(4093, 2)
    m, b = O.silu_bwd_bound(x)
    assert 2.0 ** -26 < m < 2.0 ** -20 and np.all(np.abs(O.silu_bwd_f32(np.ones_like(x), x) - O.act_bwd('silu', np.ones_like(x), x)) <= b / 4 * (1 + 1e-12))
    print(f'[act bound] silu derivative: measured {m:.3e} bound {4 * m:.3e} (units of sg (1 + |x|))')
