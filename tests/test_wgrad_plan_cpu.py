"""CPU tests of the conv weight gradient's host decision (no GPU needed: vp_conv1d_wgrad_plan and vp_conv1d_wgrad_workspace_bytes make
no device call; csrc/wgrad.hip: wgrad_validate, wgrad_plan, wgrad_splits_bound): the kernel family and row splits of the layer shapes
the training step runs, the properties every plan must have -- the workspace bound among them -- on a grid of seeded descriptors, the
workspace byte count against a NumPy restatement of its rule, and the error paths."""
import ctypes as C
import os

import numpy as np
import pytest

_PTR = 0x1000                                    # dummy non-null 16-byte-aligned pointers: the plan reads the struct, never through it
CUS = (8, 64, 256, 304)


@pytest.fixture(scope='module')
def N():
    from ppvector import _native as N
    N.load_library()
    assert (N.VP_WGRAD_F32, N.VP_WGRAD_AMP, N.VP_WGRAD_X3, N.VP_WGRAD_N64, N.VP_WGRAD_TR256) == (0, 1, 2, 3, 4)
    return N


@pytest.fixture
def wg(N):
    """The library for the tests whose expected plans are those of the default switch.  VPMI_WGRAD_TR256_OFF is an A/B knob the
    library reads once per process; with it exported no layer is planned on VP_WGRAD_TR256 and these tests cannot say anything about
    the default: they fail, naming the variable.  (The error-path test holds under either setting and does not come through here.)"""
    assert os.environ.get('VPMI_WGRAD_TR256_OFF') is None, 'unset VPMI_WGRAD_TR256_OFF: the plans pinned here are those of the default dispatch'
    return N


def chunk_rows(N, family):
    """rows per staged chunk of a family's kernel"""
    return 32 if family in (N.VP_WGRAD_F32, N.VP_WGRAD_TR256) else 64


def wdesc(N, dt, B, T, Cin, Cout, kw=1, dil=1, mode=0, stride=1, F=0, ldx=None, xoff=0):
    """A valid forward descriptor for the weight gradient, M = B T rows (B T F with F > 0: a 2-D conv, kw = 9 taps as 3 x 3, zero
    padding); 'same' reflect padding for tapped 1-D layers (zero where T is too short to reflect), none for 1x1 layers."""
    d = N.Conv1dDesc()
    d.dtype_in = d.dtype_out = dt
    d.B, d.T_in, d.T_out = B, T * stride, T
    d.Cin, d.Cout, d.KW, d.dilation, d.stride = Cin, Cout, kw, dil, stride
    if F:
        d.KF, d.F_in, d.F_out, d.stride_f, d.pad_f, d.pad_mode, d.pad_left = 3, F, F, 1, 1, N.VP_PAD_ZERO, dil
    elif kw > 1:
        d.pad_left = dil * (kw - 1) // 2
        d.pad_mode = N.VP_PAD_REFLECT if d.pad_left < T else N.VP_PAD_ZERO
    else:
        d.pad_mode = N.VP_PAD_NONE
    d.x, d.w, d.y = _PTR, _PTR + 64, _PTR + 128
    d.ldx, d.xoff, d.ldy = Cin if ldx is None else ldx, xoff, Cout
    d.mfma_bf16 = mode
    return d


def rows_of(d):
    return d.B * d.T_out * (d.F_out if d.KF > 1 else 1)


def plan(N, d, nbatch=1, cus=256, dz=_PTR + 256, lddz=None):
    """(rc, family, tile_n, tile_k, splits, rows_per_split)"""
    out = [C.c_int(-1) for _ in range(5)]
    rc = N.lib().vp_conv1d_wgrad_plan(C.byref(d) if d is not None else None, dz, d.Cout if lddz is None and d is not None else (lddz or 0),
                                      nbatch, cus, *[C.byref(o) for o in out])
    return (rc,) + tuple(o.value for o in out)


def ws_bytes(N, d):
    return int(N.lib().vp_conv1d_wgrad_workspace_bytes(C.byref(d)))


def test_wgrad_plan_table(wg):
    """The plan of the layer shapes the training steps run, on a 256-CU chip: M 76 288 = 256 utterances x 298 frames, 9 536 = 32 x 298;
    the 2-D row is ResNetSE's first stage, 8 x 298 x 80 positions."""
    N = wg
    BF, F32 = N.VP_BF16, N.VP_F32
    F, AMP, X3, N64, TR = N.VP_WGRAD_F32, N.VP_WGRAD_AMP, N.VP_WGRAD_X3, N.VP_WGRAD_N64, N.VP_WGRAD_TR256
    table = [
        ('512->512 1x1, M 76 288', wdesc(N, BF, 256, 298, 512, 512, mode=1), 1, TR, 63, 1216),
        ('1536->1536 1x1, M 76 288', wdesc(N, BF, 256, 298, 1536, 1536, mode=1), 1, TR, 7, 10912),
        ('1536->128 1x1, M 76 288', wdesc(N, BF, 256, 298, 1536, 128, mode=1), 1, TR, 42, 1824),
        ('128->1536 1x1, M 76 288', wdesc(N, BF, 256, 298, 128, 1536, mode=1), 1, TR, 42, 1824),
        ('512->512 1x1, M 9 536', wdesc(N, BF, 32, 298, 512, 512, mode=1), 1, AMP, 30, 320),
        ('512->192 1x1, M 3 000', wdesc(N, BF, 10, 300, 512, 192, mode=1), 1, AMP, 47, 64),
        ('64->64 k3, M 76 288, 7 convs', wdesc(N, BF, 256, 298, 64, 64, kw=3, dil=2, mode=1), 7, N64, 71, 1088),
        ('64->64 k3, M 76 288', wdesc(N, BF, 256, 298, 64, 64, kw=3, dil=2, mode=1), 1, N64, 239, 320),
        ('64->64 k3, M 9 536, exact f32', wdesc(N, F32, 32, 298, 64, 64, kw=3, dil=2, mode=0), 1, F, 149, 64),
        ('80->512 k5, M 76 288, f32 operands', wdesc(N, F32, 256, 298, 80, 512, kw=5, mode=1), 1, AMP, 32, 2432),
        ('32->32 3x3 2-D, M 190 720', wdesc(N, F32, 8, 298, 32, 32, kw=9, mode=1, F=80), 1, AMP, 166, 1152),
        ('512->512 1x1, M 9 536, split precision', wdesc(N, F32, 32, 298, 512, 512, mode=2), 1, X3, 30, 320),
        ('64->64 1x1, M 19', wdesc(N, F32, 1, 19, 64, 64, mode=0), 1, F, 1, 32),
    ]
    tiles = {F: (64, 64), AMP: (128, 128), X3: (128, 128), N64: (64, 256), TR: (256, 256)}
    for name, d, nbatch, family, splits, rps in table:
        rc, k, tn, tk, s, r = plan(N, d, nbatch)
        assert rc == N.VP_OK, (name, rc)
        assert (k, s, r) == (family, splits, rps), (name, (k, s, r), (family, splits, rps))
        assert (tn, tk) == tiles[family], (name, tn, tk)
    # cus <= 0 means 256; any output pointer may be NULL
    d = table[10][1]
    assert plan(N, d, cus=0) == plan(N, d, cus=256) == plan(N, d, cus=-3)
    s = C.c_int()
    assert N.lib().vp_conv1d_wgrad_plan(C.byref(d), _PTR, 32, 1, 256, None, None, None, C.byref(s), None) == N.VP_OK and s.value == 166
    assert N.lib().vp_conv1d_wgrad_plan(C.byref(d), _PTR, 32, 1, 256, None, None, None, None, None) == N.VP_OK


MS = (1, 19, 31, 32, 33, 63, 64, 65, 777, 3000, 9536, 76288, 76289, 1900000)
COUTS = (4, 32, 64, 96, 128, 192, 256, 512, 1536)
CINS = (4, 32, 64, 80, 128, 256, 512, 1536)


def wgrad_grid(N, n=3000, seed=23):
    """n seeded valid (descriptor, nbatch, cus): 1x1 / tapped / strided / 2-D layers, f32 operands in modes 0..3 and bf16 operands
    (alone and batched), around the row counts at which a split rule changes."""
    rng = np.random.RandomState(seed)
    pick = lambda xs: xs[rng.randint(len(xs))]
    out = []
    while len(out) < n:
        M, Cout, Cin, kw = int(pick(MS)), int(pick(COUTS)), int(pick(CINS)), int(pick((1, 1, 3, 5, 9)))
        bf = bool(rng.randint(2))
        mode = int(rng.randint(4))
        nbatch = int(pick((1, 1, 2, 7, 15))) if bf else 1
        B = int(pick((1, 2, 8))) if M % 8 == 0 else 1
        F = 0
        if kw == 9:
            F = 10 if M >= 10 and (M // B) % 10 == 0 else 1
        T = M // B // max(F, 1)
        stride = 2 if kw == 1 and rng.randint(4) == 0 else 1
        ldx, xoff = (Cin, 0) if rng.randint(3) else (Cin + 8 * int(rng.randint(1, 5)), 4 * int(rng.randint(3)))
        if M >= 1900000 and ldx > 512:                       # (keep the imagined tensors under the library's 32-bit row offsets)
            ldx, xoff = Cin, 0
        d = wdesc(N, N.VP_BF16 if bf else N.VP_F32, B, T, Cin, Cout, kw=kw, dil=int(pick((1, 2, 3))), mode=mode, stride=stride, F=F, ldx=ldx,
                  xoff=xoff)
        assert rows_of(d) == M
        out.append((d, nbatch, int(pick(CUS))))
    return out


def tr256_splits(M, Cout, K):
    """rows of the 256-tile kernel: one workgroup per CU of a 256-CU chip, no split shorter than a 32-row stage, whole stages"""
    S = max(1, 256 // (-(-Cout // 256) * -(-K // 256)))
    if S * 32 > M:
        S = -(-M // 32)
    rps = -(-(-(-M // S)) // 32) * 32
    return -(-M // rps)


def tr256_sides(Cout, K):
    return (Cout % 256 == 0 or Cout == 128) and (K % 256 == 0 or K == 128)


def ref_workspace(d):
    """S = clamp(2048 / (ceil(Cout / 64) ceil(K / 64)), 1, 256), capped at ceil(M / 64), raised to the 256-tile split count where the
    geometry admits that kernel; bytes = S Cout K 4 + 256"""
    M, K = rows_of(d), d.KW * d.Cin
    S = min(256, max(1, 2048 // (-(-d.Cout // 64) * -(-K // 64))))
    if S * 64 > M:
        S = -(-M // 64)
    if d.KW == 1 and tr256_sides(d.Cout, K) and M >= 32:
        S = max(S, tr256_splits(M, d.Cout, K))
    return S * d.Cout * K * 4 + 256


def test_wgrad_plan_grid_properties(wg):
    """Every plan of 3 000 valid descriptors: at least one split, splits of whole staged chunks, no empty split and every row covered,
    the partials inside the workspace vp_conv1d_wgrad_workspace_bytes sizes -- whatever operand type and mode the descriptor had
    when it was sized -- and each family only where its kernel applies."""
    N = wg
    BF, F32 = N.VP_BF16, N.VP_F32
    seen = set()
    for d, nbatch, cus in wgrad_grid(N):
        M, K = rows_of(d), d.KW * d.Cin
        bf, two_d = d.dtype_in == BF, d.KF > 1
        rc, k, tn, tk, S, rps = plan(N, d, nbatch, cus)
        what = (M, d.Cout, d.Cin, d.KW, d.dtype_in, d.mfma_bf16, nbatch, cus, d.stride, d.ldx, d.xoff, (k, tn, tk, S, rps))
        assert rc == N.VP_OK, (rc, what)
        assert S >= 1, what
        assert rps % chunk_rows(N, k) == 0, what
        assert (S - 1) * rps < M <= S * rps, what
        need = nbatch * (S * d.Cout * K * 4 + 256)
        assert need <= nbatch * ws_bytes(N, d), what
        sized = ws_bytes(N, d)
        for dt, modes in ((F32, (0, 1, 2, 3)), (BF, (0, 1, 2))):   # the byte count is geometry only
            for m in modes:
                e = N.Conv1dDesc.from_buffer_copy(d)
                e.dtype_in, e.mfma_bf16, e.x, e.ldx, e.xoff = dt, m, None, 0, 0
                assert ws_bytes(N, e) == sized, (dt, m, what)
        if k == N.VP_WGRAD_TR256:
            Ne, Ke = max(d.Cout, 256), max(K, 256)
            assert bf and d.KW == 1 and d.stride == 1 and d.pad_left == 0 and d.T_in == d.T_out and not two_d and nbatch == 1, what
            assert tr256_sides(d.Cout, K) and not (d.Cout == 128 and K == 128) and 2.0 * M * Ne * Ke >= 3e10, what
            assert S == tr256_splits(M, d.Cout, K), what
        if k == N.VP_WGRAD_N64:
            assert bf and d.Cout <= 64 and K > 128 and not two_d and d.stride == 1, what
        assert (k == N.VP_WGRAD_X3) == (not bf and d.mfma_bf16 in (2, 3)), what
        assert (k == N.VP_WGRAD_F32) == (not bf and d.mfma_bf16 == 0), what
        if not bf and d.mfma_bf16 == 3:
            e = N.Conv1dDesc.from_buffer_copy(d)
            e.mfma_bf16 = 2
            assert plan(N, e, nbatch, cus) == (rc, k, tn, tk, S, rps), what
        seen.add(k)
    assert seen == {N.VP_WGRAD_F32, N.VP_WGRAD_AMP, N.VP_WGRAD_X3, N.VP_WGRAD_N64, N.VP_WGRAD_TR256}, seen


def test_wgrad_workspace_bytes_match_the_rule(N):
    """vp_conv1d_wgrad_workspace_bytes against the NumPy restatement of its rule, on the same grid (under any switch: the count does
    not depend on one)."""
    for d, _, _ in wgrad_grid(N):
        assert ws_bytes(N, d) == ref_workspace(d), (rows_of(d), d.Cout, d.Cin, d.KW, ws_bytes(N, d), ref_workspace(d))
    assert N.lib().vp_conv1d_wgrad_workspace_bytes(None) == 0


def test_wgrad_plan_error_paths(N):
    """vp_conv1d_wgrad_plan runs the launch's validation: the same codes, and the outputs left alone."""
    BF, F32 = N.VP_BF16, N.VP_F32
    E, U = N.VP_EINVAL, N.VP_EUNSUP
    untouched = (-1,) * 5
    ok = lambda dt=F32, **kw: wdesc(N, dt, 2, 100, 64, 64, kw=3, **kw)
    assert plan(N, ok())[0] == N.VP_OK
    assert plan(N, None, lddz=64) == (E,) + untouched
    assert plan(N, ok(), dz=None) == (E,) + untouched
    d = ok()
    d.x = None
    assert plan(N, d) == (E,) + untouched
    assert plan(N, wdesc(N, F32, 2, 100, 6, 64, kw=3)) == (E,) + untouched                   # Cin % 4
    assert plan(N, ok(), lddz=66) == (E,) + untouched                                         # lddz % 4
    d = wdesc(N, F32, 2, 100, 32, 32, kw=9, F=10)
    d.pad_mode = N.VP_PAD_REFLECT                                                             # 2-D: zero padding only
    assert plan(N, d) == (E,) + untouched
    d = wdesc(N, F32, 2, 100, 32, 32, kw=8, F=10)                                             # 8 taps are not 3 x KT
    assert plan(N, d) == (E,) + untouched
    assert plan(N, ok(mode=4)) == (E,) + untouched
    assert plan(N, ok(mode=-1)) == (E,) + untouched
    assert plan(N, ok(BF, mode=1), nbatch=0) == (E,) + untouched
    assert plan(N, ok(), nbatch=2) == (E,) + untouched                                        # batched launches take bf16 operands
    assert plan(N, ok(BF, mode=1), nbatch=2)[0] == N.VP_OK
    assert plan(N, ok(N.VP_HL32)) == (U,) + untouched
    assert plan(N, wdesc(N, F32, 0, 100, 64, 64)) == (E,) + untouched                         # empty batch
