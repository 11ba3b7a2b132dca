"""CPU tests of the engine's three host-side decisions (no GPU needed: none of the entry points touches the device): the time-segment
plan of the fused Res2 chain (vp_res2_chain_x3_plan, csrc/res2_x3.hip: rx_plan), the ECAPA driver's choice between its split-plane
fast path and the generic split-precision path (vp_ecapa_x3_fast_path, csrc/ecapa.hip: ecapa_hl_ok), each against a NumPy / Python
restatement of its contract, and the kernel family and tile geometry vp_conv1d_fwd gives a layer (vp_conv1d_plan,
csrc/conv_gemm.hip: conv_plan) against a table of layer shapes and the properties every plan must have."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

LDS_BYTES = 160 * 1024
WT_BYTES = 3 * 2 * 64 * 128                   # one conv's split weights, three taps
PRM_BYTES = 3 * 64 * 4                        # bias, BN scale, BN shift of one conv
MAX_SEG = 64
T_MAX = 10000


@pytest.fixture(scope='module')
def N():
    from ppvector import _native as N
    N.load_library()
    return N


def _windows(T, ns, ts, H):
    """Largest held window (own frames + halos of H on each interior side) over the ns segments, per T (vectorised)."""
    need = np.zeros_like(T)
    for s in range(int(ns.max()) if np.size(ns) else 0):
        o0 = s * ts
        o1 = np.minimum(T, o0 + ts)
        w = np.minimum(T, o1 + H) - np.maximum(0, o0 - H)
        need = np.where(s < ns, np.maximum(need, w), need)
    return need


def ref_plan(T, nconv, dil):
    """Brute force: the fewest counts ns <= 64 of whole-tile segments (ts = ceil(T / ns) rounded up to 16) with a non-empty last segment,
    dil < ts, every window in tp <= 256 frames (16 waves' tiles) and 4 tp 128 + weights + nconv per-channel terms <= 160 KiB.
    Returns (planned, nsplit, tseg, tp, lds) arrays over T."""
    T = np.asarray(T, np.int64)
    H = nconv * dil
    plan = np.zeros((4, T.size), np.int64)
    done = np.zeros(T.size, bool)
    for ns in range(1, MAX_SEG + 1):
        ts = (-(-T // ns) + 15) // 16 * 16
        tp = (_windows(T, np.full_like(T, ns), ts, H) + 15) // 16 * 16
        lds = 4 * tp * 128 + WT_BYTES + nconv * PRM_BYTES
        ok = ~done & (T >= 2) & (dil < T) & ((ns - 1) * ts < T) & (dil < ts) & (tp <= 256) & (lds <= LDS_BYTES)
        plan[:, ok] = np.stack([np.full_like(T, ns), ts, tp, lds])[:, ok]
        done |= ok
    return done, plan[0], plan[1], plan[2], plan[3]


def lib_plan(N, Ts, nconv, dil):
    lib = N.lib()
    ns, ts, tp, lds = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    out = np.zeros((5, len(Ts)), np.int64)
    for i, T in enumerate(Ts):
        rc = lib.vp_res2_chain_x3_plan(int(T), nconv, dil, C.byref(ns), C.byref(ts), C.byref(tp), C.byref(lds))
        assert rc in (N.VP_OK, N.VP_EUNSUP), (T, nconv, dil, rc)
        out[:, i] = (rc == N.VP_OK, ns.value, ts.value, tp.value, lds.value)
    return out[0].astype(bool), out[1], out[2], out[3], out[4]


@pytest.mark.parametrize('nconv', [1, 2, 3, 7, 10, 11, 15])
def test_res2_x3_plan_contract(N, nconv):
    """For every T = 2 .. 10 000 and dilation 1 .. 4: a returned plan cuts into whole-tile segments with no empty one, holds every
    segment's window (own frames + halos) in tp frames, asks for exactly the LDS it needs and no more than the CU has, and uses the
    fewest segments that do all that; VP_EUNSUP exactly when no count up to 64 does.  At ECAPA's 7 convs and dilation <= 4, every
    T up to 9 216 frames has a plan (a planner that stops at the first count with an empty last segment loses 1 585 .. 1 600 at
    dilation 4, and everything from 2 161 on)."""
    T = np.arange(2, T_MAX + 1, dtype=np.int64)
    for dil in (1, 2, 3, 4):
        H = nconv * dil
        ok, ns, ts, tp, lds = lib_plan(N, T, nconv, dil)
        r_ok, r_ns, r_ts, r_tp, r_lds = ref_plan(T, nconv, dil)
        miss = T[ok != r_ok]
        assert miss.size == 0, (nconv, dil, 'planned by one side only at T =', miss[:10], int(ok.sum()), int(r_ok.sum()))
        assert np.all(ns[~ok] == 0) and np.all(ts[~ok] == 0) and np.all(tp[~ok] == 0) and np.all(lds[~ok] == 0)
        Tp, ns, ts, tp, lds = T[ok], ns[ok], ts[ok], tp[ok], lds[ok]
        assert np.all(ts % 16 == 0) and np.all(tp % 16 == 0)
        assert np.all((ns >= 1) & (ns <= MAX_SEG))
        assert np.all(((ns - 1) * ts < Tp) & (Tp <= ns * ts)), 'an empty or missing segment'
        assert np.all(_windows(Tp, ns, ts, H) <= tp) and np.all(tp <= 256)
        assert np.all(lds == 4 * tp * 128 + WT_BYTES + nconv * PRM_BYTES) and np.all(lds <= LDS_BYTES)
        assert np.all(dil < ts)
        for name, got, want in (('nsplit', ns, r_ns), ('tseg', ts, r_ts), ('tp', tp, r_tp), ('lds', lds, r_lds)):
            bad = Tp[got != want[ok]]
            assert bad.size == 0, (nconv, dil, name, bad[:10])
        assert np.all(~ok[T <= dil]), 'dil >= T has no reflect padding'
        if nconv == 7:
            assert np.all(ok[(T > dil) & (T <= 9216)]), (dil, T[~ok & (T > dil) & (T <= 9216)][:10])
        print(f'[plan nconv={nconv} dil={dil}] planned {int(ok.sum())} of {T.size} T, largest {int(Tp.max())}, '
              f'up to {int(ns.max())} segments, tp <= {int(tp.max())}, LDS <= {int(lds.max())} B')


def test_res2_x3_plan_refuses_outside_the_abi(N):
    lib = N.lib()
    ns = C.c_int(-1)
    for T, nconv, dil in ((1, 7, 1), (300, 0, 2), (300, 16, 2), (300, 7, 0), (4, 7, 4), (9217, 7, 4)):
        assert lib.vp_res2_chain_x3_plan(T, nconv, dil, C.byref(ns), None, None, None) == N.VP_EUNSUP, (T, nconv, dil)
        assert ns.value == 0
    assert lib.vp_res2_chain_x3_plan(298, 7, 2, C.byref(ns), None, None, None) == N.VP_OK and ns.value == 2


# ------------------------------------------------------------------------------------------- the ECAPA fast-path predicate
_PTR = 0x1000                                    # dummy non-null pointers: the predicate reads the struct, never through it


def _layer(L, cin, cout, kw, dil, split=True):
    L.w, L.bias, L.bn_scale, L.bn_shift = _PTR, _PTR + 8, _PTR + 16, _PTR + 24
    L.cin, L.cout, L.kw, L.dil = cin, cout, kw, dil
    L.w_hl = _PTR + 32 if split else None


def ecapa_weights(N, C_=512, Cm=1536, scale=8, dils=(2, 3, 4), att=128, dtype=None):
    W = N.EcapaWeights()
    W.dtype = N.VP_F32X3 if dtype is None else dtype
    W.feat_dim, W.embd_dim, W.n_blocks, W.res2_scale, W.se_ch = 80, 192, len(dils), scale, 128
    _layer(W.block0, 80, C_, 5, 1)
    width = C_ // scale
    for i, d in enumerate(dils):
        S = W.blk[i]
        _layer(S.tdnn1, C_, C_, 1, 1)
        for j in range(scale - 1):
            _layer(S.res2[j], width, width, 3, d)
        _layer(S.tdnn2, C_, C_, 1, 1)
        S.se_w1, S.se_b1, S.se_w2, S.se_b2 = _PTR, _PTR, _PTR, _PTR
    _layer(W.mfa, len(dils) * C_, Cm, 1, 1)
    _layer(W.asp.tdnn, 3 * Cm, att, 1, 1)
    W.asp.w_ctx, W.asp.conv_w, W.asp.conv_b, W.asp.C, W.asp.att = _PTR, _PTR, _PTR, Cm, att
    W.fc_w, W.fc_b = _PTR, _PTR
    return W


def ref_fast_path(N, W, B, T):
    """ecapa_hl_ok (csrc/ecapa.hip) restated, with the Res2 chain's own shape check and the plan restatement above."""
    if os.environ.get('VPMI_X3_GENERIC') is not None:
        return False
    C_, Cm, sc = W.block0.cout, W.mfa.cout, W.res2_scale
    if W.dtype != N.VP_F32X3 or not 1 <= W.n_blocks <= N.VP_MAX_SE_BLOCKS or not 2 <= sc <= N.VP_MAX_RES2 + 1:
        return False
    if (C_ % 32 or Cm % 32 or C_ % sc or W.asp.att != 128 or not W.mfa.w_hl or not W.asp.tdnn.w_hl or not W.asp.w_ctx or T < 128 or
            B * T < 128 * 32 or C_ < 256 or Cm < 256):
        return False
    nconv, width = sc - 1, C_ // sc
    for i in range(W.n_blocks):
        S = W.blk[i]
        if not S.tdnn1.w_hl or not S.tdnn2.w_hl:
            return False
        if width != 64 or T < 2 or C_ % 32 or not 1 <= B <= 65535 or B * T * C_ * 4 >= 0xffffff00:
            return False
        dil = S.res2[0].dil
        for j in range(nconv):
            L = S.res2[j]
            if (L.kw, L.cin, L.cout, L.dil) != (3, 64, 64, dil) or not (L.bias and L.bn_scale and L.bn_shift and L.w_hl):
                return False
        if not _ref_planned(T, nconv, dil):
            return False
    return True


@functools.lru_cache(maxsize=None)
def _ref_planned(T, nconv, dil):
    return bool(ref_plan([T], nconv, dil)[0][0])


def _check(N, W, B, T, want):
    got = N.lib().vp_ecapa_x3_fast_path(C.byref(W), B, T)
    ref = ref_fast_path(N, W, B, T)
    assert got in (0, 1)
    assert bool(got) == ref == want, (B, T, got, ref, want)


def test_ecapa_x3_fast_path_predicate(N):
    """vp_ecapa_x3_fast_path on both sides of every condition of ecapa_hl_ok, against the restatement and the expected answer:
    T 127 / 128, B T 4095 / 4096, a missing split weight, Res2 width != 64, the T windows a planner that stops early lost at each
    dilation, the largest planned T at dilation 4 (9 216 / 9 217), and the 32-bit byte offsets of the Res2 chain's input."""
    W = ecapa_weights(N)
    _check(N, W, 64, 127, False)
    _check(N, W, 64, 128, True)
    _check(N, W, 33, 127, False)                           # B T = 4191 >= 4096: T alone refuses
    _check(N, W, 1, 4095, False)
    _check(N, W, 1, 4096, True)
    _check(N, W, 32, 128, True)
    _check(N, W, 31, 132, False)                           # 4092 frames
    _check(N, W, 3, 1592, True)
    _check(N, W, 2, 4000, True)
    _check(N, W, 1, 4000, False)
    _check(N, W, 3, 2000, True)
    _check(N, W, 1, 9216, True)
    _check(N, W, 1, 9217, False)                           # no plan at dilation 4 (the third block)
    _check(N, W, 1023, 2048, True)                         # 1023 x 2048 x 512 x 4 B < 4 GiB - 256
    _check(N, W, 1024, 2048, False)                        # = 4 GiB
    # the T windows a planner that stops at the first count with an empty last segment loses, per dilation (single-block backbones)
    lost = {4: [1585, 1600, 1729, 1760, 1873, 1936, 2017, 2112, 2161, 3000, 6000], 3: [1921, 2500, 7000], 2: [2289, 5000, 9216]}
    for d, Ts in lost.items():
        Wd = ecapa_weights(N, dils=(d,))
        for T in Ts:
            _check(N, Wd, 4, T, True)
    # missing split weights anywhere the fast path reads them
    for where in ('tdnn1', 'tdnn2', 'res2', 'mfa', 'asp'):
        Wm = ecapa_weights(N)
        {'tdnn1': lambda: setattr(Wm.blk[1].tdnn1, 'w_hl', None), 'tdnn2': lambda: setattr(Wm.blk[2].tdnn2, 'w_hl', None),
         'res2': lambda: setattr(Wm.blk[2].res2[3], 'w_hl', None), 'mfa': lambda: setattr(Wm.mfa, 'w_hl', None),
         'asp': lambda: setattr(Wm.asp.tdnn, 'w_hl', None)}[where]()
        _check(N, Wm, 16, 298, False)
    Wc = ecapa_weights(N)
    Wc.asp.w_ctx = None
    _check(N, Wc, 16, 298, False)
    # Res2 width != 64 (res2net_scale 4 at 512 channels), and width 64 with 15 convs (1024 channels, scale 16: LDS-limited)
    _check(N, ecapa_weights(N, scale=4), 16, 298, False)
    Wb = ecapa_weights(N, C_=1024, scale=16)
    _check(N, Wb, 16, 298, True)
    _check(N, Wb, 1, 4096, True)
    _check(N, Wb, 1, 4097, False)                          # 15 convs at dilation 4: T <= 4 096
    _check(N, ecapa_weights(N, att=64), 16, 298, False)
    _check(N, ecapa_weights(N, dtype=N.VP_F32), 16, 298, False)
    _check(N, ecapa_weights(N, dtype=N.VP_BF16), 16, 298, False)


def test_ecapa_x3_fast_path_predicate_sweep(N):
    """The predicate against its restatement on a grid of (B, T) around the cliffs, for ECAPA's dilations and a single-block
    backbone at each dilation."""
    Ts = sorted({2, 3, 100, 127, 128, 129, 298, 1584, 1585, 1600, 1601, 1920, 1921, 2160, 2161, 2288, 2289, 4095, 4096, 4097,
                 6000, 9215, 9216, 9217, 10000})
    Bs = (1, 2, 3, 31, 32, 33, 256)
    for dils in ((2, 3, 4), (2,), (3,), (4,)):
        W = ecapa_weights(N, dils=dils)
        for B in Bs:
            for T in Ts:
                got = N.lib().vp_ecapa_x3_fast_path(C.byref(W), B, T)
                assert bool(got) == ref_fast_path(N, W, B, T), (dils, B, T, got)


# ------------------------------------------------------------------------------------------- the conv forward's kernel choice
CONV_ENV = ('VPMI_CONV256', 'VPMI_RING_MIN_COUT', 'VPMI_HL_BN128', 'VPMI_BN64', 'VPMI_GROUP_M')
TILE_ROWS = {0: 128, 1: 256, 2: 256, 3: 128}        # VP_CONV_K128, _K256_TWO_STAGE, _K256_RING, _K128X256_RING
GROUP_CLAMP = {0: 16, 1: 16, 2: 16, 3: 32}


@pytest.fixture
def conv(N):
    """The library for the tests whose expected plans are those of the default switches.  The switches are A/B knobs the library
    reads once per process, so with one of them exported these tests cannot say anything about the defaults: they fail, naming the
    variable.  (test_conv1d_plan_batch_slices and test_conv1d_plan_error_paths hold under any setting and do not come through here.)"""
    exported = [v for v in CONV_ENV if os.environ.get(v) is not None]
    assert not exported, f'unset {", ".join(exported)}: the plans pinned here are those of the default conv dispatch switches'
    assert (N.VP_CONV_K128, N.VP_CONV_K256_TWO_STAGE, N.VP_CONV_K256_RING, N.VP_CONV_K128X256_RING) == (0, 1, 2, 3)
    return N


def conv_desc(N, dt_in, dt_out, B, T_in, Cin, Cout, kw=1, dil=1, stride=1, T_out=None, pad_mode=None, psum=False, ldx=None, **more):
    """A valid vp_conv1d_desc with dummy non-null tensor pointers (the plan reads the struct, never through it): 'same' padding for
    tapped layers (reflect unless pad_mode says otherwise), none for 1x1 layers."""
    d = N.Conv1dDesc()
    d.dtype_in, d.dtype_out = dt_in, dt_out
    d.B, d.T_in, d.T_out = B, T_in, T_in if T_out is None else T_out
    d.Cin, d.Cout, d.KW, d.dilation, d.stride = Cin, Cout, kw, dil, stride
    d.pad_mode = pad_mode if pad_mode is not None else (N.VP_PAD_REFLECT if kw > 1 else N.VP_PAD_NONE)
    d.pad_left = dil * (kw - 1) // 2 if d.pad_mode != N.VP_PAD_NONE else 0
    d.x, d.w, d.y = _PTR, _PTR + 64, _PTR + 128
    d.ldx, d.ldy = Cin if ldx is None else ldx, Cout
    if psum:
        d.psum = d.psumsq = _PTR + 192
    if N.VP_HL32 in (dt_in, dt_out):
        d.mfma_bf16 = 2
    for k, v in more.items():
        setattr(d, k, v)
    return d


def conv_plan(N, d):
    """(rc, kernel, tile_n, tiles_m, tiles_n, group_m, launches)"""
    out = [C.c_int(-1) for _ in range(6)]
    rc = N.lib().vp_conv1d_plan(C.byref(d), *[C.byref(o) for o in out])
    return (rc,) + tuple(o.value for o in out)


def _table(N):
    """name -> (descriptor, kernel, tile_n, tiles_m, tiles_n, group_m) at the default schedule; None = not pinned.  B 57 x T 298 =
    16 986 rows = 133 tiles of 128 = 67 of 256; the wide tiles want 128 x 32 (K128X256_RING) or 256 x 64 = 16 384 rows."""
    BF, F32, HL = N.VP_BF16, N.VP_F32, N.VP_HL32
    K128, TWO, RING, R128 = 0, 1, 2, 3
    return {
        'bf16 1x1 512->512': (conv_desc(N, BF, BF, 57, 298, 512, 512), R128, 256, 133, 2, 32),
        'bf16 1x1 512->512 psum': (conv_desc(N, BF, BF, 57, 298, 512, 512, psum=True), R128, 256, 133, 2, 32),
        'bf16->f32 1x1 512->512 (data gradient)': (conv_desc(N, BF, F32, 57, 298, 512, 512), R128, 256, 133, 2, 32),
        'bf16 taps 64->256 k3 dil 2': (conv_desc(N, BF, BF, 66, 250, 64, 256, kw=3, dil=2), TWO, 256, 65, 1, 16),         # MODE_TAPS
        'bf16 taps 80->512 k5': (conv_desc(N, BF, BF, 70, 241, 80, 512, kw=5), TWO, 256, 66, 2, 16),                       # MODE_TAPS_GEN
        'bf16 taps 64->256 k3 dil 2, 15 000 rows': (conv_desc(N, BF, BF, 60, 250, 64, 256, kw=3, dil=2), K128, 128, 118, 2, 16),
        'bf16 1x1 512->512 stride 2': (conv_desc(N, BF, BF, 57, 596, 512, 512, stride=2, T_out=298), TWO, 256, 67, 2, 16),
        'bf16 1x1 1536->128': (conv_desc(N, BF, BF, 57, 298, 1536, 128), K128, 128, 133, 1, 16),
        'hl32 1x1 1536->128': (conv_desc(N, HL, HL, 57, 298, 1536, 128), K128, 64, 133, 2, 16),
        'hl32 1x1 512->512': (conv_desc(N, HL, HL, 57, 298, 512, 512), R128, 256, 133, 2, 32),
        'f32 64->32': (conv_desc(N, F32, F32, 2, 100, 64, 32), K128, 32, 2, 1, 16),
        'f32 1x1 pro 64->128': (conv_desc(N, F32, F32, 2, 100, 64, 128, pro_scale=_PTR, pro_shift=_PTR), K128, 64, None, 2, None),
    }


class _selected:
    """with _selected(N, s): vp_conv256_select(s) inside, the previous selection restored after."""

    def __init__(self, N, sched):
        self.N, self.sched = N, sched

    def __enter__(self):
        self.prev = self.N.lib().vp_conv256_select(self.sched)

    def __exit__(self, *exc):
        self.N.lib().vp_conv256_select(self.prev)


def test_conv1d_plan_table(conv):
    """The plan of the layer shapes the backbones and the training step run, at the default schedule."""
    for name, (d, *want) in _table(conv).items():
        rc, *got = conv_plan(conv, d)
        assert rc == conv.VP_OK, (name, rc)
        assert got[5] == 1, (name, got)
        for what, g, w in zip(('kernel', 'tile_n', 'tiles_m', 'tiles_n', 'group_m'), got, want):
            assert w is None or g == w, (name, what, g, w)
    # any output pointer may be NULL
    d = _table(conv)['bf16 1x1 512->512'][0]
    tm = C.c_int()
    assert conv.lib().vp_conv1d_plan(C.byref(d), None, None, C.byref(tm), None, None, None) == conv.VP_OK and tm.value == 133
    assert conv.lib().vp_conv1d_plan(C.byref(d), None, None, None, None, None, None) == conv.VP_OK


def test_conv1d_plan_under_select(conv):
    """vp_conv256_select: 4 = K256_RING (f32 output then falls to K128), 3 = K256_TWO_STAGE, 1 and 2 run as 3, 5 as 4, 7 = 6 for
    K <= 1024 else 4, 0 = K128 everywhere; the call returns the previous selection and ignores values outside -1 .. 7."""
    N, lib = conv, conv.lib()
    table = _table(N)
    wide = conv_desc(N, N.VP_BF16, N.VP_BF16, 57, 298, 1536, 1536)
    prev = lib.vp_conv256_select(-1)
    try:
        assert lib.vp_conv256_select(8) == -1 and lib.vp_conv256_select(-2) == -1          # out of range: query only
        plans = {}
        for s in range(0, 8):
            assert lib.vp_conv256_select(s) == (s - 1 if s else -1)
            plans[s] = {name: conv_plan(N, d) for name, (d, *_) in table.items()}
            plans[s]['wide'] = conv_plan(N, wide)
        assert lib.vp_conv256_select(-1) == 7
        assert plans[4]['bf16 1x1 512->512'] == (N.VP_OK, 2, 256, 67, 2, 16, 1)
        assert plans[4]['bf16->f32 1x1 512->512 (data gradient)'] == (N.VP_OK, 0, 128, 133, 4, 16, 1)
        assert plans[3]['bf16 1x1 512->512'] == (N.VP_OK, 1, 256, 67, 2, 16, 1)
        assert plans[1] == plans[3] and plans[2] == plans[3]
        assert plans[5] == plans[4]
        assert plans[6] == {**{name: conv_plan(N, d) for name, (d, *_) in table.items()}, 'wide': conv_plan(N, wide)}      # -1 = 6
        assert plans[6]['wide'] == (N.VP_OK, 3, 256, 133, 6, 10, 1) and plans[4]['wide'] == (N.VP_OK, 2, 256, 67, 6, 5, 1)
        assert plans[7]['bf16 1x1 512->512'] == plans[6]['bf16 1x1 512->512']               # K = 512
        assert plans[7]['wide'] == plans[4]['wide']                                         # K = 1536
        # the tapped and the strided layers are on the two-stage kernel under 3, 4, 6 and 7 alike
        for name in ('bf16 taps 64->256 k3 dil 2', 'bf16 taps 80->512 k5', 'bf16 1x1 512->512 stride 2'):
            assert len({plans[s][name] for s in (3, 4, 6, 7)}) == 1 and plans[3][name][1] == 1, name
        for name, p in plans[0].items():
            assert p[0] == N.VP_OK and p[1] == 0, (name, p)
        assert plans[0]['hl32 1x1 512->512'] == (N.VP_OK, 0, 128, 133, 4, 16, 1)
    finally:
        lib.vp_conv256_select(prev)


def conv_grid(N, n=2000, seed=20):
    """n seeded valid descriptors: 1x1 / tapped / strided 1x1 / gated / input-prologue / 2-D layers in every precision pair the
    library builds, with and without fused time sums, around the row and column thresholds of the wide tiles."""
    rng = np.random.RandomState(seed)
    BF, F32, HL = N.VP_BF16, N.VP_F32, N.VP_HL32
    pairs = ((BF, BF), (BF, F32), (F32, F32), (HL, HL), (HL, F32), (F32, HL))
    pick = lambda xs: xs[rng.randint(len(xs))]
    out = []
    while len(out) < n:
        dt_in, dt_out = pick(pairs)
        hl = HL in (dt_in, dt_out)
        kind = pick(('1x1', '1x1', 'taps', 'taps', 'strided', 'gate', 'pro', '2d'))
        if hl and kind in ('gate', 'pro', '2d'):
            kind = '1x1'
        B, T = int(pick((1, 2, 8, 13, 32, 55, 57, 64, 66, 130))), int(pick((24, 100, 127, 128, 200, 250, 298, 512)))
        Cin = int(pick((32, 64, 96, 128, 256, 512, 1024, 1536) + (() if hl else (80, 40))))
        Cout = int(pick((32, 64, 96, 128, 224, 256, 320, 512, 1536)))
        psum = bool(rng.randint(2)) and kind != '2d' and (T // 2 if kind == 'strided' else T) >= 22      # (<= 8 segments per M-tile)
        if dt_in == HL and dt_out == F32:                    # built on the ring only: wide 1x1 layers
            kind, Cout, B, T = '1x1', max(Cout, 256), max(B, 32), max(T, 128)
        kw = dict(psum=psum)
        if dt_in == F32 and not hl:
            kw['mfma_bf16'] = int(rng.randint(4))
        if kind == 'taps':
            kw.update(kw=int(pick((3, 5))), dil=int(pick((1, 2, 3))), pad_mode=pick((N.VP_PAD_REFLECT, N.VP_PAD_ZERO)))
        elif kind == 'strided':
            kw.update(stride=2, T_out=T // 2)
        elif kind == 'gate':
            kw.update(gate=_PTR, gate_len=100, gate_nseg=(T + 99) // 100)
        elif kind == 'pro':
            kw.update(pro_scale=_PTR, pro_shift=_PTR)
        elif kind == '2d':
            kw.update(kw=9, KF=3, F_in=10, F_out=10, stride_f=1, pad_f=1, pad_mode=N.VP_PAD_ZERO)
        d = conv_desc(N, dt_in, dt_out, B, T, Cin, Cout, **kw)
        if kind == '2d':
            d.pad_left = 1
        out.append((kind, d))
    return out


def test_conv1d_plan_grid_properties(conv):
    """Every plan of ~2 000 valid descriptors, under every selection: the tile grid covers the M x N problem with no empty row or
    column of tiles, the group size is within its family's clamp, f32 output never gets a 256-row family, gated and 2-D layers
    always get K128, and fused time sums with T_out < 128 never get a wide family (its epilogue writes two utterance segments
    per 128 rows)."""
    N, lib = conv, conv.lib()
    grid = conv_grid(N)
    seen = set()
    prev = lib.vp_conv256_select(-1)
    try:
        for s in (-1, 0, 1, 2, 3, 4, 5, 6, 7):
            lib.vp_conv256_select(s)
            for kind, d in grid:
                rc, k, tn, tm_, tn_, gm, nl = conv_plan(N, d)
                what = (s, kind, d.dtype_in, d.dtype_out, d.B, d.T_in, d.T_out, d.Cin, d.Cout, d.KW, bool(d.psum), (k, tn, tm_, tn_, gm, nl))
                if s == 0 and (d.dtype_in, d.dtype_out) == (N.VP_HL32, N.VP_F32):
                    assert rc == N.VP_EUNSUP, (rc, what)         # built on the ring only
                    continue
                assert rc == N.VP_OK and nl == 1, (rc, what)
                M = d.B * d.T_out * (d.F_out if kind == '2d' else 1)
                rows = TILE_ROWS[k]
                assert tn in ((32, 64, 128) if k == 0 else (256,)), what
                assert tm_ * rows >= M > (tm_ - 1) * rows, what
                assert tn_ * tn >= d.Cout > (tn_ - 1) * tn, what
                assert 1 <= gm <= GROUP_CLAMP[k], what
                if d.dtype_out == N.VP_F32:
                    assert rows == 128, what
                if kind in ('gate', '2d') or s == 0:
                    assert k == 0, what
                if d.psum and d.T_out < 128:
                    assert k == 0, what
                if k in (2, 3):                              # the rings: plain 1x1 layers only
                    assert d.KW == 1 and d.stride == 1 and d.T_in == d.T_out and kind != 'pro', what
                if k != 0:
                    assert d.dtype_in in (N.VP_BF16, N.VP_HL32) and d.Cout >= 256 and M >= 128 * 32, what
                seen.add((s if s in (0, 3, 4, 6) else None, k))
    finally:
        lib.vp_conv256_select(prev)
    assert {(0, 0), (3, 0), (3, 1), (4, 1), (4, 2), (6, 1), (6, 3), (4, 3), (3, 3)} <= seen, sorted(seen, key=str)     # (hl32: always 3)


def test_conv1d_plan_batch_slices(N):
    """Activations past the 32-bit buffer offsets run as launches over slices of bc utterances: bc = the most whose activations stay
    under 0xe0000000 bytes, rounded down -- when time sums are fused -- to a count whose rows end on an M-tile boundary of the
    partial-sum arrays (bc T_out % 128 == 0).  The plan reports the launches and describes the first slice.  (f32 layers: no
    dispatch switch touches them.)"""
    for B, T, psum in ((128, 20000, True), (128, 20000, False), (8000, 298, True), (8000, 298, False)):
        d = conv_desc(N, N.VP_F32, N.VP_F32, B, T, 64, 64, ldx=512, psum=psum)
        assert B * T * 512 * 4 > 1 << 32
        rc, k, tn, tm_, tn_, gm, nl = conv_plan(N, d)
        assert (rc, k, tn, tn_) == (N.VP_OK, 0, 64, 1), (B, T, psum, rc, k, tn, tn_)
        bc = 0xe0000000 // (T * 512 * 4)
        if psum:
            q = 128 // np.gcd(T, 128)
            bc = bc // q * q
            assert bc * T % 128 == 0 and tm_ * 128 == bc * T, (B, T, bc, tm_)
        assert 1 <= bc < B and bc * T * 512 * 4 < 1 << 32
        assert nl == -(-B // bc) and nl > 1, (B, T, psum, nl, bc)
        assert tm_ == -(-bc * T // 128), (B, T, psum, tm_, bc)
    d = conv_desc(N, N.VP_F32, N.VP_F32, 2, 4200000, 512, 512)          # the first utterance alone is past 4 GiB: no slice helps
    assert conv_plan(N, d)[0] == N.VP_EUNSUP


def test_conv1d_plan_error_paths(N):
    """vp_conv1d_plan runs vp_conv1d_fwd's validation: the descriptors tests/test_gpu_kernels.py sees refused before any launch
    (test_conv1d_rejects_bad_shapes, test_conv1d_mfma_mode_contract) and a few more return the same code here, and leave the
    outputs alone.  None of it depends on a dispatch switch."""
    BF, F32, HL = N.VP_BF16, N.VP_F32, N.VP_HL32
    E, U = N.VP_EINVAL, N.VP_EUNSUP
    cases = [
        ('Cin % 8 != 0 (bf16)', conv_desc(N, BF, BF, 1, 8, 20, 16, kw=3), None, None, E),
        ('reflect pad >= T', conv_desc(N, F32, F32, 1, 2, 16, 16, kw=3, dil=4), None, None, E),
        ('one utterance past 4 GiB', conv_desc(N, BF, BF, 1, 4200000, 512, 512, pad_mode=N.VP_PAD_REFLECT), None, None, U),
        ('empty batch', conv_desc(N, BF, BF, 0, 4200000, 512, 512, pad_mode=N.VP_PAD_REFLECT), None, None, E),
        ('null x', conv_desc(N, BF, BF, 2, 100, 64, 64), 'x', None, E),
        ('null w', conv_desc(N, BF, BF, 2, 100, 64, 64), 'w', None, E),
        ('null y', conv_desc(N, BF, BF, 2, 100, 64, 64), 'y', None, E),
        ('bad dtype', conv_desc(N, BF, BF, 2, 100, 64, 64), 'dtype_in', 9, E),
        ('f32 -> bf16', conv_desc(N, F32, BF, 2, 100, 64, 64), None, None, U),
        ('hl32 Cin % 32', conv_desc(N, HL, HL, 2, 100, 48, 64), None, None, E),
        ('hl32 tapped 2-D', conv_desc(N, HL, HL, 2, 100, 64, 64, KF=3, kw=9, F_in=4, F_out=4, stride_f=1), None, None, U),
        ('hl32 -> f32 off the ring', conv_desc(N, HL, F32, 2, 100, 64, 64), None, None, U),
        ('time sums with T_out 16', conv_desc(N, F32, F32, 4, 16, 64, 64, psum=True), None, None, U),
        ('2-D with time sums', conv_desc(N, F32, F32, 2, 20, 16, 16, kw=9, KF=3, F_in=4, F_out=4, stride_f=1, pad_mode=N.VP_PAD_ZERO,
                                         psum=True), None, None, U),
        ('un-padded window leaves the input', conv_desc(N, F32, F32, 2, 20, 16, 16, kw=3, pad_mode=N.VP_PAD_NONE), None, None, E),
        ('ysplit without y2', conv_desc(N, F32, F32, 2, 20, 16, 16, ysplit=8), None, None, E),
        ('gate without segments', conv_desc(N, F32, F32, 2, 20, 16, 16, gate=_PTR), None, None, E),
        ('prologue on a tapped conv', conv_desc(N, F32, F32, 2, 20, 16, 16, kw=3, pro_scale=_PTR, pro_shift=_PTR), None, None, E),
    ]
    for dt, cin, kw in ((F32, 64, 3), (HL, 64, 1)):                      # test_conv1d_mfma_mode_contract
        for mode in (-1, 4, 7) + ((3,) if dt == HL else ()):
            cases.append((f'mfma_bf16 {mode} dtype {dt}', conv_desc(N, dt, dt, 2, 300, cin, 64, kw=kw), 'mfma_bf16', mode, E))
    for name, d, field, value, want in cases:
        if field:
            setattr(d, field, value)
        assert conv_plan(N, d) == (want, -1, -1, -1, -1, -1, -1), name
    assert N.lib().vp_conv1d_plan(None, None, None, None, None, None, None) == E
    ok = conv_desc(N, HL, HL, 2, 300, 64, 64)                            # ... and the same descriptors in mode 2 plan
    assert conv_plan(N, ok)[:2] == (N.VP_OK, 0)
