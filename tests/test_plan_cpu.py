"""CPU tests of the split-precision engine's two host-side decisions (no GPU needed: neither entry point touches the device):
the time-segment plan of the fused Res2 chain (vp_res2_chain_x3_plan, csrc/res2_x3.hip: rx_plan) and the ECAPA driver's choice between
its split-plane fast path and the generic split-precision path (vp_ecapa_x3_fast_path, csrc/ecapa.hip: ecapa_hl_ok), each against a
NumPy / Python restatement of its contract."""
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
