"""The energy voice-activity detector on the MI355X (csrc/vad.hip) against tests/vad_oracle.py: stage A (frame energies) against float64
with a bound taken from what f32 rounding costs the restatement on the same input, stage B (thresholds and regions) bit-exactly on
planted energies, both through EnergyVad on a planted waveform, and PPVectorPredictor with a detector set."""
import functools

import numpy as np
import pytest
import torch

from tests import vad_oracle as ov

pytestmark = pytest.mark.gpu

# 64 is the kernel's tile of frames for every (win, hop) here ((12288 - win) / hop + 1 >= 64), so 63 / 64 / 65 are its tile edges too
FRAME_COUNTS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)
WIN_HOP = ((400, 160), (401, 161), (200, 80))
SENTINEL = -12345.0


def _lengths(win, hop):
    """One recording per frame count; some samples past the last frame's window, fewer than a hop."""
    return [win - 1 if F == 0 else win + (F - 1) * hop + (F * 37) % hop for F in FRAME_COUNTS]


@functools.lru_cache(maxsize=None)
def _signal(kind, win, hop):
    rng = np.random.RandomState(len(kind) * 1000 + win)
    out = []
    for n in _lengths(win, hop):
        g = rng.standard_normal(n)
        x = {'noise-20dB': 0.1 * g, 'dc0.5+noise-70dB': 0.5 + 10 ** (-70 / 20) * g, 'dc0.9+noise-60dB': 0.9 + 10 ** (-60 / 20) * g,
             'zeros': np.zeros(n)}[kind].astype(np.float32)
        x.setflags(write=False)
        out.append(x)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _stage_a_reference(kind, win, hop, c):
    """float64 energies of the f32 samples and the float32 restatement's largest error against them, per batch."""
    ref = [ov.frame_db(x, win, hop, c) for x in _signal(kind, win, hop)]
    own = max(np.abs(ov.frame_db(x, win, hop, c, dtype=np.float32).astype(np.float64) - r).max() for x, r in zip(_signal(kind, win, hop), ref)
              if r.size)
    return ref, float(own)


def _frame_db_raw(waves, win, hop, c, lead=7, trail=9, junk=5):
    """vp_vad_frame_db_f32 straight through the binding: the recordings back to back after `junk` foreign samples, the output laid out
    from frame `lead` of a buffer pre-filled with a sentinel.  -> (rc, the whole buffer, frame_offsets)."""
    from ppvector import _native as N
    lib, ctx = N.lib(), N.ctx()
    lens = [len(w) for w in waves]
    frames = [ov.num_frames(n, win, hop) for n in lens]
    wave = torch.from_numpy(np.concatenate([np.full(junk, 1e3, np.float32)] + [np.asarray(w, np.float32) for w in waves])).cuda()
    off = torch.from_numpy((junk + np.concatenate([[0], np.cumsum(lens)])).astype(np.int32)).cuda()
    foff_h = (lead + np.concatenate([[0], np.cumsum(frames)])).astype(np.int32)
    foff = torch.from_numpy(foff_h).cuda()
    e = torch.full((lead + sum(frames) + trail,), SENTINEL, dtype=torch.float32, device='cuda')
    rc = lib.vp_vad_frame_db_f32(ctx, wave.data_ptr(), off.data_ptr(), foff.data_ptr(), len(waves), win, hop, c, e.data_ptr(), N.stream_ptr())
    return rc, e.cpu().numpy(), foff_h


# ------------------------------------------------------------------------------------------------ 1. stage A against float64
@pytest.mark.parametrize('c', [0.0, 0.97])
@pytest.mark.parametrize('win,hop', WIN_HOP)
@pytest.mark.parametrize('kind', ['noise-20dB', 'dc0.5+noise-70dB', 'dc0.9+noise-60dB', 'zeros'])
def test_frame_db_against_float64(kind, win, hop, c):
    """All frame counts as one ragged batch of 13.  Bound: 16 x the float32 restatement's own largest error against float64 on this input
    (the factor covers another summation order; a one-pass variance is off by tenths of a dB on the DC inputs).  Nothing outside
    [frame_offsets[0], frame_offsets[B]) is written; exact zeros give exactly -100; two runs the same bits."""
    from ppvector import _native as N
    waves = _signal(kind, win, hop)
    ref, own = _stage_a_reference(kind, win, hop, c)
    rc, buf, foff = _frame_db_raw(waves, win, hop, c)
    assert rc == N.VP_OK
    assert (buf[:foff[0]] == SENTINEL).all() and (buf[foff[-1]:] == SENTINEL).all() and not (buf[foff[0]:foff[-1]] == SENTINEL).any()
    worst = 0.0
    for b, r in enumerate(ref):
        got = buf[foff[b]:foff[b + 1]]
        assert got.shape == r.shape == (FRAME_COUNTS[b],)
        if r.size:
            worst = max(worst, float(np.abs(got.astype(np.float64) - r).max()))
    print(f'[frame_db {kind} win={win} hop={hop} c={c}] max |GPU - float64| {worst:.3g} dB   float32 restatement {own:.3g} dB   '
          f'bound {16 * own:.3g} dB')
    assert worst <= 16 * own, (worst, own)
    if kind == 'zeros':
        assert (buf[foff[0]:foff[-1]] == -100.0).all()
    assert np.array_equal(_frame_db_raw(waves, win, hop, c)[1], buf)


def test_frame_db_ragged_batch_through_energy_vad():
    """A batch of 5 with an empty recording and one shorter than a window inside it, host arrays and a device tensor mixed; a single
    array returns a single tensor."""
    from ppvector.infer_utils.vad import EnergyVad
    rng = np.random.RandomState(3)
    lens = [5000, 0, 16000, 399, 400 + 160 * 70]
    waves = [(0.05 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    vad = EnergyVad()
    got = vad.frame_db([waves[0], waves[1], torch.from_numpy(waves[2]).cuda(), waves[3], waves[4]])
    assert [g.shape[0] for g in got] == [ov.num_frames(n, 400, 160) for n in lens] == [29, 0, 98, 0, 71]
    for g, w in zip(got, waves):
        r = ov.frame_db(w, 400, 160, 0.97)
        if r.size:
            own = np.abs(ov.frame_db(w, 400, 160, 0.97, dtype=np.float32) - r).max()
            assert np.abs(g.cpu().numpy() - r).max() <= 16 * own
    one = vad.frame_db(waves[2])
    assert isinstance(one, torch.Tensor) and torch.equal(one, got[2])
    assert vad.frame_db(waves[3]).shape == (0,)


def test_frame_db_rejects_what_is_outside_the_contract():
    from ppvector import _native as N
    x = [np.zeros(2000, np.float32), np.zeros(1000, np.float32)]
    assert _frame_db_raw(x, 400, 160, 0.97)[0] == N.VP_OK
    for win, hop, c in ((160, 400, 0.97), (4097, 160, 0.97), (400, 160, 1.0), (400, 160, -0.5), (400, 160, float('nan'))):
        rc, buf, _ = _frame_db_raw(x, win, hop, c)
        assert rc == N.VP_EINVAL and (buf == SENTINEL).all(), (win, hop, c)
    lib, ctx = N.lib(), N.ctx()
    wave = torch.zeros(3000, device='cuda')
    e = torch.full((64,), SENTINEL, device='cuda')

    def call(off, foff, B=2, win=400, hop=160):
        o, f = (torch.tensor(v, dtype=torch.int32, device='cuda') for v in (off, foff))
        return lib.vp_vad_frame_db_f32(ctx, wave.data_ptr(), o.data_ptr(), f.data_ptr(), B, win, hop, 0.97, e.data_ptr(), N.stream_ptr())

    assert call([0, 2000, 3000], [0, 11, 15]) == N.VP_OK
    assert call([0, 2000, 1000], [0, 11, 11]) == N.VP_EINVAL          # decreasing
    assert call([-1, 2000, 3000], [0, 11, 15]) == N.VP_EINVAL
    assert call([0, 2000, 3000], [0, 11, 16]) == N.VP_EINVAL          # not vp_vad_num_frames
    assert call([0, 2000, 3000], [0, 11, 15], B=0) == N.VP_EINVAL
    assert call([0, 2000, 3000], [0, 11, 15], hop=0) == N.VP_EINVAL and call([0, 2000, 3000], [0, 11, 15], win=0, hop=0) == N.VP_EINVAL
    torch.cuda.synchronize()
    assert (e[15:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ 2. stage B on planted energies
DEFAULTS = dict(floor_pct=0.10, peak_pct=0.95, margin_db=6.0, onset=0.5, offset=0.2, min_gap=10, min_speech=5, pad=3)
Q, M, S = -50.0, -40.0, -20.0           # quiet, a mid level between off (-44) and on (-35) when fl = -50 and pk = -20, speech


def _e(*parts):
    return np.concatenate([np.full(n, v, np.float32) for v, n in parts] + [np.zeros(0, np.float32)])


def _regions_raw(energies, cap=None, lead=3, ws_extra=64, **kw):
    """vp_vad_regions_f32 straight through the binding on a ragged batch of planted energies, the workspace filled with 0xFF bytes,
    thr / counts / regions pre-filled with sentinels.  -> (rc, thr (B, 4), counts (B,), regions (B, cap + 1, 2): one row more than cap)."""
    from ppvector import _native as N
    p = dict(DEFAULTS, **kw)
    lib, ctx = N.lib(), N.ctx()
    B = len(energies)
    frames = [len(v) for v in energies]
    cap = (max(frames) + 1) // 2 if cap is None else cap
    e = torch.from_numpy(np.concatenate([np.full(lead, 77.0, np.float32)] + [np.asarray(v, np.float32) for v in energies])).cuda()
    foff = torch.from_numpy((lead + np.concatenate([[0], np.cumsum(frames)])).astype(np.int32)).cuda()
    thr = torch.full((B, 4), SENTINEL, device='cuda')
    counts = torch.full((B,), -7, dtype=torch.int32, device='cuda')
    regions = torch.full((B * cap + 1, 2), -7, dtype=torch.int32, device='cuda')          # (B, cap, 2) and one row past it
    nbytes = lib.vp_vad_workspace_bytes(sum(frames), B)
    assert nbytes == 16 * (sum(frames) // 64 + B + 1)
    ws = torch.full((nbytes + ws_extra,), 0xFF, dtype=torch.uint8, device='cuda')
    rc = lib.vp_vad_regions_f32(ctx, e.data_ptr(), foff.data_ptr(), B, p['floor_pct'], p['peak_pct'], p['margin_db'], p['onset'], p['offset'],
                                p['min_gap'], p['min_speech'], p['pad'], thr.data_ptr(), counts.data_ptr(), regions.data_ptr(), cap,
                                ws.data_ptr(), nbytes, N.stream_ptr())
    torch.cuda.synchronize()
    assert (ws[nbytes:] == 0xFF).all()                                # nothing past the stated workspace
    return rc, thr.cpu().numpy(), counts.cpu().numpy(), regions.cpu().numpy(), cap


def _check(energies, cap=None, **kw):
    """Exact equality of thr, counts and regions with the oracle for every recording of the batch; -> the oracle's regions."""
    from ppvector import _native as N
    p = dict(DEFAULTS, **kw)
    rc, thr, counts, regions, cap = _regions_raw(energies, cap=cap, **kw)
    assert rc == N.VP_OK
    want = []
    for b, v in enumerate(energies):
        t, reg = ov.regions(v, **p)
        want.append(reg)
        assert thr[b].tobytes() == np.asarray(t, np.float32).tobytes(), (b, thr[b], t)
        assert counts[b] == len(reg), (b, counts[b], reg)
        rows = regions[b * cap:b * cap + min(cap, len(reg))]
        assert [tuple(r) for r in rows.tolist()] == reg[:cap], (b, rows.tolist(), reg)
        rest = regions[b * cap + min(cap, len(reg)):(b + 1) * cap]
        assert (rest == -7).all(), (b, 'rows past the count were written')
    assert (regions[len(energies) * cap:] == -7).all()
    return want


def test_regions_hysteresis_and_thresholds_at_the_edge():
    """fl = -50, pk = -20: on = -35, off = -44.  Mid level after speech stays speech, after silence stays silence, at the start is
    silence.  A frame exactly at `on` is speech, nextafter below is not; the same at `off` (with onset = offset = 0: on = off = -44)."""
    raw = dict(min_gap=1, min_speech=1, pad=0)
    want = _check([_e((M, 20), (Q, 30), (S, 20), (M, 15), (Q, 30), (M, 15), (S, 12), (Q, 40))], **raw)
    assert want == [[(50, 85), (130, 142)]]
    below = np.nextafter(np.float32(-44.0), np.float32(-100.0))
    exact = _e((Q, 40), (-44.0, 3), (Q, 10), (below, 3), (Q, 10), (S, 5), (Q, 3))
    _, thr, _, _, _ = _regions_raw([exact], onset=0.0, offset=0.0, **raw)
    assert thr[0].tolist() == [-50.0, -20.0, -44.0, -44.0]
    assert _check([exact], onset=0.0, offset=0.0, **raw) == [[(40, 43), (66, 71)]]
    # off: speech, then exactly -44 (not under off: stays speech), then just under it (silence)
    assert _check([_e((Q, 40), (S, 5), (-44.0, 4), (below, 4), (Q, 20))], **raw) == [[(40, 49)]]
    # on: with onset 0.5 it is -35
    b35 = np.nextafter(np.float32(-35.0), np.float32(-100.0))
    assert _check([_e((Q, 40), (b35, 4), (-35.0, 4), (Q, 20), (S, 10))], **raw) == [[(44, 48), (68, 78)]]


def test_regions_gap_burst_padding_rules():
    g, s = DEFAULTS['min_gap'], DEFAULTS['min_speech']
    assert (g, s) == (10, 5)
    nopad = dict(pad=0)
    want = _check([_e((Q, 30), (S, 20), (Q, g - 1), (S, 20), (Q, g), (S, 20), (Q, g + 1), (S, 20), (Q, 30))], **nopad)
    assert want == [[(30, 79), (89, 109), (120, 140)]]            # the gap of 9 filled, those of 10 and 11 not
    want = _check([_e((Q, 30), (S, s - 1), (Q, 30), (S, s), (Q, 30), (S, s + 1), (Q, 30))], **nopad)
    assert want == [[(64, 69), (99, 105)]]                           # the burst of 4 dropped, those of 5 and 6 kept
    # speech at frame 0 and at frame F - 1; padding clipped at both ends; short silence at either end is not filled
    assert _check([_e((S, 20), (Q, 60), (S, 20))]) == [[(0, 23), (77, 100)]]
    assert _check([_e((Q, 2), (S, 20), (Q, 60), (S, 20), (Q, 1))]) == [[(0, 25), (79, 103)]]
    assert _check([_e((Q, 2), (S, 20), (Q, 60), (S, 20), (Q, 1))], **nopad) == [[(2, 22), (82, 102)]]
    # padding that merges two runs: a gap of min_gap survives the fill, 2 pad >= the gap closes it; one frame more keeps them apart
    assert _check([_e((Q, 30), (S, 20), (Q, 10), (S, 20), (Q, 30))], pad=5) == [[(25, 85)]]
    assert _check([_e((Q, 30), (S, 20), (Q, 11), (S, 20), (Q, 30))], pad=5) == [[(25, 55), (56, 86)]]
    # no clean-up at all
    alt = _e(*([(Q, 3)] + [(S, 1), (Q, 1)] * 20 + [(S, 2)]))
    assert len(_check([alt], min_gap=1, min_speech=1, pad=0)[0]) == 21
    # a large pad swallows the recording
    assert _check([_e((Q, 30), (S, 20), (Q, 30))], pad=10 ** 9) == [[(0, 80)]]


def test_regions_order_statistics():
    """Ranks inside runs of tied values, many frames at exactly -100, the extreme ranks, F = 1, distinct values, negative zero."""
    rng = np.random.RandomState(11)
    many = _e((-100.0, 500), (S, 40), (-100.0, 300), (-30.0, 60), (-100.0, 100))
    _check([many])                                                    # 900 of 1000 frames tie at -100: fl inside the tie, pk = -30
    _check([many], floor_pct=0.0, peak_pct=1.0)
    _check([many], floor_pct=0.9, peak_pct=0.9)
    _check([many], floor_pct=0.899, peak_pct=0.901)                   # either side of the end of the tie
    distinct = (rng.permutation(3001).astype(np.float32) * np.float32(0.0173) - np.float32(60.0))
    for fp, pp in ((0.1, 0.95), (0.0, 1.0), (0.5, 0.5), (0.3333, 0.6667), (1.0, 1.0), (0.0, 0.0)):
        _check([distinct], floor_pct=fp, peak_pct=pp)
    wide = np.concatenate([rng.standard_normal(700) * 30, [0.0, -0.0, 1e-30, -1e-30, 3e38, -3e38]]).astype(np.float32)
    for fp, pp in ((0.1, 0.95), (0.0, 1.0), (0.49, 0.51)):
        rc, thr, _, _, _ = _regions_raw([wide], floor_pct=fp, peak_pct=pp)
        srt = np.sort(wide)
        assert rc == 0 and thr[0, 0] == srt[ov.rank(fp, wide.size)] and thr[0, 1] == srt[ov.rank(pp, wide.size)]
    for v in (S, -100.0, 0.0):
        assert _check([_e((v, 1))], min_gap=1, min_speech=1, pad=0) == [[]]           # F = 1: on = fl + 6 is never reached
    assert _check([_e((S, 2))]) == [[]]


def test_regions_long_recording_across_chunk_edges():
    """12 000 frames.  The kernel works in words of 64 frames, wave-0 steps of 4096 frames and 16 waves x 64 = 1024 frames per sweep; a
    gap, a burst and a mid-level stretch each straddle 1024 k, 4096 k and word edges."""
    F = 12000
    e = np.full(F, Q, np.float32)

    def put(a, b, v):
        e[a:b] = v

    put(100, 1000, S); put(1000, 1020, M); put(1020, 1028, Q); put(1028, 1100, S)          # mid level then a filled gap over 1024
    put(2040, 2052, S)                                                                       # a burst over 2048, kept (12 >= 5)
    put(3070, 3073, S)                                                                       # a burst over 3072, dropped
    put(4000, 4090, S); put(4090, 4102, M); put(4102, 4200, Q); put(4200, 4300, M)           # mid level over 4096 after speech, then after silence
    put(5000, 5120, S); put(5120, 5129, Q); put(5129, 5200, S)                               # a filled gap from a word / 1024 edge
    put(8000, 8192, S); put(8192, 8202, Q); put(8202, 8300, S)                               # a gap of exactly min_gap at 8192: not filled
    put(8189, 8192, S)
    put(11990, 12000, S)                                                                     # speech to the last frame
    put(6100, 6144, S); put(6144, 6208, M); put(6208, 6209, S)                               # a whole word undecided between two speech words
    put(7000, 7040, S); put(7040, 7168 + 64, M)                                              # three undecided words carry speech on
    want = _check([e])[0]
    assert (97, 1103) in want and (2037, 2055) in want and (3997, 4105) in want and (4997, 5203) in want
    assert (7997, 8195) in want and (8199, 8303) in want and (11987, 12000) in want and (6097, 6212) in want and (6997, 7235) in want
    assert not any(a <= 3071 < b for a, b in want) and not any(a <= 4250 < b for a, b in want)
    rc, thr, counts, regions, cap = _regions_raw([e])
    again = _regions_raw([e])
    assert np.array_equal(thr, again[1]) and np.array_equal(counts, again[2]) and np.array_equal(regions, again[3])        # two calls, the same bits
    # the same with every level moved so that word edges fall elsewhere: a recording of 12 000 - 37 frames
    _check([e[37:]])


def test_regions_ragged_batch_cap_and_workspace():
    rng = np.random.RandomState(5)
    a = _e((Q, 30), (S, 20), (Q, 60), (S, 20), (Q, 30), (S, 9), (Q, 31))
    b = np.zeros(0, np.float32)                                      # F = 0: count 0, thresholds 0, nothing else
    c = (rng.standard_normal(4100) * 12 - 45).astype(np.float32)
    d = _e((Q, 64), (S, 64), (Q, 64), (S, 64))
    want = _check([a, b, c, d], min_gap=3, min_speech=2, pad=1)
    assert want[0] == [(29, 51), (109, 131), (159, 170)] and want[1] == [] and want[3] == [(63, 129), (191, 256)] and len(want[2]) > 20
    _check([b])
    _check([b, b, d, b])
    # cap smaller than the count: the first cap rows, the row after them untouched (inside _check), counts true
    from ppvector import _native as N
    rc, thr, counts, regions, cap = _regions_raw([a, c], cap=2, min_gap=3, min_speech=2, pad=1)
    assert rc == N.VP_OK and counts.tolist() == [3, len(want[2])]
    assert regions[:2].tolist() == [list(r) for r in want[0][:2]] and regions[2:4].tolist() == [list(r) for r in want[2][:2]]
    assert (regions[4:] == -7).all()
    _check([a, c], cap=2, min_gap=3, min_speech=2, pad=1)
    rc, _, counts, regions, _ = _regions_raw([a], cap=0)
    assert rc == N.VP_OK and counts.tolist() == [3] and (regions == -7).all()


def test_regions_with_a_nan_and_invalid_arguments():
    from ppvector import _native as N
    e = _e((Q, 100), (S, 50), (Q, 100), (S, 51))
    for pos, val in ((10, np.nan), (120, np.nan), (0, -np.nan), (300, np.inf), (5, -np.inf)):
        v = e.copy()
        v[pos] = val
        rc, thr, counts, regions, cap = _regions_raw([v], min_gap=1, min_speech=1, pad=0)
        assert rc == N.VP_OK and 0 <= counts[0] <= (v.size + 1) // 2
        assert (regions[cap:] == -7).all()
    allnan = np.full(130, np.nan, np.float32)
    rc, _, counts, _, _ = _regions_raw([allnan, e])
    assert rc == N.VP_OK and 0 <= counts[0] <= 65 and counts[1] == 2
    for bad in (dict(onset=0.2, offset=0.3), dict(onset=1.5), dict(offset=-0.1), dict(floor_pct=0.96), dict(floor_pct=-0.1), dict(peak_pct=1.01),
                dict(margin_db=-1.0), dict(margin_db=float('nan')), dict(onset=float('nan')), dict(min_gap=0), dict(min_speech=0), dict(pad=-1),
                ):
        rc, thr, counts, regions, _ = _regions_raw([e], **bad)
        assert rc == N.VP_EINVAL and (thr == SENTINEL).all() and (counts == -7).all() and (regions == -7).all(), bad
    lib, ctx = N.lib(), N.ctx()
    t = torch.zeros(256, device='cuda')
    thr, counts = torch.zeros(8, device='cuda'), torch.zeros(2, dtype=torch.int32, device='cuda')
    out = torch.zeros((2, 8, 2), dtype=torch.int32, device='cuda')
    ws = torch.zeros(1024, dtype=torch.uint8, device='cuda')

    def call(foff, B, nbytes=1024, cap=8):
        f = torch.tensor(foff, dtype=torch.int32, device='cuda')
        return lib.vp_vad_regions_f32(ctx, t.data_ptr(), f.data_ptr(), B, 0.1, 0.95, 6.0, 0.5, 0.2, 1, 1, 0, thr.data_ptr(), counts.data_ptr(),
                                      out.data_ptr(), cap, ws.data_ptr(), nbytes, N.stream_ptr())

    assert call([0, 100, 200], 2) == N.VP_OK
    assert call([0, 100, 50], 2) == N.VP_EINVAL and call([-1, 100, 200], 2) == N.VP_EINVAL and call([0, 100, 200], 0) == N.VP_EINVAL
    assert call([0, 100, 200], 2, cap=-1) == N.VP_EINVAL
    assert call([0, 100, 200], 2, nbytes=16 * (200 // 64 + 3) - 1) == N.VP_EWORKSPACE
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. both stages on a planted waveform
@functools.lru_cache(maxsize=None)
def _planted_wave():
    """About 2 400 frames of white noise at -50 dB on a DC of 0.25, with stretches at -20 dB and at a mid level (-38 dB); every level
    change falls on a multiple of the hop, so a frame holds no, 20 %, 60 % or all of the new level and none sits near a threshold."""
    hop, win, F = 160, 400, 2400
    n = win + (F - 1) * hop + 57
    rng = np.random.RandomState(2024)
    g = rng.standard_normal(n)
    level = np.full(n, 10 ** (-50 / 20))
    for a, b, db in ((100, 400, -20), (400, 460, -38), (520, 560, -38), (700, 712, -20), (760, 1100, -20), (1100, 1108, -50), (1108, 1300, -20),
                     (1500, 1503, -20), (1700, 1800, -38), (1800, 2000, -20), (2000, 2100, -38), (2330, 2400, -20)):
        level[a * hop:(b * hop if b < F else n)] = 10 ** (db / 20)
    x = (0.25 + level * g).astype(np.float32)
    x.setflags(write=False)
    return x


def test_energy_vad_on_a_planted_waveform():
    from ppvector.infer_utils.vad import EnergyVad
    kw = dict(onset=0.5, offset=0.2)
    vad = EnergyVad(**kw)
    x = _planted_wave()
    F = vad.num_frames(x.size)
    assert F == 2400
    # precondition, from the oracle alone: every frame's float64 energy is at least 0.05 dB from both float64 thresholds
    e64 = ov.frame_db(x, vad.win, vad.hop, 0.97)
    srt = np.sort(e64)
    fl, pk = srt[ov.rank(0.10, F)], srt[ov.rank(0.95, F)]
    on, off = fl + max(6.0, 0.5 * (pk - fl)), fl + max(6.0, 0.2 * (pk - fl))
    closest = min(np.abs(e64 - on).min(), np.abs(e64 - off).min())
    e32 = ov.frame_db(x, vad.win, vad.hop, 0.97, dtype=np.float32)
    print(f'[planted waveform] fl {fl:.3f} pk {pk:.3f} on {on:.3f} off {off:.3f}   closest frame {closest:.3g} dB from a threshold   '
          f'float32 restatement max error {np.abs(e32 - e64).max():.3g} dB')
    assert closest >= 0.05
    want = ov.clean(ov.hysteresis(e64, on, off), vad.min_gap, vad.min_run, vad.pad)
    assert len(want) >= 4
    (got, thr), (secs, thr2) = vad.frame_regions(x), vad.regions(torch.from_numpy(np.array(x)).cuda())
    assert [tuple(r) for r in got.tolist()] == want, (got.tolist(), want)
    assert thr == thr2 and abs(thr.floor - fl) < 1e-3 and abs(thr.peak - pk) < 1e-3 and abs(thr.on - on) < 1e-3 and abs(thr.off - off) < 1e-3
    assert secs == [ov.to_seconds(a, b, x.size, vad.win, vad.hop, 16000) for a, b in want]
    assert want[-1][1] == F and secs[-1][1] == x.size / 16000          # the tail no frame covers stays in the last region
    # a list goes through one ragged call and gives the same regions per recording
    both = vad.regions([x, x[:160000]])
    assert both[0] == (secs, thr) and both[1][0] == vad.regions(x[:160000])[0]


# ------------------------------------------------------------------------------------------------ 4. PPVectorPredictor
def _cfg():
    from ppvector.utils.utils import dict_to_object
    return dict_to_object(dict(
        dataset_conf=dict(dataset=dict(min_duration=0.3, max_duration=3, sample_rate=16000, use_dB_normalization=True, target_dB=-20)),
        preprocess_conf=dict(feature_method='Fbank', method_args=dict(sr=16000, n_mels=80)),
        model_conf=dict(model='EcapaTdnn', model_args=dict(embd_dim=192, pooling_type='ASP', channels=[512, 512, 512, 512, 1536]))))


@pytest.fixture(scope='module')
def predictor():
    from oracle import models as om
    from ppvector.predict import PPVectorPredictor
    state = {'0.' + k: v for k, v in om.ecapa_params(80, seed=1000).items()}
    return PPVectorPredictor(_cfg(), model_path=state)


SPEECH = [(0.5, 4.5), (5.5, 9.5), (10.0, 12.0)]                       # the loud stretches of the recording, seconds


@pytest.fixture(scope='module')
def recording():
    """The three stretches of tests/test_gpu_diarization.py's recording (different loudness), with near-silent stretches between them."""
    from oracle import fbank as ofb
    w = ofb.synth_waves(3, 64000, seed=77, lowpass=0.9)
    hush = lambda n, seed: (1e-4 * np.random.RandomState(seed).standard_normal(n)).astype(np.float32)
    return np.concatenate([hush(8000, 1), w[0], hush(16000, 2), 0.3 * w[1], hush(8000, 3), 2.0 * w[2][:32000], hush(8000, 4)]).astype(np.float32)


def test_predictor_with_a_detector(predictor, recording, monkeypatch):
    from ppvector.infer_utils.vad import EnergyVad
    seen = []

    def fixed(embeddings, speaker_num=None):                         # k-means is seeded by the clock: fix the labels, keep the embeddings
        emb = np.asarray(embeddings)
        seen.append(emb)
        return (np.arange(emb.shape[0]) >= emb.shape[0] // 2).astype(np.int64), np.eye(2, emb.shape[1], dtype=np.float32)

    monkeypatch.setattr(predictor.speaker_diarize, 'clustering', fixed)
    predictor.set_vad(EnergyVad())
    regions = predictor.vad(recording.copy())
    print('[predictor.vad]', regions)
    assert len(regions) == 3                                         # one per loud stretch, each reaching no further than the padding
    for (a, b), (sa, sb) in zip(regions, SPEECH):
        assert sa - 0.15 <= a <= sa + 0.03 and sb - 0.03 <= b <= sb + 0.15, (a, b, sa, sb)
    out = predictor.speaker_diarization(recording.copy())
    given = predictor.speaker_diarization(recording.copy(), vad_segments=regions)
    assert out == given and len(out) >= 2
    assert np.array_equal(seen[0], seen[1])                          # the same windows, the same embeddings, bit for bit
    assert all(regions[0][0] - 0.01 <= o['start'] < o['end'] <= regions[-1][1] + 0.01 for o in out)      # postprocess rounds to 10 ms
    # an explicit vad_segments still wins over the detector
    other = [(0.5, 5.0), (6.0, 11.3), (11.5, 11.9)]
    predictor.speaker_diarization(recording.copy(), vad_segments=other)
    assert seen[2].shape[0] == 13 != seen[0].shape[0]
    # without a detector the call raises as it always did
    predictor.set_vad(None)
    with pytest.raises(NotImplementedError, match='vad'):
        predictor.speaker_diarization(recording.copy())
    assert len(seen) == 3
