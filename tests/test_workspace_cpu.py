"""Workspace sizes of the six backbone forwards, pinned (no GPU needed: vp_X_workspace_bytes is host-only and reads the integer fields
of the weight struct and, for ECAPA, whether w_hl / w_ctx are null -- never through a pointer).  The structs are filled by the engine's
own packing of each backbone at its shipped default configuration, from a CPU module (the pointers then name host memory, which is
all the query needs).  A carve that changes a buffer's size, drops or adds a buffer, or reorders across a differently padded one
moves these numbers.

EXPECTED was produced by running `workspace_sizes()` below at commit d054151 (the parent of the change that moved workspace carving
and descriptor construction into csrc/launch.h), with that commit's library and Python packing."""
import ctypes as C

import pytest

SHAPES = ((1, 298), (1, 101), (4, 301), (64, 298))          # (B, T): B = 1, odd T, a BASELINE-sized batch
DTYPES = ('float32', 'bfloat16', 'float32x3')
MODELS = ('EcapaTdnn', 'TDNN', 'CAMPPlus', 'ResNetSE', 'ERes2Net', 'ERes2NetV2', 'Res2Net')

EXPECTED = {
    'EcapaTdnn/float32': (8340480, 2856960, 33644544, 532733952),
    'EcapaTdnn/bfloat16': (5136384, 1771264, 20699136, 327671808),
    'EcapaTdnn/float32x3': (8836352, 3025152, 35648000, 564469760),
    'EcapaTdnn/float32x3/no-split-block0': (8340480, 2856960, 33644544, 532733952),
    'TDNN/float32': (1964544, 641024, 7913472, 125321216),
    'TDNN/bfloat16': (1289728, 420096, 5186560, 82132992),
    'TDNN/float32x3': (1964544, 641024, 7913472, 125321216),
    'CAMPPlus/float32': (7418112, 2529792, 29963264, 474243072),
    'CAMPPlus/bfloat16': (3718144, 1273600, 15005696, 237445120),
    'CAMPPlus/float32x3': (7418112, 2529792, 29963264, 474243072),
    'ResNetSE/float32': (37598208, 12803072, 151869952, 2406260736),
    'ResNetSE/bfloat16': (19279360, 6594304, 77857280, 1233854464),
    'ResNetSE/float32x3': (37598208, 12803072, 151869952, 2406260736),
    'ERes2Net/float32': (58909440, 20088320, 238305280, 3770204160),
    'ERes2Net/bfloat16': (29475328, 10064640, 119234560, 1886412800),
    'ERes2Net/float32x3': (58909440, 20088320, 238305280, 3770204160),
    'ERes2NetV2/float32': (44605440, 15191040, 180060160, 2854748160),
    'ERes2NetV2/bfloat16': (22323456, 7616000, 90112000, 1428684800),
    'ERes2NetV2/float32x3': (44605440, 15191040, 180060160, 2854748160),
    'Res2Net/float32': (1480704, 540672, 6034432, 94740480),
    'Res2Net/bfloat16': (786176, 299776, 3198464, 50270208),
    'Res2Net/float32x3': (1480704, 540672, 6034432, 94740480),
}


def _sizes(lib, eng):
    fn = getattr(lib, 'vp_' + _WS_NAME[type(eng).__name__] + '_workspace_bytes')
    return tuple(int(fn(C.byref(eng.W), B, T)) for B, T in SHAPES)


_WS_NAME = {'EcapaEngine': 'ecapa', 'TdnnEngine': 'tdnn', 'CamppEngine': 'campplus', 'ResNetSEEngine': 'resnetse',
            'Eres2netEngine': 'eres2net', 'Res2NetEngine': 'res2net'}


def workspace_sizes(models=MODELS, dtypes=DTYPES):
    """{'<model>/<engine dtype>[/variant]': bytes at each of SHAPES} for the shipped default configuration of every backbone."""
    import torch
    from ppvector import _native as N
    from ppvector.models import _BUILT
    lib = N.load_library()
    out = {}
    for name in models:
        torch.manual_seed(0)
        m = _BUILT[name](input_size=80).eval()
        for dt in dtypes:
            with torch.no_grad():
                eng = m._engine_cls(m, dt)
            out[f'{name}/{dt}'] = _sizes(lib, eng)
            if name == 'EcapaTdnn' and dt == 'float32x3':
                assert eng.W.block0.w_hl and eng.W.mfa.w_hl and eng.W.asp.w_ctx       # split weights present above ...
                eng.W.block0.w_hl = None                                              # ... and absent: no im2col plane buffer
                out[f'{name}/{dt}/no-split-block0'] = _sizes(lib, eng)
    return out


@pytest.mark.parametrize('name', MODELS)
def test_workspace_bytes_are_pinned(name):
    got = workspace_sizes(models=(name,))
    want = {k: v for k, v in EXPECTED.items() if k.split('/')[0] == name}
    assert set(got) == set(want) and len(want) >= len(DTYPES)
    for k in sorted(want):
        print(k, got[k])
        assert got[k] == want[k], (k, dict(zip(SHAPES, zip(got[k], want[k]))))
        assert all(v > 0 and v % 256 == 0 for v in got[k]), k


def test_split_weights_move_only_the_ecapa_fast_path_buffer():
    """The split-precision engine's extra workspace is ECAPA's im2col plane buffer alone: without block0's split weights it asks for
    what the f32 engine asks for, and no other backbone's size depends on the engine being split-precision."""
    assert EXPECTED['EcapaTdnn/float32x3/no-split-block0'] == EXPECTED['EcapaTdnn/float32']
    for B_T, x3, f32 in zip(SHAPES, EXPECTED['EcapaTdnn/float32x3'], EXPECTED['EcapaTdnn/float32']):
        B, T = B_T
        assert x3 - f32 == (B * T * 416 * 4 + 255) // 256 * 256, B_T           # (B T, roundup(5 x 80, 32) = 416) f32-sized elements
    for name in MODELS[1:]:
        assert EXPECTED[f'{name}/float32x3'] == EXPECTED[f'{name}/float32'], name
