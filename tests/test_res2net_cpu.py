"""Res2Net (reference ppvector/models/res2net.py) without a GPU: the float64 helper oracle against the reference-generated golden, the
model's construction from the res2net.yml sections, its state-dict names, its refusals, and the C struct layout of vp_res2net_weights."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import res2net_oracle as o2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'res2net_ref_small.npz'))
    return g, json.loads(str(g['configs']))


def _split_kwargs(kw):
    okw = {k: v for k, v in kw.items() if k not in ('input_size', 'embd_dim')}
    return okw


def test_golden_covers_shipped_small_and_f64(golden_dir):
    g, names = _golden(golden_dir)
    cfgs = [json.loads(str(g[f'config__{n}'])) for n in names]
    assert any(c['input_size'] == 80 and c['m_channels'] == 32 and c['scale'] == 2 and c['layers'] == [3, 4, 6, 3] for c in cfgs)
    assert any(c['input_size'] == 64 for c in cfgs)
    assert any(c['scale'] > 2 and c['layers'] == [1, 1, 1, 1] for c in cfgs)     # nums > 1 in 'stage' blocks only: no chaining
    # a 'normal' block (second block of a layer) with nums > 1: the sp + spx[i] chain
    assert any(c['scale'] > 2 and max(c['layers']) >= 2 for c in cfgs)


def test_oracle_reproduces_reference_golden(golden_dir):
    g, names = _golden(golden_dir)
    for n in names:
        kw = json.loads(str(g[f'config__{n}']))
        okw = _split_kwargs(kw)
        p = o2.res2net_params(input_size=kw['input_size'], embd_dim=kw['embd_dim'], seed=int(g[f'param_seed__{n}']), dtype=torch.float64,
                              **okw)
        with torch.no_grad():
            e = o2.res2net_forward(p, torch.from_numpy(g[f'x__{n}']).double(), **okw).numpy()
        ref = g[f'emb_eval__{n}']
        rel = np.linalg.norm(e - ref) / np.linalg.norm(ref)
        assert rel <= 1e-5, (n, rel)


def _res2net_conf():
    from ppvector.utils.utils import dict_to_object
    raw = dict(preprocess_conf=dict(feature_method='Fbank', method_args=dict(sr=16000, n_mels=80)),
               model_conf=dict(model='Res2Net', model_args=dict(embd_dim=192, pooling_type='ASP', m_channels=32),
                               classifier=dict(classifier_type='Cosine', num_speakers=2796, num_blocks=0)),
               loss_conf=dict(loss='AAMLoss', loss_args=dict(margin=0.2, scale=32, easy_margin=False, label_smoothing=0.0)))
    return dict_to_object(raw)


def test_res2net_yml_builds():
    from ppvector.data_utils.featurizer import AudioFeaturizer
    from ppvector.models import build_model
    from ppvector.models.res2net import Res2Net
    configs = _res2net_conf()
    fz = AudioFeaturizer(feature_method=configs.preprocess_conf.feature_method, method_args=configs.preprocess_conf.get('method_args', {}))
    model = build_model(input_size=fz.feature_dim, configs=configs)
    assert isinstance(model, Res2Net) and model.embd_dim == 192
    n = sum(p.numel() for p in model.parameters())
    assert 5.5e6 < n < 5.8e6


@pytest.mark.parametrize('kw', [dict(input_size=80), dict(input_size=64),
                                dict(input_size=80, m_channels=8, layers=[1, 1, 1, 1], scale=4)])
def test_state_dict_matches_reference_names(kw):
    from ppvector.models.res2net import Res2Net
    m = Res2Net(**kw)
    okw = {k: v for k, v in kw.items() if k != 'input_size'}
    p = o2.res2net_params(input_size=kw['input_size'], **okw)
    sd = m.state_dict()
    assert set(sd.keys()) == set(p.keys()), sorted(set(sd.keys()) ^ set(p.keys()))[:10]
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(p[k].shape), k
    for k in ('conv1.weight', 'layer2.0.convs.0.weight', 'layer2.0.bns.0._mean', 'layer2.0.downsample.1._variance',
              'pooling.tdnn.conv.conv.weight', 'bn2.norm.weight', 'linear.weight'):
        assert k in sd, k
    m.load_state_dict(p)
    assert torch.equal(m.state_dict()['layer1.0.conv3.bias'], p['layer1.0.conv3.bias'])


@pytest.mark.parametrize('pt', ['SAP', 'TAP', 'TSP'])
def test_other_pooling_types_refuse(pt):
    from ppvector.models.res2net import Res2Net
    with pytest.raises(NotImplementedError):
        Res2Net(80, pooling_type=pt)


@pytest.mark.parametrize('F', [96, 128, 160])
def test_input_size_mismatching_the_reference_pooling_refuses(F):
    from ppvector.models.res2net import Res2Net, feature_bins
    assert feature_bins(F) != F // 32
    with pytest.raises(ValueError, match='frequency bins'):
        Res2Net(F)


def test_feature_bins_follow_the_reference_shapes():
    from ppvector.models.res2net import feature_bins
    for F in (32, 64, 80, 100, 160):
        x = torch.zeros(1, 1, F, 40)
        x = torch.nn.functional.conv2d(x, torch.zeros(1, 1, 7, 7), stride=3, padding=1)
        x = o2.max_pool(x)
        for _ in range(3):
            x = torch.nn.functional.conv2d(x, torch.zeros(1, 1, 1, 1), stride=2)
        assert feature_bins(F) == x.shape[2], F


def _header_struct_size(name, workdir):
    """sizeof(name) and its field names in offset order as the C++ compiler lays include/vpmi.h out (tests/abi_compiler.py)."""
    from ppvector import _native as N
    from tests import abi_compiler as ac
    fields = [f for f, _ in getattr(N, N.STRUCT_CLASSES[name])._fields_]
    sizes, members, _ = ac.compiler_view({name: fields}, [], workdir)
    return sizes[name], sorted(fields, key=lambda f: members[name, f][0])


def test_struct_sizes_match_header(tmp_path):
    from ppvector import _native as N
    size, names = _header_struct_size('vp_r2n_block', tmp_path)
    assert names == [f[0] for f in N.R2nBlock._fields_]
    assert C.sizeof(N.R2nBlock) == size == (3 + N.VP_MAX_R2N_SCALE) * C.sizeof(N.TdnnLayer) + 5 * 4 + 4
    size, names = _header_struct_size('vp_res2net_weights', tmp_path)
    assert names == [f[0] for f in N.Res2netWeights._fields_]
    assert C.sizeof(N.Res2netWeights) == size


def test_new_entry_points_are_declared_and_exported():
    from ppvector import _native as N
    lib = N.load_library()
    for name in ('vp_res2net_workspace_bytes', 'vp_res2net_fwd', 'vp_res2net_stem_fwd', 'vp_avgpool3x3_fwd', 'vp_avgpool3x3_bwd_f32',
                 'vp_maxpool3x3_fwd_f32', 'vp_maxpool3x3_bwd_f32'):
        assert name in N.EXPORTED_SYMBOLS and hasattr(lib, name), name


def test_workspace_query_needs_no_gpu():
    """vp_res2net_workspace_bytes reads the struct's geometry only; the packing itself happens on the GPU engine."""
    from ppvector import _native as N
    W = N.Res2netWeights()
    assert N.load_library().vp_res2net_workspace_bytes(C.byref(W), 4, 298) == 0        # no blocks: refused
    W.feat_dim, W.m_channels, W.n_blocks = 80, 32, 1
    b = W.blk[0]
    b.conv1.cin, b.conv1.cout, b.width, b.scale, b.stride, b.stage = 32, 32, 16, 2, 1, 1
    b.conv3.cin, b.conv3.cout, b.has_down, b.down.cout = 32, 128, 1, 128
    W.asp.att = 128
    n = N.load_library().vp_res2net_workspace_bytes(C.byref(W), 4, 298)
    assert n >= 2 * 4 * 49 * 13 * 128 * 4        # two activation buffers of the block output at least
