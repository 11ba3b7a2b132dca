"""Parity of the path bench.py TIMES -- not a sibling of it.

bench.py's headline step (BASELINE configs[1]) is `bench.make_infer_step`: waveforms -> Fbank + CMN -> ECAPA-TDNN forward -> cosine
head -> AAM loss, the batch cut into shards that run as concurrent launch sequences on side streams (engine.forward_streams with
the featurizer as each shard's producer), everything replayed from ONE captured HIP graph.  These tests hold exactly that object:
  (a) forward_streams(wav, S, producer=featurizer) is bit-identical to forward(featurizer(wav)) for S = 2, 4, both engines;
  (b) the captured graph, replayed twice with NEW inputs, reproduces the eager single-stream embeddings and loss bit for bit;
  (c) wave -> oracle Fbank -> oracle ECAPA -> all-pairs cosine scores at B = 256 x 3 s (the oracle fed its OWN features, nothing
      from the HIP front end) within north_star's 1e-4, for the bf16 engine the bench runs and for the f32 engine.
Every measured value is printed (run with -s; the log is committed under profiles/)."""
import os

import numpy as np
import pytest
import torch

from oracle import fbank as ofb
from oracle import models as om

pytestmark = pytest.mark.gpu

B, L, T = 256, 48000, 298


@pytest.fixture(scope='module')
def rig():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: these tests must run on an MI355X (no CPU fallback exists)')
    import bench
    dev = torch.device('cuda', 0)
    parts = {dt: bench.build_ecapa(dev, dt) for dt in ('bfloat16',)}
    parts['float32'] = parts['float32x3'] = parts['bfloat16']      # same modules: the engine dtype is chosen per call
    wavs = [torch.from_numpy(bench.synth_waves(B, L, seed=s)).to(dev) for s in (1000, 4321, 777)]
    labels = (torch.arange(B, device=dev) * 7) % bench.N_CLASSES
    return bench, dev, parts, wavs, labels


@pytest.mark.parametrize('dtype', ['bfloat16', 'float32x3', 'float32'])
@pytest.mark.parametrize('streams', [2, 4])
def test_forward_streams_with_producer_is_bit_identical(rig, dtype, streams):
    bench, dev, parts, wavs, labels = rig
    fz, model, head, _, _ = parts[dtype]
    model.eval()
    eng = model.engine(dtype)
    want16 = dtype == 'bfloat16'
    ref = eng.forward(fz(wavs[0], want_bf16=want16))
    for rep in range(2):                               # twice: the shards' workspaces are reused
        emb = eng.forward_streams(wavs[0], streams, producer=lambda w: fz(w, want_bf16=want16))
        torch.cuda.synchronize()
        assert emb.shape == (B, 192)
        d = (emb - ref).abs().max().item()
        print(f'[timed path] forward_streams S={streams} {dtype} rep {rep}: max |emb - single-stream emb| = {d:.1e} (bit-identical: {torch.equal(emb, ref)})')
        assert torch.equal(emb, ref)


@pytest.mark.parametrize('dtype', ['bfloat16', 'float32x3', 'float32'])
def test_captured_step_replays_equal_the_eager_single_stream_step(rig, dtype):
    """bench.make_infer_step(streams=2, graph=True) -- the object run_infer times -- against the plain eager call chain on one
    stream, on inputs the capture never saw."""
    bench, dev, parts, wavs, labels = rig
    static_wav = wavs[0].clone()
    run, info = bench.make_infer_step(dev, dtype, 2, static_wav, labels, graph=True, parts=parts[dtype])
    assert info['graph'], 'HIP graph capture of the bench step failed'
    fz, model, head, crit = info['fz'], info['model'], info['head'], info['crit']
    eng = model.engine(dtype)
    want16 = dtype == 'bfloat16'
    for k in (1, 2, 1):                                 # new inputs, then back again
        static_wav.copy_(wavs[k])
        loss_g = run()
        torch.cuda.synchronize()
        emb_g = info['emb'].clone()
        loss_g = float(loss_g)
        emb_e = eng.forward(fz(wavs[k], want_bf16=want16))
        loss_e = float(crit(head(emb_e), labels))
        d = (emb_g - emb_e).abs().max().item()
        print(f'[timed path] graph replay {dtype} input {k}: loss {loss_g:.6f} vs eager {loss_e:.6f}; max |emb diff| {d:.1e}')
        assert torch.equal(emb_g, emb_e)
        assert loss_g == loss_e


def test_bench_shape_scores_vs_oracle_on_its_own_features(rig):
    """wave -> ORACLE Fbank + CMN -> ORACLE ECAPA (f32, CPU) -> all-pairs cosine scores of 256 utterances, against the timed HIP
    path's embeddings (graph replay, 2 streams, bf16), the split-precision engine's and the f32 engine's.  north_star: scores within 1e-4 of the fp32
    reference."""
    bench, dev, parts, wavs, labels = rig
    fz, model, head, state, head_w = parts['bfloat16']
    w = wavs[1]
    torch.set_num_threads(min(32, len(os.sched_getaffinity(0))))
    feats_ref = ofb.featurize(w.cpu().numpy(), method_args=dict(sr=16000, n_mels=80))
    assert feats_ref.shape == (B, T, 80)
    with torch.no_grad():
        ref = om.ecapa_forward({k: v.detach().cpu().float() for k, v in model.state_dict().items()}, torch.from_numpy(feats_ref)).double()
    rn = ref / ref.norm(dim=1, keepdim=True)
    sref = rn @ rn.t()
    feats_hip = fz(w).cpu().numpy()
    print(f'[timed path] Fbank+CMN at the bench shape: max |HIP - oracle| = {np.abs(feats_hip - feats_ref).max():.3e} (log-mel units)')
    static_wav = w.clone()
    res = {}
    for dt in ('bfloat16', 'float32x3', 'float32'):
        run, info = bench.make_infer_step(dev, dt, 2, static_wav, labels, graph=True, parts=parts[dt])
        run()
        torch.cuda.synchronize()
        e = info['emb'].double().cpu()
        en = e / e.norm(dim=1, keepdim=True)
        res[dt] = ((en @ en.t()) - sref).abs().max().item()
        worst = (1 - (en * rn).sum(1)).max().item()
        print(f'[timed path] wave -> scores, {dt} engine (graph, 2 streams) vs oracle on its OWN features: all-pairs ({B} x {B}) '
              f'max |score - oracle| = {res[dt]:.3e}; worst 1 - cos(emb, oracle) = {worst:.3e}')
    assert res['float32'] < 1e-4, res
    assert res['float32x3'] < 1e-4, res                 # the split-precision step bench.py reports as "parity_engine_x3"
    assert res['bfloat16'] < 1e-4, res                  # (random-init weights: every pair scores ~1; at trained weights bf16 is 2e-3)


def test_concurrent_launch_sequences_stay_bit_identical_under_load(rig):
    """Co-run screen of what bench.py runs (two launch sequences) and of four: 40 forwards each, every embedding compared bit for bit
    with the single-stream result -- at the default schedule (ring GEMMs; the ASP attention TDNN on the 128-column tile round 3 had
    fenced) AND at schedule 0 (every wide layer on the 128-wide kernel: the worst neighbour found, 59 / 60 forwards differed there in
    round 3).  Root cause (round 4): packed-f32 VALU instructions in the VICTIM kernels (se_gate, Fbank, ...) read
    stale registers beside an MFMA-heavy wave; the library is built without them (tests/test_isa_cpu.py)."""
    from ppvector import _native as N
    bench, dev, parts, wavs, labels = rig
    fz, model, head, _, _ = parts['bfloat16']
    model.eval()
    eng = model.engine('bfloat16')
    ref = eng.forward(fz(wavs[2], want_bf16=True)).clone()
    prev = N.lib().vp_conv256_select(-1)
    try:
        for sched in (-1, 0):
            N.lib().vp_conv256_select(sched)
            ref_s = eng.forward(fz(wavs[2], want_bf16=True)).clone()
            bad = {2: 0, 4: 0}
            for _ in range(40):
                for S in (2, 4):
                    e = eng.forward_streams(wavs[2], S, producer=lambda w: fz(w, want_bf16=True))
                    torch.cuda.synchronize()
                    bad[S] += int(not torch.equal(e, ref_s))
            print(f'[timed path] schedule {sched}: 40 forwards per setting, embeddings differing from the single-stream run: {bad}')
            assert bad == {2: 0, 4: 0}, (sched, bad)
            if sched == -1:
                assert torch.equal(ref_s, ref)
    finally:
        N.lib().vp_conv256_select(prev)


def test_featurizer_beside_the_backbone_stays_bit_identical(rig):
    """Fbank on one stream while the ECAPA backbone (schedule 0: 128-wide MFMA kernels, two workgroups per CU with room for a third
    kernel's waves on their SIMDs) runs on another: round 4 measured 83 / 180 featurizer calls differing here when the frame
    kernel still had packed-f32 instructions (tools/stress_fbank.py)."""
    from ppvector import _native as N
    bench, dev, parts, wavs, labels = rig
    fz, model, head, _, _ = parts['bfloat16']
    model.eval()
    eng = model.engine('bfloat16')
    f16 = fz(wavs[1], want_bf16=True)._vp_bf16
    ref = fz(wavs[1][:128], want_bf16=True)
    ref32, ref16 = ref.clone(), ref._vp_bf16.clone()
    prev = N.lib().vp_conv256_select(0)
    try:
        emb_ref = eng.forward(f16[128:].contiguous()).clone()
        torch.cuda.synchronize()
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        bad = [0, 0, 0]
        for _ in range(40):
            with torch.cuda.stream(sb):
                e = eng.forward(f16[128:].contiguous())
            with torch.cuda.stream(sa):
                outs = [fz(wavs[1][:128], want_bf16=True) for _ in range(3)]
            torch.cuda.synchronize()
            bad[0] += sum(int(not torch.equal(o, ref32)) for o in outs)
            bad[1] += sum(int(not torch.equal(o._vp_bf16, ref16)) for o in outs)
            bad[2] += int(not torch.equal(e, emb_ref))
    finally:
        N.lib().vp_conv256_select(prev)
    print(f'[timed path] Fbank beside the backbone: f32 features / bf16 twin / backbone embeddings differing from quiet runs: {bad} of 120 / 120 / 40')
    assert bad == [0, 0, 0], bad


def test_plain_bench_run_dumps_the_timed_step(rig, tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` (no --full): the contract line and nothing of the side measurements,
    and DIR holds the timed step's last loss and embeddings -- bit-identical to the eager single-stream call chain on the same seeded
    waveforms and weights (rank 0's shard, bench.shard_seed(1000, 0))."""
    import json
    import subprocess
    import sys
    bench, dev, parts, wavs, labels = rig
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(bench.__file__), 'bench.py'), '--gpus', '1', '--steps', '7',
                        '--warmup', '2', '--dump-outputs', str(tmp_path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-3000:]
    out = json.loads(lines[0])
    print(f"[timed path] plain bench line: {out['value']} {out['unit']}, {out['ms_per_step']} ms per step")
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in out, k
    assert out['steps'] == 7 and out['warmup'] == 2 and out['dtype'] == 'bf16' and out['ms_per_step'] > 0
    assert not {'roofline', 'cpu_baseline', 'dp_train', 'parity_engine_x3', 'clocks'} & set(out)
    emb_d = np.load(tmp_path / 'embeddings.npy')
    loss_d = np.load(tmp_path / 'loss.npy')
    assert emb_d.dtype == np.float32 and emb_d.shape == (B, 192) and loss_d.shape == ()
    fz, model, head, _, _ = parts['bfloat16']
    model.eval()
    wav = torch.from_numpy(bench.synth_waves(B, L, seed=bench.shard_seed(1000, 0))).to(dev)
    from ppvector.loss.aamloss import AAMLoss
    crit = AAMLoss(margin=0.2, scale=32, easy_margin=False, label_smoothing=0.0)
    emb_e = model.engine('bfloat16').forward(fz(wav, want_bf16=True))
    loss_e = float(crit(head(emb_e), labels))
    emb_e = emb_e.float().cpu().numpy()
    print(f'[timed path] dumped loss {float(loss_d):.6f} vs eager {loss_e:.6f}; max |emb diff| {np.abs(emb_d - emb_e).max():.1e}')
    np.testing.assert_array_equal(emb_d, emb_e)
    assert float(loss_d) == np.float32(loss_e)
