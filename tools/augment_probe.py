"""Cost of the noise / reverb augmentation calls (ppvector/data_utils/wave_batch.py noise_perturb, reverb_perturb) beside the
training step they feed.  B = 64 utterances of 6 s, each selected with probability 0.5 (seeded), noise files of 10 s, impulse
responses of 1 s (and, second line, 10 s utterances with 3 s responses -- the long end of the range); HIP events around the whole
Python call (pointer tables, output allocation and workspace included: what the trainer pays), 5 warm-up calls, median of 30.
The training step (TDNN and ECAPA-TDNN, f32 engine, 3 s features, forward + backward + Adam: code this change does not touch)
is timed the same way.  Usage: python tools/augment_probe.py [B]"""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'voiceprintrecognition-paddlepaddle_amd'))
import torch  # noqa: E402
from oracle import models as om  # noqa: E402
from ppvector.data_utils.wave_batch import noise_perturb, reverb_perturb  # noqa: E402
from ppvector.loss.aamloss import AAMLoss  # noqa: E402
from ppvector.models.ecapa_tdnn import EcapaTdnn  # noqa: E402
from ppvector.models.fc import SpeakerIdentification  # noqa: E402
from ppvector.models.tdnn import TDNN  # noqa: E402
from ppvector.optimizer.adam import Adam  # noqa: E402
from ppvector.train.step import TrainStep  # noqa: E402

SR = 16000


def timed(fn, warm=5, reps=30):
    """Median milliseconds of fn() between HIP events on the current stream."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def augment_times(B, utt_s, rir_s, noise_s=10.0, prob=0.5, seed=7):
    rng = random.Random(seed)
    g = torch.Generator(device='cuda').manual_seed(seed)
    waves = [0.1 * torch.randn(int(utt_s * SR), device='cuda', generator=g) for _ in range(B)]
    noises = [0.05 * torch.randn(int(noise_s * SR), device='cuda', generator=g) if rng.random() < prob else None for _ in range(B)]
    rirs = []
    for _ in range(B):
        if rng.random() < prob:
            h = torch.randn(int(rir_s * SR), device='cuda', generator=g) * torch.exp(-torch.arange(int(rir_s * SR), device='cuda') / (0.15 * rir_s * SR))
            rirs.append(h / h.double().pow(2).sum().sqrt().float())
        else:
            rirs.append(None)
    snrs = [rng.uniform(10, 50) for _ in range(B)]
    starts = [rng.randrange(0, int((noise_s - utt_s) * SR) + 1) if noise_s >= utt_s else 0 for _ in range(B)]
    t_noise = timed(lambda: noise_perturb(waves, noises, snrs, starts))
    t_reverb = timed(lambda: reverb_perturb(waves, rirs))
    return t_noise, t_reverb, sum(z is not None for z in noises), sum(h is not None for h in rirs)


def step_time(cls, params, B):
    m = cls(80)
    m.load_state_dict(params)
    model = torch.nn.Sequential(m, SpeakerIdentification(192, 2796)).cuda()
    step = TrainStep(model, AAMLoss(), Adam(model.parameters(), learning_rate=1e-4, weight_decay=1e-6))
    x = torch.randn(B, 298, 80, device='cuda') * 3
    y = torch.randint(0, 2796, (B,), device='cuda')
    return timed(lambda: step(x, y), warm=3, reps=10)


if __name__ == '__main__':
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    rows = []
    for utt_s, rir_s in ((6.0, 1.0), (10.0, 3.0)):
        tn, tr, kn, kr = augment_times(B, utt_s, rir_s)
        rows.append((tn, tr))
        print(f'B={B} utterances {utt_s:g} s, RIR {rir_s:g} s, p=0.5: noise_perturb {tn:.3f} ms ({kn} selected)  '
              f'reverb_perturb {tr:.3f} ms ({kr} selected)  together {tn + tr:.3f} ms', flush=True)
    for name, cls, params in (('TDNN', TDNN, om.tdnn_params(80)), ('EcapaTdnn', EcapaTdnn, om.ecapa_params(80))):
        ms = step_time(cls, params, B)
        print(f'{name} training step f32 B={B}: {ms:.2f} ms; the two augmentation calls (6 s / 1 s) are {100 * sum(rows[0]) / ms:.1f} % of it',
              flush=True)
