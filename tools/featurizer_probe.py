"""Cost of AudioFeaturizer.forward_ragged on a ragged batch, beside the training step it feeds.  B = 64 utterances of 2-3 s drawn
at a fixed seed, rows padded to the longest; the README's mel arguments (sr 16000, n_fft 1024, hop_length 320, win_length 1024,
n_mels 64, f_min 50) for MelSpectrogram, LogMelSpectrogram and MFCC, and Fbank (n_mels 80) for scale; the lengths are passed as
the GPU tensor the trainer holds.  HIP events around the whole Python call (length check, output allocation, workspace: what the
trainer pays), 5 warm-up calls, median of 30 -- the protocol of tools/augment_probe.py.  The TDNN training step (f32 engine,
3 s features, forward + backward + Adam) is timed the same way.  The tool uses only forward_ragged's public signature, so it
runs unchanged on a commit where the mel family still loops over the batch.  Usage: python tools/featurizer_probe.py [B]"""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'voiceprintrecognition-paddlepaddle_amd'))
import torch  # noqa: E402
from oracle import models as om  # noqa: E402
from ppvector.data_utils.featurizer import AudioFeaturizer  # noqa: E402
from ppvector.loss.aamloss import AAMLoss  # noqa: E402
from ppvector.models.fc import SpeakerIdentification  # noqa: E402
from ppvector.models.tdnn import TDNN  # noqa: E402
from ppvector.optimizer.adam import Adam  # noqa: E402
from ppvector.train.step import TrainStep  # noqa: E402

SR = 16000
MEL = dict(sr=SR, n_fft=1024, hop_length=320, win_length=1024, n_mels=64, f_min=50.0)


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


def step_time(B):
    m = TDNN(80)
    m.load_state_dict(om.tdnn_params(80))
    model = torch.nn.Sequential(m, SpeakerIdentification(192, 2796)).cuda()
    step = TrainStep(model, AAMLoss(), Adam(model.parameters(), learning_rate=1e-4, weight_decay=1e-6))
    x = torch.randn(B, 298, 80, device='cuda') * 3
    y = torch.randint(0, 2796, (B,), device='cuda')
    return timed(lambda: step(x, y), warm=3, reps=10)


if __name__ == '__main__':
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    rng = random.Random(7)
    lens = [rng.randint(2 * SR, 3 * SR) for _ in range(B)]
    g = torch.Generator(device='cuda').manual_seed(7)
    wav = 0.1 * torch.randn(B, max(lens), device='cuda', generator=g)
    n = torch.tensor(lens, dtype=torch.int32, device='cuda')
    wav *= (torch.arange(max(lens), device='cuda')[None, :] < n[:, None])             # zeros past each utterance, as assemble_waves leaves them
    print(f'B={B} utterances of {min(lens) / SR:.2f}-{max(lens) / SR:.2f} s (seed 7), rows of {max(lens)} samples', flush=True)
    times = {}
    for method, args in (('MelSpectrogram', MEL), ('LogMelSpectrogram', MEL), ('MFCC', dict(MEL, n_mfcc=40)),
                         ('Fbank', dict(sr=SR, n_mels=80))):
        fz = AudioFeaturizer(method, args)
        times[method] = timed(lambda: fz.forward_ragged(wav, n))
        print(f'forward_ragged {method}: {times[method]:.3f} ms', flush=True)
    ms = step_time(B)
    print(f'TDNN training step f32 B={B}: {ms:.2f} ms; forward_ragged MelSpectrogram is {100 * times["MelSpectrogram"] / ms:.1f} % of it',
          flush=True)
