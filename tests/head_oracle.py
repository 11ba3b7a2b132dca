"""Oracle (CPU, float64) of the cosine classifier + AAM-softmax loss, and the inputs that put its margin arithmetic to work.
Test helper, not a test module; imports nothing of the engine.

Random embeddings against random class weights give target cosines within about +-0.25 of zero at D = 192: the hard-margin branch
cos <= cos(pi - m) never runs and the derivative term cos * sin m / sin stays below 0.05 cos m.  `plant` builds embeddings whose
TARGET cosine is a chosen value instead (emb_b = n_b (c_b w_hat + sqrt(1 - c_b^2) u_b), built in float64, rounded to f32), and
`REGIMES` names the values: both sides of th = cos(pi - m), both sides of zero, and what a trained model has (0.6 ... 0.999).  One
batch holds one regime, so a whole-tensor rel-L2 speaks about that regime alone.  The scale falls with the cosine: at scale 32 a
target cosine above ~0.8 saturates the softmax (p_y -> 1, p_y - q_y cancels in any f32 implementation) and the gradient would say
nothing about d margin / d cos.

`reference` is the closed form in float64 on the f32-rounded operands (tests/test_head_oracle_cpu.py pins its gradients on float64
autograd over oracle.models); `logits_reference` is float64 autograd over a loss of oracle.losses / oracle.models on formed logits.
"""
import math
import types

import numpy as np
import torch

from oracle import models as om


def th_of(m):
    return math.cos(math.pi - m)


# regime -> (planted target cosines as a function of th = cos(pi - m), scale)
REGIMES = {
    'below_th': (lambda th: (-0.999, -0.99, th - 0.003), 32.0),
    'just_above_th': (lambda th: (th + 0.003, th + 0.02), 32.0),
    'neg': (lambda th: (-0.6, -0.2, -0.003), 32.0),
    'small_pos': (lambda th: (0.003, 0.1, 0.3), 32.0),
    'mid': (lambda th: (0.45, 0.6), 32.0),
    'high': (lambda th: (0.8, 0.9), 12.0),
    'very_high': (lambda th: (0.97, 0.99, 0.999), 8.0),
}
MARGINS = (0.2, 0.5)
BRANCH_GAP = 1e-3            # every planted cosine keeps this far from th and from 0 (the f32 cosine error is ~1e-7)
PRED_GAP = 1e-4              # float64 top-2 cosine gap of every row whose prediction is compared


def regime(name, m):
    """(cosines, scale) of a regime at margin m."""
    f, scale = REGIMES[name]
    return tuple(f(th_of(m))), scale


# (B, D, C) of the regime batches -> seed.  The seeds are the first at which no row of any regime, margin, easy flag or label smoothing
# has p_y > 0.99 ('mid' at cosine 0.6, scale 32, m = 0.2 sits at 0.98 ... 0.99: about one seed in ten keeps every row below).
REGIME_SEEDS = {(48, 192, 1003): 4, (48, 100, 1003): 1, (96, 192, 1003): 1, (130, 192, 1003): 12}
REGIME_SHAPES = tuple(REGIME_SEEDS)


def regime_batch(name, m, shape=REGIME_SHAPES[0], seed=None):
    """emb, W, labels, cosines, scale: one batch that holds one regime."""
    cs, scale = regime(name, m)
    B, D, C = shape
    return plant(B, D, C, cs, REGIME_SEEDS[shape] if seed is None else seed) + (cs, scale)


def edge_cosines(B, m):
    """The batch of the width / tile-edge cases: the 'mid' regime, and one row below th (row B // 2) when there are two rows or more."""
    cs = [(0.45, 0.6)[b % 2] for b in range(B)]
    if B >= 2:
        cs[B // 2] = th_of(m) - 0.003
    return cs


def plant(B, D, C, cosines, seed, labels=None):
    """f32 emb (B, D), f32 W (D, C), int64 labels (B,): row b has cosine cosines[b % len(cosines)] with the column of its label.
    labels: None (random; labels[0] = 0, labels[-1] = C - 1), 'shared' (the same, and rows 1, 2, 3 share one label) or an explicit array."""
    rng = np.random.RandomState(seed)
    W = rng.standard_normal((D, C)).astype(np.float32)
    if labels is None or isinstance(labels, str):
        y = rng.randint(0, C, size=B)
        if labels == 'shared':
            assert B >= 5
            y[2] = y[3] = y[1]
        y[0] = 0
        y[-1] = C - 1
    else:
        y = np.asarray(labels, dtype=np.int64)
        assert y.shape == (B,)
    Wd = W.astype(np.float64)
    w_hat = (Wd[:, y] / np.linalg.norm(Wd[:, y], axis=0)).T                    # (B, D)
    u = rng.standard_normal((B, D))
    u -= (u * w_hat).sum(1, keepdims=True) * w_hat
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    c = np.array([cosines[b % len(cosines)] for b in range(B)], dtype=np.float64)
    n = rng.uniform(0.5, 4.5, size=B)
    emb = n[:, None] * (c[:, None] * w_hat + np.sqrt(1.0 - c * c)[:, None] * u)
    return torch.from_numpy(emb.astype(np.float32)), torch.from_numpy(W), torch.from_numpy(y.astype(np.int64))


def plant_logits(B, C, K, cosines, seed, other_range=(-0.7, 0.7)):
    """f32 logits (B, C * K) (column c * K + k = sub-centre k of class c), int64 labels, winning sub-centre per row.  Non-target
    entries are uniform in other_range; the target's sub-centre b % K holds cosines[b % len(cosines)], its other sub-centres lie
    2e-3 ... 5.2e-2 below (they only enter a max, so they may pass -1)."""
    rng = np.random.RandomState(seed)
    lg = rng.uniform(other_range[0], other_range[1], size=(B, C, K))
    y = rng.randint(0, C, size=B)
    y[0] = 0
    y[-1] = C - 1
    win = np.arange(B) % K
    for b in range(B):
        v = cosines[b % len(cosines)]
        lg[b, y[b], :] = v - 2e-3 - rng.uniform(0.0, 0.05, size=K)
        lg[b, y[b], win[b]] = v
    return torch.from_numpy(lg.reshape(B, C * K).astype(np.float32)), torch.from_numpy(y.astype(np.int64)), torch.from_numpy(win)


def margin_of(ct, margin, easy, clamp=False):
    """AAM margin on target cosines ct (float64): (margined value, d margined / d cos)."""
    rad = 1.0 - ct * ct
    if clamp:
        rad = rad.clamp(min=0.0)
    sine = torch.sqrt(rad)
    cos_m, sin_m, th = math.cos(margin), math.sin(margin), th_of(margin)
    phi = ct * cos_m - sine * sin_m
    use = ct > 0 if easy else ct > th
    other = ct if easy else ct - (1.0 + th)
    return torch.where(use, phi, other), torch.where(use, cos_m + ct * sin_m / sine, torch.ones_like(ct))


def loss_of_cosines(cos, labels, margin, scale, easy=False, ls=0.0, clamp=False):
    """The loss half of `reference` on a float64 cosine matrix: row losses, log-sum-exps, p_y, q_y, mean loss and d loss / d cos."""
    B, C = cos.shape
    idx = torch.arange(B)
    ct = cos[idx, labels]
    tgt, dm = margin_of(ct, margin, easy, clamp)
    out = cos.clone()
    out[idx, labels] = tgt
    out = out * scale
    lse = torch.logsumexp(out, dim=1)
    p = torch.exp(out - lse[:, None])
    q = torch.full_like(p, ls / C)
    q[idx, labels] += 1.0 - ls
    row_loss = (1.0 - ls) * (lse - out[idx, labels]) + ls * (lse - out.mean(dim=1))
    dcos = (p - q) * (scale / B)
    dcos[idx, labels] *= dm
    return types.SimpleNamespace(row_loss=row_loss, lse=lse, loss=row_loss.mean(), dcos=dcos, p_y=p[idx, labels], q_y=q[idx, labels])


def reference(emb, W, labels, margin, scale, easy=False, ls=0.0, clamp=False):
    """Cosine head + AAM loss in float64 on the operands as given (f32-rounded).  Fields: cosines (B, C), row_loss, lse, loss, demb,
    dW, dcos (d loss / d cosines), argmax (first index), gap (top-2 cosine gap), p_y, q_y, cinv (1 / column norms).  Gradients are the
    closed form.  clamp: the radicand 1 - cos^2 is clamped at 0 (what the engine does when an f32 cosine rounds above 1)."""
    e, w, y = emb.double(), W.double(), labels.long()
    rn = e.norm(dim=1, keepdim=True).clamp(min=1e-12)
    cn = w.norm(dim=0, keepdim=True).clamp(min=1e-12)
    xn, wn = e / rn, w / cn
    cos = xn @ wn
    r = loss_of_cosines(cos, y, margin, scale, easy, ls, clamp)
    dxn, dwn = r.dcos @ wn.t(), xn.t() @ r.dcos
    r.demb = (dxn - xn * (xn * dxn).sum(1, keepdim=True)) / rn
    r.dW = (dwn - wn * (wn * dwn).sum(0, keepdim=True)) / cn
    r.cosines = cos
    r.argmax = torch.from_numpy(np.argmax(cos.numpy(), axis=1))                # numpy: the first index of the maximum
    if cos.shape[1] >= 2:
        top = torch.topk(cos, 2, dim=1)[0]
        r.gap = top[:, 0] - top[:, 1]
    else:
        r.gap = torch.full((cos.shape[0],), float('inf'), dtype=torch.float64)
    r.cinv = (1.0 / cn).reshape(-1)
    return r


def rel(a, b):
    """rel-L2 of a against the reference b, in float64 on the CPU."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-300)).item()


def head_autograd(emb, W, labels, margin, scale, easy, ls, dtype):
    """(loss, d emb, d W) by autograd over oracle.models in `dtype` -- float64: the independent check of `reference`; float32: what
    plain f32 arithmetic loses on these inputs (the yardstick of the 'very_high' bounds)."""
    e, w = emb.detach().clone().to(dtype).requires_grad_(), W.detach().clone().to(dtype).requires_grad_()
    loss = om.aam_loss(om.cosine_head(e, w), labels, margin, scale, easy, ls)
    loss.backward()
    return loss.detach(), e.grad, w.grad


def logits_reference(fn, logits, labels, dtype=torch.float64, bias=None):
    """(loss, d logits, d bias or None) by autograd in `dtype`; fn(logits, labels[, bias]) is a loss of oracle.losses / oracle.models."""
    lg = logits.detach().clone().to(dtype).requires_grad_()
    b = None if bias is None else torch.full((), float(bias), dtype=dtype, requires_grad=True)
    loss = fn(lg, labels) if b is None else fn(lg, labels, b)
    loss.backward()
    return loss.detach(), lg.grad, None if b is None else b.grad


# ---------------------------------------------------------------------------------------------- the shapes of the GPU tests
# (tests/test_gpu_head_margins.py runs them; tests/test_head_oracle_cpu.py checks the conditions they rest on)
EDGE_M, EDGE_LS, EDGE_SCALE = 0.3, 0.05, 32.0
# id -> (B, D, C, labels mode, seed).  P1 = evaluation, class-tiled; P2 = training, class-tiled; P3 = training, logits tensor.
P1_EDGES = {f'D{D}': (33, D, 130, None, 100 + D) for D in (4, 20, 100, 200, 248, 256)}
P1_EDGES.update({f'B{B}': (B, 192, 127, None, 200 + B) for B in (1, 31, 32, 33, 64, 65, 200)})
P1_EDGES.update({f'C{C}': (48, 192, C, None, 300 + C) for C in (3, 63, 64, 65, 1003)})
P1_EDGES.update({'C2560_B200': (200, 192, 2560, None, 11),            # 40 tiles: ysplit = 5 over 7 row blocks, two grid rows do two blocks each
                 'C12352_B70': (70, 192, 12352, None, 12),            # 193 tiles: ysplit = 1, three row blocks in one workgroup
                 'C16453_B5': (5, 192, 64 * 257 + 5, None, 13)})      # 258 tiles: the merge kernel's per-thread loop takes a second tile
P1_FALLBACK = {f'D{D}': (33, D, 130, None, 100 + D) for D in (102, 260)}             # not % 4 / wider than 256: the logits path
P2_EDGES = {f'B{B}': (B, 192, 1003, None, 400 + B) for B in (1, 63, 64, 65, 127, 128)}
P2_EDGES.update({'C5_B64': (64, 192, 5, None, 21),                    # 64 rows on 5 classes: every dW column sums several rows
                 'C64': (48, 192, 64, None, 22), 'C65': (48, 192, 65, None, 23),
                 'C19207': (70, 192, 64 * 300 + 7, None, 24),         # 301 tiles on 256 workgroups: the backward's tile loop runs twice
                 'shared': (40, 192, 1003, 'shared', 25)})            # three rows on one label, and a label in the last, partial tile
P3_EDGES = {f'B{B}_D{D}': (B, D, 1003, None, 500 + B + D) for B, D in ((129, 192), (256, 192), (40, 100), (40, 256), (7, 64))}
P3_EDGES.update({'C5': (40, 100, 5, None, 31), 'C65': (40, 100, 65, None, 32)})


def edge_case(spec, m=EDGE_M):
    B, D, C, mode, seed = spec
    return plant(B, D, C, edge_cosines(B, m), seed, labels=mode)


# (c) exact ties: id -> (C, smaller column, larger column); the two columns are bit-identical and hold the maximum of TIE_ROWS
TIES = {
    'same_wave': (1003, 3, 9),                                  # one DPP row of 16 classes
    'two_waves': (1003, 3, 40),                                 # waves 0 and 2 of tile 0
    'two_tiles': (4600, 64 * 5 + 7, 64 * 70 + 2),               # merge threads 5 and 70
    'same_merge_thread': (64 * 300, 64 * 3 + 7, 64 * 259 + 2),  # tiles 3 and 259: both walked by merge thread 3
    'thread_order': (64 * 300, 64 * 5 + 7, 64 * 259 + 2),       # tile 259 sits in merge thread 3, ahead of tile 5's thread 5
}
TIE_ROWS = (0, 7, 33, 39)
TIE_B = 40


def tie_case(name):
    """emb, W, labels: the tie rows are planted at cosine 0.6 on column j and labelled elsewhere, column j2 is a bit-for-bit copy of
    column j; the other rows are an edge batch on their own labels."""
    C, j, j2 = TIES[name]
    y = torch.tensor([(100 + 13 * b) % C for b in range(TIE_B)])
    assert j not in y.tolist() and j2 not in y.tolist()
    planted = y.clone()
    planted[list(TIE_ROWS)] = j
    cs = edge_cosines(TIE_B, EDGE_M)
    for r in TIE_ROWS:
        cs[r] = 0.6
    emb, W, _ = plant(TIE_B, 192, C, cs, 50 + len(name), labels=planted.numpy())
    W[:, j2] = W[:, j]
    return emb, W, y


# the logits-level family (e): B = 37; id -> (C, seed)
LOGIT_B = 37
LOGIT_CS = {300: 41, 1003: 45}
ARM_COSINES = (0.95, -0.95, 0.1, 0.3, -0.2)          # with other_range (-0.6, 0.6) and m = 0.25: rows whose target is the row maximum / minimum
ARM_M, ARM_RANGE = 0.25, (-0.6, 0.6)
ARM_GAP = 1e-5                                       # no entry this close to the target's (cos - m): the zeroing decision is the same in f32

# (f): W = randn(192, 1003), emb = 1.7 * W[:, :64].T: exactly aligned rows, whose f32 cosine rounds above 1 on some
ALIGNED_SEED = 0


def aligned_case():
    g = torch.Generator().manual_seed(ALIGNED_SEED)
    W = torch.randn(192, 1003, generator=g)
    emb = (1.7 * W[:, :64].t()).contiguous()
    return emb, W, torch.arange(64)
