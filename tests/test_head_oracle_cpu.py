"""Pins tests/head_oracle.py -- the float64 reference and the planted inputs of tests/test_gpu_head_margins.py -- on the CPU: the
planted cosines are what they claim, they keep clear of the margin's branch points, the closed-form gradients equal float64 autograd
over oracle.models, no regime batch is saturated, every row whose prediction the GPU test compares has a clear winner, and the planted
logits have the rows the ARM / sub-centre cases need.  These are CONDITIONS of the GPU tests: if a seed breaks one, change the seed."""
import itertools

import pytest
import torch

from oracle import losses as ol
from oracle import models as om
from tests import head_oracle as ho

REGIME_SHAPE = ho.REGIME_SHAPES[0]
_regime_batch = ho.regime_batch


@pytest.mark.parametrize('m', ho.MARGINS + (ho.EDGE_M, 0.35))
@pytest.mark.parametrize('name', list(ho.REGIMES))
def test_planted_cosines_and_branch_distance(name, m):
    emb, W, y, cs, scale = _regime_batch(name, m)
    ref = ho.reference(emb, W, y, m, scale)
    got = ref.cosines[torch.arange(len(y)), y]
    want = torch.tensor([cs[b % len(cs)] for b in range(len(y))], dtype=torch.float64)
    assert (got - want).abs().max().item() < 1e-6
    assert y[0] == 0 and y[-1] == W.shape[1] - 1
    assert (got - ho.th_of(m)).abs().min().item() >= ho.BRANCH_GAP and got.abs().min().item() >= ho.BRANCH_GAP
    # f32 takes the same side of both branch points
    c32 = om.cosine_head(emb, W)[torch.arange(len(y)), y].double()
    assert torch.equal(c32 > ho.th_of(m), got > ho.th_of(m)) and torch.equal(c32 > 0, got > 0)


@pytest.mark.parametrize('D', [100, 4])
def test_planted_cosines_at_other_widths_and_shared_labels(D):
    emb, W, y = ho.plant(40, D, 65, ho.edge_cosines(40, ho.EDGE_M), 3, labels='shared')
    assert y[1] == y[2] == y[3]
    ref = ho.reference(emb, W, y, ho.EDGE_M, 32.0)
    got = ref.cosines[torch.arange(40), y]
    assert (got - torch.tensor(ho.edge_cosines(40, ho.EDGE_M), dtype=torch.float64)).abs().max().item() < 1e-6
    assert got[20].item() < ho.th_of(ho.EDGE_M) - 2e-3


@pytest.mark.parametrize('m,easy,ls', list(itertools.product(ho.MARGINS, (False, True), (0.0, 0.1))))
def test_closed_form_gradients_equal_float64_autograd(m, easy, ls):
    for name in ho.REGIMES:
        emb, W, y, cs, scale = _regime_batch(name, m, shape=(24, 100, 130), seed=7)
        ref = ho.reference(emb, W, y, m, scale, easy, ls)
        loss, de, dw = ho.head_autograd(emb, W, y, m, scale, easy, ls, torch.float64)
        assert abs(ref.loss.item() - loss.item()) < 1e-12 * max(1.0, abs(loss.item())), name
        assert ho.rel(ref.demb, de) < 1e-10 and ho.rel(ref.dW, dw) < 1e-10, name
        # and d loss / d cosines against autograd over the loss alone
        _, dl, _ = ho.logits_reference(lambda l, t: om.aam_loss(l, t, m, scale, easy, ls), ref.cosines, y)
        assert ho.rel(ref.dcos, dl) < 1e-10, name


@pytest.mark.parametrize('m', ho.MARGINS)
@pytest.mark.parametrize('name', list(ho.REGIMES))
def test_no_regime_batch_is_saturated(name, m):
    for shape, easy, ls in itertools.product(ho.REGIME_SHAPES, (False, True), (0.0, 0.1)):
        emb, W, y, cs, scale = _regime_batch(name, m, shape)
        ref = ho.reference(emb, W, y, m, scale, easy, ls)
        live = ((ref.p_y - ref.q_y).abs() >= 0.05).double().mean().item()
        assert live >= 0.5 and ref.p_y.max().item() <= 0.99, (shape, easy, ls, live, ref.p_y.max().item())


PRED_SHAPES = [('P1', k, v) for k, v in ho.P1_EDGES.items()] + [('P2', k, v) for k, v in ho.P2_EDGES.items()]


@pytest.mark.parametrize('case', PRED_SHAPES, ids=[f'{p}-{k}' for p, k, _ in PRED_SHAPES])
def test_every_prediction_row_has_a_clear_winner(case):
    emb, W, y = ho.edge_case(case[2])
    ref = ho.reference(emb, W, y, ho.EDGE_M, ho.EDGE_SCALE, False, ho.EDGE_LS)
    if W.shape[1] >= 2:
        assert ref.gap.min().item() >= ho.PRED_GAP, ref.gap.min().item()
    got = ref.cosines[torch.arange(len(y)), y]
    assert (got - torch.tensor(ho.edge_cosines(len(y), ho.EDGE_M), dtype=torch.float64)).abs().max().item() < 1e-6


@pytest.mark.parametrize('name', list(ho.TIES))
def test_tie_batches_tie_exactly_where_they_should_and_nowhere_else(name):
    C, j, j2 = ho.TIES[name]
    emb, W, y = ho.tie_case(name)
    assert j < j2 and torch.equal(W[:, j], W[:, j2]) and not {j, j2} & set(y.tolist())
    ref = ho.reference(emb, W, y, ho.EDGE_M, ho.EDGE_SCALE, False, ho.EDGE_LS)
    c = ref.cosines
    for r in range(ho.TIE_B):
        top = torch.topk(c[r], 3)
        if r in ho.TIE_ROWS:                        # the two copies lead (0.6, equal up to the float64 summation order), the rest is far below
            assert set(top[1][:2].tolist()) == {j, j2} and abs(top[0][0].item() - 0.6) < 1e-6 and top[0][2].item() < 0.5
            assert abs(c[r, j].item() - c[r, j2].item()) < 1e-15
        else:
            assert ref.gap[r].item() >= ho.PRED_GAP
            if r != ho.TIE_B // 2:                  # (the row planted below th predicts whatever class float64 finds)
                assert ref.argmax[r] == y[r]


@pytest.mark.parametrize('spec', list(ho.P1_FALLBACK.values()) + list(ho.P3_EDGES.values()), ids=list(ho.P1_FALLBACK) + list(ho.P3_EDGES))
def test_edge_batches_hold_their_planted_values(spec):
    emb, W, y = ho.edge_case(spec)
    ref = ho.reference(emb, W, y, ho.EDGE_M, ho.EDGE_SCALE, False, ho.EDGE_LS)
    got = ref.cosines[torch.arange(len(y)), y]
    assert (got - torch.tensor(ho.edge_cosines(len(y), ho.EDGE_M), dtype=torch.float64)).abs().max().item() < 1e-6
    assert torch.isfinite(ref.demb).all() and torch.isfinite(ref.dW).all()


@pytest.mark.parametrize('K', [1, 2, 3])
@pytest.mark.parametrize('C', list(ho.LOGIT_CS))
def test_planted_logits(C, K):
    for name, m in itertools.product(ho.REGIMES, ho.MARGINS):
        cs, _ = ho.regime(name, m)
        lg, y, win = ho.plant_logits(ho.LOGIT_B, C, K, cs, ho.LOGIT_CS[C], (-0.98, 0.98) if K == 1 else (-0.7, 0.7))
        t = lg.reshape(ho.LOGIT_B, C, K)[torch.arange(ho.LOGIT_B), y]                     # (B, K) the target's sub-centres
        top = torch.topk(t, 2, dim=1)[0] if K > 1 else None
        assert torch.equal(t.argmax(dim=1), win) and set(win.tolist()) == set(range(K))
        if K > 1:
            assert (top[:, 0] - top[:, 1]).min().item() >= 1e-3
        want = torch.tensor([cs[b % len(cs)] for b in range(ho.LOGIT_B)], dtype=torch.float64)
        assert (t.max(dim=1)[0].double() - want).abs().max().item() < 1e-6
        assert y[0] == 0 and y[-1] == C - 1
        assert lg.reshape(ho.LOGIT_B, C, K).max(dim=2)[0].abs().max().item() < 1.0        # every class value stays inside (-1, 1)


@pytest.mark.parametrize('C', list(ho.LOGIT_CS))
def test_arm_logits_have_a_maximal_and_a_minimal_target_and_no_near_tie(C):
    lg, y, _ = ho.plant_logits(ho.LOGIT_B, C, 1, ho.ARM_COSINES, ho.LOGIT_CS[C], ho.ARM_RANGE)
    idx = torch.arange(ho.LOGIT_B)
    z = lg.double().clone()
    z[idx, y] -= ho.ARM_M
    zy = z[idx, y][:, None]
    others = torch.ones_like(z, dtype=torch.bool)
    others[idx, y] = False
    is_max = ((z < zy) | ~others).all(dim=1)
    is_min = ((z > zy) | ~others).all(dim=1)
    assert is_max.any() and is_min.any() and (~is_max & ~is_min).any()
    assert (z - zy).abs()[others].min().item() >= ho.ARM_GAP
    # the oracle's loss sees the zeroing: the all-zeroed rows differ from the AM loss
    assert abs(ol.arm_loss(lg.double(), y, ho.ARM_M, 30.0, 0.0).item() - ol.am_loss(lg.double(), y, ho.ARM_M, 30.0, 0.0).item()) > 1e-3


def test_aligned_rows_round_above_one_in_f32_and_the_clamped_reference_is_finite():
    emb, W, y = ho.aligned_case()
    c32 = om.cosine_head(emb, W)[torch.arange(64), y]
    assert ((1.0 - c32 * c32) < 0).any()
    assert torch.isnan(om.aam_loss(om.cosine_head(emb, W), y, 0.2, 32.0))              # the reference's own arithmetic in f32: NaN
    ref = ho.reference(emb, W, y, 0.2, 32.0, False, 0.0, clamp=True)
    assert torch.isfinite(ref.row_loss).all() and torch.isfinite(ref.loss)
    # the clamp changes nothing where |cos| <= 1
    e2, W2, y2, cs, scale = _regime_batch('very_high', 0.2)
    a, b = ho.reference(e2, W2, y2, 0.2, scale), ho.reference(e2, W2, y2, 0.2, scale, clamp=True)
    assert torch.equal(a.row_loss, b.row_loss) and torch.equal(a.demb, b.demb)
