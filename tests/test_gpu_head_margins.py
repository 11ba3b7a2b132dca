"""GPU tests of the cosine head + margin losses at PLANTED target cosines and at the edges of the class / row tiling, against the float64
reference of tests/head_oracle.py (pinned on the CPU by tests/test_head_oracle_cpu.py).  Run with -m gpu on an MI355X.

The margin arithmetic is written once (vp_aam_margin, csrc/head_common.h) and has five users (head_tile_fwd / head_tile_bwd in
csrc/head_tiled.hip, aam_ce_bwd_rows in csrc/head.hip, margin_out / sphere_term in csrc/losses.hip); Python picks by shape.  Every test
goes through the product's objects and asserts which path ran:
  P1  evaluation, class-tiled   SpeakerIdentification.eval() -> AAMLoss           outputs.pred set, no 'logits' key
  P2  training, class-tiled     SpeakerIdentification.train() -> AAMLoss           outputs.pred set (HeadLoss.apply(..)[1].numel() == B)
  P3  training, logits tensor   the same with B > 128, D != 192 or VPMI_HEAD_UNTILED  outputs.pred None (.. numel() == 0), no 'logits' key
  P4  logits-level              somebody read outputs['logits'] first: AamCe (grad) / vp_aam_ce_fwd (no grad); SubCenterLoss,
                                SphereFace2('A'), AMLoss, ARMLoss on planted logits
(a) every regime of head_oracle.REGIMES x m in {0.2, 0.5} x easy x label smoothing {0, 0.1} on the four paths; (b) widths, batch sizes
and class counts at the edges of the tiling (what each shape crosses: head_oracle.P1_EDGES / P2_EDGES / P3_EDGES); (c) predictions,
and exact ties between two bit-identical class columns: the smaller index wins in the DPP row, across the four waves, in the merge
kernel's per-thread tile walk and across its threads; (d) the margin table; (e) the logits-level family; (f) a cosine that rounds above 1.
No entry point refused a P3 shape of (b): all of them run and meet the bounds.

Bounds (the ones tests/test_gpu_losses.py and test_cosine_head_and_aam_at_named_class_counts hold these paths to): loss 2e-5 relative,
row loss 5e-5 of the largest row, gradients 1e-4 rel-L2; logits-level: d logits max-abs 2e-5 of the largest reference entry, SphereFace2
bias gradient 1e-4.  In 'very_high' (cosines 0.97 ... 0.999) f32 arithmetic itself amplifies (d dm / d cos ~ sin m / sin^3): the gradient
bound there is max(bound, 4 x err_f32cpu), err_f32cpu = float32 CPU autograd over the oracle against float64 on the same inputs, both
printed.

Worst measured figures on an MI355X, all cases of a path together (bound in brackets); the engine stays inside the fixed 1e-4 in
'very_high' too, where f32 CPU autograd itself is 1.7e-5 ... 4.8e-5 (d emb) and 2.1e-5 ... 4.5e-5 (d W) from float64:
  path                        loss [2e-5]  row loss [5e-5]  d emb [1e-4]  d W [1e-4]
  P1  all but very_high       9.5e-7       5.6e-6
  P1  very_high               1.0e-6       1.4e-5
  P2  all but very_high       3.4e-7                        6.4e-6        5.4e-6
  P2  very_high               2.9e-7                        3.3e-5        4.4e-5    [bounds 1.4e-4 ... 1.9e-4]
  P3  all but very_high       7.3e-7                        2.0e-6        2.1e-6
  P3  very_high               6.2e-7                        1.9e-5        2.0e-5    [bounds 1.1e-4 ... 1.8e-4]
  P4  AamCe / no-grad         3.4e-7       6.5e-6           2.2e-6        2.2e-6    (very_high: 1.2e-5, 1.5e-5)
  margin table (P1 ... P4)    2.2e-7       2.4e-7           5.5e-6        1.5e-5
  by regime, worst path (d emb / d W): below_th 1.7e-6 / 1.8e-6, just_above_th 4.2e-6 / 3.5e-6, neg 5.5e-7 / 5.4e-7,
  small_pos 4.2e-7 / 4.4e-7, mid 1.4e-6 / 2.2e-6, high 6.4e-6 / 4.5e-6, very_high 3.3e-5 / 4.4e-5; P1 column norms 1.8e-7 [2e-6]
  logits-level                loss [2e-5]  d logits [2e-5]
  SubCenterLoss K = 2, 3      2.4e-7       1.1e-6           (very_high 1.5e-7; f32 CPU autograd itself 6e-7 ... 3.2e-6)
  SphereFace2 'A'             1.7e-7       1.7e-6           bias gradient 1.1e-7 [1e-4]
  AMLoss / ARMLoss            8.0e-8       8.5e-7
Before the radicand was clamped, test_exactly_aligned_embeddings_give_a_finite_loss returned NaN on all seven value paths.
"""
import functools
import itertools
import types

import pytest
import torch

from oracle import losses as ol
from oracle import models as om
from tests import head_oracle as ho

pytestmark = pytest.mark.gpu

LOSS_TOL, ROW_TOL, GRAD_TOL, DLOGIT_TOL, BIAS_TOL = 2e-5, 5e-5, 1e-4, 2e-5, 1e-4
CONFIGS = list(itertools.product(ho.MARGINS, (False, True), (0.0, 0.1)))             # (m, easy, label smoothing)


@pytest.fixture(scope='module')
def N():
    from ppvector import _native as N
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: these tests must run on an MI355X (no CPU fallback exists)')
    N.ctx(0)
    return N


@pytest.fixture(autouse=True)
def _no_table_left_behind(N):
    """The margin table is context-wide state: whatever a test did, the next one starts without one."""
    yield
    N.lib().vp_set_margin_table(N.ctx(0), None)


def _build(name, **kw):
    from ppvector.loss import build_loss
    return build_loss(types.SimpleNamespace(loss_conf={'loss': name, 'loss_args': kw})).cuda()


def _aam(m, scale, easy=False, ls=0.0):
    from ppvector.loss.aamloss import AAMLoss
    return AAMLoss(margin=m, scale=scale, easy_margin=easy, label_smoothing=ls)


def _head(W, train):
    from ppvector.models.fc import SpeakerIdentification
    head = SpeakerIdentification(W.shape[0], W.shape[1])
    head.load_state_dict({'weight': W})
    head = head.cuda()
    return head.train() if train else head.eval()


def _ran(outs, path, B):
    """Which path ran, read off what it leaves behind."""
    from ppvector.models.fc import CosineHeadOutputs
    assert isinstance(outs, CosineHeadOutputs)
    formed = dict.__contains__(outs, 'logits')
    if path in ('P1', 'P2'):
        assert outs.pred is not None and outs.pred.numel() == B and not formed, path
    elif path == 'P3':
        assert outs.pred is None and not formed, path
    else:
        assert outs.pred is None and formed, path


def _eval(emb, W, y, crit, path):
    """Evaluation-mode head -> criterion: (loss, row losses, outputs).  path P4: the logits are formed first."""
    head = _head(W, False)
    with torch.no_grad():
        outs = head(emb.cuda())
        if path == 'P4':
            outs['logits']
        loss = crit(outs, y.cuda())
    _ran(outs, path, emb.shape[0])
    return loss.item(), crit.row_loss.double().cpu(), outs


def _train(emb, W, y, crit, path):
    """Training-mode head -> criterion -> backward: (loss, d emb, d W, outputs)."""
    head = _head(W, True)
    ed = emb.cuda().requires_grad_()
    outs = head(ed)
    if path == 'P4':
        outs['logits']
    loss = crit(outs, y.cuda())
    loss.backward()
    _ran(outs, path, emb.shape[0])
    return loss.item(), ed.grad, head.weight.grad, outs


@functools.lru_cache(maxsize=24)
def _regime_ref(name, m, shape, easy, ls):
    """One regime batch with its float64 reference, shared by the paths that run the same shape; in 'very_high' also what f32
    arithmetic on the CPU loses on it."""
    emb, W, y, cs, scale = ho.regime_batch(name, m, shape)
    ref = ho.reference(emb, W, y, m, scale, easy, ls)
    ref.cosines = ref.dcos = None
    ref.f32 = None
    if name == 'very_high':
        _, de, dw = ho.head_autograd(emb, W, y, m, scale, easy, ls, torch.float32)
        ref.f32 = (ho.rel(de, ref.demb), ho.rel(dw, ref.dW))
    return emb, W, y, scale, ref


@functools.lru_cache(maxsize=4)
def _edge_ref(spec, m=ho.EDGE_M, ls=ho.EDGE_LS):
    emb, W, y = ho.edge_case(spec, m)
    return emb, W, y, ho.reference(emb, W, y, m, ho.EDGE_SCALE, False, ls)


class Figures:
    """Collects (figure, bound) pairs, prints them, and fails at the end with every miss (NaN misses)."""

    def __init__(self, tag):
        self.tag, self.bad, self.worst = tag, [], {}

    def add(self, what, key, value, bound):
        value = float(value)
        w = self.worst.get(key)
        if w is None or not value <= w[0]:
            self.worst[key] = (value, bound)
        if not value < bound:
            self.bad.append(f'{what}: {key} {value:.3e} >= {bound:.3e}')

    def head(self, what, ref, loss, rows=None, demb=None, dW=None, gtol=(GRAD_TOL, GRAD_TOL)):
        self.add(what, 'loss', abs(loss - ref.loss.item()) / abs(ref.loss.item()), LOSS_TOL)
        if rows is not None:
            self.add(what, 'row', ((rows - ref.row_loss).abs().max() / ref.row_loss.abs().max()).item(), ROW_TOL)
        if demb is not None:
            self.add(what, 'demb', ho.rel(demb, ref.demb), gtol[0])
            self.add(what, 'dW', ho.rel(dW, ref.dW), gtol[1])

    def done(self):
        print(f'[{self.tag}] worst ' + '  '.join(f'{k} {v:.2e} [{b:.1e}]' for k, (v, b) in self.worst.items()))
        assert not self.bad, '\n'.join(self.bad)


# ------------------------------------------------------------------------------------------------ (a) regimes on the four paths
# id -> (path, mode, shape); same-shape cases are neighbours, so the float64 references are computed once
A_CASES = {
    'P1': ('P1', 'eval', (48, 192, 1003)), 'P2_B48': ('P2', 'train', (48, 192, 1003)),
    'P4_AamCe': ('P4', 'train', (48, 192, 1003)), 'P4_nograd': ('P4', 'eval', (48, 192, 1003)),
    'P1_D100': ('P1', 'eval', (48, 100, 1003)), 'P3_D100': ('P3', 'train', (48, 100, 1003)),
    'P2_B96': ('P2', 'train', (96, 192, 1003)), 'P3_B130': ('P3', 'train', (130, 192, 1003)),
}


def _gtol(name, ref):
    if name != 'very_high':
        return GRAD_TOL, GRAD_TOL
    return max(GRAD_TOL, 4 * ref.f32[0]), max(GRAD_TOL, 4 * ref.f32[1])


@pytest.mark.parametrize('case', list(A_CASES))
@pytest.mark.parametrize('name', list(ho.REGIMES))
def test_regimes_on_every_path(N, name, case):
    path, mode, shape = A_CASES[case]
    fig = Figures(f'margins {case} {name}')
    for m, easy, ls in CONFIGS:
        emb, W, y, scale, ref = _regime_ref(name, m, shape, easy, ls)
        what = f'm={m} easy={int(easy)} ls={ls}'
        crit = _aam(m, scale, easy, ls)
        if mode == 'eval':
            loss, rows, _ = _eval(emb, W, y, crit, path)
            fig.head(what, ref, loss, rows)
        else:
            loss, de, dw, _ = _train(emb, W, y, crit, path)
            gt = _gtol(name, ref)
            if ref.f32:
                print(f'[margins {case} very_high {what}] f32-CPU d emb {ref.f32[0]:.2e} d W {ref.f32[1]:.2e} -> bounds {gt[0]:.2e} {gt[1]:.2e}; '
                      f'engine d emb {ho.rel(de, ref.demb):.2e} d W {ho.rel(dw, ref.dW):.2e}')
            fig.head(what, ref, loss, None, de, dw, gt)
    fig.done()


@pytest.mark.parametrize('name', ['below_th', 'mid', 'very_high'])
def test_untiled_switch_runs_the_logits_tensor_path(N, monkeypatch, name):
    """VPMI_HEAD_UNTILED sends a shape the class-tiled backward takes (B = 48, D = 192) through vp_cosine_aam_ce_bwd."""
    from ppvector.train.functions import HeadLoss
    monkeypatch.setenv('VPMI_HEAD_UNTILED', '1')
    fig = Figures(f'margins P3_untiled {name}')
    for m, easy, ls in ((0.5, False, 0.1), (0.2, True, 0.0)):
        emb, W, y, scale, ref = _regime_ref(name, m, (48, 192, 1003), easy, ls)
        loss, de, dw, _ = _train(emb, W, y, _aam(m, scale, easy, ls), 'P3')
        fig.head(f'm={m} easy={int(easy)} ls={ls}', ref, loss, None, de, dw, _gtol(name, ref))
        assert HeadLoss.apply(emb.cuda(), W.cuda(), y.cuda(), m, scale, ls, easy)[1].numel() == 0
    monkeypatch.delenv('VPMI_HEAD_UNTILED')
    assert HeadLoss.apply(emb.cuda(), W.cuda(), y.cuda(), m, scale, ls, easy)[1].numel() == 48
    fig.done()


# ------------------------------------------------------------------------------------------------ (b) widths and tile edges, (c) predictions
def _pred_check(outs, ref):
    pred = outs.pred.cpu().long()
    wrong = (pred != ref.argmax).nonzero().reshape(-1).tolist()
    assert not wrong, f'pred differs from the float64 argmax on rows {wrong[:8]}: {pred[wrong[:8]].tolist()} vs {ref.argmax[wrong[:8]].tolist()}'


@pytest.mark.parametrize('case', list(ho.P1_EDGES))
def test_p1_width_batch_and_class_edges(N, case):
    emb, W, y, ref = _edge_ref(ho.P1_EDGES[case])
    fig = Figures(f'margins P1 edge {case}')
    loss, rows, outs = _eval(emb, W, y, _aam(ho.EDGE_M, ho.EDGE_SCALE, False, ho.EDGE_LS), 'P1')
    fig.head(case, ref, loss, rows)
    _pred_check(outs, ref)
    fig.done()


@pytest.mark.parametrize('case', list(ho.P1_FALLBACK))
def test_p1_refused_widths_take_the_logits_path(N, case):
    """D = 102 (not a multiple of 4) and D = 260 (wider than the tile kernel's 256): AAMLoss forms the logits, same bounds; the C
    entry point itself refuses both."""
    emb, W, y, ref = _edge_ref(ho.P1_FALLBACK[case])
    fig = Figures(f'margins P1 fallback {case}')
    head = _head(W, False)
    crit = _aam(ho.EDGE_M, ho.EDGE_SCALE, False, ho.EDGE_LS)
    with torch.no_grad():
        outs = head(emb.cuda())
        loss = crit(outs, y.cuda())
    _ran(outs, 'P4', emb.shape[0])
    fig.head(case, ref, loss.item(), crit.row_loss.double().cpu())
    with pytest.raises(N.VpmiError):
        _tiled_fwd_c(N, emb, W, y)
    fig.done()


def _tiled_fwd_c(N, emb, W, y, m=ho.EDGE_M, scale=ho.EDGE_SCALE, ls=ho.EDGE_LS, easy=False):
    """vp_cosine_aam_tiled_fwd with every optional output asked for: (loss, row losses, lse, cinv, pred)."""
    lib, ctx = N.lib(), N.ctx(0)
    x, Wd, yd = emb.cuda().contiguous(), W.cuda().contiguous(), y.cuda().contiguous()
    B, D = x.shape
    C = Wd.shape[1]
    out = torch.empty(1 + 2 * B, dtype=torch.float32, device='cuda')
    pred = torch.empty(B, dtype=torch.int32, device='cuda')
    cinv = torch.empty(C, dtype=torch.float32, device='cuda')
    ws = torch.empty(max(1, lib.vp_cosine_aam_tiled_workspace_bytes(B, D, C)), dtype=torch.uint8, device='cuda')
    N.check(lib.vp_cosine_aam_tiled_fwd(ctx, x.data_ptr(), Wd.data_ptr(), yd.data_ptr(), B, D, C, float(m), float(scale), float(ls), int(easy),
                                        out.data_ptr(), out[1:].data_ptr(), out[1 + B:].data_ptr(), cinv.data_ptr(), pred.data_ptr(),
                                        ws.data_ptr(), ws.numel(), N.stream_ptr()), ctx)
    torch.cuda.synchronize()
    return out[0].item(), out[1:1 + B].double().cpu(), out[1 + B:].double().cpu(), cinv.double().cpu(), pred.cpu().long()


@pytest.mark.parametrize('case', ['D4', 'D20', 'D100', 'D200', 'D248', 'D256', 'C3', 'C65', 'C2560_B200', 'C16453_B5'])
def test_p1_c_entry_point_with_column_norms(N, case):
    """The C entry point with its cinv by-product (1 / column norms, 2e-6 relative), row losses, log-sum-exps and predictions."""
    emb, W, y, ref = _edge_ref(ho.P1_EDGES[case])
    loss, rows, lse, cinv, pred = _tiled_fwd_c(N, emb, W, y)
    fig = Figures(f'margins P1 C-entry {case}')
    fig.head(case, ref, loss, rows)
    fig.add(case, 'cinv', ((cinv - ref.cinv).abs() / ref.cinv).max().item(), 2e-6)
    fig.add(case, 'lse', ((lse - ref.lse).abs().max() / ref.lse.abs().max()).item(), ROW_TOL)
    assert torch.equal(pred, ref.argmax)
    fig.done()


@pytest.mark.parametrize('case', list(ho.P2_EDGES))
def test_p2_batch_and_class_edges(N, case):
    spec = ho.P2_EDGES[case]
    emb, W, y, ref = _edge_ref(spec)
    if case == 'shared':
        assert y[1] == y[2] == y[3] and y[-1] >= (W.shape[1] // 64) * 64
    if case == 'C5_B64':
        assert torch.bincount(y).max().item() >= 3
    fig = Figures(f'margins P2 edge {case}')
    loss, de, dw, outs = _train(emb, W, y, _aam(ho.EDGE_M, ho.EDGE_SCALE, False, ho.EDGE_LS), 'P2')
    fig.head(case, ref, loss, None, de, dw)
    _pred_check(outs, ref)
    fig.done()


@pytest.mark.parametrize('case', list(ho.P3_EDGES))
def test_p3_batch_width_and_class_edges(N, case):
    from ppvector.train.functions import HeadLoss
    emb, W, y, ref = _edge_ref(ho.P3_EDGES[case])
    fig = Figures(f'margins P3 edge {case}')
    loss, de, dw, _ = _train(emb, W, y, _aam(ho.EDGE_M, ho.EDGE_SCALE, False, ho.EDGE_LS), 'P3')
    fig.head(case, ref, loss, None, de, dw)
    assert HeadLoss.apply(emb.cuda(), W.cuda(), y.cuda(), ho.EDGE_M, ho.EDGE_SCALE, ho.EDGE_LS, False)[1].numel() == 0
    fig.done()


def test_tiled_backward_declines_what_it_does_not_take(N):
    """vp_cosine_aam_tiled_bwd answers VP_EUNSUP (no error text, nothing written) for B > 128 and D != 192: HeadLoss then takes P3."""
    lib, ctx = N.lib(), N.ctx(0)
    for B, D in ((129, 192), (40, 100)):
        C = 65
        emb, W = torch.zeros(B, D, device='cuda'), torch.zeros(D, C, device='cuda')
        y = torch.zeros(B, dtype=torch.int64, device='cuda')
        de, dw = torch.zeros_like(emb), torch.zeros_like(W)
        out = torch.zeros(1, device='cuda')
        pred = torch.zeros(B, dtype=torch.int32, device='cuda')
        ws = torch.empty(lib.vp_cosine_aam_tiled_bwd_workspace_bytes(B, D, C), dtype=torch.uint8, device='cuda')
        rc = lib.vp_cosine_aam_tiled_bwd(ctx, emb.data_ptr(), W.data_ptr(), y.data_ptr(), B, D, C, 0.2, 32.0, 0.0, 0, 1.0, de.data_ptr(),
                                         dw.data_ptr(), out.data_ptr(), pred.data_ptr(), ws.data_ptr(), ws.numel(), N.stream_ptr())
        assert rc == N.VP_EUNSUP


@functools.lru_cache(maxsize=2)
def _tie_case(name):
    emb, W, y = ho.tie_case(name)
    return emb, W, y, ho.reference(emb, W, y, ho.EDGE_M, ho.EDGE_SCALE, False, ho.EDGE_LS)


@pytest.mark.parametrize('path', ['P1', 'P2'])
@pytest.mark.parametrize('name', list(ho.TIES))
def test_tied_cosines_predict_the_smaller_class_index(N, name, path):
    """Two bit-identical class columns hold the maximum of the tie rows (head_oracle.TIES says where they sit in the tiling):
    first index wins.  The other rows predict their label; tests/test_head_oracle_cpu.py holds the gaps."""
    C, j, j2 = ho.TIES[name]
    emb, W, y, ref = _tie_case(name)
    assert torch.equal(W[:, j], W[:, j2])
    crit = _aam(ho.EDGE_M, ho.EDGE_SCALE, False, ho.EDGE_LS)
    fig = Figures(f'margins ties {name} {path}')
    if path == 'P1':
        loss, rows, outs = _eval(emb, W, y, crit, 'P1')
        fig.head(name, ref, loss, rows)
    else:
        loss, de, dw, outs = _train(emb, W, y, crit, 'P2')
        fig.head(name, ref, loss, None, de, dw)
    pred = outs.pred.cpu().long()
    want = y.clone()
    want[list(ho.TIE_ROWS)] = j
    want[len(y) // 2] = ref.argmax[len(y) // 2]                    # the row planted below th: whatever class float64 finds
    assert torch.equal(pred, want), (pred[list(ho.TIE_ROWS)].tolist(), j, j2)
    fig.done()


# ------------------------------------------------------------------------------------------------ (d) margin table
@pytest.mark.parametrize('case', ['P1', 'P2', 'P3', 'P4_AamCe', 'P4_nograd'])
def test_margin_table_overrides_the_launch_scalar(N, case):
    """criterion.margin = 0.35 and `with MarginTable(criterion)`: the kernels read 0.35 from the table when they run -- also for a SECOND
    criterion that passes the scalar 0.1 (the table wins); after __exit__ the scalar counts again."""
    from ppvector.loss._margin import MarginTable
    path = case[:2]
    shape = (130, 192, 1003) if path == 'P3' else (40, 192, 1003)
    emb, W, y = ho.plant(*shape, ho.edge_cosines(shape[0], 0.35), 61)
    ref35 = ho.reference(emb, W, y, 0.35, 32.0, False, 0.05)
    ref10 = ho.reference(emb, W, y, 0.1, 32.0, False, 0.05)
    assert abs(ref35.loss.item() - ref10.loss.item()) > 0.1
    owner, other = _aam(0.2, 32.0, False, 0.05), _aam(0.1, 32.0, False, 0.05)
    owner.margin = 0.35
    fig = Figures(f'margins table {case}')

    def run(crit, ref, what):
        if case in ('P1', 'P4_nograd'):
            loss, rows, _ = _eval(emb, W, y, crit, path)
            fig.head(what, ref, loss, rows)
        else:
            loss, de, dw, _ = _train(emb, W, y, crit, path)
            fig.head(what, ref, loss, None, de, dw)
    with MarginTable(owner, 'cuda'):
        run(owner, ref35, 'owner under its table')
        run(other, ref35, 'scalar 0.1 under the table')
    run(other, ref10, 'scalar 0.1 after __exit__')
    fig.done()


@pytest.mark.parametrize('K', [2, 3])
def test_margin_table_subcenter(N, K):
    from ppvector.loss._margin import MarginTable
    C = 300
    lg, y, _ = ho.plant_logits(ho.LOGIT_B, C, K, ho.edge_cosines(ho.LOGIT_B, 0.35), 62)
    owner = _build('SubCenterLoss', margin=0.2, scale=32, K=K, label_smoothing=0.05)
    other = _build('SubCenterLoss', margin=0.1, scale=32, K=K, label_smoothing=0.05)
    owner.margin = 0.35
    fig = Figures(f'margins table SubCenter K={K}')
    with MarginTable(owner, 'cuda'):
        _logit_case(fig, 'owner under its table', owner, lambda l, t: ol.subcenter_loss(l, t, 0.35, 32.0, False, K, 0.05), lg, y)
        _logit_case(fig, 'scalar 0.1 under the table', other, lambda l, t: ol.subcenter_loss(l, t, 0.35, 32.0, False, K, 0.05), lg, y)
    _logit_case(fig, 'scalar 0.1 after __exit__', other, lambda l, t: ol.subcenter_loss(l, t, 0.1, 32.0, False, K, 0.05), lg, y)
    fig.done()


# ------------------------------------------------------------------------------------------------ (e) logits-level family
def _maxabs(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


def _logit_case(fig, what, crit, fn, lg, y, bias=None, f32_yardstick=False):
    """Eval-time value, then value + d logits (+ d bias) through the criterion, against float64 autograd over fn.  Returns d logits."""
    loss64, dl64, db64 = ho.logits_reference(fn, lg, y, torch.float64, bias)
    tol = DLOGIT_TOL
    if f32_yardstick:
        _, dl32, _ = ho.logits_reference(fn, lg, y, torch.float32, bias)
        err = _maxabs(dl32, dl64)
        tol = max(DLOGIT_TOL, 4 * err)
    with torch.no_grad():
        l0 = crit({'features': None, 'logits': lg.cuda()}, y.cuda())
    fig.add(what, 'loss(eval)', abs(l0.item() - loss64.item()) / abs(loss64.item()), LOSS_TOL)
    ld = lg.cuda().requires_grad_()
    if bias is not None:
        crit.bias.grad = None
    l1 = crit({'features': None, 'logits': ld}, y.cuda())
    l1.backward()
    fig.add(what, 'loss', abs(l1.item() - loss64.item()) / abs(loss64.item()), LOSS_TOL)
    got = _maxabs(ld.grad, dl64)
    if f32_yardstick:
        print(f'[{fig.tag} {what}] f32-CPU d logits {err:.2e} -> bound {tol:.2e}; engine {got:.2e}')
    fig.add(what, 'dlogits', got, tol)
    if bias is not None:
        fig.add(what, 'dbias', abs(crit.bias.grad.item() - db64.item()) / abs(db64.item()), BIAS_TOL)
    return ld.grad


@pytest.mark.parametrize('name', list(ho.REGIMES))
@pytest.mark.parametrize('C', list(ho.LOGIT_CS))
@pytest.mark.parametrize('K', [2, 3])
def test_subcenter_on_planted_logits(N, K, C, name):
    fig = Figures(f'margins SubCenter K={K} C={C} {name}')
    for m, easy, ls in CONFIGS:
        cs, scale = ho.regime(name, m)
        lg, y, win = ho.plant_logits(ho.LOGIT_B, C, K, cs, ho.LOGIT_CS[C])
        crit = _build('SubCenterLoss', margin=m, scale=scale, easy_margin=easy, K=K, label_smoothing=ls)
        g = _logit_case(fig, f'm={m} easy={int(easy)} ls={ls}', crit, lambda l, t: ol.subcenter_loss(l, t, m, scale, easy, K, ls), lg, y,
                        f32_yardstick=name == 'very_high')
        # the gradient lands on the winning sub-centre only; the others get exactly 0
        g3, l3 = g.reshape(ho.LOGIT_B, C, K).cpu(), lg.reshape(ho.LOGIT_B, C, K)
        winner = torch.nn.functional.one_hot(l3.argmax(dim=2), K).bool()
        assert (g3[~winner] == 0).all() and (g3[winner] != 0).all()
        assert torch.equal(l3[torch.arange(ho.LOGIT_B), y].argmax(dim=1), win)
    fig.done()


@pytest.mark.parametrize('name', list(ho.REGIMES))
@pytest.mark.parametrize('C', list(ho.LOGIT_CS))
def test_sphereface2_type_a_on_planted_logits(N, C, name):
    """Type 'A' sends the non-target columns through the square root as well: they range over (-0.98, 0.98)."""
    fig = Figures(f'margins SphereFace2-A C={C} {name}')
    for m in ho.MARGINS:
        cs, scale = ho.regime(name, m)
        lg, y, _ = ho.plant_logits(ho.LOGIT_B, C, 1, cs, ho.LOGIT_CS[C], (-0.98, 0.98))
        crit = _build('SphereFace2', margin=m, scale=scale, lanbuda=0.7, t=3, margin_type='A')
        with torch.no_grad():
            crit.bias.fill_(0.3)
        _logit_case(fig, f'm={m}', crit, lambda l, t, b: ol.sphereface2_loss(l, t, b, m, scale, 0.7, 3, 'A'), lg, y, bias=0.3,
                    f32_yardstick=name == 'very_high')
    fig.done()


@pytest.mark.parametrize('C', list(ho.LOGIT_CS))
@pytest.mark.parametrize('kind', ['AMLoss', 'ARMLoss'])
def test_am_and_arm_on_planted_logits(N, kind, C):
    """ARM: the batch holds rows whose target is the row maximum (every other logit zeroed) and the row minimum (none zeroed)."""
    fn = ol.am_loss if kind == 'AMLoss' else ol.arm_loss
    fig = Figures(f'margins {kind} C={C}')
    lg, y, _ = ho.plant_logits(ho.LOGIT_B, C, 1, ho.ARM_COSINES, ho.LOGIT_CS[C], ho.ARM_RANGE)
    for ls in (0.0, 0.1):
        crit = _build(kind, margin=ho.ARM_M, scale=30, label_smoothing=ls)
        _logit_case(fig, f'ls={ls}', crit, lambda l, t: fn(l, t, ho.ARM_M, 30.0, ls), lg, y)
    fig.done()


# ------------------------------------------------------------------------------------------------ (f) a cosine that rounds above 1
def test_exactly_aligned_embeddings_give_a_finite_loss(N):
    """emb = 1.7 * W[:, :64].T: in f32 the cosine of such a row rounds above 1 on some rows, sqrt(1 - cos^2) is NaN and so was the loss on
    every value path.  The engine clamps the radicand at 0: finite, and within 2e-5 of float64 with the same clamp.  (Gradients at
    cos = 1 are unbounded in exact arithmetic and are not asserted.)"""
    emb, W, y = ho.aligned_case()
    c32 = om.cosine_head(emb, W)[torch.arange(64), y]
    assert ((1.0 - c32 * c32) < 0).any()
    m, scale = 0.2, 32.0
    ref = ho.reference(emb, W, y, m, scale, False, 0.0, clamp=True)
    got = {}
    for easy in (False, True):
        refe = ho.reference(emb, W, y, m, scale, easy, 0.0, clamp=True)
        got[f'P1 easy={int(easy)}'] = (_eval(emb, W, y, _aam(m, scale, easy), 'P1')[0], refe.loss.item())
        got[f'vp_aam_ce_fwd easy={int(easy)}'] = (_eval(emb, W, y, _aam(m, scale, easy), 'P4')[0], refe.loss.item())
    with torch.no_grad():
        lg = _head(W, False)(emb.cuda())['logits']
        lib, ctx = N.lib(), N.ctx(0)
        out = torch.empty(1 + 64, dtype=torch.float32, device='cuda')
        N.check(lib.vp_margin_ce_fwd(ctx, lg.data_ptr(), y.cuda().data_ptr(), 64, lg.shape[1], 1, N.VP_LOSS_AAM, m, scale, 0.0, 0,
                                     out.data_ptr(), out[1:].data_ptr(), N.stream_ptr()), ctx)
        got['vp_margin_ce_fwd AAM'] = (out[0].item(), ref.loss.item())
        sub = _build('SubCenterLoss', margin=m, scale=scale, K=1)
        got['vp_margin_ce_fwd SubCenter'] = (sub({'features': None, 'logits': lg}, y.cuda()).item(), ref.loss.item())
        sf2 = _build('SphereFace2', margin=m, scale=scale, lanbuda=0.7, t=3, margin_type='A')
        c64 = ref.cosines.clamp(-1.0, 1.0)                               # float64 with the radicand clamped at 0
        want = ol.sphereface2_loss(c64, y, torch.zeros((), dtype=torch.float64), m, scale, 0.7, 3, 'A').item()
        got['vp_sphereface2 A'] = (sf2({'features': None, 'logits': lg}, y.cuda()).item(), want)
    for k, (v, want) in got.items():
        print(f'[margins aligned {k}] loss {v:.6e} (float64, clamped: {want:.6e})')
    bad = [k for k, (v, want) in got.items() if not abs(v - want) < 2e-5 * max(1.0, abs(want))]
    assert not bad, (bad, got)
