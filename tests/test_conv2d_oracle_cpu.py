"""The precision-aware float64 reference of the 2-D conv path (tests/conv2d_oracle.py) checked on its own, without a GPU: mode 'f32' is
torch autograd of the plain graph, the distance of the 'amp' and 'x3' references from it is pinned (a broken `terms` moves it), and the
inputs of the GPU unit tests keep every pre-activation away from the clamp edges."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv2d_oracle as co

PLAIN_SEED = 3
UNIT_KEYS = ('y', 'dx', 'dW', 'dgamma', 'dbeta')


def _plain(case, terms=None):
    """forward / dgrad / wgrad of one case in every mode, optionally with another `terms`."""
    x, w, dz = co.conv_inputs(case, PLAIN_SEED)
    g = co.geom_of(case)
    keep = co.terms
    if terms is not None:
        co.terms = terms
    try:
        return {m: (co.conv2d_fwd(x, w, g, m), co.conv2d_dgrad(dz, w, x.shape, g, m), co.conv2d_wgrad(x, dz, w.shape, g, m)) for m in co.MODES}
    finally:
        co.terms = keep


@pytest.mark.parametrize('case', list(co.CASES))
def test_f32_mode_is_plain_autograd(case):
    """Mode 'f32' of the three conv references, and of the whole unit through Conv2dMode, against torch autograd of F.conv2d in float64."""
    x, w, dz = co.conv_inputs(case, PLAIN_SEED)
    g = co.geom_of(case)
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = F.conv2d(xr, wr, None, **g)
    y.backward(dz)
    B, T, Fq, Cin, Cout, k, st, sf, dil, pad_t, pad_f, To, Fo = co.dims(case)
    assert y.shape == (B, Cout, Fo, To)
    for got, ref in ((co.conv2d_fwd(x, w, g, 'f32'), y.detach()), (co.conv2d_dgrad(dz, w, x.shape, g, 'f32'), xr.grad),
                     (co.conv2d_wgrad(x, dz, w.shape, g, 'f32'), wr.grad)):
        assert got.shape == ref.shape and co.rel(got, ref) < 1e-14
    act = 'hardtanh' if case == 'B' else 'relu'
    inp = co.unit_inputs(case, PLAIN_SEED, act)
    leaves = {k_: v.clone().requires_grad_() for k_, v in inp.items() if k_ != 'dy'}
    yu, _ = co.unit_forward(leaves['x'], leaves['w'], leaves['bias'], leaves['gamma'], leaves['beta'], g, 'f32', act,
                            conv=lambda a, b, geom, mode: F.conv2d(a, b, None, **geom))
    yu.backward(inp['dy'])
    ref = co.unit_reference(case, 'f32', PLAIN_SEED, act)
    for name, got in (('y', yu.detach()), ('dx', leaves['x'].grad), ('dW', leaves['w'].grad), ('dgamma', leaves['gamma'].grad),
                      ('dbeta', leaves['beta'].grad)):
        assert co.rel(got, ref[name]) < 1e-14, name


def test_terms_split_is_pack_hl32s():
    """'x3' carries an operand as pack_hl32 stores it: hi = bf16(v), lo = bf16(v - hi); 'amp' keeps hi alone."""
    from ppvector.models.utils import pack_hl32
    g = torch.Generator().manual_seed(1)
    a = torch.randn(5, 64, generator=g)
    planes = pack_hl32(a).view(torch.bfloat16).reshape(5, 2, 64).double()          # per 32-channel group [32 hi | 32 lo]
    hi, lo = planes[:, :, :32].reshape(5, 64), planes[:, :, 32:].reshape(5, 64)
    b = torch.ones(1, dtype=torch.float64)
    (ah, _), (ah2, _), (al, _) = co.terms(a.double(), b, 'x3')
    assert torch.equal(ah, hi) and torch.equal(ah2, hi) and torch.equal(al, lo)
    assert torch.equal(co.terms(a.double(), b, 'amp')[0][0], hi)
    assert [len(co.terms(a.double(), b, m)) for m in co.MODES] == [1, 1, 3]


@pytest.mark.parametrize('case', list(co.CASES))
def test_plain_conv_gaps(case):
    """rel-L2 of the 'amp' / 'x3' references from the unrounded one, forward, dgrad and wgrad.  bf16 rounding is ~1.65e-3 rms relative per
    operand, two independent operands give ~2.3e-3 (measured 2.28e-3 ... 2.68e-3 over the cases); split precision drops lo*lo and
    rounds each lo, ~(1.65e-3)^2 x sqrt(3) = 4.5e-6 (measured 3.6e-6 ... 4.6e-6).  The forward's largest 'x3' error on outputs of
    magnitude <= 5 stays under 3e-5 (measured <= 2.4e-5), which is what the GPU bound of 5e-5 leaves room for."""
    r = _plain(case)
    for a, x3, f in zip(r['amp'], r['x3'], r['f32']):
        assert 1.9e-3 < co.rel(a, f) < 2.9e-3, co.rel(a, f)
        assert 3e-6 < co.rel(x3, f) < 6e-6, co.rel(x3, f)
    assert (r['x3'][0] - r['f32'][0]).abs().max().item() < 3e-5


@pytest.mark.parametrize('case', ['A', 'C', 'H'])
def test_gap_ranges_notice_a_broken_terms(case):
    """The pinned ranges are tight enough to see the two easy mistakes: 'amp' that rounds one operand only falls below its range, 'x3'
    without its lo terms is a bf16 pass (three orders above its range)."""
    def broken(a, b, mode):
        if mode == 'amp':
            return [(co.bf(a), b)]
        if mode == 'x3':
            return [(co.bf(a), co.bf(b))]
        return [(a, b)]
    r = _plain(case, broken)
    for a, x3, f in zip(r['amp'], r['x3'], r['f32']):
        assert co.rel(a, f) < 1.9e-3
        assert co.rel(x3, f) > 1e-3


@pytest.mark.parametrize('case', list(co.UNIT_CASES))
def test_unit_inputs_keep_clear_of_the_clamp_edges(case):
    """Every (case, seed) of the GPU unit tests: no pre-activation of the unrounded, the amp or the x3 reference within
    EDGE_MARGIN of 0 (or 20), and for Hardtanh both clamps active on more than 5 % of the elements.  A condition on the inputs, checked on the reference alone."""
    act, seed = co.UNIT_CASES[case]
    for mode in co.MODES:
        r = co.unit_reference(case, mode, seed, act)
        assert r['edge_margin'] >= co.EDGE_MARGIN, (mode, r['edge_margin'])
        assert r['lo'] > 0.05
        if act == 'hardtanh':
            assert r['hi'] > 0.05


@pytest.mark.parametrize('case', list(co.UNIT_CASES))
def test_unit_gaps(case):
    """The BatchNorm + clamp unit: rounding the conv's operands to bf16 moves y by 1.5e-3 ... 2.1e-3 and the gradients by 2.7e-3 ... 5.4e-2
    (dz now carries the forward's rounding through BatchNorm's backward, and the Hardtanh case's gamma x 14 amplifies it); split
    precision stays within 8e-6 of the unrounded unit everywhere.  dbeta = sum of the masked dy does not see the conv at all unless a mask
    element differs: it is identical in 'x3' and differs in 'amp' only through the mask."""
    act, seed = co.UNIT_CASES[case]
    r = {m: co.unit_reference(case, m, seed, act) for m in co.MODES}
    gap = {m: {k: co.rel(r[m][k], r['f32'][k]) for k in UNIT_KEYS} for m in ('amp', 'x3')}
    print(case, act, gap)
    assert 1.3e-3 < gap['amp']['y'] < 2.5e-3
    for k in ('dx', 'dW', 'dgamma', 'dbeta'):
        assert 2e-3 < gap['amp'][k] < 8e-2, (k, gap['amp'][k])
    for k in ('y', 'dx', 'dW', 'dgamma'):
        assert 2e-6 < gap['x3'][k] < 1e-5, (k, gap['x3'][k])
    assert gap['x3']['dbeta'] == 0.0
