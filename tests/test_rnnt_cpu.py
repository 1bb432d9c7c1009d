"""not-gpu: ``rnnt_loss`` / ``RNNTLoss`` — the float64 reference of tests/rnnt_rules.py against closed forms, the CPU route of the op
against that reference, reductions, clamp, the unfused form, argument checks and the fake kernel."""
import math

import pytest
import torch

import rnnt_rules as R


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


def ref_of(shape, blank=-1, fused=True, scale=1.0):
    case = R.make_case(*shape, blank=blank, seed=3, scale=scale)
    return case, R.reference(('cpu', shape, blank, fused, scale), *case, blank=blank, fused=fused)


# ----------------------------------------------------------------------------- 1. the reference itself
def test_reference_single_cell():
    logits = torch.randn((1, 1, 1, 5), generator=torch.Generator().manual_seed(1))
    one, empty = torch.ones(1, dtype=torch.int32), torch.zeros((1, 0), dtype=torch.int32)
    ref = R.Reference(logits, empty, one, torch.zeros(1, dtype=torch.int32), blank=2)
    want = -torch.log_softmax(logits.double(), -1)[0, 0, 0, 2]
    assert abs(float(ref.costs[0] - want)) < 1e-14


@pytest.mark.parametrize('T,U,V', [(1, 0, 3), (4, 3, 5), (6, 1, 2), (2, 5, 7)])
def test_reference_constant_logits(T, U, V):
    """every path has probability V^-(T+U) and there are C(T-1+U, U) of them"""
    logits = torch.full((1, T, U + 1, V), 0.25)
    targets = torch.zeros((1, U), dtype=torch.int32)
    ref = R.Reference(logits, targets, torch.tensor([T], dtype=torch.int32), torch.tensor([U], dtype=torch.int32), blank=V - 1)
    want = (T + U) * math.log(V) - math.log(math.comb(T - 1 + U, U))
    assert abs(float(ref.costs[0]) - want) < 1e-12


@pytest.mark.parametrize('shape', R.SHAPES)
@pytest.mark.parametrize('fused', [True, False])
def test_reference_beta_and_closed_gradient(shape, fused):
    (logits, targets, tl, ul), ref = ref_of(shape, fused=fused, scale=1.0 if fused else 0.3)
    assert float((ref.beta_cost - ref.costs).abs().max()) < 1e-10
    err = float((ref.grad_closed - ref.grad).abs().max())
    print('closed expression against float64 autograd at %r: %.2e' % (shape, err))
    assert err < 1e-10
    assert float(ref.grad[1, int(tl[1]):].abs().max() if int(tl[1]) < shape[1] else 0.0) == 0.0


# ----------------------------------------------------------------------------- 2. the CPU route of the op
@pytest.mark.parametrize('shape', R.SHAPES)
@pytest.mark.parametrize('blank', [-1, 0, 1])
def test_cpu_route_float64(tac, shape, blank):
    if blank >= shape[3] - 1 and blank > 0:
        blank = shape[3] - 2
    (logits, targets, tl, ul), ref = ref_of(shape, blank=blank)
    x = logits.double().requires_grad_(True)
    costs = tac.rnnt_loss(x, targets, tl, ul, blank=blank, reduction='none')
    assert costs.dtype == torch.float64 and tuple(costs.shape) == (shape[0],)
    assert float((costs.detach() - ref.costs).abs().max()) < 1e-10
    weights = torch.linspace(0.5, -1.5, shape[0], dtype=torch.float64)
    (grad,) = torch.autograd.grad((costs * weights).sum(), x)
    assert float((grad - ref.grad * weights[:, None, None, None]).abs().max()) < 1e-10


def test_cpu_route_float32_within_bounds(tac):
    (logits, targets, tl, ul), ref = ref_of(R.SHAPES[1])
    x = logits.clone().requires_grad_(True)
    costs = tac.rnnt_loss(x, targets, tl, ul, reduction='none')
    assert costs.dtype == torch.float32
    R.assert_costs(costs, ref, 'CPU route, float32')
    (grad,) = torch.autograd.grad(costs.sum(), x)
    R.assert_grad(grad, ref, 'CPU route, float32')


def test_reductions_and_mean_scale(tac):
    (logits, targets, tl, ul), ref = ref_of(R.SHAPES[0])
    x = logits.double().requires_grad_(True)
    none = tac.rnnt_loss(x, targets, tl, ul, reduction='none')
    total = tac.rnnt_loss(x, targets, tl, ul, reduction='sum')
    mean = tac.rnnt_loss(x, targets, tl, ul)
    assert total.dim() == 0 and mean.dim() == 0
    assert abs(float((total - none.sum()).detach())) < 1e-12 and abs(float((mean - none.mean()).detach())) < 1e-12
    (g_mean,) = torch.autograd.grad(mean, x)
    assert float((g_mean - ref.grad / x.shape[0]).abs().max()) < 1e-10
    with pytest.raises(ValueError, match='reduction'):
        tac.rnnt_loss(x, targets, tl, ul, reduction='batchmean')
    with pytest.raises(ValueError, match='reduction'):
        tac.RNNTLoss(reduction='each')


def test_clamp_acts_before_the_incoming_gradient(tac):
    (logits, targets, tl, ul), ref = ref_of(R.SHAPES[0])
    clamp = 0.05
    clipped = float((ref.grad.abs() > clamp).double().mean())
    assert 0.0 < clipped < 1.0
    x = logits.double().requires_grad_(True)
    (g,) = torch.autograd.grad(tac.rnnt_loss(x, targets, tl, ul, clamp=clamp), x)         # 'mean': the 1 / B comes after the clip
    assert float((g - ref.grad.clamp(-clamp, clamp) / x.shape[0]).abs().max()) < 1e-10
    assert float(g.abs().max()) <= clamp / x.shape[0] + 1e-15


def test_unfused_takes_log_probabilities(tac):
    shape = R.SHAPES[0]
    (logits, targets, tl, ul), ref = ref_of(shape, fused=False, scale=0.3)
    x = logits.double().requires_grad_(True)
    costs = tac.rnnt_loss(x, targets, tl, ul, reduction='none', fused_log_softmax=False)
    assert float((costs.detach() - ref.costs).abs().max()) < 1e-10
    (g,) = torch.autograd.grad(costs.sum(), x)
    assert float((g - ref.grad).abs().max()) < 1e-10
    # on log-probabilities the two forms agree in value
    lp = torch.log_softmax(logits.double(), -1)
    a = tac.rnnt_loss(lp, targets, tl, ul, reduction='none', fused_log_softmax=False)
    b = tac.rnnt_loss(lp, targets, tl, ul, reduction='none')
    assert float((a - b).abs().max()) < 1e-10


def test_negative_blank_counts_from_the_end(tac):
    logits, targets, tl, ul = R.make_case(3, 7, 4, 6, blank=-2, seed=5)
    a = tac.rnnt_loss(logits.double(), targets, tl, ul, blank=-2, reduction='none')
    b = tac.rnnt_loss(logits.double(), targets, tl, ul, blank=4, reduction='none')
    assert torch.equal(a, b)


def test_layer_equals_functional(tac):
    logits, targets, tl, ul = R.make_case(3, 7, 4, 6, blank=0, seed=6)
    layer = tac.RNNTLoss(blank=0, clamp=0.1, reduction='sum', fused_log_softmax=True)
    assert not list(layer.parameters()) and not layer.state_dict()
    x1, x2 = logits.clone().requires_grad_(True), logits.clone().requires_grad_(True)
    a, b = layer(x1, targets, tl, ul), tac.rnnt_loss(x2, targets, tl, ul, blank=0, clamp=0.1, reduction='sum')
    assert torch.equal(a, b)
    assert torch.equal(torch.autograd.grad(a, x1)[0], torch.autograd.grad(b, x2)[0])
    assert 'rnnt_loss' in tac.functional.__all__ and tac.functional.rnnt_loss is tac.rnnt_loss


def test_double_backward_on_the_host(tac):
    logits, targets, tl, ul = R.make_case(1, 3, 2, 4, seed=7)
    x = logits.double().requires_grad_(True)
    assert torch.autograd.gradgradcheck(lambda z: tac.rnnt_loss(z, targets, tl, ul, reduction='sum'), (x,))


# ----------------------------------------------------------------------------- 3. argument checks
def test_argument_checks(tac):
    logits, targets, tl, ul = R.make_case(3, 7, 4, 6, seed=8)
    ok = (logits, targets, tl, ul)

    def bad(match, **change):
        args = dict(zip(('logits', 'targets', 'logit_lengths', 'target_lengths'), ok))
        kw = {k: change.pop(k) for k in list(change) if k in ('blank',)}
        args.update(change)
        with pytest.raises(ValueError, match=match):
            tac.rnnt_loss(args['logits'], args['targets'], args['logit_lengths'], args['target_lengths'], **kw)

    bad('floating', logits=logits.long())
    bad('int32', targets=targets.long())
    bad('int32', logit_lengths=tl.long())
    bad('int32', target_lengths=ul.float())
    bad('dimension', logits=logits[0])
    bad('dimension', targets=targets[0])
    bad('dimension', logit_lengths=tl[:, None])
    bad('dimension', target_lengths=ul[0])
    bad('targets of shape', targets=targets[:, :3].contiguous())
    bad('targets of shape', targets=targets[:2])
    bad('targets of shape', logits=logits[:, :, :4])
    bad('lengths', logit_lengths=tl[:2])
    bad('lengths', target_lengths=torch.cat([ul, ul]))
    bad('blank', blank=6)
    bad('blank', blank=-7)
    # torchaudio's two checks that read the lengths: made for CPU tensors
    bad('longest logit length', logit_lengths=torch.tensor([6, 5, 3], dtype=torch.int32))
    bad('longest logit length', logit_lengths=torch.tensor([8, 5, 3], dtype=torch.int32))
    bad('longest target length', target_lengths=torch.tensor([3, 2, 0], dtype=torch.int32))
    bad('longest target length', target_lengths=torch.tensor([5, 2, 0], dtype=torch.int32))
    assert tac.rnnt_loss(*ok).dim() == 0


def test_empty_batch(tac):
    out = tac.rnnt_loss(torch.zeros((0, 4, 3, 5)), torch.zeros((0, 2), dtype=torch.int32), torch.zeros(0, dtype=torch.int32),
                        torch.zeros(0, dtype=torch.int32), reduction='none')
    assert tuple(out.shape) == (0,)


# ----------------------------------------------------------------------------- 4. the fake kernels
@pytest.mark.parametrize('dtype,work', [(torch.float32, torch.float32), (torch.float64, torch.float64), (torch.float16, torch.float32)])
def test_fake_kernels(tac, dtype, work):
    from torch._subclasses.fake_tensor import FakeTensorMode
    B, T, U, V = 3, 7, 4, 6
    with FakeTensorMode():
        logits = torch.empty((B, T, U + 1, V), dtype=dtype)
        targets = torch.empty((B, U), dtype=torch.int32)
        tl, ul = torch.empty(B, dtype=torch.int32), torch.empty(B, dtype=torch.int32)
        costs, alphas, betas, denoms = torch.ops.tac_amd.rnnt_loss(logits, targets, tl, ul, V - 1, -1.0, True)
        assert tuple(costs.shape) == (B,) and costs.dtype == dtype
        for t in (alphas, betas, denoms):
            assert tuple(t.shape) == (B, T, U + 1) and t.dtype == work
        grad = torch.ops.tac_amd.rnnt_loss_grad(logits, targets, tl, ul, alphas, betas, denoms, costs, costs, V - 1, -1.0, True)
        assert tuple(grad.shape) == (B, T, U + 1, V) and grad.dtype == dtype and grad.is_contiguous()


def test_real_outputs_match_the_fake_ones(tac):
    logits, targets, tl, ul = R.make_case(3, 7, 4, 6, seed=9)
    for dtype, work in ((torch.float32, torch.float32), (torch.float64, torch.float64), (torch.float16, torch.float32)):
        costs, alphas, betas, denoms = torch.ops.tac_amd.rnnt_loss(logits.to(dtype), targets, tl, ul, 5, -1.0, True)
        assert costs.dtype == dtype and alphas.dtype == betas.dtype == denoms.dtype == work
        assert tuple(alphas.shape) == (3, 7, 5)
        grad = torch.ops.tac_amd.rnnt_loss_grad(logits.to(dtype), targets, tl, ul, alphas, betas, denoms, costs, torch.ones_like(costs),
                                                5, -1.0, True)
        assert grad.dtype == dtype and tuple(grad.shape) == (3, 7, 5, 6)
