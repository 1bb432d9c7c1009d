"""not-gpu: ``ctc_loss`` / ``CTCLoss`` — names, entry points, the CPU route, argument checks, route reasons, Meta shapes"""
import os

import pytest
import torch

import ctc_loss_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    if not os.path.exists(t._native.LIB_PATH):
        t.build_native()
    return t


def test_names_and_entry_points(tac):
    assert 'ctc_loss' in tac.functional.__all__ and tac.ctc_loss is tac.functional.ctc_loss and tac.CTCLoss is tac.layers.CTCLoss
    assert tac._composite.ctc_loss is torch.nn.functional.ctc_loss
    header = open(os.path.join(ROOT, 'include', 'tac_amd.h')).read()
    for name in ('tac_ctc_loss_max_targets', 'tac_ctc_loss_max_classes', 'tac_ctc_loss_f32', 'tac_ctc_loss_grad_f32'):
        assert name + '(' in header and name in tac._native.PROTOTYPES
    for op in ('ctc_loss', 'ctc_loss_grad'):
        assert op in tac._ops.cuda_kernels and hasattr(torch.ops.tac_amd, op)
    assert tac._hip.ctc_loss_max_targets() == 1024 and tac._hip.ctc_loss_max_classes() >= 5000


@pytest.mark.parametrize('reduction', ['none', 'mean', 'sum'])
@pytest.mark.parametrize('flat', [False, True])
def test_cpu_route_is_torchs_operator(tac, reduction, flat):
    lp, targets, il, tl = R.make_case(7, 3, 6, 3)
    if flat:
        targets, il, tl = torch.cat([targets[b, :int(tl[b])] for b in range(3)]), tuple(il.tolist()), tuple(tl.tolist())
    x, y = lp.clone().requires_grad_(True), lp.clone().requires_grad_(True)
    got = tac.CTCLoss(reduction=reduction, zero_infinity=True)(x, targets, il, tl)
    want = torch.nn.functional.ctc_loss(y, targets, il, tl, reduction=reduction, zero_infinity=True)
    assert torch.equal(got, want)
    assert torch.equal(torch.autograd.grad(got.sum(), x)[0], torch.autograd.grad(want.sum(), y)[0])
    costs = torch.ops.tac_amd.ctc_loss(x, targets, torch.as_tensor(il), torch.as_tensor(tl), 0, False, 3, True)[0]
    raw = torch.nn.functional.ctc_loss(y, targets, il, tl, reduction='none')
    assert torch.equal(costs, raw)
    assert torch.equal(torch.autograd.grad(costs.sum(), x)[0], torch.autograd.grad(raw.sum(), y)[0])


def test_argument_checks(tac):
    lp, targets, il, tl = R.make_case(7, 3, 6, 3)
    check = tac._ops.ctc_check
    assert check(lp, targets, il, tl, 0)[4:] == (3, True) and check(lp[:, 0], targets[0], il[:1], tl[:1], 0)[4:] == (3, False)
    assert check(lp, targets.flatten(), il, (3, 1, 2), 0)[4] == 3 and check(lp, targets.flatten(), il, tl.to('meta'), 0)[4] == 7
    for bad in [(lp.long(), targets, il, tl, 0), (lp[0, 0], targets, il, tl, 0), (lp, targets.float(), il, tl, 0),
                (lp, targets[:2], il, tl, 0), (lp, targets, il[:2], tl, 0), (lp, targets, il.float(), tl, 0),
                (lp, targets, il, tl, 6), (lp, targets, il, tl, -1), (lp[:0], targets, il, tl, 0)]:
        with pytest.raises(ValueError, match='ctc_loss'):
            check(*bad)
    for fn in (lambda: tac.ctc_loss(lp, targets, il, tl, reduction='batchmean'), lambda: tac.CTCLoss(reduction='batchmean')):
        with pytest.raises(ValueError, match='reduction'):
            fn()


def test_reasons_and_meta_shapes(tac):
    reason = tac._hip.ctc_loss_reason
    lp = torch.zeros((5, 2, 4))
    assert reason(lp, 3) is None and reason(lp.transpose(0, 1), 1023) is None
    assert reason(lp.double(), 3) == 'dtype float64' and reason(lp.half(), 3) == 'dtype float16'
    assert 'a target axis of 1024 + 1' in reason(lp, 1024)
    assert reason(lp[:, :1].expand(5, 2, 4), 3) == 'expanded or non-positive strides'
    assert '%d classes' % (tac._hip.ctc_loss_max_classes() + 1) in reason(torch.zeros((1, 1, tac._hip.ctc_loss_max_classes() + 1)), 3)
    meta = [torch.zeros((5, 2, 4), device='meta'), torch.zeros((2, 3), dtype=torch.int64, device='meta'),
            torch.zeros(2, dtype=torch.int64, device='meta'), torch.zeros(2, dtype=torch.int64, device='meta')]
    for lattice, shape in ((True, (2, 5, 7)), (False, (0,))):
        costs, alphas, betas = torch.ops.tac_amd.ctc_loss(*meta, 0, False, 3, lattice)
        assert costs.shape == (2,) and alphas.shape == shape and betas.shape == shape and alphas.dtype == torch.float32
    grad = torch.ops.tac_amd.ctc_loss_grad(meta[0].transpose(0, 1), *meta[1:], alphas, betas, costs, costs, 0, False, 3)
    assert grad.shape == (2, 5, 4) and grad.device.type == 'meta'
