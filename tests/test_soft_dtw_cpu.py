"""``soft_dtw`` / ``SoftDTW`` without a GPU: the composite route against the float64 reference of tests/soft_dtw_rules.py, the closed
forms against float64 autograd, the divergence, the public names, the argument errors and the limits."""
import numpy as np
import pytest
import torch

import soft_dtw_rules as R
import torchaudio_contrib_amd as tac


def weights_for(B):
    return 0.5 - 0.7 * torch.arange(B, dtype=torch.float32)


@pytest.mark.parametrize('shape,lengths', [((2, 1, 1, 1), None), ((3, 5, 7, 3), None), ((3, 9, 6, 4), ([9, 1, 5], [6, 6, 2]))])
def test_composite_against_reference(shape, lengths):
    x, y = R.make_case(*shape)
    xl, yl = lengths or (None, None)
    w = weights_for(shape[0])
    ref = R.reference((shape, 1.0), x, y, 1.0, xl, yl, w)
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    value, E = tac.soft_dtw(xg, yg, 1.0, xl, yl, return_alignment=True)
    gx, gy = torch.autograd.grad(value, (xg, yg), w)
    assert value.dtype == torch.float32 and E.dtype == torch.float32 and not E.requires_grad
    what = '(B, N, M, D) = %r' % (shape,)
    R.assert_within(value, ref.value, ref.value_bound, what + ' value')
    R.assert_within(E, ref.E, ref.E_bound, what + ' alignment')
    R.assert_within(gx, ref.gx, ref.gx_bound, what + ' grad_x'), R.assert_within(gy, ref.gy, ref.gy_bound, what + ' grad_y')


def test_closed_form_is_the_autograd_gradient():
    x, y = R.make_case(1, 6, 4, 3)
    ref = R.reference(('autograd', 0.7), x, y, 0.7)
    xd, yd = x[0].double().requires_grad_(True), y[0].double().requires_grad_(True)
    delta = ((xd[:, None] - yd[None]) ** 2).sum(-1)
    inf = torch.tensor(float('inf'), dtype=torch.float64)
    rows = {(-1, -1): torch.zeros((), dtype=torch.float64)}
    for i in range(6):
        for j in range(4):
            prev = torch.stack([rows.get((i - 1, j), inf), rows.get((i, j - 1), inf), rows.get((i - 1, j - 1), inf)])
            rows[(i, j)] = delta[i, j] - 0.7 * torch.logsumexp(-prev / 0.7, 0)
    gx, gy = torch.autograd.grad(rows[(5, 3)], (xd, yd))
    assert abs(float(rows[(5, 3)].detach()) - ref.value[0]) < 1e-12
    assert np.abs(gx.numpy() - ref.gx[0]).max() < 1e-12 and np.abs(gy.numpy() - ref.gy[0]).max() < 1e-12


def test_divergence_reductions_and_layer():
    x, y = R.make_case(2, 6, 5, 3)
    assert torch.equal(tac.soft_dtw(x, x, 0.5, normalize=True), torch.zeros(2))
    assert torch.equal(tac.soft_dtw(x, y, 0.5, normalize=True), tac.soft_dtw(y, x, 0.5, normalize=True))
    values = tac.soft_dtw(x, y, 0.5)
    assert torch.equal(tac.soft_dtw(x[0], y[0], 0.5), values[0])
    assert torch.equal(tac.soft_dtw(x, y, 0.5, reduction='sum'), values.sum())
    layer = tac.SoftDTW(gamma=0.5)
    assert torch.equal(layer(x, y), values.mean()) and not layer.state_dict()
    assert 'soft_dtw' in tac.functional.__all__ and tac.functional.soft_dtw is tac.soft_dtw and tac.layers.SoftDTW is tac.SoftDTW
    with pytest.raises(RuntimeError, match='double backward'):
        xg = x.clone().requires_grad_(True)
        torch.autograd.grad(tac.soft_dtw(xg, y).sum(), xg, create_graph=True)


@pytest.mark.parametrize('kw', [dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=float('nan')), dict(gamma=float('inf')),
                                dict(reduction='max'), dict(y=torch.zeros(2, 5, 4)), dict(y=torch.zeros(3, 5, 3))])
def test_value_errors(kw):
    args = dict(x=torch.zeros(2, 6, 3), y=torch.zeros(2, 5, 3))
    args.update(kw)
    with pytest.raises(ValueError):
        tac.soft_dtw(**args)


def test_limits():
    lib = tac._native.lib()
    assert lib.tac_soft_dtw_max_len() >= 4096 and lib.tac_soft_dtw_max_dim() >= 256 and lib.tac_abi_version() == 5
    assert tac._hip.soft_dtw_max_len() == lib.tac_soft_dtw_max_len() == lib.tac_soft_dtw_lanes() * 4
    lanes = lib.tac_soft_dtw_lanes()
    assert [lib.tac_soft_dtw_rows_per_lane(n) for n in (1, lanes, lanes + 1, 2 * lanes, 2 * lanes + 1, 4 * lanes)] == [1, 1, 2, 2, 4, 4]
