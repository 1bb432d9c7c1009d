"""``pcen`` / ``PCEN`` without a device: the composite and its closed-form gradient against tests/pcen_rules.py in float64, the
argument errors, the registered ops and the public names."""
import numpy as np
import pytest
import torch

import pcen_rules as R
import torchaudio_contrib_amd as tac


def tensors(params, dtype=torch.float64, grad=False):
    return [torch.tensor(v, dtype=dtype).requires_grad_(grad) for v in params]


@pytest.mark.parametrize('per_band', [False, True])
@pytest.mark.parametrize('shape', [(1, 1), (3, 1), (2, 5, 70)])
def test_composite_is_the_definition_in_float64(shape, per_band):
    E = R.signal(shape, 1).astype(np.float64)
    kw = dict(zip(('gain', 'bias', 'power', 'b'), tensors(R.band_params(shape[-2], 2)))) if per_band else dict(R.DEFAULTS)
    kw['eps'] = 1e-6
    got = tac.pcen(torch.from_numpy(E), **kw)
    want = R.pcen(E, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in kw.items()})
    assert got.dtype == torch.float64 and got.shape == E.shape and got.transpose(-1, -2).is_contiguous()
    assert np.all(np.abs(got.numpy() - want) <= 1e-12 * (np.abs(want) + 2.0))
    if not per_band:
        assert torch.equal(tac.PCEN(**kw)(torch.from_numpy(E)), got)


def test_default_b_and_a_constant_input():
    E = torch.full((4, 50), 3.0, dtype=torch.float64)
    tc = 0.4 * 22050 / 512
    b = (np.sqrt(1 + 4 * tc ** 2) - 1) / (2 * tc ** 2)
    assert torch.equal(tac.pcen(E), tac.pcen(E, b=b))
    x = R.signal((4, 50), 3).astype(np.float64)
    assert np.abs(tac.pcen(torch.from_numpy(x)).numpy() - R.pcen(x, 0.98, 2.0, 0.5, b, 1e-6)).max() <= 1e-12
    flat = (3.0 / (1e-6 + 3.0) ** 0.98 + 2.0) ** 0.5 - 2.0 ** 0.5                # M == E
    assert float((tac.pcen(E) - flat).abs().max()) <= 1e-14


def test_gradients_of_all_five_inputs():
    """the closed form of ``_composite.pcen_grad`` (the formulas of csrc/pcen.hip) against float64 autograd of the restatement
    (whose own subtractive bias and power terms, 140 a band and near 1, round at ``2**-53`` each: the absolute ``1e-12``)"""
    E, g, params = R.signal((2, 5, 70), 4), np.random.default_rng(5).standard_normal((2, 5, 70)), R.band_params(5, 6)
    ins = tensors((E,) + params, grad=True)
    out = tac.pcen(ins[0], gain=ins[1], bias=ins[2], power=ins[3], eps=1e-6, b=ins[4])
    got = torch.autograd.grad(out, ins, torch.from_numpy(g))
    for name, a, w, s in zip(('E', 'gain', 'bias', 'power', 'b'), got, R.gradients(E, g, params, 1e-6), R.scales(E, g, params, 1e-6)):
        assert a.shape == w.shape and np.all(np.abs(a.numpy() - w) <= 1e-10 * s + 1e-12), name


@pytest.mark.parametrize('kw', [dict(gain=-1), dict(bias=-1), dict(power=-1), dict(eps=0), dict(b=0), dict(b=1.5), dict(time_constant=0),
                                dict(gain=torch.ones(3)), dict(b=torch.ones(4, 1)), dict(specgram=torch.ones(4))])
def test_argument_errors(kw):
    kw = dict(kw)
    with pytest.raises(ValueError, match='pcen'):
        tac.pcen(kw.pop('specgram', torch.ones(4, 9)), **kw)
    with pytest.raises(TypeError):
        tac.pcen([[1.0]])


def test_registered_ops_and_public_names():
    from torch.library import opcheck
    E = torch.from_numpy(R.signal((2, 5, 9), 7))
    table = torch.stack(tensors(R.band_params(5, 8), torch.float32))
    utils = ('test_schema', 'test_faketensor')
    opcheck(torch.ops.tac_amd.pcen.default, (E, table, 1e-6, 0, True, 15), test_utils=utils)
    opcheck(torch.ops.tac_amd.pcen_grad.default, (torch.rand(2, 5, 9), E, torch.empty(0), table, 1e-6, 0, True, 15), test_utils=utils)
    assert 'pcen' in tac.functional.__all__ and tac.pcen is tac.functional.pcen and tac.PCEN is tac.layers.PCEN
    assert {'pcen', 'pcen_grad'} <= set(tac._ops.cuda_kernels)


def test_trainable_layer_holds_four_parameters():
    layer = tac.PCEN(n_bands=6, trainable=True, gain=0.8, b=0.1)
    assert {n: tuple(p.shape) for n, p in layer.named_parameters()} == dict.fromkeys(('gain', 'bias', 'power', 'b'), (6,))
    assert float(layer.gain[0]) == pytest.approx(0.8) and float(layer.b[3]) == pytest.approx(0.1)
    layer(torch.from_numpy(R.signal((2, 6, 20), 9))).sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in layer.parameters())
    assert not list(tac.PCEN().parameters()) and not tac.PCEN().state_dict()
    with pytest.raises(ValueError, match='n_bands'):
        tac.PCEN(trainable=True)
