"""Not gpu: ``sosfilt`` / ``tf2sos`` / ``filtfilt`` on CPU tensors (``_composite.sosfilt``: ``_composite.lfilter`` section by section
with a float64 intermediate), the section design, argument errors, gradients, tracing, the layer — and the stage-composed bound
itself, which a float64 emulation of the kernel's tile scan has to stay far inside.  References and bounds: tests/sos_rules.py."""
import inspect

import numpy as np
import pytest
import torch

import lfilter_rules as LR
import sos_rules as R

SHAPE = (3, 301)


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


@pytest.fixture(scope='module')
def wave():
    return R.waveform(SHAPE, seed=71)


def t64(v):
    return torch.tensor(v, dtype=torch.float64)


# ----------------------------------------------------------------------------- the composite against the rules
@pytest.mark.parametrize('name', R.NAMES)
def test_sosfilt_and_filtfilt_within_the_bounds(tac, wave, name):
    _, b, a = R.named(name)
    sos = tac.tf2sos(b, a)
    x = torch.from_numpy(wave)
    for clamp in (False, True):
        scale = 4.0 if clamp else 1.0
        got = tac.sosfilt(scale * x, sos, clamp=clamp)
        assert got.dtype == torch.float32 and got.shape == x.shape and got.is_contiguous()
        ref, bound = R.reference(scale * wave, sos, clamp=clamp)
        ratio = R.assert_close(got, ref, bound, '%s, clamp %s' % (name, clamp))
        print('%s, clamp %s: worst |err| / bound %.3f' % (name, clamp, ratio))
    # the second yardstick: the direct-form float64 filter of the transfer function itself
    ref, bound = LR.reference(wave, b, a)
    ratio = R.assert_close(tac.sosfilt(x, sos), ref, bound, '%s against the direct form' % name)
    print('%s against the direct form: worst |err| / bound %.3f' % (name, ratio))
    for clamp in (False, True):
        got = tac.filtfilt(x, t64(a), t64(b), clamp=clamp)
        assert got.dtype == torch.float32 and got.shape == x.shape
        ref, bound = R.filtfilt_reference(wave, sos, clamp=clamp)
        ratio = R.assert_close(got, ref, bound, 'filtfilt, %s, clamp %s' % (name, clamp))
        print('filtfilt, %s, clamp %s: worst |err| / bound %.3f' % (name, clamp, ratio))


def test_filtfilt_up_to_order_two_is_lfilter_twice(tac, wave):
    x = torch.from_numpy(wave)
    for name, b, a in LR.filters(tac):
        for clamp in (False, True):
            got = tac.filtfilt(x, t64(a), t64(b), clamp=clamp)
            want = tac.lfilter(tac.lfilter(x, t64(a), t64(b), clamp=False).flip(-1), t64(a), t64(b), clamp=clamp).flip(-1)
            assert torch.equal(got, want), name
            n = 3 - len(b)
            ref, bound = R.filtfilt_reference(wave, np.array([list(b) + [0.0] * n + list(a) + [0.0] * n]), clamp=clamp)
            R.assert_close(got, ref, bound, 'filtfilt, %s, clamp %s' % (name, clamp))


def test_filtfilt_signature_is_torchaudios(tac):
    sig = inspect.signature(tac.filtfilt)
    assert list(sig.parameters) == ['waveforms', 'a_coeffs', 'b_coeffs', 'clamp']
    assert sig.parameters['clamp'].default is True
    assert all(p.default is inspect.Parameter.empty for p in list(sig.parameters.values())[:3])
    assert inspect.signature(tac.sosfilt).parameters['clamp'].default is False


# ----------------------------------------------------------------------------- tf2sos
def _product(sos):
    b, a = np.array([1.0]), np.array([1.0])
    for row in sos:
        b, a = np.convolve(b, row[:3]), np.convolve(a, row[3:])
    return b, a


@pytest.mark.parametrize('name', R.NAMES)
def test_tf2sos_sections(tac, name):
    _, b, a = R.named(name)
    got = tac.tf2sos(b, a)
    order = len(a) - 1
    assert got.dtype == torch.float64 and got.device.type == 'cpu' and tuple(got.shape) == ((order + 1) // 2, 6)
    assert tac.tf2sos(list(b), t64(a)) is got                                    # cached by value
    sos = got.numpy()
    assert np.isrealobj(sos) and np.isfinite(sos).all() and (sos[:, 3] == 1.0).all()
    pb, pa = _product(sos)
    bn, an = np.array(b) / a[0], np.array(a) / a[0]
    assert (np.abs(pb[:order + 1] - bn) <= 2.0 ** -40 * np.abs(bn).sum()).all(), name
    assert (np.abs(pa[:order + 1] - an) <= 2.0 ** -40 * np.abs(an).sum()).all(), name
    assert not pb[order + 1:].any() and not pa[order + 1:].any()
    first_order = [row for row in sos if row[2] == 0.0 and row[5] == 0.0]
    assert len(first_order) == order % 2, name
    # the last section holds the pole nearest the unit circle
    radii = [np.abs(1.0 - np.abs(np.roots(row[3:]))).min() for row in sos if row[4:].any()]
    assert radii[-1] == min(radii), name
    assert np.isclose(np.abs(1.0 - np.abs(np.roots(a))).min(), radii[-1], rtol=1e-3, atol=1e-9)


def test_tf2sos_small_orders_and_odd_inputs(tac):
    assert torch.equal(tac.tf2sos((0.4, 0.2), (2.0, -1.0)), t64([[0.2, 0.1, 0.0, 1.0, -0.5, 0.0]]))
    assert torch.equal(tac.tf2sos((0.2, 0.3, 0.1), (1.0, -1.2, 0.52)), t64([[0.2, 0.3, 0.1, 1.0, -1.2, 0.52]]))
    assert torch.equal(tac.tf2sos((3.0,), (2.0,)), t64([[1.5, 0.0, 0.0, 1.0, 0.0, 0.0]]))
    # a numerator that starts with zeros (a delay), one with a0 = 2, and an all-zero numerator
    for b, a in (((0.0, 0.0, 1.0, 0.5), (1.0, -0.3, 0.2, 0.1)), ((0.1, 0.3, 0.3, 0.1), (2.0, -1.0, 0.6, -0.1)),
                 ((0.0, 0.0, 0.0, 0.0), (1.0, -0.3, 0.2, 0.1))):
        sos = tac.tf2sos(b, a).numpy()
        assert sos.shape == (2, 6)
        pb, pa = _product(sos)
        assert np.allclose(pb[:4], np.array(b) / a[0], rtol=0, atol=1e-14) and np.allclose(pa[:4], np.array(a) / a[0], rtol=0, atol=1e-14)
    for b, a in (((1.0, 2.0), (1.0,)), ((), ()), ((1.0, 0.0), (0.0, 1.0)), ((float('nan'), 0.0), (1.0, 0.5))):
        with pytest.raises(ValueError):
            tac.tf2sos(b, a)
    with pytest.raises(ValueError):
        tac.tf2sos(torch.ones(2, 2), torch.ones(2, 2))


# ----------------------------------------------------------------------------- arguments
def test_value_errors(tac):
    x = torch.randn(2, 50)
    good = t64([[0.2, 0.3, 0.1, 1.0, -1.2, 0.52]])
    for bad in (good[0], good[:, :5], good.reshape(1, 1, 6), good[:0], good.long(), [[0.2, 0.3, 0.1, 1.0, -1.2, 0.52]],
                t64([[1.0, 0.0, 0.0, 0.0, 0.5, 0.0]]), t64([[1.0, 0.0, 0.0, float('inf'), 0.5, 0.0]]),
                t64([[1.0, 0.0, 0.0, float('nan'), 0.5, 0.0]])):
        with pytest.raises(ValueError):
            tac.sosfilt(x, bad)
        if torch.is_tensor(bad):
            with pytest.raises(ValueError):
                tac.SosFilt(bad)
    with pytest.raises(ValueError):
        tac.filtfilt(x, t64([0.0, 1.0]), t64([1.0, 0.0]))
    with pytest.raises(ValueError):
        tac.filtfilt(x, t64([1.0, 1.0]), t64([1.0]))
    assert tuple(tac.sosfilt(x[:, :0], good).shape) == (2, 0) and tuple(tac.filtfilt(x[:, :0], good[0, 3:], good[0, :3]).shape) == (2, 0)
    # a0 other than 1 normalises the section, float32 sections convert exactly
    scaled = good.clone()
    scaled[0] *= 2.0
    assert torch.equal(tac.sosfilt(x, scaled), tac.sosfilt(x, good))
    assert torch.equal(tac.sosfilt(x, good.float()), tac.sosfilt(x, good.float().double()))


# ----------------------------------------------------------------------------- gradients
def test_gradcheck_of_the_composite(tac):
    x = torch.randn(2, 12, dtype=torch.float64, requires_grad=True)
    sos = t64([[0.3, 0.2, 0.1, 1.1, -0.5, 0.2], [0.5, -0.25, 0.0, 1.0, 0.4, 0.0]]).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x_, s_: tac.sosfilt(x_, s_), (x, sos))
    assert torch.autograd.gradcheck(lambda x_: tac.sosfilt(0.3 * x_, sos.detach(), clamp=True), (x,))
    assert torch.autograd.gradgradcheck(lambda x_: tac.sosfilt(x_, sos.detach()), (x,))
    b, a = t64([0.3, 0.2, 0.1, 0.05]), t64([1.0, -0.5, 0.2, -0.05])
    assert torch.autograd.gradcheck(lambda x_: tac.filtfilt(x_, a, b, clamp=False), (x,))
    assert torch.autograd.gradcheck(lambda x_: tac.filtfilt(x_, a[:3], b[:3], clamp=False), (x,))
    ag, bg = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a_, b_: tac.filtfilt(x.detach(), a_, b_, clamp=False), (ag, bg))


def test_float32_gradient_is_the_adjoint(tac, wave):
    sos = R.sections_of(tac, R.BANDPASS8)
    gy = R.waveform(SHAPE, seed=72)
    for clamp, scale in ((False, 1.0), (True, 4.0)):
        x = torch.from_numpy(scale * wave).requires_grad_(True)
        raw, rb = R.reference(scale * wave, sos)
        g_eff = gy
        if clamp:
            assert (np.abs(raw) > 1.0).any() and (np.abs(np.abs(raw) - 1.0) > rb).all()
            g_eff = gy * (np.abs(raw) < 1.0)
        tac.sosfilt(x, torch.from_numpy(sos), clamp=clamp).backward(torch.from_numpy(gy))
        ref, bound = R.adjoint_reference(g_eff, sos)
        R.assert_close(x.grad, ref, bound, 'gradient, clamp %s' % clamp)


# ----------------------------------------------------------------------------- the layer, tracing, exports
def test_layer_and_exports(tac, wave):
    sos = tac.tf2sos(*R.named(R.ODD)[1:])
    layer = tac.SosFilt(sos, clamp=True)
    x = torch.from_numpy(wave)
    assert torch.equal(layer(x), tac.sosfilt(x, sos, clamp=True))
    assert layer.state_dict() == {} and layer.sos.dtype == torch.float64 and 'sections=2' in repr(layer)
    assert tac.SosFilt(sos.tolist()).sos.dtype == torch.float64 and tac.SosFilt(sos).clamp is False
    for name in ('sosfilt', 'tf2sos', 'filtfilt'):
        assert name in tac.functional.__all__ and getattr(tac, name) is getattr(tac.functional, name)
    assert tac.SosFilt is tac.layers.SosFilt
    for op in ('sosfilt', 'sosfilt_reverse', 'lfilter_reverse'):
        assert op in tac._ops.cuda_kernels and hasattr(torch.ops.tac_amd, op) and op in tac._ops._HIP_BACKWARD


def test_fake_kernel_shape_under_compile(tac):
    seen = []

    def capture(gm, example_inputs):
        seen.extend(n.target for n in gm.graph.nodes if n.op == 'call_function')
        return gm.forward

    sos = tac.tf2sos(*R.named(R.BANDPASS8)[1:])
    x = torch.randn(2, 3, 500)
    layer = tac.SosFilt(sos)
    torch._dynamo.reset()
    out = torch.compile(layer, backend=capture, fullgraph=True)(x)
    names = [str(t) for t in seen]
    assert sum('tac_amd.sosfilt' in n for n in names) == 1 and len(names) == 1, names
    assert torch.equal(out, layer(x))
    from torch._subclasses.fake_tensor import FakeTensorMode
    xt = x.transpose(0, 1)
    with FakeTensorMode() as mode:
        fake = torch.ops.tac_amd.sosfilt(mode.from_tensor(xt), mode.from_tensor(sos), False)
    eager = tac.sosfilt(xt, sos)
    assert tuple(fake.shape) == tuple(eager.shape) == (3, 2, 500) and fake.dtype == eager.dtype
    assert fake.stride() == eager.stride() == (1000, 500, 1)


# ----------------------------------------------------------------------------- the bound leaves the kernel room
@pytest.mark.parametrize('name', R.NAMES)
def test_tile_scan_emulation_stays_far_inside_the_budget(tac, name):
    """40000 samples: two full tiles and a part of a third, so the scan, the carries and a partial tile all take part.  The
    bound's ``2^-126`` stays whole: inside the stretch of zeros the response decays below 1e-45, where ``d_S`` itself underflows
    (or, a difference of two roundings, comes out as -1e-54) and float64 products flush."""
    x = R.waveform((1, 40000), seed=73)
    sos = R.sections_of(tac, name)
    ref, budget = R.arithmetic_budget(x, sos)
    got = R.emulate(x, sos)
    err = np.abs(got - ref)
    counted = budget > R.TINY
    share = float((err[counted] / budget[counted]).max())
    print('%s: float64 tile scan at %.2g of the stage-composed budget' % (name, share))
    assert (err <= 0.1 * np.maximum(budget, 0.0) + R.TINY).all(), '%s: the emulated scan takes %.3g of the budget' % (name, share)
