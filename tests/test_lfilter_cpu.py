"""Not gpu: ``lfilter`` / the biquads / ``preemphasis`` / ``deemphasis`` on CPU tensors (``_composite.lfilter``: the time loop with
float64 accumulation), the cookbook designs, argument errors, tracing and the layers.  Reference and bound: tests/lfilter_rules.py."""
import math
import warnings

import numpy as np
import pytest
import torch

import lfilter_rules as R

LENGTH = 3000           # room for the zero stretch and the 1e-30 stretch, and > 10 time constants of every filter but the 20 Hz one


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


@pytest.fixture(scope='module')
def wave():
    return R.waveform((2, 2, LENGTH), seed=21)


def t64(v):
    return torch.tensor(v, dtype=torch.float64)


# ----------------------------------------------------------------------------- the composite against the rules
def test_lfilter_within_the_bound(tac, wave):
    x = torch.from_numpy(wave)
    for name, b, a in R.filters(tac):
        for clamp in (False, True):
            got = tac.lfilter(x, t64(a), t64(b), clamp=clamp)
            assert got.dtype == torch.float32 and got.shape == x.shape
            ref, bound = R.reference(wave, b, a, clamp=clamp)
            ratio = R.assert_close(got, ref, bound, '%s, clamp %s' % (name, clamp))
            print('%s, clamp %s: worst |err| / bound %.3f' % (name, clamp, ratio))


def test_float32_coefficients_are_taken_exactly(tac, wave):
    x = torch.from_numpy(wave[0])
    b = torch.tensor([0.3, 0.2, 0.1])
    a = torch.tensor([1.1, -0.7, 0.3])
    ref, bound = R.reference(wave[0], b.double().numpy(), a.double().numpy())
    R.assert_close(tac.lfilter(x, a, b, clamp=False), ref, bound, 'float32 coefficient tensors')


def test_higher_order_and_float64(tac, wave):
    b = (0.1, 0.2, 0.3, 0.2, 0.1)
    a = (1.0, -0.4, 0.3, -0.2, 0.05)
    ref, bound = R.reference(wave[0], b, a)
    R.assert_close(tac.lfilter(torch.from_numpy(wave[0]), t64(a), t64(b), clamp=False), ref, bound, 'order 4')
    got = tac.lfilter(torch.from_numpy(wave[0]).double(), t64(a), t64(b), clamp=False)
    assert got.dtype == torch.float64
    assert np.abs(got.numpy() - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def test_every_biquad_design(tac, wave):
    x = torch.from_numpy(wave)
    f = tac._filters
    designs = [
        (tac.lowpass_biquad, (16000, 1000.0), {}, f.lowpass(16000, 1000.0)),
        (tac.lowpass_biquad, (16000, 1000.0, 10.0), {}, f.lowpass(16000, 1000.0, 10.0)),
        (tac.highpass_biquad, (48000, 20.0), {}, f.highpass(48000, 20.0)),
        (tac.bandpass_biquad, (16000, 2000.0), {}, f.bandpass(16000, 2000.0)),
        (tac.bandpass_biquad, (16000, 2000.0, 2.0), dict(const_skirt_gain=True), f.bandpass(16000, 2000.0, 2.0, True)),
        (tac.bandreject_biquad, (16000, 3000.0), {}, f.bandreject(16000, 3000.0)),
        (tac.allpass_biquad, (16000, 500.0), {}, f.allpass(16000, 500.0)),
        (tac.equalizer_biquad, (16000, 1500.0, 6.0), {}, f.equalizer(16000, 1500.0, 6.0)),
    ]
    for fn, args, kw, (b, a) in designs:
        ref, bound = R.reference(wave, b, a, clamp=True)             # biquad clamps, as torchaudio's does
        R.assert_close(fn(x, *args, **kw), ref, bound, fn.__name__)
    b, a = f.lowpass(16000, 1000.0)
    ref, bound = R.reference(wave, b, a, clamp=True)
    R.assert_close(tac.biquad(x, b[0], b[1], b[2], a[0], a[1], a[2]), ref, bound, 'biquad')


def response(b, a, freq, sample_rate):
    z = np.exp(-1j * 2.0 * np.pi * freq / sample_rate)
    return (b[0] + b[1] * z + b[2] * z * z) / (a[0] + a[1] * z + a[2] * z * z)


def test_cookbook_coefficients_closed_form(tac):
    f = tac._filters
    sr = 16000.0
    for cutoff, q in ((100.0, 0.707), (1000.0, 10.0), (3500.0, 0.5)):
        b, a = f.lowpass(sr, cutoff, q)
        assert abs(response(b, a, 0.0, sr) - 1.0) < 1e-12
        b, a = f.highpass(sr, cutoff, q)
        assert abs(response(b, a, 0.0, sr)) < 1e-12 * abs(a[0]) + 1e-15 / (1.0 - math.cos(2 * math.pi * cutoff / sr))
        assert abs(abs(response(b, a, sr / 2.0, sr)) - 1.0) < 1e-12
        b, a = f.allpass(sr, cutoff, q)
        for freq in (0.0, 50.0, cutoff, 2999.0, sr / 2.0):
            assert abs(abs(response(b, a, freq, sr)) - 1.0) < 1e-12
        b, a = f.bandreject(sr, cutoff, q)
        assert abs(response(b, a, cutoff, sr)) < 1e-12
        for gain in (-12.0, 3.0, 6.0):
            b, a = f.equalizer(sr, cutoff, gain, q)
            assert abs(abs(response(b, a, cutoff, sr)) - 10.0 ** (gain / 20.0)) < 1e-12 * 10.0 ** (abs(gain) / 20.0)
        b, a = f.bandpass(sr, cutoff, q)
        assert abs(abs(response(b, a, cutoff, sr)) - 1.0) < 1e-12                  # 0 dB peak gain
        b, a = f.bandpass(sr, cutoff, q, True)
        assert abs(abs(response(b, a, cutoff, sr)) - q) < 1e-12 * max(q, 1.0)       # peak gain Q
    # the designs against their formulas, spelled out once
    w0 = 2.0 * math.pi * 1000.0 / sr
    alpha = math.sin(w0) / (2.0 * 0.707)
    assert f.lowpass(sr, 1000.0) == (((1 - math.cos(w0)) / 2, 1 - math.cos(w0), (1 - math.cos(w0)) / 2),
                                     (1 + alpha, -2 * math.cos(w0), 1 - alpha))


def test_preemphasis_and_deemphasis(tac, wave):
    x = torch.from_numpy(wave)
    y = tac.preemphasis(x)
    want = wave.astype(np.float64).copy()
    want[..., 1:] -= 0.97 * wave[..., :-1].astype(np.float64)
    ref, bound = R.reference(wave, (1.0, -0.97), (1.0, 0.0))
    assert np.abs(ref - want).max() <= 1e-15 * np.abs(want).max()
    R.assert_close(y, ref, bound, 'preemphasis')
    assert torch.equal(y[..., 0], x[..., 0])
    ref, bound = R.reference(wave, (1.0, 0.0), (1.0, -0.97))
    R.assert_close(tac.deemphasis(x), ref, bound, 'deemphasis')
    # neither clamps
    assert float(tac.preemphasis(10.0 * x).abs().max()) > 1.0 and float(tac.deemphasis(10.0 * x).abs().max()) > 1.0
    # the round trip is the identity within the bound of the second filter applied to the first one's (rounded) output, plus what
    # the first one's rounding, 2^-24 |y| per sample, becomes on its way through 1 / (1 - 0.97 z^-1)
    back = tac.deemphasis(y, 0.97)
    ref2, bound2 = R.reference(y.numpy(), (1.0, 0.0), (1.0, -0.97))
    R.assert_close(back, ref2, bound2, 'deemphasis of preemphasis')
    carried, _ = R.reference(np.abs(ref) * R.EPS32 + R.TINY, (1.0, 0.0), (1.0, -0.97))
    R.assert_close(back, wave.astype(np.float64), bound2 + carried, 'the round trip')
    for coeff in (0.0, 0.5, 1.0):
        assert tac.preemphasis(x, coeff).shape == x.shape and tac.deemphasis(x, coeff).shape == x.shape
    assert torch.equal(tac.preemphasis(x, 0.0), x) and torch.equal(tac.deemphasis(x, 0.0), x)


def test_nan_goes_forward_only(tac):
    x = R.waveform((3, 200), seed=4)
    x[1, 77] = np.nan
    b, a = tac._filters.highpass(16000, 100.0)
    got = tac.lfilter(torch.from_numpy(x), t64(a), t64(b), clamp=False).numpy()
    assert np.isfinite(got[[0, 2]]).all() and np.isfinite(got[1, :77]).all() and np.isnan(got[1, 77:]).all()
    ref, bound = R.reference(x[:, :77], b, a)
    R.assert_close(got[:, :77], ref, bound, 'before the NaN')
    pre = tac.preemphasis(torch.from_numpy(x)).numpy()
    assert np.array_equal(np.isnan(pre[1]), np.isin(np.arange(200), (77, 78))) and np.isfinite(pre[[0, 2]]).all()


def test_shapes_and_degenerate_lengths(tac):
    b, a = tac._filters.lowpass(16000, 1000.0)
    for shape in ((1,), (2,), (3,), (0,), (2, 0), (4, 1), (2, 3, 5)):
        x = torch.from_numpy(R.waveform(shape, seed=sum(shape)))
        got = tac.lfilter(x, t64(a), t64(b), clamp=False)
        assert got.shape == x.shape and got.dtype == x.dtype
        if x.numel():
            ref, bound = R.reference(x.numpy(), b, a)
            R.assert_close(got, ref, bound, 'shape %r' % (shape,))
    x = torch.randn(5, 40)
    assert torch.equal(tac.lfilter(x.t(), t64(a), t64(b)), tac.lfilter(x.t().contiguous(), t64(a), t64(b)))


def test_argument_errors(tac):
    x = torch.randn(2, 30)
    one = t64([1.0, 0.5])
    with pytest.raises(ValueError):
        tac.lfilter(x, t64([1.0, 0.5, 0.2]), one)                   # unequal lengths
    with pytest.raises(ValueError):
        tac.lfilter(x, t64([0.0, 0.5]), one)                        # a0 == 0
    with pytest.raises(ValueError):
        tac.lfilter(x, t64([[1.0, 0.5], [1.0, 0.2]]), t64([[1.0, 0.5], [1.0, 0.2]]))     # 2-D coefficient banks
    with pytest.raises(ValueError):
        tac.lfilter(x, t64([]), t64([]))
    with pytest.raises(ValueError):
        tac.lfilter(x, t64(1.0), t64(1.0))                          # 0-D
    with pytest.raises(ValueError):
        tac.lfilter(x, [1.0, 0.5], one)                             # not a tensor
    with pytest.raises(ValueError):
        tac.lfilter(x, torch.tensor([1, 2]), torch.tensor([1, 2]))  # integer coefficients
    with pytest.raises(ValueError):
        tac.biquad(x, 1.0, 0.0, 0.0, 0.0, 0.5, 0.2)
    with pytest.raises(ValueError):
        tac.lowpass_biquad(x, 16000, 100.0, Q=0.0)
    with pytest.raises(ValueError):
        tac.LFilter([0.0, 1.0], [1.0, 1.0])
    with pytest.raises(ValueError):
        tac.LFilter([1.0, 1.0], [1.0])
    with pytest.raises(TypeError):
        tac.lfilter([0.0, 1.0], one, one)
    with pytest.raises(RuntimeError):
        tac.lfilter(torch.zeros(3, dtype=torch.int64), one, one)
    with pytest.raises(RuntimeError):
        tac.preemphasis(torch.tensor(1.0))
    assert not hasattr(tac, 'bass_biquad') and not hasattr(tac, 'treble_biquad')


# ----------------------------------------------------------------------------- gradients
def test_gradcheck_of_the_composite(tac):
    x = torch.randn(2, 12, dtype=torch.float64, requires_grad=True)
    a = torch.tensor([1.1, -0.5, 0.2], dtype=torch.float64, requires_grad=True)
    b = torch.tensor([0.3, 0.2, 0.1], dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x_, a_, b_: tac.lfilter(x_, a_, b_, clamp=False), (x, a, b))
    assert torch.autograd.gradcheck(lambda x_: tac.lfilter(0.3 * x_, a.detach(), b.detach(), clamp=True), (x,))
    assert torch.autograd.gradcheck(lambda x_: tac.preemphasis(x_), (x,))
    assert torch.autograd.gradcheck(lambda x_: tac.deemphasis(x_), (x,))
    assert torch.autograd.gradgradcheck(lambda x_: tac.lfilter(x_, a.detach(), b.detach(), clamp=False), (x,))


def test_float32_gradient_is_the_reversed_filter(tac):
    for name, b, a in R.filters(tac):
        x = torch.from_numpy(R.waveform((2, 300), seed=8)).requires_grad_(True)
        gy = R.waveform((2, 300), seed=9)
        tac.lfilter(x, t64(a), t64(b), clamp=False).backward(torch.from_numpy(gy))
        ref, bound = R.adjoint_reference(gy, b, a)
        # autograd's chain through the float64 time loop: float64 arithmetic, rounded once
        R.assert_close(x.grad, ref, bound, 'gradient, %s' % name)
    # clamp: no gradient where the result was clipped
    b, a = tac._filters.lowpass(16000, 1000.0)
    x = torch.from_numpy(3.0 * R.waveform((2, 300), seed=8)).requires_grad_(True)
    y = tac.lfilter(x, t64(a), t64(b), clamp=True)
    raw, rb = R.reference(x.detach().numpy(), b, a)
    assert (np.abs(raw) > 1.0).any() and (np.abs(np.abs(raw) - 1.0) > rb).all()
    y.backward(torch.from_numpy(gy))
    ref, bound = R.adjoint_reference(gy * (np.abs(raw) < 1.0), b, a)
    R.assert_close(x.grad, ref, bound, 'gradient through the clamp')


# ----------------------------------------------------------------------------- tracing
def test_fake_kernel_shape_under_compile(tac):
    seen = []

    def capture(gm, example_inputs):
        seen.extend(n.target for n in gm.graph.nodes if n.op == 'call_function')
        return gm.forward

    b, a = tac._filters.highpass(16000, 100.0)
    x = torch.randn(2, 3, 500)
    for layer in (tac.LFilter(a, b), tac.Preemphasis(0.95), tac.Deemphasis()):
        torch._dynamo.reset()
        del seen[:]
        out = torch.compile(layer, backend=capture, fullgraph=True)(x)
        names = [str(t) for t in seen]
        assert sum('tac_amd.lfilter' in n for n in names) == 1 and len(names) == 1, names
        assert torch.equal(out, layer(x))
    from torch._subclasses.fake_tensor import FakeTensorMode
    xt, at, bt = x.transpose(0, 1), t64(a), t64(b)
    with FakeTensorMode() as mode:
        fake = torch.ops.tac_amd.lfilter(mode.from_tensor(xt), mode.from_tensor(at), mode.from_tensor(bt), True)
    eager = tac.lfilter(x.transpose(0, 1), t64(a), t64(b))
    assert tuple(fake.shape) == tuple(eager.shape) == (3, 2, 500) and fake.dtype == eager.dtype
    assert fake.stride() == eager.stride() == (1000, 500, 1)


# ----------------------------------------------------------------------------- the layers
def test_layers(tac):
    b, a = tac._filters.highpass(16000, 100.0)
    m = tac.LFilter(a, b, clamp=False)
    assert repr(m) == 'LFilter(order=2, clamp=False)'
    assert m.state_dict() == {} and [n for n, _ in m.named_buffers()] == ['a_coeffs', 'b_coeffs']
    assert m.a_coeffs.dtype == torch.float64 and m.a_coeffs.tolist() == list(a) and m.b_coeffs.tolist() == list(b)
    m.load_state_dict({})
    kept = tac.LFilter(torch.tensor([1.0, -0.5]), torch.tensor([0.5, 0.5]))
    assert kept.a_coeffs.dtype == torch.float32 and kept.clamp
    x = torch.randn(2, 1, 2048)
    assert torch.equal(m(x), tac.lfilter(x, t64(a), t64(b), clamp=False))
    pre, de = tac.Preemphasis(), tac.Deemphasis(0.9)
    assert repr(pre) == 'Preemphasis(coeff=0.97)' and repr(de) == 'Deemphasis(coeff=0.9)'
    assert pre.state_dict() == {} and de.state_dict() == {} and not list(pre.buffers())
    assert torch.equal(pre(x), tac.preemphasis(x)) and torch.equal(de(x), tac.deemphasis(x, 0.9))
    mel = dict(num_mels=40, sample_rate=16000, fft_length=512, hop_length=128)
    chain = torch.nn.Sequential(tac.Preemphasis(), *tac.Melspectrogram(**mel), tac.AmplitudeToDb())
    assert chain.state_dict() == {}
    got = chain(x)
    want = tac.AmplitudeToDb()(tac.Melspectrogram(**mel)(tac.preemphasis(x)))
    assert type(got) is torch.Tensor and tuple(got.shape) == (2, 1, 40, 17) and torch.equal(got, want)
    xg = x.clone().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac.CompositeRouteWarning)         # CPU tensors are no announced route
        chain(xg).square().mean().backward()
    assert bool(torch.isfinite(xg.grad).all()) and bool(xg.grad.any())


def test_names_are_exported(tac):
    names = ('lfilter', 'biquad', 'lowpass_biquad', 'highpass_biquad', 'bandpass_biquad', 'bandreject_biquad', 'allpass_biquad',
             'equalizer_biquad', 'preemphasis', 'deemphasis')
    for name in names:
        assert name in tac.functional.__all__ and getattr(tac, name) is getattr(tac.functional, name)
    for name in ('LFilter', 'Preemphasis', 'Deemphasis'):
        assert getattr(tac, name) is getattr(tac.layers, name)
    assert 'lfilter' in tac._ops.cuda_kernels and hasattr(torch.ops.tac_amd, 'lfilter') and 'lfilter' in tac._ops._HIP_BACKWARD
    assert tac._hip.LFILTER_TILE == 1024 * tac._hip.LFILTER_C
