"""not-gpu: ``griffinlim`` / ``GriffinLim`` on CPU tensors (``_composite.griffinlim`` behind ``tac_amd::griffinlim``) against the
definition restated in tests/griffinlim_rules.py, the argument checks, the layer, the fake kernel, and the conditions on the
inputs that give the GPU file's bounds their meaning."""
import warnings

import pytest
import torch

import griffinlim_rules as R


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


def call(tac, spec, w, case, n_iter, momentum=0.99, length=None, rand_init=False):
    n_fft, hop, wl, user, rows, frames, power = case
    return tac.griffinlim(spec, w, n_fft, hop, wl, power, n_iter, momentum, length, rand_init)


SMALL = ('256/64', '400/160', '512/128 win 400 user')


# ----------------------------------------------------------------------------- the op is the definition
@pytest.mark.parametrize('tag', SMALL)
def test_cpu_op_is_the_reference_to_the_bit(tac, tag):
    case = R.CASES[tag]
    n_fft, hop, wl, user, rows, frames, power = case
    w, spec = R.case_input(tag)
    for n_iter, momentum, length in ((0, 0.99, None), (1, 0.99, None), (3, 0.0, None), (5, 0.99, hop * (frames - 1) + 3)):
        got = call(tac, spec, w, case, n_iter, momentum, length)
        want = R.reference(spec, w, n_fft, hop, wl, power, n_iter, momentum, length, None, torch.float32)
        assert got.dtype == torch.float32 and got.shape == (rows, hop * (frames - 1) if length is None else length)
        assert torch.equal(got, want), (tag, n_iter, momentum, length, float((got - want).abs().max()))
    # the draw: torch.rand complex64 of the specgram's shape, before the op
    torch.manual_seed(17)
    got = call(tac, spec, w, case, 4, rand_init=True)
    torch.manual_seed(17)
    angles0 = torch.rand(spec.shape, dtype=torch.complex64)
    want = R.reference(spec, w, n_fft, hop, wl, power, 4, 0.99, None, angles0, torch.float32)
    assert torch.equal(got, want)
    assert not torch.equal(got, call(tac, spec, w, case, 4))


def test_zero_iterations_is_istft_of_the_root(tac):
    case = R.CASES['256/64']
    n_fft, hop, wl, user, rows, frames, power = case
    w, spec = R.case_input('256/64')
    got = call(tac, spec, w, case, 0)
    z = torch.stack([spec.pow(1.0 / power), torch.zeros_like(spec)], dim=-1)
    assert torch.equal(got, tac.istft(z, n_fft, hop, wl, w))


@pytest.mark.parametrize('lead', [(), (2,), (2, 3)])
def test_leading_dims_are_restored(tac, lead):
    case = R.CASES['256/64']
    n_fft, hop, wl, user, rows, frames, power = case
    w, spec = R.case_input('256/64')
    one = spec[0]
    x = one.expand(lead + tuple(one.shape)).contiguous()
    got = call(tac, x, w, case, 2)
    assert got.shape == lead + (hop * (frames - 1),)
    flat = R.reference(x.reshape((-1,) + tuple(one.shape)), w, n_fft, hop, wl, power, 2, 0.99, None, None, torch.float32)
    assert torch.equal(got.reshape(flat.shape), flat)
    # (a batch of one and a batch of several go through different FFT plans on the host: close, not the same bits)
    assert torch.allclose(got.reshape(-1, got.shape[-1])[-1], call(tac, one, w, case, 2), rtol=0.0, atol=1e-4)


# ----------------------------------------------------------------------------- argument checks
def test_errors(tac):
    case = R.CASES['256/64']
    n_fft, hop, wl, user, rows, frames, power = case
    w, spec = R.case_input('256/64')
    with pytest.raises(ValueError, match=r'momentum must be in range \[0, 1\)\. Found: 1\.0'):
        call(tac, spec, w, case, 2, momentum=1.0)
    with pytest.raises(ValueError, match='momentum must be in range'):
        call(tac, spec, w, case, 2, momentum=-0.1)
    with pytest.raises(TypeError):
        tac.griffinlim(spec.numpy(), w, n_fft, hop, wl, power, 2, 0.99, None, False)
    with pytest.raises(RuntimeError, match='real floating point'):
        call(tac, spec.to(torch.complex64), w, case, 2)
    with pytest.raises(RuntimeError, match='real floating point'):
        call(tac, spec.to(torch.int32), w, case, 2)
    with pytest.raises(RuntimeError, match='specgram for n_fft'):
        call(tac, spec[:, :-1], w, case, 2)
    with pytest.raises(RuntimeError, match='n_iter'):
        call(tac, spec, w, case, -1)
    for bad in (0.0, -2.0):
        with pytest.raises(RuntimeError, match='power'):
            tac.griffinlim(spec, w, n_fft, hop, wl, bad, 2, 0.99, None, False)
    with pytest.raises(RuntimeError, match='length'):
        call(tac, spec, w, case, 2, length=hop * frames + 1)
    with pytest.raises(RuntimeError, match='length'):
        call(tac, spec, w, case, 2, length=hop * (frames - 1) - 1)
    with pytest.raises(RuntimeError, match='reflect'):                     # 2 frames of hop 64: 64 samples <= n_fft // 2
        call(tac, spec[..., :2], w, case, 2)
    with pytest.raises(RuntimeError, match='NOLA|overlap'):
        tac.griffinlim(spec, torch.hann_window(64), n_fft, 64, 64, power, 2, 0.99, None, False)


# ----------------------------------------------------------------------------- the layer
def test_layer(tac):
    layer = tac.GriffinLim()
    assert (layer.n_fft, layer.n_iter, layer.win_length, layer.hop_length, layer.power, layer.momentum, layer.length,
            layer.rand_init) == (400, 32, 400, 200, 2.0, 0.99, None, True)
    assert repr(layer) == 'GriffinLim(n_fft=400, n_iter=32, win_length=400, hop_length=200, power=2.0, momentum=0.99, ' \
                          'length=None, rand_init=True)'
    assert torch.equal(layer.window, torch.hann_window(400)) and 'window' not in layer.state_dict() and not layer.state_dict()
    assert layer.to(torch.float64).window.dtype == torch.float64
    layer = tac.GriffinLim(n_fft=256, n_iter=3, win_length=200, window_fn=torch.hamming_window, wkwargs={'periodic': False},
                           power=1.0, momentum=0.5, rand_init=False)
    assert layer.hop_length == 100 and torch.equal(layer.window, torch.hamming_window(200, periodic=False))
    with pytest.raises(ValueError, match='momentum must be in range'):
        tac.GriffinLim(momentum=1.0)
    case = R.CASES['256/64']
    n_fft, hop, wl, user, rows, frames, power = case
    w, spec = R.case_input('256/64')
    layer = tac.GriffinLim(n_fft=n_fft, n_iter=3, hop_length=hop, power=power, rand_init=False)
    assert torch.equal(layer(spec), call(tac, spec, w, case, 3))
    assert 'GriffinLim' in tac.layers.__dict__ and 'griffinlim' in tac.functional.__all__


def test_compile_goes_through_the_fake_kernel(tac):
    case = R.CASES['256/64']
    n_fft, hop, wl, user, rows, frames, power = case
    w, spec = R.case_input('256/64')

    def fn(s, win):
        return tac.griffinlim(s, win, n_fft, hop, wl, power, 2, 0.99, None, False) * 2.0

    fake = torch.ops.tac_amd.griffinlim(spec.to('meta'), w.to('meta'), None, n_fft, hop, wl, power, 2, 0.5, None)
    assert fake.device.type == 'meta' and fake.shape == (rows, hop * (frames - 1)) and fake.dtype == torch.float32
    assert torch.ops.tac_amd.griffinlim(spec.to('meta'), w.to('meta'), None, n_fft, hop, wl, power, 2, 0.5, 77).shape == (rows, 77)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        got = torch.compile(fn, fullgraph=True, backend='aot_eager')(spec, w)
    assert torch.equal(got, fn(spec, w))


def test_gradient_flows_through_the_composite(tac):
    case = R.CASES['256/64']
    w, spec = R.case_input('256/64')
    s = (spec[:1] + 1e-3).clone().requires_grad_(True)
    call(tac, s, w, case, 2).square().sum().backward()
    assert s.grad is not None and bool(torch.isfinite(s.grad).all()) and bool(s.grad.abs().sum() > 0)


# ----------------------------------------------------------------------------- conditions on the inputs of the GPU file
@pytest.mark.parametrize('tag', sorted(R.CASES))
def test_inputs_converge_and_float32_tracks_float64_early(tac, tag):
    """with the float64 reference, conv after 32 iterations is at most conv after 0 iterations / 1.5 on every non-silent row; the
    float32 CPU reference stays within 1e-4 of each row's maximum of the float64 one at n_iter <= 4 (measured worst 1.2e-5)"""
    n_fft, hop, wl, user, rows, frames, power = R.CASES[tag]
    w, spec = R.case_input(tag)
    s_lin = R.linear_magnitude(spec, power)
    runs = {n: R.reference(spec, w, n_fft, hop, wl, power, n, 0.99, None, None, torch.float64) for n in (0, 1, 4, 32)}
    c0, c32 = R.conv(runs[0], s_lin, n_fft, hop, w), R.conv(runs[32], s_lin, n_fft, hop, w)
    print('%s: conv after 0 iterations %s, after 32 %s' % (tag, c0.tolist(), c32.tolist()))
    for row in range(rows):
        if bool(spec[row].any()):
            assert float(c32[row]) <= float(c0[row]) / 1.5, (tag, row, float(c0[row]), float(c32[row]))
        else:
            assert not bool(runs[32][row].any())
    for n in (1, 4):
        y32 = R.reference(spec, w, n_fft, hop, wl, power, n, 0.99, None, None, torch.float32)
        worst = float(R.row_max_rel(y32, runs[n]).max())
        print('%s: float32 against float64 at n_iter=%d: %.3g' % (tag, n, worst))
        assert worst <= 1e-4, (tag, n, worst)
