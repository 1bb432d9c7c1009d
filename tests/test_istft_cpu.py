"""``istft`` / ``ISTFT`` without a device: the operand rule of the frame kernels' inverse mode against ``numpy.fft.irfft``, the
CPU route against ``torch.istft`` bit for bit, the NOLA error, tracing as one node, and the gradient recipe the HIP backward
implements against autograd through ``torch.istft`` in float64."""
import math

import numpy as np
import pytest
import torch

import istft_rules as R


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


# ----------------------------------------------------------------------------- A
@pytest.mark.parametrize('n_fft', [32, 400, 960, 2048])
def test_operand_rule_is_irfft(n_fft):
    """irfft(X) = (1 / N) C2R(H) with the two end bins taken once and their imaginary parts ignored; the gradient mode's
    operands (ends doubled) give N / 2 times Re sum_{k <= NC} G[k] e^{+2 pi i k n / N}: the same transform, another weight."""
    rng = np.random.default_rng(n_fft)
    nc = n_fft // 2
    x = rng.standard_normal(nc + 1) + 1j * rng.standard_normal(nc + 1)          # DC and Nyquist carry imaginary parts
    want = np.fft.irfft(x, n_fft)
    got = R.c2r(R.inverse_operands(x), n_fft) / n_fft
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    clean = x.copy()
    clean[0], clean[-1] = clean[0].real, clean[-1].real
    assert np.array_equal(R.inverse_operands(x), R.inverse_operands(clean))
    n = np.arange(n_fft)
    adj = (x[:, None] * np.exp(2j * np.pi * ((np.arange(nc + 1)[:, None] * n[None, :]) % n_fft) / n_fft)).real.sum(0)
    assert np.abs(0.5 * R.c2r(R.adjoint_operands(x), n_fft) - adj).max() <= 1e-11 * np.abs(adj).max()


def test_formulas_agree_with_torch_istft():
    """the numpy restatement of the four formulas against ``torch.istft`` in float64 (the reference of the GPU tests)"""
    for n_fft, hop, wl, center, normalized, length in ((512, 128, 512, True, False, None), (400, 160, 256, True, True, 1000),
                                                       (64, 16, 64, True, False, 700), (128, 32, 128, False, False, None)):
        w = torch.hann_window(wl, dtype=torch.float64) if center else torch.ones(wl, dtype=torch.float64)
        z = R.random_spec(1, n_fft, 9, seed=n_fft + hop)[0]
        want = R.torch_istft(z, n_fft, hop, w, center, normalized, length)
        got, low = R.numpy_istft(z.numpy(), n_fft, hop, w.numpy(), center, normalized, length)
        assert got.shape == tuple(want.shape) and low > 1e-11
        assert np.abs(got - want.numpy()).max() <= 1e-12 * np.abs(want.numpy()).max()


# ----------------------------------------------------------------------------- B
@pytest.mark.parametrize('length', [None, 3000, 5000])
@pytest.mark.parametrize('normalized', [False, True])
def test_cpu_route_is_torch_istft(tac, length, normalized):
    x = torch.randn(2, 3, 4000)
    for n_fft, hop, wl in ((512, 128, None), (400, 100, 256)):
        z = tac.stft(x, n_fft, hop, wl, normalized=normalized)
        w = torch.hann_window(wl or n_fft)
        for spec in (z, z.reshape(-1, *z.shape[-3:]), z[0], torch.randn_like(z)):
            if wl and length and length > hop * (spec.shape[-2] - 1) + (n_fft - wl) // 2:
                # a length that reaches into the zeros a short window is padded with: the envelope vanishes, both raise
                with pytest.raises(RuntimeError, match='window overlap add'):
                    R.torch_istft(spec, n_fft, hop, w, True, normalized, length, dtype=torch.float32)
                with pytest.raises(RuntimeError, match='window overlap add'):
                    tac.istft(spec, n_fft, hop, wl, normalized=normalized, length=length)
                continue
            got = tac.istft(spec, n_fft, hop, wl, normalized=normalized, length=length)
            want = R.torch_istft(spec, n_fft, hop, w, True, normalized, length, dtype=torch.float32)
            assert got.shape == tuple(spec.shape[:-3]) + (length or hop * (spec.shape[-2] - 1),)
            assert torch.equal(got, want)
    user = torch.hann_window(512) + 0.25
    assert torch.equal(tac.istft(z[:, :, :201], 400, 100, window=user[:400], length=777),
                       R.torch_istft(z[:, :, :201], 400, 100, user[:400], True, False, 777, dtype=torch.float32))


def test_layer(tac):
    m = tac.ISTFT(512, 128)
    assert repr(m) == 'ISTFT(fft_length=512, hop_length=128, win_length=None)(center=True, normalized=False, onesided=True)'
    assert repr(tac.ISTFT(400, 100, 256, center=False, normalized=True)) == \
        'ISTFT(fft_length=400, hop_length=100, win_length=256)(center=False, normalized=True, onesided=True)'
    assert len(m.state_dict()) == 0 and 'window' in dict(m.named_buffers())
    assert torch.equal(m.window, torch.hann_window(512))
    assert m.double().window.dtype == torch.float64 and m.float().window.dtype == torch.float32
    m.load_state_dict({})
    x = torch.randn(1, 2, 2048)
    z = tac.STFT(512, 128)(x)
    assert torch.equal(m(z), tac.istft(z, 512, 128)) and m(z, length=2048).shape == (1, 2, 2048)
    assert (m(z, 2048) - x).abs().max() < 1e-5
    assert 'istft' in tac.functional.__all__ and tac.istft is tac.functional.istft and tac.ISTFT is tac.layers.ISTFT


def test_argument_errors(tac):
    z = torch.randn(1, 257, 8, 2)
    with pytest.raises(RuntimeError):
        tac.istft(z, 400, 100)                          # 257 bins are not fft_length 400
    with pytest.raises(RuntimeError):
        tac.istft(z[..., 0], 512, 128)
    with pytest.raises(RuntimeError):
        tac.istft(z, 512, 128, window=torch.ones(100))
    with pytest.raises(TypeError):
        tac.istft(z.numpy(), 512, 128)


# ----------------------------------------------------------------------------- C
def test_nola(tac):
    z = torch.randn(2, 257, 10, 2)
    with pytest.raises(RuntimeError, match='window overlap add'):
        tac.istft(z, 512, 512)                          # Hann, hop == fft_length: the envelope touches zero
    with pytest.raises(RuntimeError, match='window overlap add'):
        tac.istft(z, 512, 128, center=False)            # Hann, first sample kept
    got = tac.istft(z, 512, 128, window=torch.ones(512), center=False)
    assert got.shape == (2, 128 * 9 + 512) and bool(torch.isfinite(got).all())


# ----------------------------------------------------------------------------- D
@pytest.mark.parametrize('length', [None, 1000, 2000])
def test_traces_as_one_node(tac, length):
    seen = []

    def capture(gm, example_inputs):
        seen.extend(n.target for n in gm.graph.nodes if n.op == 'call_function')
        return gm.forward

    torch._dynamo.reset()                               # (a fresh trace per length: no dynamic-shape bookkeeping nodes)
    z = torch.randn(3, 257, 12, 2)
    w = torch.hann_window(512)
    fn = torch.compile(lambda s: tac.istft(s, 512, 128, window=w, length=length), backend=capture, fullgraph=True)
    out = fn(z)
    names = [str(t) for t in seen]
    assert sum('tac_amd.istft' in n for n in names) == 1 and len(names) == 1, names
    eager = tac.istft(z, 512, 128, window=w, length=length)
    assert torch.equal(out, eager)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode() as mode:
        fake = torch.ops.tac_amd.istft(mode.from_tensor(z), mode.from_tensor(w), 512, 128, 512, True, False, True, length)
    assert tuple(fake.shape) == tuple(eager.shape) and fake.dtype == eager.dtype and fake.stride() == eager.stride()


# ----------------------------------------------------------------------------- E
def test_gradcheck_cpu(tac):
    z = torch.randn(2, 17, 6, 2, dtype=torch.float64, requires_grad=True)
    w = torch.hann_window(32, dtype=torch.float64)
    assert torch.autograd.gradcheck(lambda s: tac.istft(s, 32, 8, window=w), (z,))
    assert torch.autograd.gradcheck(lambda s: tac.istft(s, 32, 8, window=w, normalized=True, length=30), (z,))


@pytest.mark.parametrize('case', [(64, 16, 64, True, False, None), (400, 160, 256, True, True, 1000), (128, 32, 128, True, False, 200),
                                  (128, 32, 128, True, False, 400), (64, 16, 64, False, False, None)])
def test_gradient_recipe(case):
    """stft of grad_out / env with the bin weights (the HIP backward's recipe) equals autograd through ``torch.istft``: both are
    exact up to summation order, 1e-10 of the row maximum in float64"""
    n_fft, hop, wl, center, normalized, length = case
    w = (torch.hann_window(wl, dtype=torch.float64) + 0.1) if center else torch.ones(wl, dtype=torch.float64)
    z = R.random_spec(3, n_fft, 11, seed=7 + n_fft)
    out_len = length or (hop * 10 + (0 if center else n_fft))
    go = torch.randn(3, out_len, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    want = R.autograd_grad(z, go, n_fft, hop, w, center, normalized, length)
    got = R.grad_recipe(go, w, n_fft, hop, 11, center, normalized)
    assert got.shape == want.shape
    err = (got - want).abs().reshape(3, -1).amax(1)
    top = want.abs().reshape(3, -1).amax(1)
    assert bool((err <= 1e-10 * top).all()), (err / top).tolist()
    assert not bool(want[:, 0, :, 1].any()) and not bool(want[:, -1, :, 1].any())       # irfft ignores these
