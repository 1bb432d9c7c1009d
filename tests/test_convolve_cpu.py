"""Not gpu: ``fftconvolve`` / ``convolve`` on CPU tensors (``_composite.fftconvolve``), the numpy restatement of the partitioned
route against ``numpy.convolve``, the crops, argument errors, tracing, gradients, the layers and the kernel-spectrum cache.
Rules: tests/convolve_rules.py."""
import numpy as np
import pytest
import torch

import convolve_rules as R


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


# ----------------------------------------------------------------------------- the restatement of the route
@pytest.mark.parametrize('n_fft', [64, 2048])
def test_overlap_save_restatement_equals_numpy_convolve(n_fft):
    b = n_fft // 2
    edges = (b - 1, b, b + 1, 2 * b + 1)
    rng = np.random.default_rng(n_fft)
    for length in edges:
        for m in edges:
            x, h = rng.standard_normal(length), rng.standard_normal(m)
            want = np.convolve(x, h)
            got = R.overlap_save(x, h, n_fft)
            assert got.shape == want.shape
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (n_fft, length, m)
    got = R.overlap_save(np.array([3.0]), np.array([-2.0]), n_fft)
    assert got.shape == (1,) and abs(got[0] + 6.0) < 1e-12


def test_delay_line_skips_frames_before_the_row():
    X = np.full((3, 5), np.nan + 0j)
    X[2] = 1.0
    H = np.ones((2, 5), dtype=complex)
    Y = R.delay_line(X, H)
    assert np.isnan(Y[:2]).all() and np.isnan(Y[2]).all()        # frame 2 reads frames 2 and 1
    X[:2] = 0.0
    assert np.array_equal(R.delay_line(X, H)[2], np.ones(5))


def test_crops_follow_numpy_and_torchaudio():
    rng = np.random.default_rng(5)
    for length, m in [(50, 7), (50, 8), (9, 9), (33, 1)]:
        x, h = rng.standard_normal(length), rng.standard_normal(m)
        full = np.convolve(x, h)
        for mode in ('full', 'valid', 'same'):
            assert np.array_equal(R.crop(full, length, m, mode), np.convolve(x, h, mode)), (length, m, mode)
    # L < M: 'valid' is symmetric in its arguments, 'same' keeps x's length (numpy keeps the longer one's)
    x, h = rng.standard_normal(7), rng.standard_normal(50)
    full = np.convolve(x, h)
    assert np.array_equal(R.crop(full, 7, 50, 'valid'), np.convolve(h, x, 'valid'))
    same = R.crop(full, 7, 50, 'same')
    assert same.shape == (7,) and np.array_equal(same, full[(56 - 7) // 2:(56 - 7) // 2 + 7])


# ----------------------------------------------------------------------------- the CPU op
@pytest.mark.parametrize('name', ['fftconvolve', 'convolve'])
def test_cpu_op_matches_the_reference(tac, name):
    fn = getattr(tac, name)
    for length, m, dtype, tol in [(500, 31, torch.float64, 1e-12), (31, 500, torch.float64, 1e-12), (2000, 300, torch.float32, 2e-5),
                                  (1, 1, torch.float64, 1e-12)]:
        x = R.waveform((2, 3, length), seed=length)
        h = R.white_kernel((2, 3, m), seed=m)
        ref = R.reference(x, h).reshape(2, 3, -1)
        for mode in ('full', 'valid', 'same'):
            got = fn(torch.from_numpy(x).to(dtype), torch.from_numpy(h).to(dtype), mode)
            want = R.crop(ref, length, m, mode)
            assert got.dtype == dtype and tuple(got.shape) == want.shape, (length, m, mode)
            assert np.abs(got.double().numpy() - want).max() <= tol * np.abs(ref).max(), (length, m, mode)


def test_crop_is_a_view_of_the_full_result(tac):
    x, h = torch.randn(2, 40, dtype=torch.float64), torch.randn(2, 9, dtype=torch.float64)
    same = tac.fftconvolve(x, h, 'same')
    assert same._base is not None and tuple(same._base.shape) == (2, 48) and same.storage_offset() == 4
    assert tac.fftconvolve(x, h, 'full')._base is None


def test_leading_dimensions_broadcast(tac):
    x = torch.from_numpy(R.waveform((2, 3, 200), seed=1)).double()
    for yshape in [(2, 1, 17), (1, 3, 17), (1, 1, 17), (2, 3, 17)]:
        h = torch.from_numpy(R.white_kernel(yshape, seed=2)).double()
        got = tac.fftconvolve(x, h)
        he = h.expand(2, 3, 17)
        for i in range(2):
            for j in range(3):
                want = np.convolve(x[i, j].numpy(), he[i, j].numpy())
                assert np.abs(got[i, j].numpy() - want).max() <= 1e-12 * np.abs(want).max()
    # x is the one that broadcasts
    got = tac.fftconvolve(x[:1], torch.from_numpy(R.white_kernel((2, 3, 5), seed=3)).double())
    assert tuple(got.shape) == (2, 3, 204)


def test_argument_errors(tac):
    x, h = torch.randn(2, 30), torch.randn(2, 5)
    for fn in (tac.fftconvolve, tac.convolve):
        for mode in ('Full', 'circular', None, 1):
            with pytest.raises(ValueError, match='mode'):
                fn(x, h, mode)
        with pytest.raises(ValueError, match='dimensions'):
            fn(x, h[0])
        with pytest.raises(ValueError, match='broadcastable'):
            fn(x, torch.randn(3, 5))
        with pytest.raises(ValueError, match='n_fft'):
            fn(x, h, n_fft=1024)
        with pytest.raises(RuntimeError, match='floating-point'):
            fn(x.long(), h)
    for layer in (tac.FFTConvolve, tac.Convolve):
        with pytest.raises(ValueError, match='mode'):
            layer('half')


def test_layers(tac):
    x, h = torch.randn(2, 3, 100, dtype=torch.float64), torch.randn(2, 1, 11, dtype=torch.float64)
    for mode in ('full', 'valid', 'same'):
        for layer, fn in ((tac.FFTConvolve(mode), tac.fftconvolve), (tac.Convolve(mode), tac.convolve)):
            assert torch.equal(layer(x, h), fn(x, h, mode))
            assert layer.state_dict() == {} and mode in repr(layer)
    assert tac.FFTConvolve().mode == 'full' and tac.layers.Convolve().mode == 'full'


def test_names_are_exported(tac):
    for name in ('fftconvolve', 'convolve', 'FFTConvolve', 'Convolve'):
        assert hasattr(tac, name), name
    assert 'fftconvolve' in tac.functional.__all__ and 'convolve' in tac.functional.__all__
    assert hasattr(torch.ops.tac_amd, 'fftconvolve')


def test_fake_kernel_shapes(tac):
    from torch._subclasses.fake_tensor import FakeTensorMode
    for xs, ys in [((3, 2, 500), (3, 1, 40)), ((1, 500), (4, 7)), ((9,), (9,))]:
        xt, yt = torch.randn(xs), torch.randn(ys)
        eager = torch.ops.tac_amd.fftconvolve(xt, yt, 0)
        with FakeTensorMode() as mode:
            fake = torch.ops.tac_amd.fftconvolve(mode.from_tensor(xt), mode.from_tensor(yt), 0)
        assert tuple(fake.shape) == tuple(eager.shape) and fake.dtype == eager.dtype and fake.stride() == eager.stride()
    compiled = torch.compile(lambda a, b: tac.fftconvolve(a, b, 'same'), backend='eager', fullgraph=True)
    xt, yt = torch.randn(2, 64, dtype=torch.float64), torch.randn(2, 9, dtype=torch.float64)
    assert torch.allclose(compiled(xt, yt), tac.fftconvolve(xt, yt, 'same'))


def test_gradients_against_conv1d_autograd(tac):
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(3, 60, dtype=torch.float64, generator=gen, requires_grad=True)
    h = torch.randn(3, 13, dtype=torch.float64, generator=gen, requires_grad=True)
    for mode in ('full', 'valid', 'same'):
        go = torch.randn(tuple(tac.fftconvolve(x, h, mode).shape), dtype=torch.float64, generator=gen)
        gx, gh = torch.autograd.grad(tac.fftconvolve(x, h, mode), (x, h), go)
        # the same convolution as a grouped conv1d: one group per row, the kernel flipped, M - 1 zeros on both sides
        full = torch.nn.functional.conv1d(x[None], h.flip(-1)[:, None], padding=12, groups=3)[0]
        rx, rh = torch.autograd.grad(R.crop(full, 60, 13, mode), (x, h), go)
        assert torch.allclose(gx, rx, rtol=0, atol=1e-11) and torch.allclose(gh, rh, rtol=0, atol=1e-11), mode
    assert torch.autograd.gradcheck(lambda a, b: tac.fftconvolve(a, b, 'same'), (x, h))
    assert torch.autograd.gradgradcheck(lambda a, b: tac.fftconvolve(a, b), (x[:, :12], h[:, :5]))
    # float32: within float32 rounding of the float64 gradient
    x32, h32 = x.detach().float().requires_grad_(True), h.detach().float().requires_grad_(True)
    go = torch.randn(3, 72, dtype=torch.float64, generator=gen)
    g32 = torch.autograd.grad(tac.fftconvolve(x32, h32), (x32, h32), go.float())
    g64 = torch.autograd.grad(tac.fftconvolve(x, h), (x, h), go)
    for a, b in zip(g32, g64):
        assert float((a.double() - b).abs().max()) <= 1e-5 * float(b.abs().max())


def test_default_transform_length_and_route_rule(tac):
    H = tac._hip
    assert H.FFTCONV_SIZES == (2048, 4096, 8192) and H.FFTCONV_MAX_PARTS == 64 and H.M_DIRECT == 256
    for m, want in [(1, 2048), (8192, 2048), (8193, 4096), (16384, 4096), (16385, 8192), (32768, 8192), (48000, 8192),
                    (262144, 8192), (10 ** 6, 8192)]:
        assert H.fftconvolve_n_fft(m) == want, m
    assert H.fftconvolve_route(256, True) == 'direct' and H.fftconvolve_route(257, True) == 2048
    assert H.fftconvolve_route(7, False) == 2048 and H.fftconvolve_route(7, True, 4096) == 4096


def test_kernel_cache_follows_in_place_writes(tac):
    H = tac._hip
    y = torch.arange(6.0)
    built = []

    def build():
        built.append(float(y.sum()))
        return y.clone()
    first = H.cached_on(y, '_tac_conv', ('spectra', 2048, False), build)
    assert H.cached_on(y, '_tac_conv', ('spectra', 2048, False), build) is first and built == [15.0]
    H.cached_on(y, '_tac_conv', ('spectra', 2048, True), build)          # another key: its own entry
    assert built == [15.0, 15.0]
    y.mul_(2.0)                                                          # an in-place write: every entry is rebuilt
    again = H.cached_on(y, '_tac_conv', ('spectra', 2048, False), build)
    assert again is not first and built == [15.0, 15.0, 30.0] and torch.equal(again, y)
    H.invalidate(y)
    H.cached_on(y, '_tac_conv', ('spectra', 2048, False), build)
    assert len(built) == 4
