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


def test_cached_on_keeps_a_none_result(tac):
    H = tac._hip
    y = torch.arange(6.0)
    calls = []

    def build():
        calls.append(1)
    assert H.cached_on(y, '_tac_adj', (), build) is None and H.cached_on(y, '_tac_adj', (), build) is None
    assert len(calls) == 1 and y._tac_adj[1] == {(): None}
    y.add_(1.0)                                                          # ... per contents: a write asks again
    assert H.cached_on(y, '_tac_adj', (), build) is None and len(calls) == 2


def test_cached_on_limit_bounds_the_slot(tac):
    H = tac._hip
    y = torch.arange(6.0)
    built = []

    def build_for(key):
        def build():
            built.append(key)
            return [key]
        return build
    a = H.cached_on(y, '_tac_dft', 'a', build_for('a'), limit=1)
    assert H.cached_on(y, '_tac_dft', 'a', build_for('a'), limit=1) is a and built == ['a']
    H.cached_on(y, '_tac_dft', 'b', build_for('b'), limit=1)             # a second key evicts the first
    assert list(y._tac_dft[1]) == ['b']
    assert H.cached_on(y, '_tac_dft', 'a', build_for('a'), limit=1) is not a and built == ['a', 'b', 'a']
    for k in range(40):                                                  # the default: 16 kept, emptied when one more arrives
        H.cached_on(y, '_tac_conv', k, build_for(k))
        assert len(y._tac_conv[1]) == k % 16 + 1


def test_cached_on_refuses_a_slot_invalidate_does_not_know(tac):
    H = tac._hip
    y = torch.arange(6.0)
    with pytest.raises(ValueError, match='_CACHE_ATTRS'):
        H.cached_on(y, '_tac_unlisted', 0, lambda: 1)
    assert not hasattr(y, '_tac_unlisted')


def test_cached_on_builds_outside_inference_mode(tac):
    H = tac._hip
    y = torch.arange(6.0)
    with torch.inference_mode():
        first = H.cached_on(y, '_tac_T', (), lambda: y.detach() * 2)
        assert H.cached_on(y, '_tac_T', (), lambda: y.detach() * 2) is first
    assert not first.is_inference() and torch.equal(first, torch.arange(6.0) * 2)


def test_cached_on_rebuilds_for_a_tensor_made_in_inference_mode(tac):
    H = tac._hip
    with torch.inference_mode():
        y = torch.arange(6.0)
    built = []

    def build():
        built.append(float(y.sum()))
        return y.detach() + 1
    first = H.cached_on(y, '_tac_T', (), build)
    with torch.inference_mode():
        y.mul_(2.0)                                                      # (no version counter records it)
    again = H.cached_on(y, '_tac_T', (), build)
    assert built == [15.0, 30.0] and again is not first
    assert torch.equal(first, torch.arange(6.0) + 1) and torch.equal(again, torch.arange(6.0) * 2 + 1)


def test_invalidate_drops_every_slot_cached_on_wrote(tac):
    H = tac._hip
    y = torch.arange(6.0)
    other = torch.arange(6.0)
    for attr in H._CACHE_ATTRS:
        H.cached_on(y, attr, 0, lambda: attr)
        H.cached_on(other, attr, 0, lambda: attr)
    assert all(hasattr(y, attr) for attr in H._CACHE_ATTRS)
    e0 = H._epoch
    H.invalidate(y)
    assert not any(hasattr(y, attr) for attr in H._CACHE_ATTRS) and H._epoch == e0      # targeted: no epoch bump
    assert all(getattr(other, attr)[1] == {0: attr} for attr in H._CACHE_ATTRS)


def _table_builders(H):
    """(name, tensor from contents, table of that tensor, slot) for the derived tables that need no library on CPU tensors"""
    window = lambda v: v[:96].clone()
    matrix = lambda v: v[:96].reshape(12, 8).clone()
    return [('dft', window, lambda w: H._dft_matrix(w, 96, 96, True, False), '_tac_dft'),
            ('dftT', window, lambda w: H._dft_matrix_t(w, 96, 96, False), '_tac_dftT'),
            ('T', matrix, H.transposed_bank, '_tac_T'),
            ('dct', matrix, lambda m: H._dct_matrix(m, True), '_tac_dct')]


@pytest.mark.parametrize('which', [0, 1, 2, 3], ids=['dft', 'dftT', 'T', 'dct'])
def test_derived_tables_follow_their_tensor(tac, which):
    H = tac._hip
    _, make, table, slot = _table_builders(H)[which]
    values = torch.linspace(0.25, 1.0, 96)
    t = make(values)
    first = table(t)
    assert table(t) is first and getattr(t, slot)[0] == H._stamp(t)      # unchanged tensor: the identical object
    t.mul_(2)
    again = table(t)
    assert again is not first and table(t) is again
    assert torch.equal(again, table(make(values * 2))) and not torch.equal(again, first)


def test_window_holds_one_dft_matrix(tac):
    H = tac._hip
    w = torch.hann_window(96)
    m96 = H._dft_matrix(w, 96, 96, True, False)
    m100 = H._dft_matrix(w, 100, 96, True, False)
    assert m96.shape == (96, 98) and m100.shape == (100, 102)
    assert list(w._tac_dft[1].values())[0] is m100 and len(w._tac_dft[1]) == 1
    H._dft_matrix_t(w, 96, 96, False)
    H._dft_matrix_t(w, 100, 96, False)
    assert len(w._tac_dftT[1]) == 1 and len(w._tac_dft[1]) == 1


def test_bounded_dict_clears_when_full(tac):
    from torchaudio_contrib_amd._bounded import Bounded
    d = Bounded(4)
    for k in range(5):
        d[k] = k
    assert len(d) == 5                                                   # limit + 1 entries
    d[2] = 'again'                                                       # an existing key never clears
    assert len(d) == 5 and d[2] == 'again'
    d[5] = 5                                                             # the next new key leaves exactly one
    assert dict(d) == {5: 5}
    import copy, io, pickle
    full = Bounded(2)
    for k in range(3):
        full[k] = [k]
    for back in (pickle.loads(pickle.dumps(full)), copy.deepcopy(full), copy.copy(full)):
        assert type(back) is Bounded and back.limit == 2 and dict(back) == {0: [0], 1: [1], 2: [2]}
        back[3] = [3]
        assert dict(back) == {3: [3]}
    stft = tac.STFT(64, 16)
    stft.__dict__['_recipes'] = Bounded(32)                              # what a deferred forward leaves on the module
    stft.__dict__['_recipes'][('shape', 64)] = (stft.window, 'template')
    buf = io.BytesIO()
    torch.save(stft, buf)                                                # a whole-module checkpoint reads back
    buf.seek(0)
    loaded = torch.load(buf, weights_only=False)
    assert type(loaded._recipes) is Bounded and loaded._recipes.limit == 32 and list(loaded._recipes) == [('shape', 64)]
    assert torch.equal(loaded.window, stft.window)
    for mod, name, limit in [(tac._hip, '_geometry_cache', 512), (tac._hip, '_ones_cache', 64), (tac._resample, '_banks', 64),
                             (tac._filters, '_tensors', 256), (tac.functional, '_window_cache', 64),
                             (tac._lazy, '_plans', 64), (tac._composite, '_kaldi_constants', 32)]:
        assert type(getattr(mod, name)) is Bounded and getattr(mod, name).limit == limit, name
