"""-m gpu: ``pcen`` on the gfx950 kernels of csrc/pcen.hip — strict mode and poisoned outputs on, counted launches, every element held
to the bound of tests/pcen_rules.py (twice the float32 CPU route's own error, floored).  Shapes: lane masking, exactly one block of
bands and a ragged second or third, the carry across chunks and across tiles, both storage layouts, more units than the grid."""
import warnings

import numpy as np
import pytest
import torch

import pcen_rules as R

pytestmark = pytest.mark.gpu

FWD, BWD = 'tac_pcen_f32', 'tac_pcen_backward_f32'
NAMES = ('gain', 'bias', 'power', 'b')
dev = R.dev


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    t.set_strict(True)
    t._hip.set_poison_outputs(True)
    yield t
    t._hip.set_poison_outputs(False)
    t.set_strict(False)


@pytest.fixture(autouse=True)
def every_output_written(tac):
    tac._hip.poison_report()
    yield
    left = tac._hip.poison_report()
    assert not left, 'kernel outputs left unwritten (poisoned elements per entry point): %r' % left


def sizes(tac_):
    return tac_._native.lib().tac_pcen_chunk_frames(), tac_._native.lib().tac_pcen_tile_frames()


def counted(tac_, fn, expected):
    """``fn()`` on the kernel route: no announcement, exactly the ``expected`` launches"""
    before = dict(tac_._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac_.CompositeRouteWarning)
        got = fn()
    now = tac_._hip.launches
    assert {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)} == expected
    return got


def laid(E, layout):
    """``E`` ``(…, F, T)`` on the device as a frame-major view or as a dense time-contiguous tensor"""
    return dev(np.swapaxes(E, -1, -2)).transpose(-1, -2) if layout == 'frame-major' else dev(E)


def keywords(F, per_band, seed=2):
    return dict(zip(NAMES, R.band_params(F, seed)), eps=1e-6) if per_band else dict(R.DEFAULTS)


def on(kw, device):
    return {k: (torch.from_numpy(v).to(device) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}


def check_forward(tac_, E, kw, what, view=None, layout='frame-major'):
    got = counted(tac_, lambda: tac_.pcen(laid(E, layout) if view is None else view, **on(kw, 'cuda')), {FWD: 1})
    assert got.dtype == torch.float32 and got.transpose(-1, -2).is_contiguous()
    E = E.astype(np.float32)
    value = R.pcen(E, **kw)
    yard = tac_.pcen(torch.from_numpy(E), **on(kw, 'cpu')).numpy()
    scale = np.abs(value) + (np.asarray(kw['bias'], np.float64) ** kw['power']).reshape(-1, 1)
    R.assert_close(got, value, yard, scale, what)


@pytest.mark.parametrize('layout', ['frame-major', 'time-contiguous'])
@pytest.mark.parametrize('F', [1, 23, 64, 65, 130])
def test_forward_over_blocks_chunks_and_tiles(tac, F, layout):
    C, tile = sizes(tac)
    for T in (1, 2, C, C + 1, tile - 1, tile, tile + 1, 2 * tile + 3):
        E = R.signal((2, F, T), 100 * F + T)
        for per_band in (False, True):
            check_forward(tac, E, keywords(F, per_band), 'F %d, T %d, %s, per band %s' % (F, T, layout, per_band), layout=layout)


def test_layouts(tac):
    F, T = 23, 70
    x = R.signal((2, 3, F, T), 5)
    kw = keywords(F, True)
    check_forward(tac, x, kw, 'leading dims (2, 3)')
    check_forward(tac, x[:, 1], kw, 'a channel slice', laid(x, 'frame-major')[:, 1])
    check_forward(tac, x[:, 2], kw, 'a channel slice, time-contiguous', dev(x)[:, 2])
    padded = dev(np.pad(np.swapaxes(x[0], -1, -2), ((0, 0), (0, 5), (0, 3))))
    check_forward(tac, x[0], kw, 'padded rows and frames', padded[:, :T, :F].transpose(-1, -2))
    half = x[0].astype(np.float16)
    check_forward(tac, half.astype(np.float32), kw, 'float16 input', laid(half, 'frame-major'))


@pytest.mark.parametrize('layout', ['frame-major', 'time-contiguous'])
@pytest.mark.parametrize('F', [23, 65])
def test_backward_against_float64_autograd(tac, F, layout):
    tile = sizes(tac)[1]
    for T in (1, tile + 1, 2 * tile + 3):
        E = R.signal((2, F, T), 7 * F + T)
        g = np.random.default_rng(T).standard_normal(E.shape).astype(np.float32)
        params = R.band_params(F, 3)
        want, scale = R.gradients(E, g, params, 1e-6), R.scales(E, g, params, 1e-6)

        def grads(device, wrt_input):
            ins = [(laid(E, layout) if device == 'cuda' else torch.from_numpy(E)).requires_grad_(wrt_input)]
            ins += [torch.from_numpy(p).to(device).requires_grad_(not wrt_input) for p in params]
            out = tac.pcen(ins[0], **dict(zip(NAMES, ins[1:])), eps=1e-6)
            gout = laid(g, layout) if device == 'cuda' else torch.from_numpy(g)
            return torch.autograd.grad(out, ins[:1] if wrt_input else ins[1:], gout)

        got = counted(tac, lambda: grads('cuda', True), {FWD: 1, BWD: 1}) + counted(tac, lambda: grads('cuda', False), {FWD: 1, BWD: 1})
        yard = grads('cpu', True) + grads('cpu', False)
        for name, a, y, w, s in zip(('E',) + NAMES, got, yard, want, scale):
            R.assert_close(a, w, y.numpy(), s, 'grad %s, F %d, T %d, %s' % (name, F, T, layout))


def test_more_units_than_the_grid(tac):
    """2 x grid + 6 units of one row each, every row different: the rows of a workgroup's second and third unit have the bits of the
    same rows run alone, forward and in the gradient of the input"""
    grid = torch.cuda.get_device_properties(0).multi_processor_count * tac._native.lib().tac_pcen_blocks_per_cu()
    rows = 2 * grid + 6
    E = R.signal((rows, 3, 70), 9)
    kw = on(keywords(3, True), 'cuda')
    x, g = laid(E, 'frame-major').requires_grad_(True), dev(np.random.default_rng(1).standard_normal(E.shape).astype(np.float32))
    out = counted(tac, lambda: tac.pcen(x.detach(), **kw), {FWD: 1})
    grad = counted(tac, lambda: torch.autograd.grad(tac.pcen(x, **kw), x, g)[0], {FWD: 1, BWD: 1})
    for i in (0, grid - 1, grid, 2 * grid - 1, 2 * grid, rows - 1):
        alone = x.detach()[i:i + 1].clone().requires_grad_(True)
        assert torch.equal(out[i:i + 1], tac.pcen(alone.detach(), **kw)), 'row %d' % i
        assert torch.equal(grad[i:i + 1], torch.autograd.grad(tac.pcen(alone, **kw), alone, g[i:i + 1])[0]), 'gradient of row %d' % i
    check_forward(tac, E[-3:], keywords(3, True), 'the last rows')


def test_mel_front_end_with_a_trainable_layer_trains_under_strict(tac):
    model = torch.nn.Sequential(*tac.Melspectrogram(num_mels=128, sample_rate=16000, fft_length=2048, hop_length=512),
                                tac.PCEN(n_bands=128, trainable=True)).to('cuda')
    wave = dev(np.random.default_rng(2).standard_normal((2, 1, 16000)).astype(np.float32))
    counted(tac, lambda: model(wave).square().mean().backward(), {'tac_melspec_sparse_f32': 1, FWD: 1, BWD: 1})
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()) for p in model.parameters())


@pytest.mark.parametrize('route', ['float64', 'power', 'bias'])
def test_other_routes_are_announced_and_refused_under_strict(tac, route):
    x = dev(R.signal((2, 5, 40), 4))
    call = {'float64': lambda: tac.pcen(x.double()), 'power': lambda: tac.pcen(x, power=0), 'bias': lambda: tac.pcen(x, bias=0)}[route]
    with pytest.raises(RuntimeError, match='strict mode forbids'):
        call()
    tac.set_strict(False)
    try:
        tac._ops._warned.clear()
        with pytest.warns(tac.CompositeRouteWarning, match='pcen'):
            assert call().shape == x.shape
    finally:
        tac.set_strict(True)
