"""-m gpu: the tables ``_hip.cached_on`` hangs on a window / filterbank / coefficient tensor, on the routes a CPU tensor cannot
take.  Strict mode and poisoned outputs are on (as in tests/test_gpu_parity.py).

Every route goes through the same four steps (``follow``): run it; write to the constant tensor in place; run it again and
compare — ``torch.equal`` — with the same call on a freshly made tensor of the new contents; run it once more and find the very
same object in each slot.  The shapes are the smallest that take each route; the CPU side of the mechanism is
tests/test_convolve_cpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    t._native.lib()
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


def rand(shape, seed):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1).cuda()


def follow(tac, run, constant, write, slots):
    """The four steps for one route.  ``run(constant)`` returns a tuple of tensors; ``slots`` are the ``_tac_*`` names the route
    fills on ``constant``.  Returns {slot: its table dict} as the last run left it."""
    H = tac._hip
    first = run(constant)
    assert all(hasattr(constant, s) for s in slots), [s for s in slots if not hasattr(constant, s)]
    write(constant)
    second = run(constant)
    fresh = run(constant.clone())
    for a, b, c in zip(second, fresh, first):
        assert torch.equal(a, b) and not torch.equal(a, c)
    held = {s: getattr(constant, s) for s in slots}
    tables = {s: dict(held[s][1]) for s in slots}
    assert all(held[s][0] == H._stamp(constant) for s in slots)
    third = run(constant)
    for a, b in zip(third, second):
        assert torch.equal(a, b)
    for s in slots:
        assert getattr(constant, s) is held[s], s
        assert list(held[s][1]) == list(tables[s]) and all(held[s][1][k] is tables[s][k] for k in tables[s]), s
    return tables


def double(t):
    t.mul_(2.0)


@pytest.mark.parametrize('n_fft', [100, 102])
def test_stft_and_its_gradient_follow_the_window(tac, n_fft):
    """fft_length 102 (half of it 3 x 17) is the DFT-matrix route, forward and gradient: ``_tac_dft`` and ``_tac_dftT``, one matrix
    each.  fft_length 100 (half of it 2 x 5 x 5) has a frame kernel of its own and reads the window itself: the same steps, no
    table."""
    H = tac._hip
    x = rand((2, 1, 2000), 1)
    go = rand((2, 1, n_fft // 2 + 1, 81, 2), 2)
    by_matrix = not H.smooth_fft_size(n_fft)
    assert by_matrix == (n_fft == 102)                                      # (the DFT-matrix route stays covered)
    ran = {}

    def run(window):
        wave = x.clone().requires_grad_()
        before = dict(H.launches)
        y = tac.stft(wave, n_fft, 25, window=window)
        (gx,) = torch.autograd.grad(y, wave, go)
        ran.update({k: v for k, v in H.launches.items() if v != before.get(k, 0)})
        return y.detach(), gx
    window = torch.hann_window(n_fft).cuda()
    tables = follow(tac, run, window, double, ('_tac_dft', '_tac_dftT') if by_matrix else ())
    assert ('tac_stft_f32' in ran) != by_matrix and ('tac_stft_backward_f32' in ran) != by_matrix, ran
    if by_matrix:
        assert list(tables['_tac_dft']) == [(n_fft, n_fft, True, False)] and list(tables['_tac_dftT']) == [(n_fft, n_fft, False)]
        assert tables['_tac_dft'][(n_fft, n_fft, True, False)].shape == (n_fft, 2 * (n_fft // 2 + 1))
        tac.stft(x, n_fft + 2, 25, win_length=n_fft, window=window)                      # another geometry on this one ...
        assert list(window._tac_dft[1]) == [(n_fft + 2, n_fft, True, False)]             # ... takes the first one's place


def test_istft_follows_the_window_and_rechecks_nola(tac):
    spec = rand((2, 1, 33, 9, 2), 3)

    def run(window):
        return (tac.istft(spec, 64, 16, window=window),)
    window = torch.hann_window(64).cuda()
    tables = follow(tac, run, window, double, ('_tac_istft',))
    (entry,) = tables['_tac_istft'].values()
    assert list(tables['_tac_istft']) == [(64, 16, 64, True, 9)] and entry[0].shape == (16 * 8 + 64,) and entry[1] == {128}
    window.zero_()
    with pytest.raises(RuntimeError, match='does not satisfy the NOLA condition'):
        run(window)
    with pytest.raises(RuntimeError, match='does not satisfy the NOLA condition'):      # (a failed check is not remembered as passed)
        run(window)


@pytest.mark.parametrize('bank', ['triangular', 'dense', 'dense_wide'])
def test_filterbank_tables_follow_the_bank(tac, bank):
    """A triangular (33, 8) bank streams through the band-sparse kernel and its per-bin adjoint table.  A dense (33, 8) bank has no
    adjoint table (more than two weights per bin: ``None``, kept as a result) and goes back through the GEMM with its transpose;
    it is small enough for the library to pack all the same.  A dense (257, 24) bank — 24 x 264 weights, over the 3072 the
    band-sparse kernels hold — has no pack either: ``None`` under key 0, and the GEMM with its tile plan forward."""
    H = tac._hip
    n_freqs, n_mels = (257, 24) if bank == 'dense_wide' else (33, 8)
    spec0 = rand((2, 16, n_freqs), 4).abs().transpose(-2, -1)               # frame-major, as the spectrogram kernels return it
    go = rand((2, n_mels, 16), 5)
    ran = []

    def run(fb):
        spec = spec0.detach().requires_grad_()
        before = dict(H.launches)
        y = tac.apply_filterbank(spec, fb)
        (gs,) = torch.autograd.grad(y, spec, go)
        ran.append({k: v - before.get(k, 0) for k, v in H.launches.items() if v != before.get(k, 0)})
        return y.detach(), gs
    if bank == 'triangular':
        fb = tac.create_mel_filter(n_freqs, n_mels, 0.0, 8000.0, False).cuda()
        slots = ('_tac_pack', '_tac_adj')
    else:
        fb = rand((n_freqs, n_mels), 6).abs() + 0.1
        slots = ('_tac_pack', '_tac_T', '_tac_adj') + (('_tac_plan',) if bank == 'dense_wide' else ())
    first = run(fb)
    assert list(fb._tac_pack[1]) == [0] and list(fb._tac_adj[1]) == [()]
    assert (fb._tac_pack[1][0] is None) == (bank == 'dense_wide')           # the negative results are IN the slots, under their keys
    assert (fb._tac_adj[1][()] is None) == (bank != 'triangular')
    if bank == 'triangular':
        assert ran[-1] == {'tac_apply_filterbank_sparse_f32': 1, 'tac_apply_filterbank_adjoint_f32': 1}, ran[-1]
    elif bank == 'dense_wide':
        assert ran[-1] == {'tac_apply_filterbank_f32': 2}, ran[-1]
    else:
        assert ran[-1].get('tac_apply_filterbank_f32', 0) >= 1 and 'tac_apply_filterbank_adjoint_f32' not in ran[-1], ran[-1]
    pack, adj = fb._tac_pack, fb._tac_adj
    again = run(fb)
    assert fb._tac_pack is pack and fb._tac_adj is adj and len(pack[1]) == 1 and len(adj[1]) == 1       # untouched by the second call
    assert ran[-1] == ran[-2] and torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    tables = follow(tac, run, fb, double, slots)
    if bank != 'triangular':
        assert tables['_tac_adj'] == {(): None} and torch.equal(tables['_tac_T'][()], fb.t())
    if bank == 'dense_wide':
        assert tables['_tac_pack'] == {0: None} and list(tables['_tac_plan']) == [fb.device]


def test_lfilter_follows_device_coefficients(tac):
    x = rand((2, 300), 7) * 0.1
    a = torch.tensor([1.0, -0.5, 0.25]).cuda()

    def run(b):
        return (tac.lfilter(x, a, b),)
    b = torch.tensor([0.5, 0.25, -0.125]).cuda()
    tables = follow(tac, run, b, double, ('_tac_coef',))
    assert tables['_tac_coef'] == {(): (1.0, 0.5, -0.25)} and a._tac_coef[1] == {(): (1.0, -0.5, 0.25)}


def test_time_stretch_rereads_phase_advance(tac):
    H = tac._hip
    x = rand((2, 88), 8)                                                    # -> a (2, 17, 12, 2) spectrogram
    stft, norm = tac.STFT(32, 8).cuda(), tac.ComplexNorm(2.0)
    ran = []

    def run(pa):
        ts = tac.TimeStretch(8, 17, fixed_rate=1.3).cuda()
        ts.phase_advance = pa
        before = dict(H.launches)
        y = tac.realize(norm(ts(stft(x))))
        ran.append({k for k, v in H.launches.items() if v != before.get(k, 0)})
        return (y,)
    pa = tac.TimeStretch(8, 17).cuda().phase_advance
    (y0,) = run(pa)
    assert tuple(y0.shape) == (2, 17, 10) and pa._tac_finite[1] == {(): True} and 'tac_stretch_norm_f32' in ran[-1]
    slot = pa._tac_finite
    run(pa)
    assert pa._tac_finite is slot
    pa[3] = float('inf')                                                    # in place: the next call reads the table back again
    (y1,) = run(pa)
    assert pa._tac_finite[1] == {(): False} and 'tac_phase_vocoder_f32' in ran[-1] and 'tac_stretch_norm_f32' not in ran[-1]
    (fresh,) = run(pa.clone())
    assert torch.equal(y1.view(torch.int32), fresh.view(torch.int32))       # (bit for bit: bin 3 is NaN in both)
    nan = torch.isnan(y1)
    assert bool(nan[:, 3, 1:].all()) and not bool(nan[:, :3].any()) and not bool(nan[:, 4:].any())   # bins are independent
    slot = pa._tac_finite
    run(pa)
    assert pa._tac_finite is slot
