"""-m gpu: ``oscillator_bank`` / ``filter_waveform`` and their gradients on the gfx950 kernels of csrc/ddsp.hip — strict mode and
poisoned outputs on, every element checked against tests/ddsp_rules.py, one counted entry per forward and per backward call.  The
shapes are the smallest that reach each boundary of a kernel, from the library's own constants."""
import warnings

import numpy as np
import pytest
import torch

import ddsp_rules as R

pytestmark = pytest.mark.gpu

OSC, OSC_GRAD = 'tac_oscbank_f32', 'tac_oscbank_grad_f32'
FW, FW_GRAD = 'tac_filter_waveform_f32', 'tac_filter_waveform_grad_kernels_f32'
SR = 8000.0
dev = R.dev


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    h, H = t._native.lib(), t._hip
    t.set_strict(True)
    H.set_poison_outputs(True)
    assert h.tac_filter_waveform_max_taps() == H.FILTER_WAVEFORM_MAX_TAPS >= 513
    yield t
    H.set_poison_outputs(False)
    t.set_strict(False)


@pytest.fixture(autouse=True)
def every_output_written(tac):
    tac._hip.poison_report()
    yield
    left = tac._hip.poison_report()
    assert not left, 'kernel outputs left unwritten (poisoned elements per entry point): %r' % left


def counted(tac_, expect, fn, *args):
    """``fn(*args)`` on the kernel route: no announcement, exactly the launches ``expect``"""
    before = dict(tac_._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac_.CompositeRouteWarning)
        got = fn(*args)
    now = tac_._hip.launches
    assert {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)} == expect
    return got


def both_ways(tac_, forward, backward, fn, tensors, g):
    """(result, gradients of ``tensors``) of one forward and one backward call on the kernel route"""
    leaves = [t.detach().requires_grad_(True) for t in tensors]
    out = counted(tac_, forward, fn, *leaves)
    assert out.dtype == torch.float32 and out.is_contiguous()
    counted(tac_, backward, out.backward, g)
    return (out.detach(),) + tuple(leaf.grad for leaf in leaves)


# ============================================================================= oscillator_bank
def osc_inputs(rows, time, n, seed):
    """cells at and beyond +-Nyquist, oscillator 0 negative throughout, the last one masked throughout (from three on)"""
    r = np.random.default_rng(seed)
    f = (r.uniform(-0.45, 0.45, (rows, time, n)) * SR).astype(np.float32)
    f[..., 0] = -np.abs(f[..., 0])
    special = np.array([SR / 2, -SR / 2, 0.7 * SR, -0.9 * SR, 3.5 * SR], np.float32)
    at = r.integers(0, time, 5), r.integers(0, n, 5)
    f[0, at[0], at[1]] = special
    if n >= 3:
        f[..., n - 1] = 0.6 * SR
    return f, r.standard_normal((rows, time, n)).astype(np.float32)


def osc_check(tac_, f, a, reduction, seed, what):
    """forward and both gradients of rows 1 and all, every element; returns the worst ratio"""
    g = np.random.default_rng(seed).standard_normal(f.shape if reduction == 'none' else f.shape[:-1]).astype(np.float32)
    ref = R.oscillator_bank(f, a, SR, reduction, g)
    worst = 0.0
    for rows in sorted(set([1, f.shape[0]])):
        y, df, da = both_ways(tac_, {OSC: 1}, {OSC_GRAD: 1}, lambda u, v: tac_.oscillator_bank(u, v, SR, reduction),
                              (dev(f[:rows]), dev(a[:rows])), dev(g[:rows]))
        for got, k, name in ((y, 0, 'y'), (da, 2, 'd a'), (df, 4, 'd f')):
            worst = max(worst, R.assert_close(got, ref[k][:rows], ref[k + 1][:rows], '%s of %s, %d rows' % (name, what, rows)))
    return worst


@pytest.mark.parametrize('reduction', ['sum', 'mean', 'none'])
def test_oscillator_bank_every_length_and_width(tac, reduction):
    H = tac._hip
    c, tile, span = H.OSCBANK_CHUNK, H.OSCBANK_TILE, H.OSCBANK_SPAN
    shapes = [(t, n) for t in (1, 2, c - 1, c + 1, tile - 1, tile, tile + 1, 2 * tile + 5) for n in (1, 2, 3, 16, 17, 64, 65, 100)]
    shapes += [(span + 1, 3), (2 * span + 5, 17)]               # rows cut into spans: the two- and three-launch forms
    worst = 0.0
    for time, n in shapes:
        f, a = osc_inputs(3, time, n, seed=time * 131 + n)
        worst = max(worst, osc_check(tac, f, a, reduction, time + n, '(%d, %d) %s' % (time, n, reduction)))
    print('oscillator_bank %s: worst |err| / bound %.3f' % (reduction, worst))
    layer = tac.OscillatorBank(SR, reduction)
    assert torch.equal(layer(dev(f), dev(a)), tac.oscillator_bank(dev(f), dev(a), SR, reduction))


def test_oscillator_bank_wraps_across_64_tiles(tac):
    time = 64 * tac._hip.OSCBANK_TILE
    f = np.full((1, time, 2), 0.499 * SR, np.float32)
    a = np.random.default_rng(5).standard_normal(f.shape).astype(np.float32)
    for reduction in ('sum', 'none'):           # (forward: d f's float64 suffix sum is bounded to 8000 steps, ddsp_rules)
        got = counted(tac, {OSC: 1}, tac.oscillator_bank, dev(f), dev(a), SR, reduction)
        ratio = R.assert_close(got, *R.oscillator_bank(f, a, SR, reduction), 'near Nyquist, %s' % reduction)
        print('oscillator_bank %s at 0.499 sample_rate over %d steps: worst |err| / bound %.3f' % (reduction, time, ratio))


def test_oscillator_bank_layouts(tac):
    """time-contiguous tensors, unaligned starts and slices of wider tensors are read where they lie: bit-identical to dense"""
    f, a = osc_inputs(3, tac._hip.OSCBANK_TILE + 3, 17, seed=77)
    g = dev(np.random.default_rng(3).standard_normal(f.shape[:-1]).astype(np.float32))
    run = lambda u, v: both_ways(tac, {OSC: 1}, {OSC_GRAD: 1}, lambda p, q: tac.oscillator_bank(p, q, SR, 'sum'), (u, v), g)
    dense = run(dev(f), dev(a))

    def time_major(x):
        return dev(x.transpose(0, 2, 1)).transpose(1, 2)

    def offset(x):
        store = torch.full((x.size + 1,), float('nan'), device='cuda')
        store[1:] = dev(x).reshape(-1)
        assert store[1:].data_ptr() % 16 == 4
        return store[1:].view(x.shape)

    def sliced(x):
        wide = torch.full((x.shape[0], x.shape[1] + 2, x.shape[2] + 3), float('nan'), device='cuda')
        wide[:, 1:-1, 2:-1] = dev(x)
        return wide[:, 1:-1, 2:-1]

    for view in (time_major, offset, sliced):
        u, v = view(f), view(a)
        assert u.data_ptr() != dev(f).data_ptr() and (view is offset or not u.is_contiguous())
        for got, want in zip(run(u, v), dense):
            assert torch.equal(got, want), view.__name__


def test_oscillator_bank_row_alone_equals_row_in_batch(tac):
    """a batch that fills the device walks each row in one span, a row alone in three: the same bits"""
    rows = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    time = 2 * tac._hip.OSCBANK_SPAN + 5
    f, a = osc_inputs(1, time, 3, seed=11)
    fb, ab = dev(np.repeat(f, rows, 0)), dev(np.repeat(a, rows, 0))
    fb[1:] *= 0.5
    assert tac._native.lib().tac_oscbank_spans(rows, time) == 1 and tac._native.lib().tac_oscbank_spans(1, time) == 3
    for reduction in ('sum', 'none'):
        alone = counted(tac, {OSC: 1}, tac.oscillator_bank, dev(f), dev(a), SR, reduction)
        batch = counted(tac, {OSC: 1}, tac.oscillator_bank, fb, ab, SR, reduction)
        assert torch.equal(alone[0], batch[0]), reduction
        assert torch.equal(alone, counted(tac, {OSC: 1}, tac.oscillator_bank, dev(f), dev(a), SR, reduction))


# ============================================================================= filter_waveform
def fw_cases(tac_):
    tile, taps, piece = tac_._hip.FILTER_WAVEFORM_TILE, tac_._hip.FILTER_WAVEFORM_MAX_TAPS, tac_._hip.FILTER_WAVEFORM_PIECE
    return [(37, 1, 4, -1), (10, 4, 1, -1), (10, 4, 3, 0), (5, 4, 3, 2), (40, 10, 7, -1), (35, 5, 7, 6), (100, 3, 8, -1), (6, 6, 3, -1),
            (tile + 1, 3, taps, -1), (tile - 1, 1, taps, taps - 1), (2 * tile + 5, 7, 513, 0), (2 * piece + 100, 1, 5, -1)]


@pytest.mark.parametrize('kind', ['shared', 'per row', 'size-1 channel'])
def test_filter_waveform_and_gradients(tac, kind):
    worst = 0.0
    for T, F, K, delay in fw_cases(tac):
        r = np.random.default_rng(T * 7 + F + K)
        x = r.standard_normal((4, T)).astype(np.float32)
        g = r.standard_normal((4, T)).astype(np.float32)
        h = r.standard_normal((F, K) if kind == 'shared' else (2, 1, F, K) if kind == 'size-1 channel' else (4, F, K)).astype(np.float32)
        if kind == 'size-1 channel':            # (batch 2, channel 2) rows: the reference sees the channels' filters repeated
            ref = list(R.filter_waveform(x, np.repeat(h[:, 0], 2, 0), delay, g, tac._hip.FILTER_WAVEFORM_PIECE, share=2))
            ref[4], ref[5] = (v.reshape(2, 2, F, K).sum(1, keepdims=True) for v in ref[4:6])
            xt, gt = dev(x.reshape(2, 2, T)), dev(g.reshape(2, 2, T))
            shape = (2, 2, T)
        else:
            ref = R.filter_waveform(x, h, delay, g, tac._hip.FILTER_WAVEFORM_PIECE)
            xt, gt, shape = dev(x), dev(g), (4, T)
        y, dx, dh = both_ways(tac, {FW: 1}, {FW: 1, FW_GRAD: 1}, lambda u, v: tac.filter_waveform(u, v, delay), (xt, dev(h)), gt)
        for got, k, name in ((y, 0, 'y'), (dx, 2, 'd x'), (dh, 4, 'd h')):
            want, bound = (ref[k], ref[k + 1]) if name == 'd h' else (ref[k].reshape(shape), ref[k + 1].reshape(shape))
            worst = max(worst, R.assert_close(got, want, bound, '%s of %r %s' % (name, (T, F, K, delay), kind)))
    print('filter_waveform %s: worst |err| / bound %.3f' % (kind, worst))
    assert torch.equal(tac.FilterWaveform(delay)(xt, dev(h)), tac.filter_waveform(xt, dev(h), delay))


def test_filter_waveform_row_alone_equals_row_in_batch(tac):
    T = tac._hip.FILTER_WAVEFORM_TILE + 9
    r = np.random.default_rng(4)
    x, h = dev(r.standard_normal((3, T)).astype(np.float32)), dev(r.standard_normal((3, 5, 33)).astype(np.float32))
    batch = counted(tac, {FW: 1}, tac.filter_waveform, x, h)
    alone = counted(tac, {FW: 1}, tac.filter_waveform, x[1:2], h[1:2])
    assert torch.equal(alone[0], batch[1]) and torch.equal(batch, counted(tac, {FW: 1}, tac.filter_waveform, x, h))


# ============================================================================= routing
@pytest.mark.parametrize('why', ['float64', 'float16', 'taps'])
def test_composite_route_is_announced_and_strict_refuses(tac, why):
    dtype = {'float64': torch.float64, 'float16': torch.float16}.get(why, torch.float32)
    K = tac._hip.FILTER_WAVEFORM_MAX_TAPS + 1 if why == 'taps' else 5
    calls = [lambda: tac.filter_waveform(torch.randn(2, 900, device='cuda', dtype=dtype), torch.randn(3, K, device='cuda', dtype=dtype))]
    if why != 'taps':
        calls.append(lambda: tac.oscillator_bank(torch.rand(2, 9, 3, device='cuda', dtype=dtype) * 100,
                                                 torch.rand(2, 9, 3, device='cuda', dtype=dtype), SR))
    for call in calls:
        before = dict(tac._hip.launches)
        with pytest.raises(RuntimeError, match='strict mode'):
            call()
        tac.set_strict(False)
        try:
            tac._ops._warned.clear()
            with pytest.warns(tac.CompositeRouteWarning):
                out = call()
        finally:
            tac.set_strict(True)
        assert out.dtype == dtype and {k: v for k, v in tac._hip.launches.items() if k in (OSC, FW)} == {
            k: v for k, v in before.items() if k in (OSC, FW)}
