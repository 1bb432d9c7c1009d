"""-m gpu: ``loudness`` / ``Loudness`` on the gfx950 kernels (csrc/loudness.hip) and ``treble_biquad`` / ``bass_biquad`` on the lfilter
kernel — strict mode and poisoned outputs on, as in tests/test_augment_gpu.py.

Reference and bound: tests/loudness_rules.py — the float64 definition and ``|got - want| <= 2^-24 |want| + (10 / ln 10) rel_E`` per
entry, with every input's margins to both gates asserted on the CPU first.  Every test prints its worst ratio to the bound.  Sizes:
4410 Hz (a block of 1764 samples, a hop of 441: odd, it cuts the lanes' chunks of 16) and 8000 Hz (3200, 800), the lengths around one
block, one hop and one and two tiles of ``T = LOUDNESS_TILE`` samples; 1, 2 and 5 channels; three entries at different levels.  Hops
longer than a wave's 1024 samples (16 and 48 kHz) and than a tile (192 kHz) have a few lengths each.  A reference is computed once
per (rate, channels, length) and shared.

A call is ONE ``tac_loudness_f32`` entry (two launches on the stream behind it); both the result and the float64 bins are poisoned
before the launch and checked after it."""
import warnings

import numpy as np
import pytest
import torch

import lfilter_rules
import loudness_rules as R

pytestmark = pytest.mark.gpu

ENTRY, LFILTER_ENTRY = 'tac_loudness_f32', 'tac_lfilter_f32'
T = R.TILE
RATES = {4410: (1764, 441), 8000: (3200, 800)}


def lengths_of(rate):
    gate, step = RATES[rate]
    return (gate, gate + step - 1, gate + step, T - 1, T, T + 1, 2 * T + step + 1)


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    t._native.lib()
    t.set_strict(True)
    t._hip.set_poison_outputs(True)
    assert t._hip.LOUDNESS_TILE == T == int(t._native.lib().tac_loudness_tile())
    yield t
    t._hip.set_poison_outputs(False)
    t.set_strict(False)
    t.set_lazy_fusion(True)


@pytest.fixture(autouse=True)
def every_output_written(tac):
    tac._hip.poison_report()
    yield
    left = tac._hip.poison_report()
    assert not left, 'kernel outputs left unwritten (poisoned elements per entry point): %r' % left


def launched_since(tac_, before):
    now = tac_._hip.launches
    return {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)}


def dev(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to('cuda')


def run(tac_, x, rate, what):
    """one call: exactly one entry, nothing announced, a float32 tensor of the leading shape"""
    before = dict(tac_._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac_.CompositeRouteWarning)
        got = tac_.loudness(x, rate)
    assert launched_since(tac_, before) == {ENTRY: 1}, what
    assert type(got) is torch.Tensor and got.dtype == torch.float32 and tuple(got.shape) == tuple(x.shape[:-2]), what
    return got


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ----------------------------------------------------------------------------- 1. lengths, channels, levels
@pytest.mark.parametrize('which', range(7))
@pytest.mark.parametrize('channels', [1, 2, 5])
@pytest.mark.parametrize('rate', sorted(RATES))
def test_lengths(tac, rate, channels, which):
    assert R.blocks(rate) == RATES[rate]
    length = lengths_of(rate)[which]
    case = R.levels(rate, channels, length)
    got = run(tac, dev(case.x), rate, case.what)
    R.assert_close(got, case.want, case.bound, case.what)


# ----------------------------------------------------------------------------- 1b. hops longer than a wave, and than a tile
# At 4410 and 8000 Hz every wave (1024 samples) holds a bin edge.  From 16 kHz up a hop is longer than a wave, so most waves hold
# none: their sums are added to what the waves in front hold, and a tile whose last wave holds none carries that sum on.  At
# 192 kHz a hop (19200 samples) is longer than a tile: whole tiles hold no edge.
LONG_HOPS = [(16000, 2, 6400), (16000, 5, 6400 + 1600), (16000, 2, T + 1), (16000, 1, 2 * T + 1600 + 1),
             (48000, 2, 19200), (48000, 1, 19200 + 4800 + 7),
             (192000, 2, 76800), (192000, 1, 76800 + 19200), (192000, 2, 76800 + 2 * 19200 + 1)]


@pytest.mark.parametrize('rate,channels,length', LONG_HOPS)
def test_long_hops(tac, rate, channels, length):
    gate, step = R.blocks(rate)
    assert gate == 4 * step and step > 1024 and length >= gate
    case = R.levels(rate, channels, length)
    x = dev(case.x)
    got = run(tac, x, rate, case.what)
    R.assert_close(got, case.want, case.bound, case.what)
    assert same_bits(got, run(tac, x, rate, case.what)), case.what + ': two calls differ'


# ----------------------------------------------------------------------------- 2. both gates, the clip, run to run
def test_gates_and_clip(tac):
    for case in (R.three_level(), R.loud()):
        x = dev(case.x)
        got = run(tac, x, case.sample_rate, case.what)
        R.assert_close(got, case.want, case.bound, case.what)
        again = tac.Loudness(case.sample_rate)(x)
        assert same_bits(got, again), case.what + ': two calls differ'
    assert R.three_level().x.shape[-1] > T and min(R.three_level().removed) > 0


# ----------------------------------------------------------------------------- 3. layouts
def test_layouts(tac):
    rate, channels = 4410, 2
    case = R.levels(rate, channels, lengths_of(rate)[2])
    x = case.x
    entries, _, length = x.shape
    off = next(o for o in (1, 2, 3) if (length + 8 + o) % 4)              # the first row starts off a 16-byte boundary
    store = torch.full((entries, channels + 2, length + 8), float('nan'), device='cuda')
    store[:, 1:channels + 1, off:length + off] = dev(x)
    sliced = store[:, 1:channels + 1, off:length + off]                 # channel- and time-sliced
    assert sliced.data_ptr() % 16 != 0 and all(s > 0 for s in sliced.stride())
    R.assert_close(run(tac, sliced, rate, 'channel slice'), case.want, case.bound, 'channel slice')
    store = torch.full((entries * channels * (length + 1),), float('nan'), device='cuda')
    late = store.view(entries, channels, length + 1)
    late[..., 1:] = dev(x)
    R.assert_close(run(tac, late[..., 1:], rate, 'time slice'), case.want, case.bound, 'time slice')
    store = torch.full((entries, channels, length + 4), float('nan'), device='cuda')            # 16-byte chunks, padded rows
    store[..., :length] = dev(x)
    R.assert_close(run(tac, store[..., :length], rate, 'padded rows'), case.want, case.bound, 'padded rows')
    nested = dev(np.stack([x, x[::-1]]))                                                        # (2, 3, C, L)
    got = run(tac, nested, rate, 'two leading dimensions')
    R.assert_close(got[0], case.want, case.bound, 'two leading dimensions')
    assert same_bits(got[1], got[0].flip(0))
    one = run(tac, dev(x[0]), rate, '(C, L)')
    assert tuple(one.shape) == () and same_bits(one, got[0, 0])
    before = dict(tac._hip.launches)
    for view in (dev(x[:1]).expand(3, channels, length), dev(x[:, :1]).expand(entries, channels, length)):
        with pytest.raises(RuntimeError, match='non-positive strides'):
            tac.loudness(view, rate)
    empty = tac.loudness(torch.zeros(0, channels, length, device='cuda'), rate)
    assert tuple(empty.shape) == (0,) and launched_since(tac, before) == {}


# ----------------------------------------------------------------------------- 4. the persistent loop
def test_rows_beyond_the_grid(tac):
    rate = 4410
    gate, step = RATES[rate]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = R.wrap_rows(cus)
    grid, _ = R.grid(cus, rows, 1)
    assert rows == 2 * grid + 5 and rows > 2 * grid
    base = R.levels(rate, 1, gate + 3 * step, entries=5)
    small = run(tac, dev(base.x), rate, base.what)
    R.assert_close(small, base.want, base.bound, base.what)
    index = torch.arange(rows) % 5
    big = run(tac, dev(base.x)[index.cuda()].contiguous(), rate, '%d rows on a grid of %d' % (rows, grid))
    assert same_bits(big, small[index.cuda()])
    print('%d rows of %d samples (%.1f MB) on %d workgroups' % (rows, gate + 3 * step, 4e-6 * rows * (gate + 3 * step), grid))


# ----------------------------------------------------------------------------- 5. non-finite samples
def test_a_non_finite_sample_stays_in_its_entry(tac):
    rate = 4410
    case = R.levels(rate, 2, lengths_of(rate)[2], entries=4)
    clean = run(tac, dev(case.x), rate, case.what)
    R.assert_close(clean, case.want, case.bound, case.what)
    x = case.x.copy()
    x[1, 1, 1000] = np.nan
    x[3, 0, 700] = np.inf
    got = run(tac, dev(x), rate, 'NaN and inf')
    assert bool(torch.isnan(got[1])) and bool(torch.isnan(got[3])), got
    assert same_bits(got[[0, 2]], clean[[0, 2]])
    assert bool(torch.isnan(run(tac, torch.zeros(2, 1, 2000, device='cuda'), rate, 'silence')).all())


# ----------------------------------------------------------------------------- 6. routes
def test_routes(tac):
    rate = 4410
    gate, step = RATES[rate]
    case = R.levels(rate, 2, gate)
    odd = R.levels(11025, 2, 4410 + 1102)
    x, xo = dev(case.x), dev(odd.x)
    before = dict(tac._hip.launches)
    with pytest.raises(RuntimeError, match='dtype float64'):
        tac.loudness(x.double(), rate)
    with pytest.raises(RuntimeError, match='not four hops'):
        tac.loudness(xo, 11025)
    assert launched_since(tac, before) == {}
    xg = x.clone().requires_grad_(True)
    y = tac.loudness(xg, rate)
    assert launched_since(tac, before) == {ENTRY: 1}
    with pytest.raises(RuntimeError, match='backward: the op has no gradient kernel'):
        y.sum().backward()
    limit32, limit_odd = R.f32_bound(case.x, rate, case.want), R.f32_bound(odd.x, 11025, odd.want)
    assert min(case.margins) > 2.0 * float(limit32.max()) and min(odd.margins) > 2.0 * float(limit_odd.max())

    def forget():
        for key in [k for k in tac._ops._warned if k[0] == 'loudness']:
            tac._ops._warned.discard(key)

    tac.set_strict(False)
    try:
        for xin, r, want, limit, what in ((x.double(), rate, case.want, 1e-9, 'float64'), (xo, 11025, odd.want, limit_odd, '11025 Hz')):
            forget()
            before = dict(tac._hip.launches)
            with pytest.warns(tac.CompositeRouteWarning):
                got = tac.loudness(xin, r)
            assert got.dtype == xin.dtype and launched_since(tac, before) == {}
            R.assert_close(got, want, limit, 'stock-torch route, ' + what)
        forget()
        xg = x.clone().requires_grad_(True)
        y = tac.loudness(xg, rate)
        R.assert_close(y.detach(), case.want, case.bound, 'forward in front of the backward')
        before = dict(tac._hip.launches)
        with pytest.warns(tac.CompositeRouteWarning):
            y.sum().backward()
        assert launched_since(tac, before) == {}
        # the gradient of the float64 definition, by the CPU route; the float32 re-evaluation sums `gate` float32 terms per block
        # (loudness_rules.f32_bound): (gate + 16) 2^-24 of the largest element, with a factor 8 for the chain of adjoint sums
        x64 = torch.from_numpy(case.x).double().requires_grad_(True)
        tac.loudness(x64, rate).sum().backward()
        err = float((xg.grad.cpu().double() - x64.grad).abs().max())
        limit = 8.0 * (gate + 16) * 2.0 ** -24 * float(x64.grad.abs().max())
        print('gradient by the stock-torch route: |err| %.3g, limit %.3g' % (err, limit))
        assert err <= limit
    finally:
        tac.set_strict(True)


# ----------------------------------------------------------------------------- 7. the two shelving biquads
@pytest.mark.parametrize('name', ['treble_biquad', 'bass_biquad'])
def test_shelf_biquads(tac, name):
    x = lfilter_rules.waveform((3, T + 37), seed=11) * np.float32(0.4)
    closed = R.treble_closed_form if name == 'treble_biquad' else R.bass_closed_form
    for args in ((16000, 4.0, 1500.0, 1.0 / np.sqrt(2.0)), (48000, -6.0, 100.0, 0.707)):
        before = dict(tac._hip.launches)
        with warnings.catch_warnings():
            warnings.simplefilter('error', tac.CompositeRouteWarning)
            got = getattr(tac.functional, name)(dev(x), *args)
        assert launched_since(tac, before) == {LFILTER_ENTRY: 1}
        b, a = closed(*args)
        ref, bound = lfilter_rules.reference(x, b, a, clamp=True)
        ratio = lfilter_rules.assert_close(got, ref, bound, '%s %r' % (name, args))
        print('%s %r: worst |err| / bound %.3g' % (name, args, ratio))
