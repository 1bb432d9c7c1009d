"""-m gpu: ``overdrive`` / ``phaser`` / ``flanger`` on the gfx950 kernels of csrc/sox_effects.hip — strict mode and poisoned outputs
on, every element checked, one launch of the entry per forward call.

References and bounds: tests/sox_rules.py (the literal float64 loops; per element ``2^-24 |raw| + 2^-40 mass + 2^-126``).  The LFOs
are short (``sample_rate = 8000``; ``mod_speed = 2``: ``P = 4000``, ``speed = 10``: ``P = 800``) so that rows of a few tiles wrap them
and cross tile boundaries at other phases.  The lengths are the smallest that reach each boundary of a kernel, from the library's
own constants."""
import warnings

import numpy as np
import pytest
import torch

import sox_rules as R

pytestmark = pytest.mark.gpu

OVERDRIVE, PHASER, FLANGER = 'tac_overdrive_f32', 'tac_phaser_f32', 'tac_flanger_f32'
dev = R.dev


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    h = t._native.lib()
    t.set_strict(True)
    t._hip.set_poison_outputs(True)
    H = t._hip
    assert (h.tac_overdrive_tile(), h.tac_phaser_tile(), h.tac_flanger_tile(), h.tac_flanger_chunk(), h.tac_flanger_max_block()) == (
        H.OVERDRIVE_TILE, H.PHASER_TILE, H.FLANGER_TILE, H.FLANGER_CHUNK, H.FLANGER_MAX_BLOCK)
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


def run(tac_, entry, fn, xt, *args, **kw):
    """one forward call on the kernel route: no announcement, exactly one launch of ``entry``"""
    before = dict(tac_._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac_.CompositeRouteWarning)
        got = fn(xt, *args, **kw)
    assert launched_since(tac_, before) == {entry: 1}, (entry, args, kw)
    assert type(got) is torch.Tensor and got.dtype == torch.float32 and got.is_contiguous() and got.shape == xt.shape
    return got


def grid_of(tac_, per_cu):
    return per_cu * torch.cuda.get_device_properties(0).multi_processor_count


# ============================================================================= overdrive
def overdrive_lengths(tac_):
    c, tile = tac_._hip.LFILTER_C, tac_._hip.OVERDRIVE_TILE
    return sorted(set([1, 2, 3, c - 1, c, c + 1, 64 * c - 1, 64 * c + 1, tile - 1, tile, tile + 1, 2 * tile + 5]))


def test_overdrive_every_length_boundary(tac):
    worst = 0.0
    for length in overdrive_lengths(tac):
        x = R.waveform((3, length), seed=300 + length, scale=0.3)
        ref, bound, _ = R.overdrive(x, 20, 20)
        for rows in (1, 3):
            got = run(tac, OVERDRIVE, tac.overdrive, dev(x[:rows]), 20, 20)
            worst = max(worst, R.assert_close(got, ref[:rows], bound[:rows], '%d rows of %d' % (rows, length)))
    print('overdrive lengths: worst |err| / bound %.3f' % worst)


@pytest.mark.parametrize('gain, colour, scale', [(0, 0, 4.0), (0, 100, 4.0), (100, 0, 1e-5), (100, 100, 1.0), (20, 20, 0.3)])
def test_overdrive_parameter_corners(tac, gain, colour, scale):
    x = R.waveform((3, tac._hip.OVERDRIVE_TILE + 37), seed=91, scale=scale)
    if scale == 4.0:
        x[1, ::2] = np.abs(x[1, ::2])           # a row whose 0.5 x + 0.75 v leaves [-1, 1] on one side for long stretches
    ref, bound, _ = R.overdrive(x, gain, colour)
    g, c = R.overdrive_constants(gain, colour)
    t = g * x.astype(np.float64) + c
    if scale != 1.0:
        assert (t < -1).any() and (t > 1).any() and (np.abs(t) < 1).any(), 'all three shaping branches'
    if scale == 4.0:
        raw = R.overdrive_literal(x, gain, colour)[0]
        assert (raw > 1).any() and (raw < -1).any(), 'the clamp acts'
    ratio = R.assert_close(run(tac, OVERDRIVE, tac.overdrive, dev(x), gain, colour), ref, bound, 'gain %r colour %r' % (gain, colour))
    print('overdrive gain %r colour %r: worst |err| / bound %.3f' % (gain, colour, ratio))
    layer = tac.Overdrive(gain, colour)
    assert torch.equal(run(tac, OVERDRIVE, layer, dev(x)), run(tac, OVERDRIVE, tac.overdrive, dev(x), gain, colour))


def layouts(x, channel_axis):
    """``(what, view)``: device views of ``x`` (rows, …, length) — unaligned row starts, padded aligned rows, a slice along
    ``channel_axis`` of a wider tensor, the dense tensor"""
    length = x.shape[-1]
    for offset in (1, 2, 3):
        store = torch.full(x.shape[:-1] + (length + 6,), float('nan'), device='cuda')
        store[..., offset:length + offset] = dev(x)
        view = store[..., offset:length + offset]
        assert view.data_ptr() % 16 == 4 * offset
        yield 'offset %d' % offset, view
    pad = (-length) % 4 + 4
    store = torch.full(x.shape[:-1] + (length + pad,), float('nan'), device='cuda')
    store[..., :length] = dev(x)
    view = store[..., :length]
    assert view.data_ptr() % 16 == 0 and view.stride(-2) % 4 == 0 and view.stride(-2) > length
    yield 'padded aligned rows', view
    shape = list(x.shape)
    shape[channel_axis] += 2
    wide = torch.full(shape, float('nan'), device='cuda')
    wide.narrow(channel_axis, 1, x.shape[channel_axis]).copy_(dev(x))
    yield 'channel slice', wide.narrow(channel_axis, 1, x.shape[channel_axis])
    yield 'dense', dev(x)


def test_overdrive_layouts(tac):
    for length in (tac._hip.OVERDRIVE_TILE + 1, 1029):
        x = R.waveform((2, 3, length), seed=length, scale=0.3)
        ref, bound, _ = R.overdrive(x, 20, 20)
        for what, view in layouts(x, 1):
            R.assert_close(run(tac, OVERDRIVE, tac.overdrive, view, 20, 20), ref, bound, '%s of %d' % (what, length))


def contained(tac_, entry, fn, x, at, args, kw=None, bad=float('nan')):
    """a non-finite sample at the flat row ``1`` position ``at`` leaves the other rows and its own earlier samples bit-identical"""
    kw = kw or {}
    clean = run(tac_, entry, fn, dev(x), *args, **kw)
    assert torch.equal(clean, run(tac_, entry, fn, dev(x), *args, **kw)), 'run-to-run bit identity'
    length = x.shape[-1]
    one = run(tac_, entry, fn, dev(x.reshape(-1, length)[1].reshape((1,) * (x.ndim - 1) + (length,))), *args, **kw)
    if x.ndim == 2:                             # (a flanger row alone is channel 0: only rows of channel 0 are comparable)
        assert torch.equal(one.reshape(-1), clean.reshape(-1, length)[1]), 'alone as inside the batch'
    y = x.copy()
    y.reshape(-1, length)[1, at] = bad
    got = run(tac_, entry, fn, dev(y), *args, **kw).reshape(-1, length)
    flat = clean.reshape(-1, length)
    others = [r for r in range(flat.shape[0]) if r != 1]
    assert torch.equal(got[others], flat[others]), 'the other rows'
    assert torch.equal(got[1, :at], flat[1, :at]), 'the row itself before the sample'
    assert not bool(torch.isfinite(got[1, at]))


def test_overdrive_containment_and_bit_identity(tac):
    x = R.waveform((3, 2 * tac._hip.OVERDRIVE_TILE + 5), seed=92, scale=0.3)
    contained(tac, OVERDRIVE, tac.overdrive, x, tac._hip.OVERDRIVE_TILE + 7, (20, 20))


def beyond_the_grid(tac_, entry, fn, base, rows, args, kw, reference):
    ref, bound, _ = reference(base)
    few = run(tac_, entry, fn, dev(base), *args, **kw)
    R.assert_close(few, ref, bound, 'the base rows')
    reps = (rows + base.shape[0] - 1) // base.shape[0]
    many = dev(base).repeat((reps,) + (1,) * (base.ndim - 1))[:rows]
    got = run(tac_, entry, fn, many, *args, **kw)
    assert torch.equal(got, few.repeat((reps,) + (1,) * (base.ndim - 1))[:rows])


def test_overdrive_rows_beyond_the_grid(tac):
    grid = grid_of(tac, tac._native.lib().tac_overdrive_blocks_per_cu())
    base = R.waveform((5, 301), seed=93, scale=0.3)
    beyond_the_grid(tac, OVERDRIVE, tac.overdrive, base, 2 * grid + 5, (20, 20), {}, lambda b: R.overdrive(b, 20, 20))


def test_overdrive_gradient_under_strict(tac):
    length = tac._hip.OVERDRIVE_TILE + 37
    for gain, colour, scale in ((20, 20, 0.3), (0, 0, 2.0)):
        x_np = R.waveform((3, length), seed=94, scale=scale)
        gy = R.waveform((3, length), seed=95)
        want, mass, raw = R.overdrive_gradient(x_np, gy, gain, colour)
        _, fb, _ = R.overdrive(x_np, gain, colour)
        decided = np.abs(np.abs(raw) - 1.0) > fb             # no reference value sits where rounding decides the clamp's mask
        if scale == 2.0:
            assert (np.abs(raw) > 1).any()
        assert decided.mean() > 0.99
        # the CPU route's float64 gradient is the yardstick the rules' closed form is held to first
        xc = torch.from_numpy(x_np.astype(np.float64)).requires_grad_(True)
        (gc,) = torch.autograd.grad(tac.overdrive(xc, gain, colour), xc, grad_outputs=torch.from_numpy(gy.astype(np.float64)))
        assert np.abs(gc.numpy() - want)[decided].max() <= 1e-11 * mass.max()
        x = dev(x_np).requires_grad_(True)
        before = dict(tac._hip.launches)
        with warnings.catch_warnings():
            warnings.simplefilter('error', tac.CompositeRouteWarning)
            y = tac.overdrive(x, gain, colour)
            (gx,) = torch.autograd.grad(y, x, grad_outputs=dev(gy))
        assert launched_since(tac, before) == {OVERDRIVE: 1, 'tac_lfilter_f32': 1}
        ratio = R.assert_close(gx.cpu().numpy()[decided], want[decided], R.bound32(mass)[decided], 'gradient')
        print('overdrive gradient, gain %r: worst |err| / bound %.3f' % (gain, ratio))


# ============================================================================= phaser
def phaser_kw(delay_ms, decay, sinusoidal=True, **more):
    return dict(dict(sample_rate=8000, mod_speed=2.0, delay_ms=delay_ms, decay=decay, sinusoidal=sinusoidal), **more)


@pytest.mark.parametrize('delay_ms, decay, sinusoidal', [(0.25, 0.99, True), (5.0, 0.4, False)])
def test_phaser_every_length_boundary(tac, delay_ms, decay, sinusoidal):
    kw = phaser_kw(delay_ms, decay, sinusoidal)
    L, P, _ = R.phaser_plan(8000, delay_ms, 2.0, sinusoidal)
    assert (L, P) == ({0.25: 2, 5.0: 40}[delay_ms], 4000)
    tile = tac._hip.PHASER_TILE
    worst = 0.0
    for length in sorted(set([1, 2, max(L - 1, 1), L, L + 1, 1023, 1025, tile - 1, tile, tile + 1, 2 * tile + 5])):
        x = R.waveform((3, length), seed=400 + length)
        ref, bound, _ = R.phaser(x, **kw)
        for rows in (1, 3):
            got = run(tac, PHASER, tac.phaser, dev(x[:rows]), **kw)
            worst = max(worst, R.assert_close(got, ref[:rows], bound[:rows], 'L %d, %d rows of %d' % (L, rows, length)))
    print('phaser L %d: worst |err| / bound %.3f' % (L, worst))


@pytest.mark.parametrize('sinusoidal', [True, False])
@pytest.mark.parametrize('decay', [0.0, 0.4, 0.99])
@pytest.mark.parametrize('delay_ms', [0.25, 3.0, 5.0])
def test_phaser_parameter_corners(tac, delay_ms, decay, sinusoidal):
    kw = phaser_kw(delay_ms, decay, sinusoidal, gain_in=1.0 if decay == 0.99 else 0.4, gain_out=0.74)
    x = R.waveform((3, 2 * tac._hip.PHASER_TILE + 5), seed=96, scale=2.0)
    ref, bound, _ = R.phaser(x, **kw)
    if decay == 0.99:
        assert (np.abs(ref) == 1.0).any(), 'the clamp acts'
    ratio = R.assert_close(run(tac, PHASER, tac.phaser, dev(x), **kw), ref, bound, repr(kw))
    print('phaser %r: worst |err| / bound %.3f' % (kw, ratio))


def test_phaser_layouts_layer_and_the_sequential_variant(tac):
    kw = phaser_kw(3.0, 0.4)
    for length in (tac._hip.PHASER_TILE + 1, 1029):
        x = R.waveform((2, 3, length), seed=length)
        ref, bound, _ = R.phaser(x, **kw)
        for what, view in layouts(x, 1):
            R.assert_close(run(tac, PHASER, tac.phaser, view, **kw), ref, bound, '%s of %d' % (what, length))
        layer = tac.Phaser(8000, delay_ms=3.0, decay=0.4, mod_speed=2.0)
        R.assert_close(run(tac, PHASER, layer, dev(x)), ref, bound, 'layer')
        # the ablation variant (one lane per row) computes the same recursion
        L, _, table = tac._sox.phaser_plan(8000, 3.0, 2.0, True)
        before = dict(tac._hip.launches)
        seq = tac._hip.phaser_rows(dev(x), table, L, 0.4, 0.74, 0.4, sequential=True)
        assert launched_since(tac, before) == {'tac_phaser_seq_f32': 1}
        R.assert_close(seq, ref, bound, 'sequential variant of %d' % length)


def test_phaser_containment_bit_identity_and_grid(tac):
    kw = phaser_kw(3.0, 0.4)
    x = R.waveform((3, 2 * tac._hip.PHASER_TILE + 5), seed=97)
    contained(tac, PHASER, tac.phaser, x, tac._hip.PHASER_TILE + 7, (), kw)
    grid = grid_of(tac, tac._native.lib().tac_phaser_blocks_per_cu())
    base = R.waveform((5, 301), seed=98)
    beyond_the_grid(tac, PHASER, tac.phaser, base, 2 * grid + 5, (), kw, lambda b: R.phaser(b, **kw))


# ============================================================================= flanger
def flanger_kw(**more):
    return dict(dict(sample_rate=8000, delay=0.0, depth=2.0, regen=0.0, width=71.0, speed=10.0, phase=25.0,
                     modulation='sinusoidal', interpolation='linear'), **more)


def flanger_reference(x, kw):
    plan = R.flanger_plan(channels=x.shape[-2], **kw)
    return (plan,) + R.flanger(x, plan)


@pytest.mark.parametrize('more, channels', [(dict(regen=0.0, delay=5.0, depth=3.0), 2),
                                            (dict(regen=50.0, delay=5.0, depth=3.0, interpolation='quadratic'), 3),
                                            (dict(regen=-50.0, delay=0.0, depth=2.0, modulation='triangular'), 1)])
def test_flanger_every_length_boundary(tac, more, channels):
    kw = flanger_kw(**more)
    plan = R.flanger_plan(channels=channels, **kw)
    assert plan.P == 800
    H = tac._hip
    edge = H.FLANGER_TILE if plan.fb == 0 else H.FLANGER_CHUNK
    lengths = [1, 2, plan.Lb - 1, plan.Lb, plan.Lb + 1, H.FLANGER_CHUNK - 1, H.FLANGER_CHUNK + 1, edge - 1, edge, edge + 1, 2 * edge + 5]
    worst = 0.0
    for length in sorted(set(lengths)):
        x = R.waveform((3, channels, length), seed=500 + length, scale=0.5)
        _, ref, bound, _ = flanger_reference(x, kw)
        for entries in (1, 3):
            got = run(tac, FLANGER, tac.flanger, dev(x[:entries]), **kw)
            worst = max(worst, R.assert_close(got, ref[:entries], bound[:entries], '%d entries of %d' % (entries, length)))
    print('flanger %r: worst |err| / bound %.3f' % (more, worst))


CORNERS = [dict(regen=r, delay=d, depth=p, interpolation=i, phase=ph, modulation=m, channels=c)
           for r, d, p, i, ph, m, c in [
               (0.0, 0.0, 0.0, 'linear', 25.0, 'sinusoidal', 2), (50.0, 0.0, 0.0, 'quadratic', 25.0, 'sinusoidal', 2),
               (0.0, 0.0, 2.0, 'quadratic', 0.0, 'sinusoidal', 1), (95.0, 0.0, 2.0, 'linear', 100.0, 'triangular', 4),
               (-50.0, 0.0, 10.0, 'quadratic', 25.0, 'sinusoidal', 3), (0.0, 5.0, 3.0, 'quadratic', 100.0, 'triangular', 4),
               (50.0, 5.0, 3.0, 'linear', 0.0, 'triangular', 2), (95.0, 5.0, 0.0, 'quadratic', 25.0, 'sinusoidal', 3),
               (0.0, 30.0, 10.0, 'linear', 25.0, 'sinusoidal', 3), (50.0, 30.0, 10.0, 'quadratic', 100.0, 'sinusoidal', 4),
               (-50.0, 30.0, 2.0, 'linear', 25.0, 'triangular', 1), (95.0, 30.0, 10.0, 'quadratic', 0.0, 'triangular', 2)]]


@pytest.mark.parametrize('corner', CORNERS, ids=lambda c: '%(regen)g-%(delay)g-%(depth)g-%(interpolation)s-%(channels)d' % c)
def test_flanger_parameter_corners(tac, corner):
    corner = dict(corner)
    channels = corner.pop('channels')
    kw = flanger_kw(**corner)
    x = R.waveform((2, channels, 2 * tac._hip.FLANGER_CHUNK + 5 if corner['regen'] else tac._hip.FLANGER_TILE + 37), seed=99, scale=0.8)
    plan, ref, bound, _ = flanger_reference(x, kw)
    assert min(64, 1 + plan.tmin) == {0.0: 1, 5.0: 41, 30.0: 64}[corner['delay']]
    if corner['delay'] == corner['depth'] == 0.0:
        assert plan.Lb == 2
    if corner['interpolation'] == 'quadratic' and corner['modulation'] == 'sinusoidal' and plan.Lb > 2:
        k = np.floor(plan.lfo)                   # P = 800 is divisible by 4: the sine reaches Lb - 2 exactly, the wrap tap occurs
        assert ((k + 2 == plan.Lb) & (plan.lfo == k)).any()
    ratio = R.assert_close(run(tac, FLANGER, tac.flanger, dev(x), **kw), ref, bound, repr(corner))
    print('flanger %r x %d: worst |err| / bound %.3f' % (corner, channels, ratio))


@pytest.mark.parametrize('regen', [0.0, 50.0])
def test_flanger_layouts_and_layer(tac, regen):
    kw = flanger_kw(regen=regen, delay=5.0, depth=3.0)
    for length in (tac._hip.FLANGER_TILE + 1, 1029):
        x = R.waveform((2, 3, length), seed=length, scale=0.5)
        _, ref, bound, _ = flanger_reference(x, kw)
        for what, view in layouts(x, 1):
            R.assert_close(run(tac, FLANGER, tac.flanger, view, **kw), ref, bound, '%s of %d' % (what, length))
        layer = tac.Flanger(**kw)
        R.assert_close(run(tac, FLANGER, layer, dev(x)), ref, bound, 'layer')


@pytest.mark.parametrize('regen', [0.0, 50.0])
def test_flanger_containment_bit_identity_and_grid(tac, regen):
    kw = flanger_kw(regen=regen, delay=5.0, depth=3.0, interpolation='quadratic')
    H = tac._hip
    edge = H.FLANGER_TILE if regen == 0.0 else H.FLANGER_CHUNK
    x = R.waveform((2, 2, 2 * edge + 5), seed=100, scale=0.5)
    contained(tac, FLANGER, tac.flanger, x, edge + 7, (), kw)        # (flat row 1: entry 0, channel 1)
    h = tac._native.lib()
    grid = grid_of(tac, h.tac_flanger_blocks_per_cu() if regen == 0.0 else h.tac_flanger_fb_blocks_per_cu())
    base = R.waveform((5, 3, 301), seed=101, scale=0.5)
    entries = (2 * grid + 5 + 2) // 3
    assert 3 * entries > 2 * grid
    beyond_the_grid(tac, FLANGER, tac.flanger, base, entries, (), kw, lambda b: flanger_reference(b, kw)[1:])


# ============================================================================= routes
def test_routes_outside_the_kernels(tac):
    x = R.waveform((2, 2, 64), seed=7, scale=0.5)
    xt = dev(x)
    pk, fk = phaser_kw(3.0, 0.4), flanger_kw(regen=50.0)
    calls = [
        ('overdrive', lambda v, **more: tac.overdrive(v, **dict(dict(gain=20, colour=20), **more)), dict(gain=101.0),
         lambda v, more: R.overdrive(v, more.get('gain', 20), 20)),
        ('phaser', lambda v, **more: tac.phaser(v, **dict(pk, **more)), dict(decay=0.995), lambda v, more: R.phaser(v, **dict(pk, **more))),
        ('flanger', lambda v, **more: tac.flanger(v, **dict(fk, **more)), dict(regen=96.0),
         lambda v, more: R.flanger(v, R.flanger_plan(channels=2, **dict(fk, **more)))),
    ]
    for name, fn, outside, reference in calls:
        before = dict(tac._hip.launches)
        for bad in (xt.double(), xt.half(), xt[:1].expand(2, 2, 64)):
            with pytest.raises(RuntimeError, match='strict mode'):
                fn(bad)
        with pytest.raises(RuntimeError, match='strict mode'):
            fn(xt, **outside)
        if name != 'overdrive':
            y = fn(xt.clone().requires_grad_(True))
            with pytest.raises(RuntimeError, match='strict mode'):
                y.sum().backward()                          # no gradient kernel: the announced composite
        assert not [k for k in launched_since(tac, before) if 'lfilter' in k or k.endswith('_seq_f32')]
        assert tuple(fn(xt[..., :0]).shape) == (2, 2, 0)
        tac.set_strict(False)
        try:
            for xin, more in ((xt.double(), {}), (xt[:1].expand(2, 2, 64), {}), (xt, outside)):
                for key in [k for k in tac._ops._warned if k[0] in (name, 'lfilter')]:
                    tac._ops._warned.discard(key)
                before = dict(tac._hip.launches)
                with pytest.warns(tac.CompositeRouteWarning):
                    got = fn(xin, **more)
                assert got.dtype == xin.dtype and got.shape == xin.shape
                assert not [k for k in launched_since(tac, before) if k in (OVERDRIVE, PHASER, FLANGER)]
                ref, _, mass = reference(xin.cpu().numpy(), more)
                R.assert_close(got, ref, R.bound32(mass), 'announced route of %s, %s' % (name, xin.dtype))
            if name != 'overdrive':
                for key in [k for k in tac._ops._warned if k[0] == name]:
                    tac._ops._warned.discard(key)
                leaf = xt.clone().requires_grad_(True)
                y = fn(leaf)
                with pytest.warns(tac.CompositeRouteWarning):
                    y.sum().backward()
                assert bool(torch.isfinite(leaf.grad).all()) and bool(leaf.grad.any())
        finally:
            tac.set_strict(True)
