"""-m gpu: ``sosfilt`` / ``filtfilt`` on the gfx950 cascade kernel (csrc/sosfilt.hip) — strict mode and poisoned outputs on, as in
tests/test_lfilter_gpu.py.

References and bounds: tests/sos_rules.py (``scipy.signal.sosfilt`` in float64; per element ``2^-24 |ref| + d_S + 2^-126`` with the
stage-composed ``d_S``); every element is checked.  The lengths are the smallest that reach each boundary of the kernel, from the
library's own constants (``C`` samples per lane, ``T = tac_sosfilt_tile()`` per tile): 1, 2, 3, C - 1 / C / C + 1, 64 C - 1 /
64 C + 1 (two waves), T - 1 / T / T + 1 and 2 T + 5 (the per-section carries from tile to tile, twice).  A reference is computed
once per (filter, input) and shared."""
import warnings

import numpy as np
import pytest
import torch

import lfilter_rules as LR
import sos_rules as R

pytestmark = pytest.mark.gpu

ENTRY = 'tac_sosfilt_f32'


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    h = t._native.lib()
    t.set_strict(True)
    t._hip.set_poison_outputs(True)
    assert h.tac_sosfilt_tile() == t._hip.SOSFILT_TILE and h.tac_sosfilt_max_sections() == t._hip.SOSFILT_MAX_SECTIONS == 8
    assert h.tac_sosfilt_blocks_per_cu() == t._hip.SOSFILT_BLOCKS_PER_CU
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


@pytest.fixture(scope='module')
def long_case(tac):
    """the shared (3, 2 T + 5) waveform of the numerical cases, loud enough for the clamp to act behind every listed filter"""
    return 4.0 * R.waveform((3, 2 * tac._hip.SOSFILT_TILE + 5), seed=81)


def launched_since(tac_, before):
    now = tac_._hip.launches
    return {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)}


def dev(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to('cuda')


def t64(v):
    return torch.tensor(np.asarray(v), dtype=torch.float64)


def run_one(tac_, xt, sos, clamp, what):
    before = dict(tac_._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac_.CompositeRouteWarning)
        got = tac_.sosfilt(xt, t64(sos), clamp=clamp)
    assert launched_since(tac_, before) == {ENTRY: 1}, what
    assert type(got) is torch.Tensor and got.dtype == torch.float32 and got.is_contiguous() and got.shape == xt.shape, what
    return got


def lengths_of(tac_):
    c, tile = tac_._hip.LFILTER_C, tac_._hip.SOSFILT_TILE
    return sorted(set([1, 2, 3, c - 1, c, c + 1, 64 * c - 1, 64 * c + 1, tile - 1, tile, tile + 1, 2 * tile + 5]))


# ----------------------------------------------------------------------------- lengths
@pytest.mark.parametrize('which', [R.BANDPASS8, R.ODD])
def test_every_length_boundary(tac, which):
    sos = R.sections_of(tac, which)
    worst = 0.0
    for length in lengths_of(tac):
        x = R.waveform((3, length), seed=200 + length)
        ref, bound = R.reference(x, sos)
        for rows in (1, 3):
            what = '%s, %d rows of %d' % (which, rows, length)
            worst = max(worst, R.assert_close(run_one(tac, dev(x[:rows]), sos, False, what), ref[:rows], bound[:rows], what))
    print('%s: worst |err| / bound %.3f' % (which, worst))


# ----------------------------------------------------------------------------- section counts
def test_section_counts_and_kinds(tac):
    bp, odd = R.sections_of(tac, R.BANDPASS8), R.sections_of(tac, R.ODD)
    fir, identity = [0.5, -0.3, 0.2, 1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    first_order = [0.5, 0.25, 0.0, 2.0, -1.8, 0.0]                       # (a0 = 2: normalised by the kernel's host side)
    sixteen = np.concatenate([bp, R.sections_of(tac, R.NAMES[5])])       # order 16: two order-8 band-passes
    cases = [('S = 1', bp[:1]), ('S = 2', bp[:2]), ('S = 3', bp[:3]), ('S = 8', sixteen), ('FIR only', np.array([fir])),
             ('identity', np.array([identity])), ('FIR first', np.array([fir, bp[0]])), ('FIR last', np.array([bp[0], fir])),
             ('identity between', np.array([bp[0], identity, bp[1]])), ('first order in the middle', np.array([bp[0], first_order, bp[3]])),
             ('FIR twice', np.array([fir, fir, odd[0]]))]
    assert len(sixteen) == 8
    x = R.waveform((3, tac._hip.SOSFILT_TILE + 37), seed=82)
    xt = dev(x)
    for what, sos in cases:
        ref, bound = R.reference(x, sos)
        ratio = R.assert_close(run_one(tac, xt, sos, False, what), ref, bound, what)
        print('%s: worst |err| / bound %.3f' % (what, ratio))
    assert torch.equal(run_one(tac, xt, np.array([identity]), False, 'identity'), xt)


@pytest.mark.parametrize('name', R.NAMES)
def test_every_filter_within_the_bound(tac, long_case, name):
    _, b, a = R.named(name)
    sos = R.sections_of(tac, name)
    xt = dev(long_case)
    raw, bound = R.reference(long_case, sos)
    assert (np.abs(raw) > 1.0).any(), name                                   # the clamp has something to do
    for clamp in (False, True):
        ref = np.clip(raw, -1.0, 1.0) if clamp else raw
        what = '%s, clamp %s' % (name, clamp)
        got = run_one(tac, xt, sos, clamp, what)
        ratio = R.assert_close(got, ref, bound, what)
        print('%s: worst |err| / bound %.3f' % (what, ratio))
        if not clamp:       # sosfilt(x, tf2sos(b, a)) against the direct-form float64 filter and its own bound
            dref, dbound = LR.reference(long_case, b, a)
            ratio = R.assert_close(got, dref, dbound, '%s against the direct form' % name)
            print('%s against the direct form: worst |err| / bound %.3f' % (name, ratio))


# ----------------------------------------------------------------------------- layouts
def test_unaligned_strided_rows_and_aligned_ones(tac):
    sos = R.sections_of(tac, R.BANDPASS8)
    tile = tac._hip.SOSFILT_TILE
    for length in (tile + 1, 1029):
        x = R.waveform((2, 3, length), seed=length)
        ref, bound = R.reference(x, sos)
        for offset in (1, 2, 3):                 # 4-byte aligned only: the dword loads
            store = torch.full((2, 3, length + 6), float('nan'), device='cuda')
            store[..., offset:length + offset] = dev(x)
            view = store[..., offset:length + offset]
            assert view.data_ptr() % 16 == 4 * offset and not view.is_contiguous()
            R.assert_close(run_one(tac, view, sos, False, 'slice'), ref, bound, 'slice at offset %d of %d' % (offset, length))
        # rows 16-byte aligned, a row stride of a multiple of four floats: the 16-byte loads, across rows and at the row's end
        pad = (-length) % 4 + 4
        store = torch.full((2, 3, length + pad), float('nan'), device='cuda')
        store[..., :length] = dev(x)
        view = store[..., :length]
        assert view.data_ptr() % 16 == 0 and view.stride(1) % 4 == 0
        R.assert_close(run_one(tac, view, sos, False, 'aligned'), ref, bound, 'aligned padded rows of %d' % length)
        # a channel slice of a larger tensor: row stride != length
        wide = torch.full((2, 5, length), float('nan'), device='cuda')
        wide[:, 1:4] = dev(x)
        R.assert_close(run_one(tac, wide[:, 1:4], sos, False, 'channels'), ref, bound, 'channel slice of %d' % length)
        dense = dev(x)
        assert dense.data_ptr() % 16 == 0
        R.assert_close(run_one(tac, dense, sos, False, 'dense'), ref, bound, 'dense rows of %d' % length)
        # a transposed input (copied by the launcher, as lfilter does), and a 1-D one
        swapped = dev(np.ascontiguousarray(np.swapaxes(x, 0, 1))).transpose(0, 1)
        R.assert_close(run_one(tac, swapped, sos, False, 'swapped'), ref, bound, 'swapped')
        R.assert_close(run_one(tac, dev(x[1, 2]), sos, False, '1-D'), ref[1, 2], bound[1, 2], '1-D')


# ----------------------------------------------------------------------------- containment
@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_non_finite_stays_in_its_row_and_goes_forward_only(tac, bad):
    tile = tac._hip.SOSFILT_TILE
    at = tile + 7
    fir = [0.5, -0.3, 0.2, 1.0, 0.0, 0.0]
    for what, sos in ((R.BANDPASS8, R.sections_of(tac, R.BANDPASS8)), (R.ODD, R.sections_of(tac, R.ODD)),
                      ('FIR then a section', np.array([fir, R.sections_of(tac, R.ODD)[1]]))):
        x = R.waveform((3, 2 * tile + 5), seed=83)
        clean = run_one(tac, dev(x), sos, False, what)
        x[1, at] = bad
        got = run_one(tac, dev(x), sos, False, what)
        assert torch.equal(got[[0, 2]], clean[[0, 2]]), what                 # bit-equal: the other rows
        assert torch.equal(got[1, :at], clean[1, :at]), what                 # ... and the row itself before the sample
        assert not bool(torch.isfinite(got[1, at])), what
        assert not bool(torch.isfinite(got[1, at:]).any()), what             # the recursion carries it to the end of the row
    # the adjoint walks from the end: what lies behind the sample stays untouched
    sos = R.sections_of(tac, R.BANDPASS8)
    x = R.waveform((3, 2 * tile + 5), seed=84)
    clean = tac._hip.sosfilt_rows(dev(x), tac._hip.host_sos(t64(sos)), False, reverse=True)
    x[1, at] = bad
    got = tac._hip.sosfilt_rows(dev(x), tac._hip.host_sos(t64(sos)), False, reverse=True)
    assert torch.equal(got[[0, 2]], clean[[0, 2]]) and torch.equal(got[1, at + 1:], clean[1, at + 1:])
    assert not bool(torch.isfinite(got[1, :at + 1]).any())


def test_runs_and_batches_are_bit_identical(tac, long_case):
    xt = dev(long_case)
    for name in (R.BANDPASS8, R.ODD, R.NAMES[-1]):
        sos = R.sections_of(tac, name)
        first = run_one(tac, xt, sos, False, name)
        assert torch.equal(first, run_one(tac, xt, sos, False, name)), name
        for r in range(3):
            assert torch.equal(first[r], run_one(tac, xt[r], sos, False, name)), name       # alone as inside the batch


# ----------------------------------------------------------------------------- grid wrap
def test_rows_beyond_the_grid(tac):
    sos = R.sections_of(tac, R.BANDPASS8)
    grid = tac._native.lib().tac_sosfilt_blocks_per_cu() * torch.cuda.get_device_properties(0).multi_processor_count
    rows = 2 * grid + 5
    assert rows == 2 * grid + rows % grid and 0 < rows % grid < grid         # every workgroup takes two rows, five a third
    for length in (301, tac._hip.SOSFILT_TILE + 37):
        base = R.waveform((5, length), seed=85 + length)
        ref, bound = R.reference(base, sos)
        five = run_one(tac, dev(base), sos, False, 'five rows')
        R.assert_close(five, ref, bound, 'five rows of %d' % length)
        reps = (rows + 4) // 5
        many = dev(base).repeat(reps, 1)[:rows]
        got = run_one(tac, many, sos, False, '%d rows of %d' % (rows, length))
        assert torch.equal(got, five.repeat(reps, 1)[:rows]), length


# ----------------------------------------------------------------------------- gradient
def test_gradient_is_the_reversed_cascade(tac):
    length = tac._hip.SOSFILT_TILE + 37
    x_np = R.waveform((3, length), seed=86)
    gy = R.waveform((3, length), seed=87)
    for name in (R.BANDPASS8, R.ODD):
        sos = R.sections_of(tac, name)
        for clamp, scale in ((False, 1.0), (True, 4.0)):
            x = dev(scale * x_np).requires_grad_(True)
            raw, rb = R.reference(scale * x_np, sos)
            g_eff = gy
            if clamp:
                # the test input must exceed +-1, and no reference value may sit where rounding decides the mask
                assert (np.abs(raw) > 1.0).any() and (np.abs(np.abs(raw) - 1.0) > rb).all(), name
                g_eff = gy * (np.abs(raw) < 1.0)
            aref, abound = R.adjoint_reference(g_eff, sos)
            before = dict(tac._hip.launches)
            with warnings.catch_warnings():
                warnings.simplefilter('error', tac.CompositeRouteWarning)
                y = tac.sosfilt(x, t64(sos), clamp=clamp)
                assert launched_since(tac, before) == {ENTRY: 1}, name
                (gx,) = torch.autograd.grad(y, x, grad_outputs=dev(gy))
            what = 'gradient, %s, clamp %s' % (name, clamp)
            assert launched_since(tac, before) == {ENTRY: 2}, what                # one per forward, one per backward
            assert gx.shape == x.shape and gx.is_contiguous()
            ratio = R.assert_close(gx, aref, abound, what)
            print('%s: worst |err| / bound %.3f' % (what, ratio))


# ----------------------------------------------------------------------------- filtfilt
def test_filtfilt(tac):
    length = tac._hip.SOSFILT_TILE + 37
    x_np = 4.0 * R.waveform((3, length), seed=88)
    gy = R.waveform((3, length), seed=89)
    _, b8, a8 = R.named(R.BANDPASS8)
    b2, a2 = tac._filters.highpass(16000, 100.0)
    for what, b, a, sos, entry in (('order 2', b2, a2, np.array([list(b2) + list(a2)]), 'tac_lfilter_f32'),
                                   ('order 8', b8, a8, R.sections_of(tac, R.BANDPASS8), ENTRY)):
        for clamp in (False, True):
            before = dict(tac._hip.launches)
            with warnings.catch_warnings():
                warnings.simplefilter('error', tac.CompositeRouteWarning)
                got = tac.filtfilt(dev(x_np), t64(a), t64(b), clamp=clamp)
            assert launched_since(tac, before) == {entry: 2}, what
            ref, bound = R.filtfilt_reference(x_np, sos, clamp=clamp)
            ratio = R.assert_close(got, ref, bound, 'filtfilt, %s, clamp %s' % (what, clamp))
            print('filtfilt, %s, clamp %s: worst |err| / bound %.3f' % (what, clamp, ratio))
        # the gradient: filtfilt without clamp is self-adjoint
        x = dev(x_np).requires_grad_(True)
        before = dict(tac._hip.launches)
        with warnings.catch_warnings():
            warnings.simplefilter('error', tac.CompositeRouteWarning)
            (gx,) = torch.autograd.grad(tac.filtfilt(x, t64(a), t64(b), clamp=False), x, grad_outputs=dev(gy))
        assert launched_since(tac, before) == {entry: 4}, what
        # the adjoint of (filter from the end) o (filter) is the same pair in the same order, applied to grad_out
        ref, bound = R.filtfilt_reference(gy, sos)
        ratio = R.assert_close(gx, ref, bound, 'filtfilt gradient, %s' % what)
        print('filtfilt gradient, %s: worst |err| / bound %.3f' % (what, ratio))


# ----------------------------------------------------------------------------- routes
def test_routes_outside_the_kernel(tac):
    x = R.waveform((2, 64), seed=3)
    xt = dev(x)
    sos = R.sections_of(tac, R.ODD)
    nine = np.concatenate([R.sections_of(tac, R.BANDPASS8)] * 2 + [sos[:1]])
    unstable = np.array([[1.0, 0.0, 0.0, 1.0, -2.4, 1.44]])                 # a double pole at 1.2: M^(1024 C) overflows
    assert len(nine) == 9
    before = dict(tac._hip.launches)
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.sosfilt(xt.double(), t64(sos))                                  # float64 on the device
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.sosfilt(xt[:1].expand(3, 64), t64(sos))                         # a stride of zero
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.sosfilt(xt, t64(nine))                                          # S = 9
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.sosfilt(xt, t64(unstable))
    st = t64(sos).cuda().requires_grad_(True)
    y = tac.sosfilt(xt, st)
    with pytest.raises(RuntimeError, match='strict mode'):
        y.sum().backward()                                                  # the sections' gradient
    assert launched_since(tac, before) == {ENTRY: 1}
    assert tuple(tac.sosfilt(xt[:, :0], t64(sos)).shape) == (2, 0)
    tac.set_strict(False)
    try:
        for xin, s in ((xt.double(), sos), (xt[:1].expand(2, 64), sos), (xt, nine), (xt, unstable)):
            for key in [k for k in tac._ops._warned if k[0] == 'sosfilt']:
                tac._ops._warned.discard(key)
            before = dict(tac._hip.launches)
            with pytest.warns(tac.CompositeRouteWarning):
                got = tac.sosfilt(xin, t64(s))
            assert got.dtype == xin.dtype and launched_since(tac, before) == {}
            ref, bound = R.reference(xin.cpu().numpy(), s)
            R.assert_close(got, ref, bound, 'stock-torch route, %s, %d sections' % (xin.dtype, len(s)))
        for key in [k for k in tac._ops._warned if k[0] == 'sosfilt']:
            tac._ops._warned.discard(key)
        st = t64(sos).cuda().requires_grad_(True)
        y = tac.sosfilt(xt, st)
        with pytest.warns(tac.CompositeRouteWarning):
            y.sum().backward()
        assert bool(torch.isfinite(st.grad).all()) and bool(st.grad.any())
    finally:
        tac.set_strict(True)
