"""-m gpu: ``lfilter`` / the biquads / ``preemphasis`` / ``deemphasis`` on the gfx950 kernel (csrc/lfilter.hip) — strict mode and
poisoned outputs on, as in tests/test_resample_gpu.py.

Reference and bound: tests/lfilter_rules.py (``scipy.signal.lfilter`` in float64; per element ``2^-24 |ref| + 2^-40 mass + 2^-126``);
every element is checked.  The lengths are the smallest that reach each boundary of the kernel, from the constants ``_hip`` exports
(``C`` samples per lane, ``TILE`` = 1024 C per tile): 1, 2, 3 (shorter than the filter's memory), C - 1 / C / C + 1 (one lane and a
sample of the next), 64 C - 1 / 64 C + 1 (the boundary between two waves), TILE - 1 / TILE / TILE + 1 and 2 TILE + 5 (the carry
from tile to tile, twice).  A reference is computed once per (filter, length) and shared by the layouts."""
import warnings

import numpy as np
import pytest
import torch

import lfilter_rules as R

pytestmark = pytest.mark.gpu

ENTRY = 'tac_lfilter_f32'


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    t._native.lib()
    t.set_strict(True)
    t._hip.set_poison_outputs(True)
    assert t._native.lib().tac_lfilter_chunk() == t._hip.LFILTER_C and t._hip.LFILTER_TILE == 1024 * t._hip.LFILTER_C
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
def filters(tac):
    return R.filters(tac)


@pytest.fixture(scope='module')
def long_case(tac):
    """the shared (3, 2 TILE + 5) waveform of the numerical cases"""
    return R.waveform((3, 2 * tac._hip.LFILTER_TILE + 5), seed=31)


def launched_since(tac_, before):
    now = tac_._hip.launches
    return {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)}


def dev(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to('cuda')


def t64(v):
    return torch.tensor(v, dtype=torch.float64)


def run_one(tac_, xt, b, a, clamp, what):
    before = dict(tac_._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac_.CompositeRouteWarning)
        got = tac_.lfilter(xt, t64(a), t64(b), clamp=clamp)
    assert launched_since(tac_, before) == {ENTRY: 1}, what
    assert type(got) is torch.Tensor and got.dtype == torch.float32 and got.is_contiguous() and got.shape == xt.shape, what
    return got


def lengths_of(tac_):
    c, tile = tac_._hip.LFILTER_C, tac_._hip.LFILTER_TILE
    return sorted(set([1, 2, 3, c - 1, c, c + 1, 64 * c - 1, 64 * c + 1, tile - 1, tile, tile + 1, 2 * tile + 5]))


# ----------------------------------------------------------------------------- lengths
@pytest.mark.parametrize('which', ['high-pass 100 Hz at 16 kHz', 'preemphasis 0.97'])
def test_every_length_boundary(tac, filters, which):
    (name, b, a), = [f for f in filters if f[0] == which]
    worst = 0.0
    for length in lengths_of(tac):
        x = R.waveform((3, length), seed=100 + length)
        ref, bound = R.reference(x, b, a)
        for rows in (1, 3):
            what = '%s, %d rows of %d' % (name, rows, length)
            worst = max(worst, R.assert_close(run_one(tac, dev(x[:rows]), b, a, False, what), ref[:rows], bound[:rows], what))
    print('%s: worst |err| / bound %.3f' % (name, worst))


def test_unaligned_strided_rows_and_aligned_ones(tac, filters):
    (name, b, a), = [f for f in filters if f[0] == 'order 2']
    tile = tac._hip.LFILTER_TILE
    for length in (tile + 1, 1029):
        x = R.waveform((2, 3, length), seed=length)
        ref, bound = R.reference(x, b, a)
        # rows that are a slice of a larger buffer, starting one float into it: 4-byte aligned only — the float loads
        store = torch.full((2, 3, length + 6), float('nan'), device='cuda')
        store[..., 1:length + 1] = dev(x)
        view = store[..., 1:length + 1]
        assert view.data_ptr() % 16 == 4 and not view.is_contiguous()
        R.assert_close(run_one(tac, view, b, a, False, 'slice'), ref, bound, 'unaligned slice of %d' % length)
        # rows 16-byte aligned, a row stride of a multiple of four floats: the 16-byte loads, across rows and at the row's end
        pad = (-length) % 4 + 4
        store = torch.full((2, 3, length + pad), float('nan'), device='cuda')
        store[..., :length] = dev(x)
        view = store[..., :length]
        assert view.data_ptr() % 16 == 0 and view.stride(1) % 4 == 0
        R.assert_close(run_one(tac, view, b, a, False, 'aligned'), ref, bound, 'aligned padded rows of %d' % length)
        dense = dev(x)
        assert dense.data_ptr() % 16 == 0
        R.assert_close(run_one(tac, dense, b, a, False, 'dense'), ref, bound, 'dense rows of %d' % length)
        # leading dims no single row stride expresses (copied by the launcher), and a 1-D input
        swapped = dev(np.ascontiguousarray(np.swapaxes(x, 0, 1))).transpose(0, 1)
        R.assert_close(run_one(tac, swapped, b, a, False, 'swapped'), ref, bound, 'swapped')
        R.assert_close(run_one(tac, dev(x[1, 2]), b, a, False, '1-D'), ref[1, 2], bound[1, 2], '1-D')


# ----------------------------------------------------------------------------- numerical cases
def test_every_filter_within_the_bound(tac, filters, long_case):
    xt = dev(long_case)
    for name, b, a in filters:
        raw, bound = R.reference(long_case, b, a)
        assert (np.abs(raw) > 1.0).any(), name                                   # the clamp has something to do
        for clamp in (False, True):
            ref = np.clip(raw, -1.0, 1.0) if clamp else raw                       # (= R.reference(..., clamp=clamp))
            what = '%s, clamp %s' % (name, clamp)
            ratio = R.assert_close(run_one(tac, xt, b, a, clamp, what), ref, bound, what)
            print('%s: worst |err| / bound %.3f' % (what, ratio))


def test_the_functions_on_top(tac, long_case):
    x = long_case[:, :tac._hip.LFILTER_TILE + 1]
    xt = dev(x)
    f = tac._filters
    cases = [
        (lambda: tac.highpass_biquad(xt, 48000, 20.0), f.highpass(48000, 20.0), True),
        (lambda: tac.lowpass_biquad(xt, 16000, 1000.0, 10.0), f.lowpass(16000, 1000.0, 10.0), True),
        (lambda: tac.bandpass_biquad(xt, 16000, 2000.0, const_skirt_gain=True), f.bandpass(16000, 2000.0, 0.707, True), True),
        (lambda: tac.bandreject_biquad(xt, 16000, 3000.0), f.bandreject(16000, 3000.0), True),
        (lambda: tac.allpass_biquad(xt, 16000, 500.0), f.allpass(16000, 500.0), True),
        (lambda: tac.equalizer_biquad(xt, 16000, 1500.0, 6.0), f.equalizer(16000, 1500.0, 6.0), True),
        (lambda: tac.preemphasis(xt), ((1.0, -0.97), (1.0, 0.0)), False),
        (lambda: tac.deemphasis(xt), ((1.0, 0.0), (1.0, -0.97)), False),
        (lambda: tac.Preemphasis(0.9).cuda()(xt), ((1.0, -0.9), (1.0, 0.0)), False),
        (lambda: tac.Deemphasis(0.9).cuda()(xt), ((1.0, 0.0), (1.0, -0.9)), False),
        (lambda: tac.LFilter(f.highpass(16000, 100.0)[1], f.highpass(16000, 100.0)[0]).cuda()(xt), f.highpass(16000, 100.0), True),
        (lambda: tac.lfilter(xt, torch.tensor([1.1, -0.7, 0.3], device='cuda'), torch.tensor([0.3, 0.2, 0.1], device='cuda')),
         (torch.tensor([0.3, 0.2, 0.1]).double().tolist(), torch.tensor([1.1, -0.7, 0.3]).double().tolist()), True),
    ]
    for i, (fn, (b, a), clamp) in enumerate(cases):
        before = dict(tac._hip.launches)
        got = fn()
        assert launched_since(tac, before) == {ENTRY: 1}, i
        ref, bound = R.reference(x, b, a, clamp=clamp)
        R.assert_close(got, ref, bound, 'case %d' % i)
    back = tac.deemphasis(tac.preemphasis(xt))
    y = tac.preemphasis(xt).cpu().numpy()
    ref2, bound2 = R.reference(y, (1.0, 0.0), (1.0, -0.97))
    R.assert_close(back, ref2, bound2, 'deemphasis of preemphasis')


# ----------------------------------------------------------------------------- behaviour
def test_nan_stays_in_its_row_and_goes_forward_only(tac, filters):
    tile = tac._hip.LFILTER_TILE
    at = tile + 7
    for name, b, a in filters:
        x = R.waveform((3, 2 * tile + 5), seed=41)
        x[1, at] = np.nan
        got = tac.lfilter(dev(x), t64(a), t64(b), clamp=False).cpu().numpy()
        ref, bound = R.reference(x[[0, 2]], b, a)
        assert np.isfinite(got[[0, 2]]).all(), name
        R.assert_close(got[[0, 2]], ref, bound, '%s: the rows next to the NaN' % name)
        ref, bound = R.reference(x[1:2, :at], b, a)
        R.assert_close(got[1:2, :at], ref, bound, '%s: before the NaN' % name)
        assert np.isnan(got[1, at]), name
        if any(v != 0.0 for v in a[1:]):
            assert np.isnan(got[1, at:]).all(), name                     # the recursion carries it to the end of the row
        else:
            assert np.isfinite(got[1, at + len(b):]).all(), name         # a finite memory forgets it


def test_two_runs_are_bit_identical(tac, filters, long_case):
    xt = dev(long_case)
    for name, b, a in filters:
        first = tac.lfilter(xt, t64(a), t64(b), clamp=False)
        assert torch.equal(first, tac.lfilter(xt, t64(a), t64(b), clamp=False)), name
    x = xt[:, :tac._hip.LFILTER_TILE + 1].clone().requires_grad_(True)
    name, b, a = filters[2]
    g = torch.randn_like(x)
    (g1,) = torch.autograd.grad(tac.lfilter(x, t64(a), t64(b)), x, grad_outputs=g)
    (g2,) = torch.autograd.grad(tac.lfilter(x, t64(a), t64(b)), x, grad_outputs=g)
    assert torch.equal(g1, g2)


# ----------------------------------------------------------------------------- gradient
def test_gradient_is_the_reversed_kernel(tac, filters):
    length = tac._hip.LFILTER_TILE + 1
    assert tac._ops.strict()
    x_np = R.waveform((3, length), seed=51)
    gy = R.waveform((3, length), seed=52)
    for name, b, a in filters:
        for clamp, scale in ((False, 1.0), (True, 4.0)):
            x = dev(scale * x_np).requires_grad_(True)
            raw, rb = R.reference(scale * x_np, b, a)
            g_eff = gy
            if clamp:
                # the test input must exceed +-1, and no reference value may sit where rounding decides the mask
                assert (np.abs(raw) > 1.0).any() and (np.abs(np.abs(raw) - 1.0) > rb).all(), name
                g_eff = gy * (np.abs(raw) < 1.0)
            aref, abound = R.adjoint_reference(g_eff, b, a)
            before = dict(tac._hip.launches)
            with warnings.catch_warnings():
                warnings.simplefilter('error', tac.CompositeRouteWarning)
                y = tac.lfilter(x, t64(a), t64(b), clamp=clamp)
                assert launched_since(tac, before) == {ENTRY: 1}, name
                (gx,) = torch.autograd.grad(y, x, grad_outputs=dev(gy))
            what = 'gradient, %s, clamp %s' % (name, clamp)
            assert launched_since(tac, before) == {ENTRY: 2}, what                # one per forward, one per backward
            assert gx.shape == x.shape and gx.is_contiguous()
            ratio = R.assert_close(gx, aref, abound, what)
            print('%s: worst |err| / bound %.3f' % (what, ratio))


def test_trains_in_front_of_the_fused_mel_chain(tac):
    mel = dict(num_mels=40, sample_rate=16000, fft_length=512, hop_length=128)
    b, a = tac._filters.highpass(16000, 100.0)
    x = dev(R.waveform((2, 1, 4096), seed=61))
    for front in (tac.Preemphasis(), tac.LFilter(a, b)):
        chain = torch.nn.Sequential(front, *tac.Melspectrogram(**mel), tac.AmplitudeToDb()).cuda()
        xg = x.clone().requires_grad_(True)
        before = dict(tac._hip.launches)
        with warnings.catch_warnings():
            warnings.simplefilter('error', tac.CompositeRouteWarning)
            out = chain(x)
            assert type(out) is torch.Tensor and tuple(out.shape) == (2, 1, 40, 33)
            assert launched_since(tac, before).get(ENTRY) == 1
            # (both without autograd: with it the chain runs as separate differentiable ops, whose bits may differ)
            assert torch.equal(out, torch.nn.Sequential(*list(chain)[1:])(front(x)))
            before = dict(tac._hip.launches)
            chain(xg).square().mean().backward()
        assert launched_since(tac, before).get(ENTRY) == 2
        assert bool(torch.isfinite(xg.grad).all()) and bool(xg.grad.any())
        assert chain.state_dict() == {}


# ----------------------------------------------------------------------------- refusals
def test_routes_outside_the_kernel(tac):
    x = R.waveform((2, 64), seed=3)
    xt = dev(x)
    b3, a3 = (0.1, 0.2, 0.2, 0.1), (1.0, -0.4, 0.3, -0.1)
    b2, a2 = tac._filters.lowpass(16000, 1000.0)
    before = dict(tac._hip.launches)
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.lfilter(xt, t64(a3), t64(b3))                                   # order 3
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.lfilter(xt.double(), t64(a2), t64(b2))                          # float64 on the device
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.lfilter(xt[:1].expand(3, 64), t64(a2), t64(b2))                 # a stride of zero
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.lfilter(xt, t64((1.0, -2.4, 1.44)), t64((1.0, 0.0, 0.0)))       # a double pole at 1.2: M^(1024 C) overflows
    at = t64(a2).cuda().requires_grad_(True)
    y = tac.lfilter(xt, at, t64(b2).cuda())
    with pytest.raises(RuntimeError, match='strict mode'):
        y.sum().backward()                                                  # the coefficients' gradient
    assert launched_since(tac, before) == {ENTRY: 1}
    assert tuple(tac.lfilter(xt[:, :0], t64(a2), t64(b2)).shape) == (2, 0)
    tac.set_strict(False)
    try:
        for xin, a, b in ((xt, a3, b3), (xt.double(), a2, b2)):
            for key in [k for k in tac._ops._warned if k[0] == 'lfilter']:
                tac._ops._warned.discard(key)
            before = dict(tac._hip.launches)
            with pytest.warns(tac.CompositeRouteWarning):
                got = tac.lfilter(xin, t64(a), t64(b), clamp=False)
            assert got.dtype == xin.dtype and launched_since(tac, before) == {}
            ref, bound = R.reference(x, b, a)
            R.assert_close(got, ref, bound, 'stock-torch route, %s' % xin.dtype)
        for key in [k for k in tac._ops._warned if k[0] == 'lfilter']:
            tac._ops._warned.discard(key)
        at = t64(a2).cuda().requires_grad_(True)
        bt = t64(b2).cuda().requires_grad_(True)
        y = tac.lfilter(xt, at, bt, clamp=False)
        with pytest.warns(tac.CompositeRouteWarning):
            y.sum().backward()
        assert bool(torch.isfinite(at.grad).all()) and bool(bt.grad.any())
    finally:
        tac.set_strict(True)
