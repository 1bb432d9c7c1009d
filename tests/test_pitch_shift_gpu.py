"""-m gpu: ``tac_amd::resample_fit`` on the wide polyphase kernel (``tac_polyphase_wide_f32``, csrc/resample.hip) and ``pitch_shift`` /
``PitchShift`` on the device — strict mode and poisoned outputs on, as in tests/test_resample_gpu.py.

Reference and bound of the resampling: tests/resample_rules.py through tests/pitch_shift_rules.py — the float64 sum per output sample
and, per element, ``(K_n + 2) * 2^-24 * sum |h64| |x|``; every element is checked.  A reference is computed once per case and shared
by the layouts: three dense rows, one row, and six rows (a partial second row group) that are ``x[:, 1:]`` of a padded buffer —
4-byte aligned only, a row stride that is no multiple of four.

``test_wide_variants_within_the_bound`` walks the table of tests/polyphase_rules.py: every instantiation
``polyphase_wide_kernel<KB, VEC>`` at every tile public arguments reach (tests/test_polyphase_rules_cpu.py holds the table to the
census), for the forward and for the adjoint bank, each asserted through the restated launcher rule before the launch; a fourth
layout there — six rows a multiple of four floats apart — gives 16-byte loads with more than one row of a group whatever the length."""
import warnings

import numpy as np
import pytest
import torch

import pitch_shift_rules as PS
import polyphase_rules as PR
import resample_rules as R

pytestmark = pytest.mark.gpu

WIDE, LDS = PS.WIDE_ENTRY, PS.LDS_ENTRY
HANN, KAISER = dict(), dict(method='sinc_interp_kaiser')
# (orig, new, L, filter): 2000 : 2001 and back cross two block wraps inside tiles; 10079 : 8000 at 1500 stays inside block 0 (off is
# negative at the left edge), at 21000 wraps at n = 8000 and 16000; 16000 : 44101 has P = 44101, K = 13; 44101 : 16000 K = 34, the
# widest tile span
CASES = [(2000, 2001, 4500, HANN), (2001, 2000, 4500, HANN), (1873, 1575, 4000, HANN), (10079, 8000, 1500, HANN),
         (10079, 8000, 21000, HANN), (16000, 44101, 17000, HANN), (44101, 16000, 45000, HANN), (1873, 1575, 4000, KAISER)]


def case_id(c):
    return '%d:%d-%d%s' % (c[0], c[1], c[2], ''.join('-%s' % v for v in c[3].values()))


def product_kw(kw):
    names = dict(lpw='lowpass_filter_width', rolloff='rolloff', method='resampling_method', beta='beta')
    return {names[k]: v for k, v in kw.items()}


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


def shifted(x):
    """``store[:, 1:]`` of a NaN-filled buffer whose row stride is no multiple of four: float loads, every row 4-byte aligned only"""
    rows, length = x.shape
    stride = length + 1 + (1 if (length + 1) % 4 == 0 else 0)
    store = torch.full((rows, stride), float('nan'), device='cuda')
    store[:, 1:length + 1] = dev(x)
    view = store[:, 1:length + 1]
    assert view.stride(0) % 4 != 0 and view.data_ptr() % 16 != 0
    return view


LAYOUTS = (('3 rows', 3, dev), ('1 row', 1, dev), ('6 rows of a padded buffer', 6, shifted))


def fit(tac_, x, key, out_len):
    return tac_._ops.call('resample_fit', x, *key, out_len)


# ----------------------------------------------------------------------------- the kernel, element by element
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_wide_kernel_within_the_bound(tac, case):
    orig, new, length, kw = case
    key = tac._resample.constants(orig, new, **product_kw(kw))
    assert not tac._hip.resample_covers(*key) and tac._hip.resample_fit_covers(key, length, 1)
    n_out = R.out_length(length, orig, new)
    x = R.waveform((6, length), seed=orig + new + length)
    g = R.waveform((6, n_out), seed=orig + new + length + 1)
    ref, bound = R.reference(x, orig, new, **kw)
    aref, abound = R.adjoint_reference(g, length, orig, new, **kw)
    worst = worst_adj = 0.0
    for tag, rows, build in LAYOUTS:
        what = '%s, %s' % (case_id(case), tag)
        xt = build(x[:rows]).requires_grad_(True)
        before = dict(tac._hip.launches)
        got = fit(tac, xt, key, n_out)
        assert launched_since(tac, before) == {WIDE: 1}, what
        assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (rows, n_out), what
        worst = max(worst, R.assert_close(got, ref[:rows], bound[:rows], what))
        before = dict(tac._hip.launches)
        with warnings.catch_warnings():
            warnings.simplefilter('error', tac.CompositeRouteWarning)
            (gx,) = torch.autograd.grad(got, xt, grad_outputs=build(g[:rows]))
        assert launched_since(tac, before) == {WIDE: 1}, what
        assert tuple(gx.shape) == (rows, length), what
        worst_adj = max(worst_adj, R.assert_close(gx, aref[:rows], abound[:rows], 'gradient, ' + what))
    print('resample_fit %s: worst |err| / bound %.3f forward, %.3f adjoint' % (case_id(case), worst, worst_adj))


# ----------------------------------------------------------------------------- every bucket of K, every tile
def sixteen_byte_rows(x):
    return x.data_ptr() % 16 == 0 and (x.shape[0] == 1 or x.stride(0) % 4 == 0)


def aligned(x):
    """the rows a multiple of four floats apart in a NaN-filled buffer: 16-byte loads whatever the length, with every row of
    a group staged behind the first (``r * pitch``)"""
    rows, length = x.shape
    store = torch.full((rows, length + ((-length) % 4 or 4)), float('nan'), device='cuda')
    store[:, :length] = dev(x)
    return store[:, :length]


VARIANT_LAYOUTS = LAYOUTS + (('6 rows a multiple of four floats apart', 6, aligned),)


@pytest.mark.parametrize('case', PR.WIDE_CASES, ids=PR.case_id)
def test_wide_variants_within_the_bound(tac, case):
    """Inputs long enough for three tiles and a remainder of the forward launch (``n_out`` outputs at the forward bank's tile) AND
    of the gradient's (``length`` outputs at the adjoint bank's), with ``out_len`` natural, cut and zero-padded; and inputs whose
    natural length is about one tile with ``out_len`` one tile minus one / exactly / plus one.  Forward and gradient of every
    layout; the gradient at the cut ``out_len`` (tests/test_polyphase_sweeps_gpu.py draws the others)."""
    orig, new, kw = case
    key = tac._resample.constants(orig, new, **product_kw(kw))
    banks = tac._resample.bank(*key), tac._resample.adjoint_bank(*key)
    fwd, adj = (PR.wide_variant(b, True) for b in banks)
    assert fwd is not None and adj is not None and tac._hip.resample_fit_covers(key, 1000, 1)
    assert fwd[:2] == PR.wide_variant(PR.case_geometry(case), True)[:2] and adj[:2] == PR.wide_variant(PR.case_geometry(case, True), True)[:2]
    assert all(tac._hip.resample_wide_plan(b)[1] == v[0] for b, v in zip(banks, (fwd, adj)))
    lds = tac._hip.resample_covers(*key)                    # (8:1, 16:1 and back: the natural out_len would take the LDS kernel)
    long = max(3 * fwd[0] * orig // new, 3 * adj[0]) + (fwd[0] // 3) * orig // new + 5
    one = fwd[0] * orig // new
    worst = worst_adj = 0.0
    loads, grad_loads = set(), set()
    for length in (long, one):
        n_out = R.out_length(length, orig, new)
        x = R.waveform((6, length), seed=orig + new + length)
        ref, bound = R.reference(x, orig, new, **kw)
        if length == long:
            assert n_out > 3 * fwd[0] and length > 3 * adj[0]
            out_lens = [n_out + 1 if lds else n_out, n_out - fwd[0] // 2 - 7, n_out + 300]
        else:
            assert fwd[0] - new - 1 <= n_out <= fwd[0]
            out_lens = [fwd[0] - 1, fwd[0] + 1] + ([] if lds and n_out == fwd[0] else [fwd[0]])
        for out_len in out_lens:
            want, allowed = PS.fit(ref, out_len), PS.fit(bound, out_len)
            gradient = length == long and out_len < n_out           # (grad_out cut short of n_out: the rest of the row reads zeros)
            if gradient:
                g = R.waveform((6, out_len), seed=orig + new + out_len)
                aref, abound = PS.fit_adjoint_reference(g, length, orig, new, **kw)
            for tag, rows, build in VARIANT_LAYOUTS:
                what = '%s, length %d to %d of %d, %s' % (PR.case_id(case), length, out_len, n_out, tag)
                xt = build(x[:rows]).requires_grad_(True)
                loads.add((rows > 1, sixteen_byte_rows(xt)))
                if gradient:
                    grad_loads.add((rows > 1, sixteen_byte_rows(build(g[:rows]))))
                before = dict(tac._hip.launches)
                got = fit(tac, xt, key, out_len)
                assert launched_since(tac, before) == {WIDE: 1}, what
                assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (rows, out_len), what
                worst = max(worst, R.assert_close(got, want[:rows], allowed[:rows], what))
                assert not bool(got[:, n_out:].any()), what                         # the zero tail: exactly 0.0, every one written
                if gradient:
                    before = dict(tac._hip.launches)
                    with warnings.catch_warnings():
                        warnings.simplefilter('error', tac.CompositeRouteWarning)
                        (gx,) = torch.autograd.grad(got, xt, grad_outputs=build(g[:rows]))
                    assert launched_since(tac, before) == {WIDE: 1}, what
                    assert tuple(gx.shape) == (rows, length), what
                    worst_adj = max(worst_adj, R.assert_close(gx, aref[:rows], abound[:rows], 'gradient, ' + what))
    # both load forms with more than one row of a group, for the input and for grad_out
    assert {(True, False), (True, True)} <= loads and {(True, False), (True, True)} <= grad_loads, (loads, grad_loads)
    print('resample_fit %s: forward tile %d, KB %d, %d per CU (K %d); adjoint tile %d, KB %d, %d per CU (K %d); VEC 0 and 1: '
          'worst |err| / bound %.3f forward, %.3f adjoint' % (PR.case_id(case), fwd[0], fwd[1], fwd[3], banks[0].K, adj[0], adj[1], adj[3],
                                                            banks[1].K, worst, worst_adj))


# ----------------------------------------------------------------------------- the same bits as the LDS kernel
@pytest.mark.parametrize('pair', [(441, 160), (160, 441), (147, 160), (3, 2)], ids=str)
def test_bit_equal_to_the_lds_kernel(tac, pair):
    orig, new = pair
    key = tac._resample.constants(orig, new)
    assert tac._hip.resample_covers(*key)
    length = 3 * 1024 * orig // new + orig // 2 + 5
    n_out = R.out_length(length, orig, new)
    for rows in (1, 6):
        x = dev(R.waveform((rows, length), seed=orig + rows))
        g = dev(R.waveform((rows, n_out), seed=new + rows))
        before = dict(tac._hip.launches)
        lds = tac._hip.polyphase(x, key, n_out)
        lds_adj = tac._hip.polyphase(g, key, length, adjoint=True)
        assert launched_since(tac, before) == {LDS: 2}
        before = dict(tac._hip.launches)
        wide = tac._hip.resample_fit(x, key, n_out, wide=True)
        wide_adj = tac._hip.resample_fit(g, key, n_out, adjoint=True, length=length, wide=True)
        assert launched_since(tac, before) == {WIDE: 2}
        assert torch.equal(wide, lds) and torch.equal(wide_adj, lds_adj)
        assert torch.equal(tac._hip.resample_fit(x, key, n_out, wide=True), wide)
        assert torch.equal(tac._hip.resample_fit(g, key, n_out, adjoint=True, length=length, wide=True), wide_adj)
        # ... and left to itself the launcher takes the LDS kernel here: the choice cannot be seen in the result
        before = dict(tac._hip.launches)
        assert torch.equal(fit(tac, x, key, n_out), lds)
        assert launched_since(tac, before) == {LDS: 1}


# ----------------------------------------------------------------------------- out_len
def test_out_len_below_at_and_above(tac):
    orig, new, length = 10079, 8000, 3000
    key = tac._resample.constants(orig, new)
    n_out = R.out_length(length, orig, new)
    x = R.waveform((5, length), seed=8)
    for out_len in (n_out - 1300, n_out - 1, n_out, n_out + 1, n_out + 1100):
        ref, bound = PS.fit_reference(x, orig, new, out_len)
        xt = dev(x).requires_grad_(True)
        got = fit(tac, xt, key, out_len)
        assert tuple(got.shape) == (5, out_len)
        R.assert_close(got, ref, bound, 'out_len %d of %d' % (out_len, n_out))
        assert not bool(got[:, n_out:].any())                               # exactly 0.0, every one written (the poison check)
        # grad_out beyond min(n_out, out_len) does not count, even where it holds NaN
        g = R.waveform((5, out_len), seed=out_len)
        g[:, n_out:] = np.nan
        aref, abound = PS.fit_adjoint_reference(np.nan_to_num(g), length, orig, new)
        before = dict(tac._hip.launches)
        (gx,) = torch.autograd.grad(got, xt, grad_outputs=dev(g))
        assert launched_since(tac, before) == {WIDE: 1}
        R.assert_close(gx, aref, abound, 'gradient, out_len %d of %d' % (out_len, n_out))
    # nothing past out_len is written: one row into the head of a longer poisoned buffer
    out_len = n_out - 1300
    store = tac._hip.poison_fill(torch.empty(out_len + 2048, device='cuda'))
    before = store.clone()
    got = tac._hip.polyphase_wide(dev(x[:1]), key, n_out, out_len, out=store[:out_len].view(1, out_len))
    assert torch.equal(got, fit(tac, dev(x[:1]), key, out_len))
    assert torch.equal(store[out_len:].view(torch.int32), before[out_len:].view(torch.int32))


# ----------------------------------------------------------------------------- NaN reach
@pytest.mark.parametrize('pair, length', [((2000, 2001), 2600), ((10079, 8000), 11000)], ids=str)
def test_nan_reaches_the_outputs_the_rules_say(tac, pair, length):
    orig, new = pair
    key = tac._resample.constants(orig, new)
    n_out = R.out_length(length, orig, new)
    for index in (0, length // 2, 1024 * orig // new - 1, length - 1):
        x = R.waveform((3, length), seed=5 + index)
        x[1, index] = np.nan
        got = fit(tac, dev(x), key, n_out)
        hit = torch.isnan(got).cpu().numpy()
        want = np.zeros_like(hit)
        want[1] = R.reached_by(index, length, orig, new)
        assert want[1].any()
        assert np.array_equal(hit, want), '%s, NaN at %d: %d NaN outputs, expected %d' % (pair, index, int(hit.sum()), int(want.sum()))


# ----------------------------------------------------------------------------- a workgroup's second and third unit
def test_grid_wrap(tac):
    orig, new, out_len = 3, 2, 1500
    key = tac._resample.constants(orig, new)
    b = tac._resample.bank(*key)
    span, tile = tac._hip.resample_wide_plan(b)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = PS.wrap_shape(cus, span, b.K, tile, out_len)
    units, grid = PS.wide_launch(cus, rows, out_len, span, b.K, tile)
    assert 0 < units - 2 * grid < grid and rows % PS.WIDE_ROWS
    length = out_len * orig // new
    assert R.out_length(length, orig, new) == out_len and rows * length * 4 <= PS.MAX_TENSOR_BYTES
    base = dev(R.waveform((5, length), seed=3))
    assert PS.wide_launch(cus, 5, out_len, span, b.K, tile)[0] <= grid
    want = tac._hip.resample_fit(base, key, out_len, wide=True)
    R.assert_close(want, *R.reference(base.cpu().numpy(), orig, new), 'the base rows')
    index = torch.arange(rows, device='cuda') % 5
    before = dict(tac._hip.launches)
    got = tac._hip.resample_fit(base[index], key, out_len, wide=True)
    assert launched_since(tac, before) == {WIDE: 1}
    assert torch.equal(got, want[index])
    # ... and the adjoint, its rows cut to a length that is no multiple of the tile
    g = dev(R.waveform((5, out_len), seed=4))
    want = tac._hip.resample_fit(g, key, out_len, adjoint=True, length=length, wide=True)
    got = tac._hip.resample_fit(g[index], key, out_len, adjoint=True, length=length, wide=True)
    assert torch.equal(got, want[index])


# ----------------------------------------------------------------------------- pitch_shift on the device
@pytest.fixture(scope='module')
def wave():
    return torch.from_numpy(np.random.default_rng(33).standard_normal((2, 2, 4000)).astype(np.float32))


@pytest.mark.parametrize('n_steps', [4, -3])
def test_pitch_shift_on_the_device(tac, wave, n_steps):
    sample_rate, n_fft, hop = 16000, 512, 128
    rate, source, pair = PS.rates(sample_rate, n_steps)
    length = wave.shape[-1]
    xt = dev(wave)
    window = torch.hann_window(n_fft, device='cuda')
    # the three stages one by one: the launches the chain may make, and the tail's input
    before = dict(tac._hip.launches)
    spec = tac.stft(xt.reshape(-1, length), n_fft, hop, n_fft, window)
    advance = torch.linspace(0, np.pi * hop, n_fft // 2 + 1, device='cuda')[:, None]
    stretched = tac.phase_vocoder(spec, rate, advance)
    y = tac.istft(stretched, n_fft, hop, n_fft, window, length=int(round(length / rate)))
    stages = launched_since(tac, before)
    assert stages and WIDE not in stages and LDS not in stages
    before = dict(tac._hip.launches)
    calls = dict(tac._ops.composite_calls)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac.CompositeRouteWarning)
        got = tac.pitch_shift(xt, sample_rate, n_steps)
    assert launched_since(tac, before) == dict(stages, **{WIDE: 1})
    assert tac._ops.composite_calls == calls
    assert tuple(got.shape) == (2, 2, length) and got.dtype == torch.float32
    layer = tac.PitchShift(sample_rate, n_steps).cuda()                      # (its window was evaluated on the host)
    assert torch.equal(layer(xt), tac.pitch_shift(xt, sample_rate, n_steps, window=layer.window))
    # the last stage alone: the device's own istft output through the float64 reference bounds the result per element
    ref, bound = PS.fit_reference(y.cpu().numpy(), source, sample_rate, length)
    ratio = R.assert_close(got.reshape(-1, length), ref, bound, 'the tail of pitch_shift, n_steps %d' % n_steps)
    # the whole chain: against the CPU float64 chain, 4 x the error the CPU float32 chain reaches against it, per row (max norm)
    want = tac.pitch_shift(wave.double(), sample_rate, n_steps).numpy().reshape(-1, length)
    cpu32 = tac.pitch_shift(wave, sample_rate, n_steps).numpy().reshape(-1, length).astype(np.float64)
    allowed = 4.0 * np.abs(cpu32 - want).max(axis=-1)
    err = np.abs(got.cpu().numpy().reshape(-1, length).astype(np.float64) - want).max(axis=-1)
    print('pitch_shift n_steps %d: tail worst |err| / bound %.3f; chain |err| per row %s, allowed %s' % (n_steps, ratio, err, allowed))
    assert (err <= allowed).all(), (err, allowed)


def test_training_through_pitch_shift(tac):
    model = torch.nn.Sequential(tac.PitchShift(16000, 4), *tac.Melspectrogram(fft_length=400, hop_length=160, num_mels=80),
                                tac.AmplitudeToDb()).cuda()
    x = dev(R.waveform((2, 2, 8000), seed=17)).requires_grad_(True)
    calls = dict(tac._ops.composite_calls)
    before = dict(tac._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac.CompositeRouteWarning)
        model(x).square().mean().backward()
    assert tac._ops.composite_calls == calls
    assert launched_since(tac, before).get(WIDE) == 2
    assert bool(torch.isfinite(x.grad).all()) and bool(x.grad.any())
    # the waveform gradient of resample_fit alone, cut and padded
    key = tac._resample.constants(20158, 16000)
    length = 6000
    n_out = R.out_length(length, 10079, 8000)
    for out_len in (n_out - 700, n_out + 300):
        w = dev(R.waveform((3, length), seed=out_len)).requires_grad_(True)
        g = R.waveform((3, out_len), seed=out_len + 1)
        (gw,) = torch.autograd.grad(fit(tac, w, key, out_len), w, grad_outputs=dev(g))
        aref, abound = PS.fit_adjoint_reference(g, length, 10079, 8000)
        R.assert_close(gw, aref, abound, 'gradient of resample_fit, out_len %d' % out_len)


# ----------------------------------------------------------------------------- refusals
def test_routes_outside_the_kernels(tac):
    key = tac._resample.constants(10079, 8000)
    far = tac._resample.constants(96001, 96000)
    x = R.waveform((2, 3000), seed=3)
    xt = dev(x)
    n_out = R.out_length(3000, 10079, 8000)
    calls = [(xt.double(), key, 10079, 8000), (xt[:1].expand(3, 3000), key, 10079, 8000), (xt, far, 96001, 96000)]
    before = dict(tac._hip.launches)
    for xin, k, _, _ in calls:
        with pytest.raises(RuntimeError, match='strict mode'):
            fit(tac, xin, k, n_out)
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.resample(xt, 2000, 2001)                                        # resample itself still refuses what it refused
    # 65 taps a phase (2001 : 2000 at width 32; 63 at width 31 runs) are one more than the last bucket holds: no plan
    wide65 = tac._resample.constants(2001, 2000, lowpass_filter_width=32)
    assert tac._resample.bank(*wide65).K == 65 and tac._hip.resample_wide_plan(tac._resample.bank(*wide65)) is None
    assert tac._hip.resample_wide_plan(tac._resample.bank(*tac._resample.constants(2001, 2000, lowpass_filter_width=31))) is not None
    with pytest.raises(RuntimeError, match='strict mode'):
        fit(tac, xt, wide65, n_out)
    assert launched_since(tac, before) == {}
    tac.set_strict(False)
    try:
        for xin, k, orig, new in calls:
            for seen in [w for w in tac._ops._warned if w[0] == 'resample_fit']:
                tac._ops._warned.discard(seen)
            with pytest.warns(tac.CompositeRouteWarning):
                got = fit(tac, xin, k, n_out)
            with warnings.catch_warnings():
                warnings.simplefilter('error', tac.CompositeRouteWarning)
                fit(tac, xin, k, n_out)                                     # announced once
            assert got.dtype == xin.dtype and launched_since(tac, before) == {}
            ref, bound = PS.fit_reference(xin.cpu().numpy(), orig, new, n_out)
            # the compact composite sums the K_n taps of a phase, in the tensor's dtype
            R.assert_close(got, ref, bound if xin.dtype == torch.float32 else bound * 1e-8 + 1e-300, 'stock-torch route, %s' % xin.dtype)
    finally:
        tac.set_strict(True)
