"""``resample`` / ``Resample`` without a device: the product's compact bank against the float64 taps of tests/resample_rules.py,
the CPU route (torch's ``conv1d`` with the full bank) under the rules' bound, output lengths, the reduced-rate and identity cases,
argument errors, the adjoint bank, tracing, the layer, and the C ABI surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import resample_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = [(2, 1), (1, 2), (3, 1), (3, 2), (2, 3), (7, 5), (147, 160), (441, 160), (160, 441)]
FILTERS = [dict(), dict(lpw=16, rolloff=0.9), dict(method='sinc_interp_kaiser'), dict(method='sinc_interp_kaiser', beta=9.5),
           dict(lpw=1, rolloff=1.0)]


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


def product_kw(kw):
    """the rules' short names -> the public argument names"""
    names = dict(lpw='lowpass_filter_width', rolloff='rolloff', method='resampling_method', beta='beta')
    return {names[k]: v for k, v in kw.items()}


def product_bank(tac_, orig, new, kw, adjoint=False):
    RS = tac_._resample
    key = RS.constants(orig, new, **product_kw(kw))
    return (RS.adjoint_bank if adjoint else RS.bank)(*key)


# ----------------------------------------------------------------------------- the bank
@pytest.mark.parametrize('kw', FILTERS, ids=lambda k: '-'.join('%s' % v for v in k.values()) or 'default')
@pytest.mark.parametrize('orig,new', RATIOS)
def test_bank_is_the_formula_rounded_once(tac, orig, new, kw):
    """float32(bank) against the rules' float64 taps to 2^-24 relative; off, run and K exactly.  (The 1e-15: torch's and numpy's
    float64 sines may differ in their last bits, which near a zero of the sinc is not a relative 2^-53 of the tap.)"""
    b = product_bank(tac, orig, new, kw)
    assert (b.phases, b.step) == (new, orig) and tuple(b.taps.shape) == (new, b.K) and b.taps.dtype == torch.float64
    b32 = b.taps.to(torch.float32).numpy().astype(np.float64)
    longest = 0
    for p in range(new):
        d, h = R.phase_taps(orig, new, p, **kw)
        longest = max(longest, len(d))
        assert len(d) > 0 and b.off[p] == d[0] and b.run[p] == len(d), (p, b.off[p], b.run[p], d[:1], len(d))
        assert (np.diff(d) == 1).all()                                   # the run is contiguous
        assert (np.abs(b32[p, :len(d)] - h) <= R.EPS * np.abs(h) + 1e-15).all(), p
        assert not b32[p, len(d):].any()
    assert b.K == longest


def test_compact_sizes_of_the_speech_pairs(tac):
    """the figures DESIGN 3.11 quotes"""
    b = product_bank(tac, 44100, 16000, {})
    assert (b.phases, b.K) == (160, 34)
    b = product_bank(tac, 16000, 44100, {})
    assert (b.phases, b.K) == (441, 13)
    b = product_bank(tac, 48000, 16000, {})
    assert (b.phases, b.K, b.off) == (1, 37, [-18])
    rates = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000)
    largest = 0
    for a in rates:
        for c in rates:
            if a != c:
                key = tac._resample.constants(a, c)
                assert tac._hip.resample_covers(*key), (a, c)
                for bank in (tac._resample.bank(*key), tac._resample.adjoint_bank(*key)):
                    largest = max(largest, bank.phases * bank.K)
    assert largest <= tac._hip.RESAMPLE_MAX_BANK == 20480
    assert not tac._hip.resample_covers(*tac._resample.constants(2000, 2001))
    assert not tac._hip.resample_covers(*tac._resample.constants(44100, 44101))      # (decided without forming 44101 x 44114)


def test_kaiser_default_beta(tac):
    a = product_bank(tac, 3, 2, dict(method='sinc_interp_kaiser'))
    b = product_bank(tac, 3, 2, dict(method='sinc_interp_kaiser', beta=14.769656459379492))
    c = product_bank(tac, 3, 2, dict(method='sinc_interp_kaiser', beta=14.0))
    assert tac._resample.KAISER_BETA == 14.769656459379492
    assert torch.equal(a.taps, b.taps) and not torch.equal(a.taps, c.taps)
    x = torch.randn(2, 50)
    assert torch.equal(tac.resample(x, 3, 2, resampling_method='sinc_interp_kaiser'),
                       tac.resample(x, 3, 2, resampling_method='sinc_interp_kaiser', beta=14.769656459379492))


# ----------------------------------------------------------------------------- the CPU route
@pytest.mark.parametrize('kw', FILTERS[:3], ids=('hann', 'wide', 'kaiser'))
@pytest.mark.parametrize('orig,new', RATIOS)
def test_cpu_float32_within_the_bound(tac, orig, new, kw):
    x = R.waveform((3, 4 * orig + 37), seed=orig + new)
    got = tac.resample(torch.from_numpy(x), orig, new, **product_kw(kw))
    assert got.dtype == torch.float32
    ratio = R.assert_within(got, x, orig, new, 'cpu float32 %d:%d %r' % (orig, new, kw), **kw)
    print('cpu %d:%d %r: worst |err| / bound %.3f' % (orig, new, kw, ratio))


@pytest.mark.parametrize('orig,new', [(3, 2), (2, 3), (7, 5), (441, 160), (160, 441)])
def test_cpu_float64_is_the_per_sample_sum(tac, orig, new):
    """the conv1d form against the per-output-sample sum, both float64: a few 1e-16 of the sum of absolute products"""
    x = torch.randn(2, 3 * orig + 11, dtype=torch.float64)
    got = tac.resample(x, orig, new)
    ref, bound = R.reference(x, orig, new)
    assert got.dtype == torch.float64 and (np.abs(got.numpy() - ref) <= 1e-8 * bound + 1e-300).all()


@pytest.mark.parametrize('orig,new', [(3, 2), (2, 3), (441, 160), (3, 1)])
def test_output_length(tac, orig, new):
    for length in (1, 2, orig - 1, orig, orig + 1, 2 * orig - 1, 2 * orig, 2 * orig + 1, 5 * orig + 2):
        if length < 1:
            continue
        got = tac.resample(torch.randn(2, 3, length), orig, new)
        assert tuple(got.shape) == (2, 3, -(-new * length // orig)), length
    assert tuple(tac.resample(torch.zeros(4, 0), orig, new).shape) == (4, 0)
    assert tuple(tac.resample(torch.randn(7), orig, new).shape) == (-(-new * 7 // orig),)


def test_equal_rates_and_reduced_pairs(tac):
    x = torch.randn(2, 100)
    assert tac.resample(x, 16000, 16000) is x and tac.resample(x, 7, 7) is x
    assert tac.Resample()(x) is x
    for a, b, ra, rb in ((48000, 16000, 3, 1), (44100, 16000, 441, 160), (32000, 48000, 2, 3)):
        assert torch.equal(tac.resample(x, a, b), tac.resample(x, ra, rb))


def test_argument_errors(tac):
    x = torch.randn(2, 50)
    for bad in ((0, 2), (2, 0), (-3, 2), (2, -1), (3.0, 2), (2, 1.5), ('3', 2), (True, 2)):
        with pytest.raises(ValueError):
            tac.resample(x, *bad)
    for kw in (dict(lowpass_filter_width=0), dict(lowpass_filter_width=-2), dict(lowpass_filter_width=6.0), dict(rolloff=0.0),
               dict(rolloff=1.01), dict(rolloff=-0.5), dict(resampling_method='linear'), dict(resampling_method='kaiser_best')):
        with pytest.raises(ValueError):
            tac.resample(x, 3, 2, **kw)
        with pytest.raises(ValueError):
            tac.Resample(3, 2, **kw)
    with pytest.raises(ValueError):
        tac.resample(x, 5, 5, rolloff=2.0)                      # (checked before the identity is taken)
    with pytest.raises(TypeError):
        tac.resample(x.numpy(), 3, 2)
    with pytest.raises(RuntimeError):
        tac.resample(torch.zeros(2, 50, dtype=torch.int64), 3, 2)
    tac.resample(x, 3, 2, rolloff=1.0)


# ----------------------------------------------------------------------------- the adjoint bank
@pytest.mark.parametrize('kw', FILTERS[:2], ids=('hann', 'wide'))
@pytest.mark.parametrize('orig,new', RATIOS)
def test_adjoint_bank_pairs_with_the_forward_bank(tac, orig, new, kw):
    """<resample(x), g> = <x, adjoint(g)> in float64 through the product's own banks, lengths that cut blocks at both ends"""
    RS = tac._resample
    f = product_bank(tac, orig, new, kw)
    a = product_bank(tac, orig, new, kw, adjoint=True)
    assert (a.phases, a.step) == (orig, new)
    gen = torch.Generator().manual_seed(orig * 1000 + new)
    for length in (1, orig + 1, 3 * orig + 5):
        n_out = RS.out_length(length, orig, new)
        x = torch.randn(2, length, dtype=torch.float64, generator=gen)
        g = torch.randn(2, n_out, dtype=torch.float64, generator=gen)
        y = RS.apply_bank64(f, x, n_out)
        back = RS.apply_bank64(a, g, length)
        lhs, rhs = float((y * g).sum()), float((x * back).sum())
        assert abs(lhs - rhs) <= 1e-12 * float((y.abs() * g.abs()).sum()), (length, lhs, rhs)
        # and both are the rules' sums
        ref, bound = R.reference(x, orig, new, **kw)
        assert (np.abs(y.numpy() - ref) <= 1e-8 * bound + 1e-300).all()
        aref, abound = R.adjoint_reference(g, length, orig, new, **kw)
        assert (np.abs(back.numpy() - aref) <= 1e-8 * abound + 1e-300).all()


def test_gradient_on_the_cpu(tac):
    x = torch.randn(2, 23, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: tac.resample(t, 3, 2), (x,))
    assert torch.autograd.gradgradcheck(lambda t: tac.resample(t, 2, 3), (x,))
    xf = torch.randn(2, 40, requires_grad=True)
    g = torch.randn(2, 27)
    tac.resample(xf, 3, 2).backward(g)
    aref, abound = R.adjoint_reference(g, 40, 3, 2)
    R.assert_close(xf.grad, aref, abound, 'cpu float32 gradient 3:2')


# ----------------------------------------------------------------------------- tracing
def test_fake_kernel_shape_under_compile(tac):
    seen = []

    def capture(gm, example_inputs):
        seen.extend(n.target for n in gm.graph.nodes if n.op == 'call_function')
        return gm.forward

    torch._dynamo.reset()
    layer = tac.Resample(44100, 16000)
    x = torch.randn(2, 3, 1000)
    out = torch.compile(layer, backend=capture, fullgraph=True)(x)
    names = [str(t) for t in seen]
    assert sum('tac_amd.resample' in n for n in names) == 1 and len(names) == 1, names
    eager = layer(x)
    assert torch.equal(out, eager)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode() as mode:
        fake = torch.ops.tac_amd.resample(mode.from_tensor(x), 441, 160, 6, 0.99, 'sinc_interp_hann', None)
    assert tuple(fake.shape) == tuple(eager.shape) == (2, 3, 363) and fake.dtype == eager.dtype
    assert fake.stride() == eager.stride() == (3 * 363, 363, 1)


# ----------------------------------------------------------------------------- the layer
def test_layer(tac):
    m = tac.Resample(48000, 16000)
    assert repr(m) == ('Resample(orig_freq=48000, new_freq=16000, lowpass_filter_width=6, rolloff=0.99, '
                       'resampling_method=sinc_interp_hann, beta=None)')
    assert repr(tac.Resample()) == ('Resample(orig_freq=16000, new_freq=16000, lowpass_filter_width=6, rolloff=0.99, '
                                    'resampling_method=sinc_interp_hann, beta=None)')
    assert m.state_dict() == {} and [n for n, _ in m.named_buffers()] == ['bank']
    assert m.bank.dtype == torch.float32 and tuple(m.bank.shape) == (1, 37)
    assert tuple(tac.Resample(44100, 16000).bank.shape) == (160, 34)
    m.load_state_dict({})
    x = torch.randn(2, 1, 3000)
    assert torch.equal(m(x), tac.resample(x, 48000, 16000))
    chain = torch.nn.Sequential(m, *tac.Melspectrogram(num_mels=80, sample_rate=16000, fft_length=400, hop_length=160),
                                tac.AmplitudeToDb())
    assert chain.state_dict() == {}
    got = chain(x)
    want = tac.AmplitudeToDb()(tac.Melspectrogram(num_mels=80, sample_rate=16000, fft_length=400, hop_length=160)(m(x)))
    assert type(got) is torch.Tensor and tuple(got.shape) == (2, 1, 80, 7) and torch.equal(got, want)


def test_names_are_exported(tac):
    assert 'resample' in tac.functional.__all__ and tac.resample is tac.functional.resample
    assert tac.Resample is tac.layers.Resample
    assert 'resample' in tac._ops.cuda_kernels and hasattr(torch.ops.tac_amd, 'resample')


# ----------------------------------------------------------------------------- a band-limited signal
def test_a_sine_below_both_nyquist_rates():
    """A 1 kHz sine, 48000 -> 16000, against the 16 kHz sine away from the edges.  Asserted: the float64 reference and the product
    agree within the bound.  Recorded, not asserted: the float64 reference's own deviation from the ideal sine over the samples
    more than 2 * width / 3 = 12 output samples from either end is 3.99e-4 of the amplitude (the Hann-windowed sinc of 6 zero
    crossings at rolloff 0.99 is not an ideal low-pass: that is its pass-band ripple at 1 kHz)."""
    import torchaudio_contrib_amd as tac
    n_in = 4800
    x = np.sin(2.0 * np.pi * 1000.0 * np.arange(n_in) / 48000.0)
    ref, bound = R.reference(x.astype(np.float32), 48000, 16000)
    got = tac.resample(torch.from_numpy(x.astype(np.float32)), 48000, 16000)
    R.assert_close(got, ref, bound, '1 kHz sine 48000 -> 16000')
    ideal = np.sin(2.0 * np.pi * 1000.0 * np.arange(ref.shape[-1]) / 16000.0)
    inner = slice(12, ref.shape[-1] - 12)
    exact64, _ = R.reference(x, 48000, 16000)
    print('1 kHz sine 48000 -> 16000: float64 reference deviates from the ideal sine by %.3g of the amplitude'
          % np.abs(exact64[inner] - ideal[inner]).max())


# ----------------------------------------------------------------------------- C ABI
def test_entry_point_is_declared_and_exported(tac):
    header = open(os.path.join(ROOT, 'include', 'tac_amd.h')).read()
    assert re.search(r'\bint\s+tac_polyphase_f32\s*\(', header) and '(15)' in header
    assert 'tac_polyphase_f32' in tac._native.EXPORTS
    if not os.path.exists(tac._native.LIB_PATH):
        tac.build_native()
    h = tac._native.lib()
    assert h.tac_abi_version() == 5
    fn = h.tac_polyphase_f32
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 15
    # refusals come before anything touches a device: null pointers, empty axes, an inconsistent table, sizes beyond the caps
    p = ctypes.c_void_p(4096)
    ok = dict(x=p, rows=1, l_in=100, stride_r=100, bank=p, table=p, phases=2, taps=13, taps_min=12, step=3, off_min=-6,
              off_max=-5, l_out=67, out=p, stream=None)

    def call(**over):
        return fn(*dict(ok, **over).values())

    inv, uns = tac._native.TAC_E_INVALID, tac._native.TAC_E_UNSUPPORTED
    for over in (dict(x=None), dict(bank=None), dict(table=None), dict(out=None), dict(rows=0), dict(l_in=0), dict(l_out=0),
                 dict(phases=0), dict(taps=0), dict(step=0), dict(taps_min=14), dict(taps_min=-1), dict(off_min=-4),
                 dict(rows=2, stride_r=0), dict(rows=2, stride_r=-100)):
        assert call(**over) == inv, over
    for over in (dict(phases=2049, taps=1, taps_min=1), dict(phases=1024, taps=21, taps_min=21), dict(step=100000),
                 dict(off_max=20000), dict(off_min=-(2 ** 31), off_max=2 ** 31 - 1)):
        assert call(**over) == uns, over
