"""Shared by tests/test_resample_cpu.py and tests/test_resample_gpu.py: the float64 reference of ``resample`` written from the
definition as a sum per output sample (no bank, no convolution: it shares no structure with the product), its adjoint, and the
bound every float32 result is held to.

With ``orig``, ``new`` the rates divided by their gcd, ``base = min(orig, new) * rolloff``, ``width = ceil(lpw * orig / base)``,
``scale = base / orig``, output ``n = j * new + p``:

    y[n] = sum_{d = -width}^{width + orig - 1} h(p, d) * x[j * orig + d]          x zero outside [0, L)
    t = base * (d / orig - p / new);   h = scale * sinc(pi t) * w(t) if |t| < lpw else 0

The bound, per element:

    |got - ref| <= (K_n + 2) * 2^-24 * sum_d |h64(p, d)| * |x[j * orig + d]|

``K_n`` the number of taps of output ``n`` with ``|t| < lpw``: the standard bound of a float32 dot product of ``K_n`` terms in ANY
summation order, plus one rounding of the tap to float32 and one of the result — the derivation of tests/dct_rules.py."""
import math

import numpy as np
import torch

EPS = 2.0 ** -24
KAISER_BETA = 14.769656459379492


def reduced(orig_freq, new_freq):
    g = math.gcd(orig_freq, new_freq)
    return orig_freq // g, new_freq // g


def filter_constants(orig, new, lpw, rolloff):
    base = min(orig, new) * rolloff
    return base, int(math.ceil(lpw * orig / base)), base / orig


def out_length(length, orig, new):
    return -((-new * length) // orig)


_phase_cache = {}


def phase_taps(orig, new, p, lpw=6, rolloff=0.99, method='sinc_interp_hann', beta=None):
    """(d, h): the offsets ``d`` of phase ``p`` with ``|t| < lpw`` inside ``[-width, width + orig)`` and their float64 taps"""
    key = (orig, new, p, lpw, rolloff, method, beta)
    hit = _phase_cache.get(key)
    if hit is None:
        base, width, scale = filter_constants(orig, new, lpw, rolloff)
        d = np.arange(-width, width + orig, dtype=np.int64)
        t = base * (d.astype(np.float64) / orig - float(p) / new)
        keep = np.abs(t) < lpw
        d, t = d[keep], t[keep]
        with np.errstate(invalid='ignore', divide='ignore'):
            sinc = np.where(t == 0.0, 1.0, np.sin(np.pi * t) / (np.pi * t))
        if method == 'sinc_interp_hann':
            w = np.cos(np.pi * t / (2.0 * lpw)) ** 2
        else:
            assert method == 'sinc_interp_kaiser'
            b = KAISER_BETA if beta is None else beta
            w = np.i0(b * np.sqrt(np.maximum(1.0 - (t / lpw) ** 2, 0.0))) / np.i0(b)
        if len(_phase_cache) > 20000:
            _phase_cache.clear()
        hit = _phase_cache[key] = (d, scale * sinc * w)
    return hit


def _np64(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(np.float64)


def reference(x, orig_freq, new_freq, lpw=6, rolloff=0.99, method='sinc_interp_hann', beta=None):
    """float64 ``(…, L) -> (…, ceil(new L / orig))`` and the per-element bound"""
    orig, new = reduced(orig_freq, new_freq)
    x64 = _np64(x)
    length = x64.shape[-1]
    n_out = out_length(length, orig, new)
    ref = np.zeros(x64.shape[:-1] + (n_out,))
    bound = np.zeros_like(ref)
    ax = np.abs(x64)
    for n in range(n_out):
        j, p = divmod(n, new)
        d, h = phase_taps(orig, new, p, lpw, rolloff, method, beta)
        idx = j * orig + d
        ok = (idx >= 0) & (idx < length)
        ref[..., n] = x64[..., idx[ok]] @ h[ok]
        bound[..., n] = (len(d) + 2) * EPS * (ax[..., idx[ok]] @ np.abs(h[ok]))
    return ref, bound


def adjoint_reference(g, length, orig_freq, new_freq, lpw=6, rolloff=0.99, method='sinc_interp_hann', beta=None):
    """float64 gradient of ``sum(resample(x) * g)`` w.r.t. ``x`` of ``length`` samples, and its bound: every output sample hands
    its taps back to the inputs it read.  ``K`` of the bound: the number of outputs that read the input sample."""
    orig, new = reduced(orig_freq, new_freq)
    g64 = _np64(g)
    assert g64.shape[-1] == out_length(length, orig, new)
    ref = np.zeros(g64.shape[:-1] + (length,))
    mass = np.zeros_like(ref)
    count = np.zeros(length)
    ag = np.abs(g64)
    for n in range(g64.shape[-1]):
        j, p = divmod(n, new)
        d, h = phase_taps(orig, new, p, lpw, rolloff, method, beta)
        idx = j * orig + d
        ok = (idx >= 0) & (idx < length)
        ref[..., idx[ok]] += g64[..., n:n + 1] * h[ok]
        mass[..., idx[ok]] += ag[..., n:n + 1] * np.abs(h[ok])
        count[idx[ok]] += 1
    return ref, (count + 2) * EPS * mass


def reached_by(index, length, orig_freq, new_freq, lpw=6, rolloff=0.99, method='sinc_interp_hann', beta=None):
    """boolean (n_out,): the outputs with a tap ``|t| < lpw`` on input sample ``index``"""
    orig, new = reduced(orig_freq, new_freq)
    n_out = out_length(length, orig, new)
    hit = np.zeros(n_out, dtype=bool)
    for n in range(n_out):
        j, p = divmod(n, new)
        d, _ = phase_taps(orig, new, p, lpw, rolloff, method, beta)
        hit[n] = bool(((j * orig + d) == index).any())
    return hit


def assert_close(got, ref, bound, what):
    """every element of ``got`` within ``bound`` of ``ref``; NaN fails.  Returns the worst |err| / bound."""
    g = _np64(got)
    assert g.shape == ref.shape, '%s: shape %s, expected %s' % (what, g.shape, ref.shape)
    assert not np.isnan(g).any(), '%s: %d NaN elements' % (what, int(np.isnan(g).sum()))
    err = np.abs(g - ref)
    bad = err > bound
    ratio = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max()) if err.size else 0.0
    assert not bad.any(), '%s: %d of %d elements beyond the bound, worst |err| / bound = %.3g (|err| %.3g)' % (
        what, int(bad.sum()), bad.size, ratio, float(err.max()))
    return ratio


def assert_within(got, x, orig_freq, new_freq, what, **kw):
    ref, bound = reference(x, orig_freq, new_freq, **kw)
    return assert_close(got, ref, bound, what)


def waveform(shape, seed):
    """``randn`` with a stretch of exact zeros and a stretch at 1e-30 scale (where the length has room for them)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    length = shape[-1]
    if length >= 16:
        x[..., length // 4: length // 4 + length // 8] = 0.0
        x[..., length // 2: length // 2 + length // 8] *= np.float32(1e-30)
    return x
