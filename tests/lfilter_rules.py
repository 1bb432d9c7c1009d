"""Shared by tests/test_lfilter_cpu.py and tests/test_lfilter_gpu.py: the float64 reference of ``lfilter``, its adjoint, and the bound
every float32 result is held to.

Reference: ``scipy.signal.lfilter(b, a, x64)`` with ``a``, ``b`` the exact doubles the op received, ``np.clip`` to [-1, 1] when
``clamp``.  The adjoint (the gradient of ``sum(lfilter(x) * gy)`` w.r.t. ``x``) is the same filter run backwards in time.

Bound, per element, with ``g`` the float64 impulse response of ``1 / A(z)`` (normalised by ``a0``) over the ``L`` samples:

    mass[n] = sum_m |g[n-m]| * ( sum_k |b_k / a0| |x[m-k]| + sum_{k>=1} |a_k / a0| |ref[m-k]| + |ref[m]| )
    |got - ref| <= 2^-24 |ref| + 2^-40 mass[n] + 2^-126

The first term is the one rounding to float32; the second float64 arithmetic in any order of evaluation — every product and sum of
the recursion at sample ``m`` is rounded at 2^-53 of its magnitude and reaches sample ``n`` through ``g[n-m]`` — with about 2^13 of
slack; the third lets the output flush denormals.  With ``clamp`` both sides are compared after clipping, under the same bound
(clipping is a contraction)."""
import numpy as np
import scipy.signal
import torch

EPS32 = 2.0 ** -24
EPS_ARITH = 2.0 ** -40
TINY = 2.0 ** -126


def _np64(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(np.float64)


def coeffs64(b, a):
    b = np.atleast_1d(_np64(b))
    a = np.atleast_1d(_np64(a))
    assert b.ndim == 1 and a.ndim == 1 and b.size == a.size and a[0] != 0.0
    return b, a


def _causal_conv(kernel, u):
    """sum_m kernel[n-m] u[..., m] over the last axis, both non-negative.  Short rows: the sums themselves.  Long rows: an FFT
    convolution, whose absolute noise is ~1e-16 of the row's largest sum; every element below 1e-10 of that (the stretches of
    zeros and of 1e-30) is recomputed as its own sum, so no element is off by more than 1e-6 of itself.  Those sums leave out
    the tail of the kernel behind its last tap of 1e-200 or more (denormal arithmetic is slow): that lowers the bound, by less
    than 1e-200 of the input, and never raises it."""
    length = u.shape[-1]
    flat = u.reshape(-1, length)
    if length <= 2048:
        out = np.stack([np.convolve(row, kernel)[:length] for row in flat])
        return out.reshape(u.shape)
    out = scipy.signal.fftconvolve(flat, kernel[None, :], mode='full', axes=-1)[:, :length]
    small = out < 1e-10 * out.max(axis=-1, keepdims=True)
    flipped = np.ascontiguousarray(kernel[::-1])                 # flipped[length - 1 - n:] = kernel[n], kernel[n - 1], ..., kernel[0]
    flat = np.ascontiguousarray(flat)
    big = np.nonzero(kernel >= 1e-200)[0]
    taps = int(big[-1]) + 1 if big.size else 1
    for n in np.nonzero(small.any(axis=0))[0]:
        lo = max(0, n + 1 - taps)
        out[:, n] = np.where(small[:, n], flat[:, lo:n + 1] @ flipped[length - 1 - n + lo:], out[:, n])
    return out.reshape(u.shape)


def reference(x, b, a, clamp=False):
    """float64 ``(…, L) -> (…, L)`` and the per-element bound"""
    b, a = coeffs64(b, a)
    x64 = _np64(x)
    length = x64.shape[-1]
    raw = scipy.signal.lfilter(b, a, x64, axis=-1)
    bn, an = np.abs(b / a[0]), np.abs(a / a[0])
    ax, ar = np.abs(x64), np.abs(raw)
    inner = ar.copy()
    for k in range(b.size):
        if k < length:
            inner[..., k:] += bn[k] * ax[..., :length - k]
            if k >= 1:
                inner[..., k:] += an[k] * ar[..., :length - k]
    impulse = np.zeros(length)
    impulse[0] = 1.0
    g = np.abs(scipy.signal.lfilter([1.0], a / a[0], impulse))
    mass = _causal_conv(g, inner)
    bound = EPS32 * ar + EPS_ARITH * mass + TINY
    ref = np.clip(raw, -1.0, 1.0) if clamp else raw
    return ref, bound


def adjoint_reference(gy, b, a):
    """float64 gradient of ``sum(lfilter(x, a, b, clamp=False) * gy)`` w.r.t. ``x`` and its bound: the filter run on the reversed
    ``gy``, reversed back.  (With ``clamp`` the caller zeroes ``gy`` where the forward result was clipped.)"""
    g64 = _np64(gy)
    ref, bound = reference(g64[..., ::-1], b, a, clamp=False)
    return ref[..., ::-1], bound[..., ::-1]


def assert_close(got, ref, bound, what):
    """every element of ``got`` within ``bound`` of ``ref``; NaN fails.  Returns the worst |err| / bound."""
    g = _np64(got)
    assert g.shape == ref.shape, '%s: shape %s, expected %s' % (what, g.shape, ref.shape)
    assert not np.isnan(g).any(), '%s: %d NaN elements' % (what, int(np.isnan(g).sum()))
    err = np.abs(g - ref)
    bad = err > bound
    ratio = float((err / bound).max()) if err.size else 0.0
    assert not bad.any(), '%s: %d of %d elements beyond the bound, worst |err| / bound = %.3g (|err| %.3g)' % (
        what, int(bad.sum()), bad.size, ratio, float(err.max()))
    return ratio


def waveform(shape, seed):
    """``randn`` with a stretch of exact zeros and a stretch at 1e-30 scale (where the length has room for them), as
    ``resample_rules.waveform``"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    length = shape[-1]
    if length >= 16:
        x[..., length // 4: length // 4 + length // 8] = 0.0
        x[..., length // 2: length // 2 + length // 8] *= np.float32(1e-30)
    return x


# The filters of the issue's numerical cases, as (name, b, a) in float64 — b, a as the product's own designs give them
def filters(tac):
    f = tac._filters
    c = 0.97
    return [
        ('order 1', (0.5, 0.25), (1.0, -0.9)),
        ('order 2', (0.2, 0.3, 0.1), (1.0, -1.2, 0.52)),
        ('high-pass 20 Hz at 48 kHz',) + f.highpass(48000, 20.0),
        ('high-pass 100 Hz at 16 kHz',) + f.highpass(16000, 100.0),
        ('low-pass 1 kHz at 16 kHz, Q 10',) + f.lowpass(16000, 1000.0, 10.0),
        ('deemphasis 0.97', (1.0, 0.0), (1.0, -c)),
        ('preemphasis 0.97', (1.0, -c), (1.0, 0.0)),
    ]
