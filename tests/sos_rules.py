"""Shared by tests/test_sosfilt_cpu.py and tests/test_sosfilt_gpu.py: the float64 references of ``sosfilt``, its adjoint and
``filtfilt``, the bound every float32 result is held to, the filters, and a float64 emulation of the kernel's tile scan.  No tests
in here, and no tolerance of its own: every bound is composed from ``lfilter_rules.reference``, as ``loudness_rules`` composes two
stages.

Reference: ``scipy.signal.sosfilt`` in float64, ``np.clip`` to [-1, 1] when ``clamp``.

Bound, per element.  Section ``s`` receives the float64 signal ``u_s`` (``u_0 = x``, ``u_{s+1}`` the section's exact output);
``(raw_s, bound_s) = lfilter_rules.reference(u_s, b_s, a_s)``; its arithmetic term is ``arith_s = bound_s - 2^-24 |raw_s| - 2^-126``
(nothing between two sections is rounded to float32); ``h_s`` is its float64 impulse response.  A section is linear, so the error
``d_{s-1}`` of its input reaches its output through ``|h_s|`` and its own arithmetic adds ``arith_s``:

    d_0 = 0,   d_s = _causal_conv(|h_s|, d_{s-1}) + arith_s,   |got - ref| <= 2^-24 |ref| + d_S + 2^-126

For ``sosfilt(x, tf2sos(b, a))`` there is a second yardstick, ``lfilter_rules.reference(x, b, a)`` unchanged (the direct-form float64
filter): root finding is backward stable in the coefficients and that bound's mass term carries ``|a_k| |ref|``.

``filtfilt``: the first half's whole bound (its rounding to float32 included) reaches the result through ``|h|`` of the second half
— a causal convolution on the reversed row — and the second half adds its own bound.  The adjoint of a cascade is the same rule on
the reversed ``grad_out`` with the sections reversed."""
import functools

import numpy as np
import scipy.signal

import lfilter_rules as L

EPS32, TINY = L.EPS32, L.TINY
assert_close = L.assert_close
waveform = L.waveform


# ----------------------------------------------------------------------------- the filters
def a_weighting(fs):
    """IEC 61672 A-weighting: the analog prototype through the bilinear transform (order 6)"""
    f1, f2, f3, f4, a1000 = 20.598997, 107.65265, 737.86223, 12194.217, 1.9997
    num = [(2 * np.pi * f4) ** 2 * 10 ** (a1000 / 20), 0.0, 0.0, 0.0, 0.0]
    den = np.polymul([1.0, 4 * np.pi * f4, (2 * np.pi * f4) ** 2], [1.0, 4 * np.pi * f1, (2 * np.pi * f1) ** 2])
    den = np.polymul(np.polymul(den, [1.0, 2 * np.pi * f3]), [1.0, 2 * np.pi * f2])
    return scipy.signal.bilinear(num, den, fs)


@functools.lru_cache(maxsize=None)
def filters():
    """``(name, b, a)`` with ``b``, ``a`` tuples of floats: scipy's designs in transfer-function form"""
    s = scipy.signal
    designs = [
        ('butter 4 band-pass 300-3400 Hz at 16 kHz', s.butter(4, [300, 3400], 'bandpass', fs=16000)),
        ('butter 3 high-pass 100 Hz at 16 kHz', s.butter(3, 100, 'highpass', fs=16000)),
        ('butter 6 low-pass 4 kHz at 16 kHz', s.butter(6, 4000, fs=16000)),
        ('butter 8 low-pass 2 kHz at 16 kHz', s.butter(8, 2000, fs=16000)),
        ('ellip 5 low-pass 3400 Hz at 16 kHz', s.ellip(5, 0.5, 60, 3400, fs=16000)),
        ('cheby1 4 band-pass 1-3 kHz at 16 kHz', s.cheby1(4, 1, [1000, 3000], 'bandpass', fs=16000)),
        ('butter 4 high-pass 20 Hz at 48 kHz', s.butter(4, 20, 'highpass', fs=48000)),
        ('butter 2 band-pass 50-150 Hz at 16 kHz', s.butter(2, [50, 150], 'bandpass', fs=16000)),
        ('butter 8 low-pass 500 Hz at 16 kHz', s.butter(8, 500, fs=16000)),
        ('butter 6 band-pass 500-2000 Hz at 16 kHz', s.butter(6, [500, 2000], 'bandpass', fs=16000)),
        ('A-weighting at 48 kHz', a_weighting(48000)),
    ]
    return tuple((name, tuple(float(v) for v in b), tuple(float(v) for v in a)) for name, (b, a) in designs)


NAMES = tuple(name for name, _, _ in filters())
BANDPASS8, ODD = NAMES[0], NAMES[1]


def named(name):
    (hit,) = [f for f in filters() if f[0] == name]
    return hit


def sections_of(tac, name):
    """``tf2sos`` of a listed filter as a float64 numpy array ``(S, 6)``"""
    _, b, a = named(name)
    return tac.tf2sos(b, a).numpy().copy()


# ----------------------------------------------------------------------------- references and bounds
def _sos64(sos):
    sos = np.asarray(L._np64(sos), dtype=np.float64)
    assert sos.ndim == 2 and sos.shape[1] == 6 and sos.shape[0] >= 1 and (sos[:, 3] != 0.0).all()
    return sos


def _unit_a0(sos):
    return sos / sos[:, 3:4]                    # (scipy.signal.sosfilt takes a0 = 1 only)


def _impulse(sos, length):
    unit = np.zeros(length)
    unit[0] = 1.0
    return scipy.signal.sosfilt(_unit_a0(sos), unit)


def _cascade(x, sos):
    """float64 result of the cascade without clamp, its bound, and the arithmetic error ``d_S`` alone"""
    sos = _sos64(sos)
    u = L._np64(x)
    d = np.zeros_like(u)
    for row in sos:
        raw, bound = L.reference(u, row[:3], row[3:])
        arith = bound - EPS32 * np.abs(raw) - TINY
        d = L._causal_conv(np.abs(_impulse(row[None, :], u.shape[-1])), d) + arith
        u = raw
    ref = scipy.signal.sosfilt(_unit_a0(sos), L._np64(x), axis=-1)
    return ref, EPS32 * np.abs(ref) + d + TINY, d


def reference(x, sos, clamp=False):
    """float64 ``(…, L) -> (…, L)`` and the per-element bound"""
    raw, bound, _ = _cascade(x, sos)
    return (np.clip(raw, -1.0, 1.0) if clamp else raw), bound


def arithmetic_budget(x, sos):
    """``(ref, d_S)``: the unclamped float64 reference and the stage-composed arithmetic error on its own"""
    raw, _, d = _cascade(x, sos)
    return raw, d


def adjoint_reference(gy, sos):
    """float64 gradient of ``sum(sosfilt(x, sos) * gy)`` w.r.t. ``x`` and its bound: the sections in reverse order over the
    reversed ``gy``, reversed back.  (With ``clamp`` the caller zeroes ``gy`` where the forward result was clipped.)"""
    ref, bound = reference(L._np64(gy)[..., ::-1], _sos64(sos)[::-1])
    return ref[..., ::-1], bound[..., ::-1]


def filtfilt_reference(x, sos, clamp=False):
    """``filtfilt`` of the filter whose sections are ``sos`` (one row ``(b, a)`` for orders up to 2): the float64 reference — the
    float64 forward result filtered again from its end — and the bound"""
    sos = _sos64(sos)
    first, first_bound = reference(x, sos)
    raw, bound = reference(first[..., ::-1], sos[::-1])
    carried = L._causal_conv(np.abs(_impulse(sos, first.shape[-1])), np.ascontiguousarray(first_bound[..., ::-1]))
    ref = np.clip(raw, -1.0, 1.0) if clamp else raw
    return ref[..., ::-1], (bound + carried)[..., ::-1]


# ----------------------------------------------------------------------------- the kernel's tile scan, in float64 numpy
C, THREADS = 16, 1024
TILE = C * THREADS


def _powers(a1, a2):
    """M^(C 2^i), i < 10, for M = [[-a1, -a2], [1, 0]]: repeated products in float64, as the host fills them"""
    m = np.array([[-a1, -a2], [1.0, 0.0]])
    q = m.copy()
    for _ in range(C - 1):
        q = q @ m
    out = []
    for _ in range(10):
        out.append(q.copy())
        q = q @ q
    return out


def _apply(m, u0, u1):
    return m[0, 0] * u0 + m[0, 1] * u1, m[1, 0] * u0 + m[1, 1] * u1


def emulate(x, sos):
    """What csrc/sosfilt.hip computes before its one rounding, in float64 numpy: tiles of ``TILE`` samples, a chunk of ``C`` per
    lane, per section the numerator, pass 1 from zero state, Kogge-Stone over ``M^(C 2^i)`` (six steps in a wave of 64 lanes, four
    across the sixteen waves, then ``M^(C lane)`` by the bits of the lane), pass 2, and the carries from tile to tile."""
    sos = _sos64(sos)
    sos = sos / sos[:, 3:4]
    x = np.atleast_2d(L._np64(x))
    rows, length = x.shape
    powers = [_powers(r[4], r[5]) for r in sos]
    lane_bits = np.arange(64)
    out = np.empty_like(x)
    hist = np.zeros((len(sos) + 1, rows, 2))
    for n0 in range(0, length, TILE):
        nt = min(TILE, length - n0)
        flat = np.zeros((rows, TILE))
        flat[:, :nt] = x[:, n0:n0 + nt]
        u = flat.reshape(rows, THREADS, C)
        carried = np.zeros_like(hist)
        carried[0] = u[:, -1, [C - 1, C - 2]]
        h1 = np.concatenate([hist[0][:, :1], u[:, :-1, C - 1]], axis=1)
        h2 = np.concatenate([hist[0][:, 1:], u[:, :-1, C - 2]], axis=1)
        for s, (b0, b1, b2, _, a1, a2) in enumerate(sos):
            p1 = np.concatenate([h1[:, :, None], u[:, :, :-1]], axis=2)
            p2 = np.concatenate([h2[:, :, None], h1[:, :, None], u[:, :, :-2]], axis=2)
            v = b0 * u + b1 * p1 + b2 * p2
            carry = hist[s + 1]
            if a1 == 0.0 and a2 == 0.0:
                y = v
                h1 = np.concatenate([carry[:, :1], y[:, :-1, C - 1]], axis=1)
                h2 = np.concatenate([carry[:, 1:], y[:, :-1, C - 2]], axis=1)
            else:
                p = powers[s]
                s0 = np.zeros((rows, THREADS))
                s1 = np.zeros((rows, THREADS))
                for k in range(C):
                    s0, s1 = -a1 * s0 + (-a2 * s1 + v[:, :, k]), s0
                add0, add1 = _apply(p[0], carry[:, 0], carry[:, 1])
                s0[:, 0] += add0
                s1[:, 0] += add1
                s0 = s0.reshape(rows, 16, 64)
                s1 = s1.reshape(rows, 16, 64)
                for i in range(6):
                    d = 1 << i
                    add0, add1 = _apply(p[i], s0[:, :, :-d].copy(), s1[:, :, :-d].copy())
                    s0[:, :, d:] += add0
                    s1[:, :, d:] += add1
                e0 = np.zeros_like(s0)
                e1 = np.zeros_like(s1)
                e0[:, :, 1:] = s0[:, :, :-1]
                e1[:, :, 1:] = s1[:, :, :-1]
                w0 = s0[:, :, 63].copy()
                w1 = s1[:, :, 63].copy()
                for i in range(4):
                    d = 1 << i
                    add0, add1 = _apply(p[6 + i], w0[:, :-d].copy(), w1[:, :-d].copy())
                    w0[:, d:] += add0
                    w1[:, d:] += add1
                u0 = np.zeros_like(s0)
                u1 = np.zeros_like(s1)
                u0[:, 1:, :] = w0[:, :-1, None]
                u1[:, 1:, :] = w1[:, :-1, None]
                for i in range(6):
                    bit = ((lane_bits >> i) & 1).astype(bool)
                    m0, m1 = _apply(p[i], u0, u1)
                    u0 = np.where(bit, m0, u0)
                    u1 = np.where(bit, m1, u1)
                in0 = (e0 + u0).reshape(rows, THREADS)
                in1 = (e1 + u1).reshape(rows, THREADS)
                in0[:, 0] = carry[:, 0]
                in1[:, 0] = carry[:, 1]
                h1, h2 = in0.copy(), in1.copy()
                y = np.empty_like(v)
                for k in range(C):
                    in0, in1 = -a1 * in0 + (-a2 * in1 + v[:, :, k]), in0
                    y[:, :, k] = in0
            carried[s + 1] = y[:, -1, [C - 1, C - 2]]
            u = y
        out[:, n0:n0 + nt] = u.reshape(rows, TILE)[:, :nt]
        hist = carried
    return out
