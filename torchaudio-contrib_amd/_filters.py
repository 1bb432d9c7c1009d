"""Host side of ``functional.lfilter`` and the filters on top of it: argument checks and the RBJ audio-EQ-cookbook biquad designs,
evaluated in float64 (Python floats) and handed to the op as float64 host tensors — they reach the kernel as the doubles computed
here, never through float32.

Every design returns ``(b, a)``, two tuples of three floats, with ``w0 = 2 pi f / sample_rate`` and ``alpha = sin(w0) / (2 Q)``;
the denominator of all of them is ``a = (1 + alpha, -2 cos w0, 1 - alpha)`` except the equalizer's."""
import math

import numpy as np
import torch

from ._bounded import Bounded


def check_coeffs(a_coeffs, b_coeffs):
    """``ValueError`` unless both are 1-D floating-point tensors of equal, non-zero length.  (``a_coeffs[0] != 0`` is checked on
    the host values, ``leading_nonzero``.)  2-D coefficient banks — torchaudio's one filter per channel — are out of scope."""
    for name, c in (('a_coeffs', a_coeffs), ('b_coeffs', b_coeffs)):
        if not torch.is_tensor(c):
            raise ValueError('lfilter: %s must be a tensor, got %s' % (name, type(c).__name__))
        if c.dim() != 1:
            raise ValueError('lfilter: %s must be 1-D, got shape %s (2-D coefficient banks are not supported)'
                             % (name, tuple(c.shape)))
        if not c.is_floating_point():
            raise ValueError('lfilter: %s must be floating point, got %s' % (name, c.dtype))
    if a_coeffs.numel() != b_coeffs.numel() or a_coeffs.numel() == 0:
        raise ValueError('lfilter: a_coeffs and b_coeffs must have the same non-zero length, got %d and %d'
                         % (a_coeffs.numel(), b_coeffs.numel()))


def _w0_alpha(sample_rate, freq, Q):
    if not sample_rate > 0:
        raise ValueError('sample_rate must be positive, got %r' % (sample_rate,))
    if not Q > 0:
        raise ValueError('Q must be positive, got %r' % (Q,))
    w0 = 2.0 * math.pi * float(freq) / float(sample_rate)
    return w0, math.sin(w0) / (2.0 * float(Q))


def lowpass(sample_rate, cutoff_freq, Q=0.707):
    w0, alpha = _w0_alpha(sample_rate, cutoff_freq, Q)
    c = math.cos(w0)
    return ((1.0 - c) / 2.0, 1.0 - c, (1.0 - c) / 2.0), (1.0 + alpha, -2.0 * c, 1.0 - alpha)


def highpass(sample_rate, cutoff_freq, Q=0.707):
    w0, alpha = _w0_alpha(sample_rate, cutoff_freq, Q)
    c = math.cos(w0)
    return ((1.0 + c) / 2.0, -1.0 - c, (1.0 + c) / 2.0), (1.0 + alpha, -2.0 * c, 1.0 - alpha)


def bandpass(sample_rate, central_freq, Q=0.707, const_skirt_gain=False):
    w0, alpha = _w0_alpha(sample_rate, central_freq, Q)
    t = math.sin(w0) / 2.0 if const_skirt_gain else alpha
    return (t, 0.0, -t), (1.0 + alpha, -2.0 * math.cos(w0), 1.0 - alpha)


def bandreject(sample_rate, central_freq, Q=0.707):
    w0, alpha = _w0_alpha(sample_rate, central_freq, Q)
    c = math.cos(w0)
    return (1.0, -2.0 * c, 1.0), (1.0 + alpha, -2.0 * c, 1.0 - alpha)


def allpass(sample_rate, central_freq, Q=0.707):
    w0, alpha = _w0_alpha(sample_rate, central_freq, Q)
    c = math.cos(w0)
    return (1.0 - alpha, -2.0 * c, 1.0 + alpha), (1.0 + alpha, -2.0 * c, 1.0 - alpha)


def equalizer(sample_rate, center_freq, gain, Q=0.707):
    w0, alpha = _w0_alpha(sample_rate, center_freq, Q)
    c = math.cos(w0)
    A = 10.0 ** (float(gain) / 40.0)
    return (1.0 + alpha * A, -2.0 * c, 1.0 - alpha * A), (1.0 + alpha / A, -2.0 * c, 1.0 - alpha / A)


def _shelf_terms(sample_rate, gain, central_freq, Q):
    w0, alpha = _w0_alpha(sample_rate, central_freq, Q)
    A = math.exp(float(gain) / 40.0 * math.log(10.0))
    c = math.cos(w0)
    return A, 2.0 * math.sqrt(A) * alpha, (A - 1.0) * c, (A + 1.0) * c


def treble(sample_rate, gain, central_freq=3000, Q=0.707):
    """High shelf of ``gain`` dB (torchaudio's ``treble_biquad``): with ``A = exp(gain / 40 ln 10)``, ``t1 = 2 sqrt(A) alpha``,
    ``t2 = (A - 1) cos w0``, ``t3 = (A + 1) cos w0``: ``b = (A ((A + 1) + t2 + t1), -2 A ((A - 1) + t3), A ((A + 1) + t2 - t1))``,
    ``a = ((A + 1) - t2 + t1, 2 ((A - 1) - t3), (A + 1) - t2 - t1)``."""
    A, t1, t2, t3 = _shelf_terms(sample_rate, gain, central_freq, Q)
    return ((A * ((A + 1.0) + t2 + t1), -2.0 * A * ((A - 1.0) + t3), A * ((A + 1.0) + t2 - t1)),
            ((A + 1.0) - t2 + t1, 2.0 * ((A - 1.0) - t3), (A + 1.0) - t2 - t1))


def bass(sample_rate, gain, central_freq=100, Q=0.707):
    """Low shelf of ``gain`` dB (torchaudio's ``bass_biquad``), the mirror image of ``treble``: ``b = (A ((A + 1) - t2 + t1),
    2 A ((A - 1) - t3), A ((A + 1) - t2 - t1))``, ``a = ((A + 1) + t2 + t1, -2 ((A - 1) + t3), (A + 1) + t2 - t1)``."""
    A, t1, t2, t3 = _shelf_terms(sample_rate, gain, central_freq, Q)
    return ((A * ((A + 1.0) - t2 + t1), 2.0 * A * ((A - 1.0) - t3), A * ((A + 1.0) - t2 - t1)),
            ((A + 1.0) + t2 + t1, -2.0 * ((A - 1.0) + t3), (A + 1.0) + t2 - t1))


#: the channel weights of ITU-R BS.1770-4 (left, right, centre, left surround, right surround) as torchaudio has them
LOUDNESS_WEIGHTS = (1.0, 1.0, 1.0, 1.41, 1.41)


def loudness_blocks(sample_rate):
    """``(gate, step)``: the block of 400 ms and its hop of a quarter of it in samples, each by Python's ``round`` as torchaudio's
    ``loudness`` takes them"""
    gate = int(round(0.4 * sample_rate))
    return gate, int(round(gate * 0.25))


def k_weighting(sample_rate):
    """``((b, a), (b, a))``: the two biquads in front of the loudness measurement, torchaudio's ``treble_biquad(4 dB, 1500 Hz,
    Q = 1 / sqrt 2)`` and ``highpass_biquad(38 Hz, Q = 0.5)``"""
    return treble(sample_rate, 4.0, 1500.0, 1.0 / math.sqrt(2.0)), highpass(sample_rate, 38.0, 0.5)


def loudness_check(waveform, sample_rate, name='loudness'):
    """The checks of ``loudness`` (``ValueError``), before anything touches a device; returns ``(gate, step)``"""
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or sample_rate <= 0:
        raise ValueError('%s: sample_rate must be a positive int, got %r' % (name, sample_rate))
    if waveform.dim() < 2:
        raise ValueError('%s: expected a waveform of shape (..., channels, time), got shape %s' % (name, tuple(waveform.shape)))
    if waveform.size(-2) > 5:
        raise ValueError('Only up to 5 channels are supported.')
    if waveform.size(-2) < 1:
        raise ValueError('%s: the waveform has no channel (shape %s)' % (name, tuple(waveform.shape)))
    if not waveform.is_floating_point():
        raise ValueError('%s: expected a floating-point waveform, got %s' % (name, waveform.dtype))
    gate, step = loudness_blocks(sample_rate)
    if gate < 1 or step < 1:
        raise ValueError('%s: sample_rate %d leaves no block (400 ms are %d samples, the hop %d)' % (name, sample_rate, gate, step))
    if waveform.size(-1) < gate:
        raise ValueError('%s: the waveform has %d samples, shorter than one block of 400 ms (%d samples at %d Hz)'
                         % (name, waveform.size(-1), gate, sample_rate))
    return gate, step


def check_sos(sos):
    """``ValueError`` unless ``sos`` is a floating-point ``(S, 6)`` tensor with ``S >= 1``.  (Every ``a0`` finite and not zero is
    checked on the host values, ``check_sos_values``.)"""
    if not torch.is_tensor(sos):
        raise ValueError('sosfilt: sos must be a tensor, got %s' % type(sos).__name__)
    if sos.dim() != 2 or sos.shape[1] != 6:
        raise ValueError('sosfilt: sos must have shape (sections, 6) with rows (b0, b1, b2, a0, a1, a2), got %s' % (tuple(sos.shape),))
    if sos.shape[0] == 0:
        raise ValueError('sosfilt: sos has no section')
    if not sos.is_floating_point():
        raise ValueError('sosfilt: sos must be floating point, got %s' % sos.dtype)


def check_sos_values(rows):
    """``rows``: the sections as tuples of Python floats"""
    for s, row in enumerate(rows):
        if row[3] == 0.0 or not math.isfinite(row[3]):
            raise ValueError('sosfilt: a0 of section %d must be finite and not zero, got %r' % (s, row[3]))


def _pair_roots(r):
    """Roots of a real polynomial as one list: a conjugate pair by its member of positive imaginary part (the mean of it and of
    the conjugate of its partner, so the pair is exact), a real root as a complex number of imaginary part zero"""
    r = np.asarray(r, dtype=np.complex128)
    real = np.abs(r.imag) <= 100.0 * np.finfo(np.float64).eps * np.abs(r)
    out = [complex(v.real, 0.0) for v in r[real]]
    pos, neg = list(r[~real & (r.imag > 0)]), list(r[~real & (r.imag < 0)])
    if len(pos) != len(neg):
        raise ValueError('tf2sos: the roots do not pair into conjugates (are the coefficients finite?)')
    for v in pos:
        k = int(np.argmin([abs(v - w.conjugate()) for w in neg]))
        out.append(0.5 * (v + neg.pop(k).conjugate()))
    return out


def _is_real(v):
    return v.imag == 0.0


def _take_nearest(pool, to, kind=None):
    """Remove and return the entry of ``pool`` nearest ``to`` among the real (``kind`` 'real'), the complex ('complex') or all"""
    ks = [k for k, v in enumerate(pool) if kind is None or _is_real(v) == (kind == 'real')]
    k = min(ks, key=lambda k: abs(pool[k] - to) if math.isfinite(pool[k].real) else math.inf)
    return pool.pop(k)


def _quadratic(r1, r2):
    """The coefficients in z^-1 of (1 - r1 z^-1)(1 - r2 z^-1): ``r2`` None is the conjugate of ``r1``, an infinite root stands for
    the factor z^-1 (a leading zero of the numerator)"""
    if r2 is None:
        return (1.0, -2.0 * r1.real, r1.real * r1.real + r1.imag * r1.imag)
    f1 = (0.0, 1.0) if math.isinf(r1.real) else (1.0, -r1.real)
    f2 = (0.0, 1.0) if math.isinf(r2.real) else (1.0, -r2.real)
    return (f1[0] * f2[0], f1[0] * f2[1] + f1[1] * f2[0], f1[1] * f2[1])


def _tf2sos(b, a):
    n = len(a) - 1
    if n <= 2:
        bn = [v / a[0] for v in b] + [0.0] * (2 - n)
        an = [v / a[0] for v in a] + [0.0] * (2 - n)
        return [bn + [1.0] + an[1:]]
    lead = next((k for k, v in enumerate(b) if v != 0.0), None)
    if lead is None:
        gain, zeros = 0.0, [complex(0.0, 0.0)] * n
    else:           # a numerator that starts with `lead` zeros is z^-lead times a shorter one: `lead` roots at infinity
        gain = b[lead] / a[0]
        zeros = _pair_roots(np.roots(np.asarray(b[lead:], dtype=np.float64))) + [complex(math.inf, 0.0)] * lead
    poles = _pair_roots(np.roots(np.asarray(a, dtype=np.float64)))
    sections = []
    while poles:
        p1 = poles.pop(int(np.argmin([abs(1.0 - abs(p)) for p in poles])))
        real_zeros = sum(1 for z in zeros if _is_real(z))
        if _is_real(p1) and not any(_is_real(p) for p in poles):
            # the last real pole of an odd order: a first-order section with the nearest real zero
            z1 = _take_nearest(zeros, p1, 'real')
            sections.append((_quadratic(z1, complex(0.0, 0.0)), _quadratic(p1, complex(0.0, 0.0))))
            continue
        # (a second-order section never takes the only real zero left: its partner would have to be complex)
        z1 = _take_nearest(zeros, p1, 'complex' if real_zeros == 1 else None)
        if not _is_real(p1):
            den = _quadratic(p1, None)
            num = _quadratic(z1, None) if not _is_real(z1) else _quadratic(z1, _take_nearest(zeros, p1, 'real'))
        elif not _is_real(z1):
            num = _quadratic(z1, None)
            den = _quadratic(p1, _take_nearest(poles, z1, 'real'))
        else:
            reals = [k for k, p in enumerate(poles) if _is_real(p)]
            p2 = poles.pop(min(reals, key=lambda k: abs(1.0 - abs(poles[k]))))
            den = _quadratic(p1, p2)
            num = _quadratic(z1, _take_nearest(zeros, p2, 'real'))
        sections.append((num, den))
    sections.reverse()                          # the section nearest the unit circle comes last
    rows = [[v + 0.0 for v in num + den] for num, den in sections]           # (+ 0.0: no negative zeros)
    rows[0][:3] = [gain * v for v in rows[0][:3]]
    return rows


_sections = Bounded(256)


def tf2sos(b_coeffs, a_coeffs):
    """The transfer function ``b / a`` (sequences of floats, equal length, ``a[0] != 0``) as second-order sections: a float64 host
    tensor ``(ceil(order / 2), 6)`` with rows ``(b0, b1, b2, 1, a1, a2)``, cached by value.  scipy's ``tf2sos`` algorithm in numpy
    and float64: the roots of both polynomials, conjugate pairs kept together, the pole (pair) nearest the unit circle matched
    with the zeros nearest it, the sections ordered so that that one comes last, the gain ``b0 / a0`` in the first.  An odd order
    leaves one first-order section (``b2 = a2 = 0``); orders 1 and 2 give the input itself, divided by ``a0``."""
    key = (tuple(float(v) for v in b_coeffs), tuple(float(v) for v in a_coeffs))
    hit = _sections.get(key)
    if hit is None:
        b, a = key
        if len(b) != len(a) or len(a) == 0:
            raise ValueError('tf2sos: b_coeffs and a_coeffs must have the same non-zero length, got %d and %d' % (len(b), len(a)))
        if a[0] == 0.0 or not all(math.isfinite(v) for v in a + b):
            raise ValueError('tf2sos: the coefficients must be finite and a_coeffs[0] not zero')
        with torch.inference_mode(False):
            hit = torch.tensor(_tf2sos(list(b), list(a)), dtype=torch.float64)
        _sections[key] = hit
    return hit


_tensors = Bounded(256)


def host_tensor(values):
    """float64 host tensor of a tuple of floats, cached (built outside inference mode: it may be saved for a backward)."""
    key = tuple(float(v) for v in values)
    hit = _tensors.get(key)
    if hit is None:
        with torch.inference_mode(False):
            hit = torch.tensor(key, dtype=torch.float64)
        _tensors[key] = hit
    return hit
