"""Host side of ``functional.lfilter`` and the filters on top of it: argument checks and the RBJ audio-EQ-cookbook biquad designs,
evaluated in float64 (Python floats) and handed to the op as float64 host tensors — they reach the kernel as the doubles computed
here, never through float32.

Every design returns ``(b, a)``, two tuples of three floats, with ``w0 = 2 pi f / sample_rate`` and ``alpha = sin(w0) / (2 Q)``;
the denominator of all of them is ``a = (1 + alpha, -2 cos w0, 1 - alpha)`` except the equalizer's."""
import math

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
