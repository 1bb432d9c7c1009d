"""Waveform augmentation: the argument checks of ``add_noise`` and the rate arithmetic of ``speed`` (torchaudio's
``functional.add_noise`` / ``functional.speed``), the one place the functionals and the layers get them from.

``add_noise`` is ONE ``tac_amd::add_noise`` op: the signal-to-noise ratio and the lengths stay tensors and are read by the kernels on
the device.  ``speed`` has no kernel of its own: it is ``tac_amd::resample`` at the reduced pair ``int(factor * orig_freq) :
int(orig_freq)`` — 9:10, 11:10, 19:20, 21:20 for the usual perturbation factors — and the new lengths are torch operators on the
lengths' device; nothing waits for the host.
"""
import math

import torch

from . import _ops


def add_noise(waveform, noise, snr, lengths=None, name='add_noise'):
    """the checks of torchaudio's ``add_noise`` (``ValueError``), then one ``tac_amd::add_noise`` call"""
    for what, t in (('waveform', waveform), ('noise', noise), ('snr', snr)) + ((('lengths', lengths),) if lengths is not None else ()):
        if not torch.is_tensor(t):
            raise TypeError('%s: %s must be a torch.Tensor, got %s' % (name, what, type(t).__name__))
    if not (waveform.dim() - 1 == noise.dim() - 1 == snr.dim() and (lengths is None or lengths.dim() == snr.dim())) or waveform.dim() < 1:
        raise ValueError("%s: input leading dimensions don't match: waveform %r, noise %r, snr %r%s"
                         % (name, tuple(waveform.shape), tuple(noise.shape), tuple(snr.shape),
                            '' if lengths is None else ', lengths %r' % (tuple(lengths.shape),)))
    if waveform.shape[-1] != noise.shape[-1]:
        raise ValueError('%s: length dimensions of waveform and noise don\'t match (got %d and %d)'
                         % (name, waveform.shape[-1], noise.shape[-1]))
    return _ops.call('add_noise', waveform, noise, snr, lengths)


def speed_rates(orig_freq, factor, name='speed'):
    """``(source, target)``: ``int(factor * orig_freq)`` and ``int(orig_freq)`` divided by their gcd — the rates ``resample`` is called
    with; ``ValueError`` for a factor that is not positive or that leaves no source rate"""
    if not factor > 0:
        raise ValueError('%s: factor must be positive, got %r' % (name, factor))
    source, target = int(factor * orig_freq), int(orig_freq)
    if source <= 0 or target <= 0:
        raise ValueError('%s: factor %r at orig_freq %r leaves no sample rate (int(factor * orig_freq) = %d)' % (name, factor, orig_freq, source))
    gcd = math.gcd(source, target)
    return source // gcd, target // gcd


def pitch_rates(sample_rate, n_steps, bins_per_octave=12, name='pitch_shift'):
    """``(rate, source)``: the time-stretch factor ``2 ** (-n_steps / bins_per_octave)`` of torchaudio's ``pitch_shift`` and the rate
    ``int(sample_rate / rate)`` its last stage resamples FROM, to ``sample_rate`` (16 kHz, 4 steps: 20158, i.e. 10079 : 8000).
    ``ValueError`` for a sample rate that is no positive int, no bins, or a shift that leaves no source rate."""
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or sample_rate <= 0:
        raise ValueError('%s: sample_rate must be a positive int, got %r' % (name, sample_rate))
    if bins_per_octave == 0:
        raise ValueError('%s: bins_per_octave must not be 0' % name)
    rate = 2.0 ** (-float(n_steps) / bins_per_octave)
    source = int(sample_rate / rate)
    if source <= 0:
        raise ValueError('%s: n_steps %r at sample_rate %d leaves no sample rate (int(sample_rate / rate) = %d)'
                         % (name, n_steps, sample_rate, source))
    return rate, source


def speed_lengths(lengths, source, target):
    """the valid lengths after ``resample(source -> target)``: ``ceil(lengths * target / source)`` in the dtype of ``lengths``, by
    torch operators where ``lengths`` lies"""
    if lengths is None:
        return None
    return torch.ceil(lengths * target / source).to(lengths.dtype)
