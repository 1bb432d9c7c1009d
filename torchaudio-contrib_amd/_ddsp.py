"""Host side of the differentiable-DSP pair (``oscillator_bank``, ``filter_waveform``): argument checks and the plan by which the
filter kernel reads broadcast ``kernels`` through strides.  Python numbers and shapes only; nothing here touches a device."""
import torch

REDUCTIONS = ('sum', 'mean', 'none')


def check_oscillator_bank(frequencies, amplitudes, sample_rate, reduction, dtype):
    if frequencies.dim() < 2 or tuple(frequencies.shape) != tuple(amplitudes.shape):
        raise ValueError('oscillator_bank: frequencies and amplitudes must be (…, time, N) tensors of one shape, got %s and %s'
                         % (tuple(frequencies.shape), tuple(amplitudes.shape)))
    if reduction not in REDUCTIONS:
        raise ValueError('oscillator_bank: reduction must be one of %r, got %r' % (REDUCTIONS, reduction))
    if not isinstance(dtype, torch.dtype) or not dtype.is_floating_point:
        raise ValueError('oscillator_bank: dtype must be a floating-point torch.dtype, got %r' % (dtype,))
    if not sample_rate > 0:
        raise ValueError('oscillator_bank: sample_rate must be positive, got %r' % (sample_rate,))


def filter_shift(taps, delay_compensation):
    """the first sample of the full convolution that is kept: ``delay_compensation``, or ``K // 2`` where it is negative"""
    s = int(delay_compensation) if delay_compensation >= 0 else taps // 2
    if s > taps - 1:
        raise ValueError('filter_waveform: delay_compensation = %d exceeds the last tap (K - 1 = %d)' % (s, taps - 1))
    return s


def check_filter_waveform(waveform, kernels, delay_compensation):
    """Returns the shift ``s``.  ``kernels``: ``(F, K)``, or ``(…, F, K)`` whose leading dims equal the waveform's or are 1."""
    if waveform.dim() < 1 or kernels.dim() < 2 or kernels.shape[-1] < 1 or kernels.shape[-2] < 1:
        raise ValueError('filter_waveform: expected a waveform (…, T) and kernels (F, K) or (…, F, K), got %s and %s'
                         % (tuple(waveform.shape), tuple(kernels.shape)))
    if kernels.dim() != 2:
        lead, klead = tuple(waveform.shape[:-1]), tuple(kernels.shape[:-2])
        if len(klead) != len(lead) or any(k != w and k != 1 for k, w in zip(klead, lead)):
            raise ValueError('filter_waveform: the leading dims of kernels %s must equal those of the waveform %s or be 1'
                             % (tuple(kernels.shape), tuple(waveform.shape)))
    if waveform.dtype != kernels.dtype:
        raise ValueError('filter_waveform: waveform is %s and kernels are %s' % (waveform.dtype, kernels.dtype))
    return filter_shift(int(kernels.shape[-1]), delay_compensation)


def kernel_rows(lead, kernels):
    """How row ``r`` of the flattened waveform finds its filters: ``(div, outer, inner)`` with the offset ``(r // div) outer +
    (r % div) inner`` elements — size-1 dims and the shared ``(F, K)`` form are zero strides, nothing is expanded.  ``None`` where
    the leading dims do not collapse into two such levels."""
    if kernels.dim() == 2:
        return 1, 0, 0
    dims = [(w, 0 if k == 1 else st) for w, k, st in zip(lead, kernels.shape[:-2], kernels.stride()[:-2]) if w != 1]
    merged = []
    for n, st in dims:
        if merged and merged[-1][1] == st * n:
            merged[-1] = (merged[-1][0] * n, st)
        else:
            merged.append((n, st))
    if len(merged) > 2:
        return None
    if not merged:
        return 1, 0, 0
    if len(merged) == 1:
        return 1, merged[0][1], 0
    return merged[1][0], merged[0][1], merged[1][1]
