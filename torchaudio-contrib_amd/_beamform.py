"""Argument checks and shapes of ``psd`` / ``mvdr_weights_souden`` / ``apply_beamforming`` and of ``rtf_evd`` / ``rtf_power`` /
``mvdr_weights_rtf``, whose RTFs are ``(…, F, C, 2)`` like the weights (host arithmetic only; shared by
``functional``, ``layers``, ``_ops``, ``_composite`` and ``_hip``).

Complex values travel as the project's trailing-``2`` pairs below ``functional``: a spectrogram is ``(…, C, F, T, 2)``, a PSD
``(…, F, C, C, 2)``, beamforming weights ``(…, F, C, 2)``.  ``functional`` views ``complex64`` / ``complex128`` tensors as pairs on the
way in and back on the way out.  An absent optional tensor (no mask, no reference vector) is the empty 1-d tensor ``none(like)``
inside the ops, whose schemas then need no optional tensors."""
import torch

#: the channel counts csrc/beamform.hip is instantiated for
MIN_CHANNELS, MAX_CHANNELS = 2, 8


def none(like):
    """the stand-in for an absent tensor argument of an op"""
    return like.new_empty(0)


def absent(t):
    return t.dim() == 1 and t.shape[0] == 0


def pairs(t, what):
    """``(pairs, was_complex)``: a complex tensor viewed as ``(…, 2)``, a real ``(…, 2)`` tensor as it is"""
    if not torch.is_tensor(t):
        raise TypeError('%s must be a tensor, got %s' % (what, type(t).__name__))
    if t.is_complex():
        return torch.view_as_real(t), True
    if not t.is_floating_point() or t.dim() < 1 or t.shape[-1] != 2:
        raise ValueError('%s must be complex or real pairs (…, 2), got %s of shape %s' % (what, t.dtype, tuple(t.shape)))
    return t, False


def unpairs(t, was_complex):
    return torch.view_as_complex(t) if was_complex else t


def spec_shape(spec):
    """``(lead, C, F, T)`` of a spectrogram in pairs"""
    if spec.dim() < 4 or spec.shape[-1] != 2:
        raise ValueError('specgram must be (…, channel, freq, time) complex, got pairs of shape %s' % (tuple(spec.shape),))
    return tuple(spec.shape[:-4]), int(spec.shape[-4]), int(spec.shape[-3]), int(spec.shape[-2])


def check_mask(mask, spec, what='mask', multi=False):
    """``ValueError`` unless the real ``mask`` is ``(…, F, T)`` for ``spec``'s ``(…, C, F, T)`` (``(…, C, F, T)`` with ``multi``)"""
    lead, C, F, T = spec_shape(spec)
    want = lead + ((C, F, T) if multi else (F, T))
    if not torch.is_tensor(mask) or mask.is_complex() or not mask.is_floating_point():
        raise ValueError('%s must be a real floating-point tensor' % what)
    if tuple(mask.shape) != want:
        raise ValueError('%s must have shape %s for a specgram of %s, got %s' % (what, want, lead + (C, F, T), tuple(mask.shape)))


def psd_shape(psd, what='psd'):
    """``(lead, F, C)`` of a PSD in pairs"""
    if psd.dim() < 4 or psd.shape[-1] != 2 or psd.shape[-2] != psd.shape[-3]:
        raise ValueError('%s must be (…, freq, channel, channel) complex, got pairs of shape %s' % (what, tuple(psd.shape)))
    return tuple(psd.shape[:-4]), int(psd.shape[-4]), int(psd.shape[-2])


def check_weights_args(psd_s, psd_n, reference_channel):
    """``(lead, F, C, ref_vector or None, ref_channel)``; ``ValueError`` for PSDs of different shapes, a channel index out of range
    or a reference vector that is not real ``(…, C)`` / ``(C,)``"""
    lead, F, C = psd_shape(psd_s, 'psd_s')
    if tuple(psd_n.shape) != tuple(psd_s.shape):
        raise ValueError('psd_s and psd_n must have the same shape, got %s and %s' % (tuple(psd_s.shape[:-1]), tuple(psd_n.shape[:-1])))
    if torch.is_tensor(reference_channel):
        u = reference_channel
        if u.is_complex() or tuple(u.shape) not in (lead + (C,), (C,)):
            raise ValueError('reference_channel as a tensor must be real of shape %s or %s, got %s of shape %s'
                             % (lead + (C,), (C,), u.dtype, tuple(u.shape)))
        return lead, F, C, u, 0
    if isinstance(reference_channel, bool) or not isinstance(reference_channel, int):
        raise TypeError('reference_channel must be an int or a tensor, got %s' % type(reference_channel).__name__)
    if not -C <= reference_channel < C:
        raise ValueError('reference_channel %d is out of range for %d channels' % (reference_channel, C))
    return lead, F, C, None, reference_channel % C


def check_n_iter(n_iter):
    """``ValueError`` for ``n_iter <= 0``, ``TypeError`` for a non-int"""
    if isinstance(n_iter, bool) or not isinstance(n_iter, int):
        raise TypeError('n_iter must be an int, got %s' % type(n_iter).__name__)
    if n_iter <= 0:
        raise ValueError('n_iter must be positive, got %d' % n_iter)
    return n_iter


def check_rtf_weights_args(rtf, psd_n, reference_channel):
    """``(lead, F, C, ref_vector or None, ref_channel)`` for an RTF ``(…, F, C, 2)`` and a PSD ``(…, F, C, C, 2)``, both in pairs;
    ``reference_channel`` may be None (``ref_channel`` is then -1: no scaling), else as in ``check_weights_args``"""
    lead, F, C = psd_shape(psd_n, 'psd_n')
    if rtf.dim() < 3 or tuple(rtf.shape) != lead + (F, C, 2):
        raise ValueError('rtf must be %s complex for a psd_n of %s, got pairs of shape %s'
                         % (lead + (F, C), lead + (F, C, C), tuple(rtf.shape)))
    if reference_channel is None:
        return lead, F, C, None, -1
    return check_weights_args(psd_n, psd_n, reference_channel)


def check_apply(weights, spec):
    lead, C, F, T = spec_shape(spec)
    if weights.dim() < 3 or tuple(weights.shape) != lead + (F, C, 2):
        raise ValueError('beamform_weights must be %s complex for a specgram of %s, got pairs of shape %s'
                         % (lead + (F, C), lead + (C, F, T), tuple(weights.shape)))
    return lead, C, F, T
