"""SpecAugment's argument checks and random draws (torchaudio's ``mask_along_axis`` / ``mask_along_axis_iid``), the one place every
route gets its spans from.

A call's masks become ONE ``tac_amd::mask_spans`` op: the draws are made with ``torch.rand`` in torchaudio's order — per mask the
width first, then the offset — so that a generator state gives the spans the sequential ``masked_fill`` form gives; the arithmetic
after the draws (scale, floor, start + width) runs once over all masks of an axis, and the ``int32`` table ``(rows, k, 2)`` is put
together by torch operators on the input's device.  The iid path calls no ``.item()`` and never waits for the device; the shared
path draws ``torch.rand(1)`` from the CPU generator, as torchaudio does, and uploads a table of one row.
"""
import torch

from . import _ops


def check(name, x, axis, p, min_dim):
    """The ``ValueError`` cases that do not depend on the draws; returns ``axis - (x.dim() - 2)``: 0 for A, 1 for B."""
    if x.dim() < min_dim:
        raise ValueError('%s: expected at least %d dimensions, got %d' % (name, min_dim, x.dim()))
    if axis not in (x.dim() - 2, x.dim() - 1):
        raise ValueError('%s: only the last two axes (frequency and time) can be masked, got axis %r of %d' % (name, axis, x.dim()))
    check_p(name, p)
    return axis - (x.dim() - 2)


def check_p(name, p):
    if not 0.0 <= p <= 1.0:
        raise ValueError('%s: p must be between 0.0 and 1.0, got %r' % (name, p))


def clamp_param(mask_param, n, p):
    """``mask_param`` as the draws use it: at most the share ``p`` of the axis (``p == 1.0``: as given)"""
    return mask_param if p == 1.0 else min(mask_param, int(n * p))


def draws_iid(x, count, mask_param, n):
    """``count`` masks of an axis of length ``n``, a span per leading index: ``(start, end)``, int64 ``(count, *lead)`` on ``x``'s
    device.  The draws are made mask by mask, width then offset; the rest is one expression over all of them."""
    lead = tuple(x.shape[:-2])
    dtype = x.dtype if x.is_floating_point() else torch.float32
    drawn = [(torch.rand(lead, device=x.device, dtype=dtype), torch.rand(lead, device=x.device, dtype=dtype)) for _ in range(count)]
    value = torch.stack([d[0] for d in drawn]) * mask_param
    min_value = torch.stack([d[1] for d in drawn]) * (n - value)
    start = min_value.long()
    return start, start + value.long()


def draws_shared(name, count, mask_param, n):
    """``count`` masks of an axis of length ``n``, one span for every leading index, drawn from the CPU generator: ``(start, end)``,
    int64 ``(count,)`` on the host"""
    drawn = [(torch.rand(1), torch.rand(1)) for _ in range(count)]
    value = torch.cat([d[0] for d in drawn]) * mask_param
    min_value = torch.cat([d[1] for d in drawn]) * (n - value)
    start = min_value.long()
    end = start + value.long()
    if bool(((end - start) >= mask_param).any()):
        raise ValueError('%s: the number of masked columns should be less than mask_param' % name)
    return start, end


def table(along_a, along_b, x):
    """The span table of ``tac_amd::mask_spans`` from the ``(start, end)`` pairs of the two axes (either may be None): int32
    ``(rows or 1, k, 2)`` on ``x``'s device, the spans along A first; returns ``(table, k_a)``"""
    pairs = [p for p in (along_a, along_b) if p is not None]
    k_a = 0 if along_a is None else int(along_a[0].shape[0])
    spans = torch.stack([torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])], dim=-1)      # (k, *lead, 2)
    k = int(spans.shape[0])
    spans = spans.movedim(0, -2).reshape((-1, k, 2)).to(torch.int32)
    return spans.to(x.device).contiguous(), k_a


def fill_args(name, mask_value, x):
    """``(value_t, value)`` of the op: a tensor fill stays a tensor (the kernel reads it on the device)"""
    if torch.is_tensor(mask_value):
        if mask_value.numel() != 1:
            raise ValueError('%s: mask_value must be a number or a tensor of one element, got shape %r' % (name, tuple(mask_value.shape)))
        return mask_value.reshape(()), 0.0
    return None, float(mask_value)


def apply(name, x, along_a, along_b, mask_value):
    """one ``tac_amd::mask_spans`` call for the spans of both axes; ``x`` is (…, A, B) with at least two dimensions"""
    spans, k_a = table(along_a, along_b, x)
    value_t, value = fill_args(name, mask_value, x)
    if x.dim() == 2:
        return _ops.call('mask_spans', x.unsqueeze(0), spans, k_a, value_t, value).squeeze(0)
    return _ops.call('mask_spans', x, spans, k_a, value_t, value)


def mask_along_axis_iid(x, mask_param, mask_value, axis, p, name='mask_along_axis_iid'):
    which = check(name, x, axis, p, 3)
    mask_param = clamp_param(mask_param, int(x.shape[axis]), p)
    if mask_param < 1:
        return x
    pair = draws_iid(x, 1, mask_param, int(x.shape[axis]))
    return apply(name, x, pair if which == 0 else None, pair if which == 1 else None, mask_value)


def mask_along_axis(x, mask_param, mask_value, axis, p, name='mask_along_axis'):
    which = check(name, x, axis, p, 2)
    mask_param = clamp_param(mask_param, int(x.shape[axis]), p)
    if mask_param < 1:
        return x
    pair = draws_shared(name, 1, mask_param, int(x.shape[axis]))
    return apply(name, x, pair if which == 0 else None, pair if which == 1 else None, mask_value)


def spec_augment(x, n_time_masks, time_mask_param, n_freq_masks, freq_mask_param, iid_masks, p, zero_masking):
    """torchaudio's ``SpecAugment.forward`` over (…, freq, time) as ONE ``mask_spans`` call: the time masks' draws first, then the
    frequency masks', each in the sequential order; ``p`` bounds the time masks only"""
    name = 'SpecAugment'
    if x.dim() < 2:
        raise ValueError('%s: expected at least 2 dimensions (…, freq, time), got %d' % (name, x.dim()))
    check_p(name, p)
    mask_value = 0.0 if zero_masking else x.mean()
    n_freq, n_time = int(x.shape[-2]), int(x.shape[-1])
    time_mask_param = clamp_param(time_mask_param, n_time, p)
    iid = iid_masks and x.dim() >= 3
    along_a = along_b = None
    if n_time_masks > 0 and time_mask_param >= 1:
        along_b = draws_iid(x, n_time_masks, time_mask_param, n_time) if iid else \
            draws_shared(name, n_time_masks, time_mask_param, n_time)
    if n_freq_masks > 0 and freq_mask_param >= 1:
        along_a = draws_iid(x, n_freq_masks, freq_mask_param, n_freq) if iid else \
            draws_shared(name, n_freq_masks, freq_mask_param, n_freq)
    if along_a is None and along_b is None:
        return x
    return apply(name, x, along_a, along_b, mask_value)
