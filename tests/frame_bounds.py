"""Per-frame and per-row comparison helpers for kernel outputs (a plain module: no tests in here).

``conftest.rel_err`` normalises by the maximum of the whole tensor, so a quiet row (gain 2^-12) or a quiet frame is held to
its own scale only loosely.  These helpers hold every frame to its own maximum instead:

* linear outputs (complex rows, |X|^p, mel power): for each (row, frame), max |got - ref| over the frame divided by
  max |ref| over the same frame; a frame whose reference is exactly zero must come out exactly zero; NaN fails.
* dB outputs of ``amplitude_to_db`` (which squares its input v and clamps v^2 at ``amin``): the linear bound
  |dv| <= tol * frame_max carries over as |d dB| <= 20 / ln 10 * tol * frame_max / v.  For mel values the caller may pass
  the tighter per-element bound of ``mel_linear_bound`` instead (the per-frame bound of the power spectrum carried
  through the bank): a smaller bound only widens the set of elements held to ``db_tol``.  Where that bound is within the dB
  tolerance (and v^2 is above the clamp by more than the linear error) the dB value must be within ``db_tol``; that mask
  must keep at least 99 % of the elements above the clamp.  Elements whose v^2 lies below the clamp by more than the linear
  error must equal the clamp value.
* gradients: per row, max |got - ref| / max |ref|.

Tensors are compared in ``frames`` layout ``(rows, frames, values)`` on whatever device they live on, in float64; only
per-frame maxima travel to the host.  Callers that compare GB-sized outputs pass row chunks and the index of the chunk's
first row (``row0``) so that the worst frame is reported by its global row.
"""
import math

import torch

DB_PER_REL = 20.0 / math.log(10.0)      # d(10 log10 v^2) / (dv / v)


def frames_of(t, kind):
    """``t`` in the logical layout the ops return -> ``(rows, frames, values)`` (a view when the storage is frame-major):
    ``kind`` 'spec' for ``(*, F, T)``, 'complex' for ``(*, F, T, 2)``."""
    if kind == 'spec':
        f, n = t.shape[-2], t.shape[-1]
        return t.reshape(-1, f, n).transpose(1, 2)
    if kind == 'complex':
        f, n = t.shape[-3], t.shape[-2]
        r = t.reshape(-1, f, n, 2).permute(0, 2, 1, 3)
        return r.reshape(r.shape[0], n, 2 * f)
    raise ValueError(kind)


def _worst(ratio, row0):
    """(value, row, frame) of the largest entry of a (rows, frames) tensor; NaN counts as the largest."""
    r = torch.nan_to_num(ratio, nan=math.inf)
    i = int(torch.argmax(r.reshape(-1)))
    row, frame = divmod(i, r.shape[1])
    return float(ratio.reshape(-1)[i]), row0 + row, frame


def linear_frame_errors(got, ref):
    """(rows, frames) float64 tensor on the device of ``ref``: max |got - ref| / max |ref| per frame; 0 for an exactly
    matching silent frame, inf for a silent frame that is not exactly zero, NaN wherever ``got`` holds a NaN."""
    got = got.to(device=ref.device, dtype=torch.float64)
    ref = ref.to(torch.float64)
    d = (got - ref).abs().amax(-1)                     # (amax propagates NaN)
    m = ref.abs().amax(-1)
    silent = m == 0
    ratio = d / torch.where(silent, torch.ones_like(m), m)
    return torch.where(silent & (d == 0), torch.zeros_like(ratio),
                       torch.where(silent & ~torch.isnan(d), torch.full_like(ratio, math.inf), ratio))


def assert_linear(got, ref, tol, what='', row0=0):
    """Every frame within ``tol`` of its own maximum; returns the worst per-frame ratio."""
    ratio = linear_frame_errors(got, ref)
    bad = ~(ratio <= tol)
    value, row, frame = _worst(ratio, row0)
    if bool(bad.any()):
        raise AssertionError('%s: %d frame(s) beyond %.1e of their own maximum; worst row %d frame %d: %.3e'
                             % (what, int(bad.sum()), tol, row, frame, value))
    return value


def db_of(v, ref=1.0, amin=1e-7):
    """``amplitude_to_db`` of the oracle in float64: 10 (log10 max(v^2, amin) - log10 ref)."""
    v = v.to(torch.float64)
    return 10.0 * (torch.log10(torch.clamp(v * v, min=amin)) - math.log10(ref))


def assert_db(got_db, ref_lin, tol, db_tol=1e-3, amin=1e-7, ref=1.0, what='', row0=0, keep=0.99, lin=None):
    """``got_db``: the kernel's dB output, ``ref_lin``: the float64 reference of the value before the dB stage, both in
    frames layout.  ``lin``: a per-element bound on the linear error to use instead of ``tol`` times the frame maximum
    (e.g. ``mel_linear_bound``).  Returns (worst |d dB| over the mask, kept fraction, worst clamp deviation)."""
    v = ref_lin.to(torch.float64)
    got = got_db.to(device=v.device, dtype=torch.float64)
    if not bool(torch.isfinite(got).all()):
        bad = ~torch.isfinite(got)
        value, row, frame = _worst(bad.any(-1).double(), row0)
        raise AssertionError('%s: %d non-finite dB value(s), first in row %d frame %d' % (what, int(bad.sum()), row, frame))
    if lin is None:
        lin = tol * v.abs().amax(-1, keepdim=True)      # the linear bound of every value of the frame
    va = v.abs()
    bound = DB_PER_REL * lin / torch.clamp(va, min=math.sqrt(amin))
    above = va * va > amin
    safe = ((va - lin).clamp(min=0) ** 2 > amin) & (bound <= db_tol)
    err = (got - db_of(v, ref, amin)).abs()
    n_above = int(above.sum())
    kept = float(safe.sum()) / n_above if n_above else 1.0
    worst = err.masked_fill(~safe, 0).amax(-1)
    value, row, frame = _worst(worst, row0)
    if value > db_tol:
        raise AssertionError('%s: |d dB| %.3e > %.1e where the linear bound guarantees %.1e; worst row %d frame %d'
                             % (what, value, db_tol, db_tol, row, frame))
    if kept < keep:
        raise AssertionError('%s: the dB mask keeps only %.4f of the %d elements above the clamp' % (what, kept, n_above))
    clamp_db = 10.0 * (math.log10(amin) - math.log10(ref))
    deep = (va + lin) ** 2 < amin
    cdev = (got - clamp_db).abs().masked_fill(~deep, 0).amax(-1)
    cval, crow, cframe = _worst(cdev, row0)
    if cval > 1e-4:
        raise AssertionError('%s: a value below the clamp is %.3e dB off the clamp value; row %d frame %d'
                             % (what, cval, crow, cframe))
    return value, kept, cval


def mel_linear_bound(power, fb, tol):
    """Per-element bound on the error of mel values ``power @ fb`` when every bin of the power spectrum is within ``tol``
    of its frame's maximum: tol * max_f P[f] * sum_f |fb[f, m]|.  ``power``: (rows, frames, F) float64; result (rows,
    frames, M).  Tighter than ``tol`` times the frame's largest mel value for the narrow low bands, whose values are small
    because their weights are, not because their bins are."""
    return tol * power.abs().amax(-1, keepdim=True) * fb.to(power).abs().sum(0)


def row_errors(got, ref):
    """(rows,) float64: max |got - ref| / max |ref| per row of ``(rows, n)`` tensors (NaN propagates)."""
    return linear_frame_errors(got.reshape(got.shape[0], 1, -1), ref.reshape(ref.shape[0], 1, -1))[:, 0]


def assert_rows(got, ref, tol, what='', row0=0):
    """Every row within ``tol`` of its own maximum; returns the worst per-row ratio."""
    ratio = row_errors(got, ref)
    bad = ~(ratio <= tol)
    value, row, _ = _worst(ratio[:, None], row0)
    if bool(bad.any()):
        raise AssertionError('%s: %d row(s) beyond %.1e of their own maximum; worst row %d: %.3e'
                             % (what, int(bad.sum()), tol, row, value))
    return value
