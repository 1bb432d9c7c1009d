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
import json
import math
import os

import numpy as np
import torch

from oracle import torch_ref

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


# ------------------------------------------------------------------ route-diverse tests (sweeps, fuzz): numpy in, report out
POW_TOL = 1e-6          # per-frame accuracy of the power spectrum the mel dB masks assume (as tests/test_gpu_fullsize.py)
KEEP_EDGE = 0.5         # dB mask share over a whole tensor: frames that read reflect / replicate padding, or a silent span's
                        # border, have peaked spectra whose quiet bins sit far below the frame maximum (a row of one or two
                        # frames under replicate padding keeps ~50 %)
KEEP_INTERIOR = 0.99    # ... over the frames that read neither (assert_db's default)


def ref64(x, n, hop, window=None, power=None, fb=None, **kw):
    """float64 oracle on the CPU (torch_ref on ``x`` in float64): complex rows (*, F, T, 2) (``power`` None), |X|^power
    (*, F, T) or the bank ``fb`` applied to it.  ``window``: the float32 window the op used (a module's), cast to float64;
    None means the periodic Hann the ops build themselves, on the device (its float32 tail values differ from the host's by up
    to 5e-4 relative, which a frame holding only window-tail samples shows)."""
    xt = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
    w = torch.hann_window(kw.get('win_length') or n, device='cuda') if window is None else window
    z = torch_ref.stft(xt.cpu().double(), n, hop, window=w.detach().cpu().double(), **kw)
    if power is None:
        return z
    p = torch_ref.complex_norm(z, power)
    return p if fb is None else torch_ref.apply_filterbank(p, torch.as_tensor(fb).detach().cpu().double())


def interior_frames(x, n, hop, center=True):
    """(rows, frames) bool for the waveform ``x`` (*, L): frames that read no padding and no zero sample (so neither an edge
    of the row nor a silent span's border; a silent frame holds no element above the dB clamp anyway)."""
    a = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)
    a = a.reshape(-1, a.shape[-1])
    length = a.shape[1]
    n_frames = 1 + (length + 2 * (n // 2) - n) // hop if center else 1 + (length - n) // hop
    start = np.arange(max(n_frames, 0)) * hop - (n // 2 if center else 0)
    zeros = np.concatenate([np.zeros((a.shape[0], 1), dtype=np.int64), np.cumsum(a == 0, axis=1)], 1)
    lo, hi = np.clip(start, 0, length), np.clip(start + n, 0, length)
    inside = (start >= 0) & (start + n <= length)
    return torch.from_numpy(inside[None, :] & (zeros[:, hi] - zeros[:, lo] == 0))


def power_db_keep(power, tol, n_bins, db_tol=1e-3, margin=2.0):
    """The dB mask share to require on interior frames of |X|^p: a dB value is fixed to ``db_tol`` where |X| >= c max_frame |X|
    with c = DB_PER_REL p tol / db_tol.  On a white-noise spectrum (|X|^2 exponential, its maximum ~ (ln F + 1) times the
    mean) a share 1 - exp(-c^2 (ln F + 1)) of the bins lies below that.  One less ``margin`` times that share, at most
    KEEP_INTERIOR."""
    c = DB_PER_REL * power * tol / db_tol
    return min(KEEP_INTERIOR, 1.0 - margin * (1.0 - math.exp(-c * c * (math.log(max(n_bins, 2)) + 1.0))))


def power_linear_bound(z_ref, power, tol):
    """Per-element bound on the error of |X|^p when every |X| of a frame is within e = ``tol`` * max_frame |X| of the
    reference: max((|X| + e)^p - |X|^p, |X|^p - max(|X| - e, 0)^p), which is p |X|^(p-1) e to first order and stays finite
    at |X| = 0 for every p (e^p there).  ``z_ref``: (rows, frames, F) complex values or magnitudes; result (rows, frames, F)
    float64, the |X|^p analogue of ``mel_linear_bound`` for ``assert_db(..., lin=...)``."""
    mag = z_ref.abs().to(torch.float64)
    e = tol * mag.amax(-1, keepdim=True)
    up = (mag + e) ** power - mag ** power
    down = mag ** power - (mag - e).clamp(min=0) ** power
    return torch.maximum(up, down)


def as_frames(a, kind):
    """numpy array or tensor in the ops' logical layout -> float64 CPU tensor in frames layout.  ``kind`` 'complex' takes
    complex arrays (*, F, T) (``oracle.numpy_ref``) as well as the real view (*, F, T, 2); 'spec' takes (*, F, T)."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu()
        if a.is_complex():
            a = torch.view_as_real(a)
    else:
        a = np.asarray(a)
        if np.iscomplexobj(a):
            a = np.stack([a.real, a.imag], -1)
        a = torch.from_numpy(np.ascontiguousarray(a))
    return frames_of(a.to(torch.float64), kind)


def report(test, case, n_fft, kind, worst, bound, kept=None, silent=None):
    """``TAC_FUZZ_REPORT=path``: append one JSON line per check (test, case tag, fft_length, kind, worst ratio, bound, dB
    kept fraction, number of silent reference frames)."""
    path = os.environ.get('TAC_FUZZ_REPORT')
    if not path:
        return
    line = dict(test=test, case=str(case), fft_length=n_fft, kind=kind, worst=worst, bound=bound, kept=kept, silent=silent)
    with open(path, 'a') as f:
        f.write(json.dumps(line) + '\n')


def _n_silent(ref):
    return int((ref.abs().amax(-1) == 0).sum())


def mel_db_keep(fb, tol=POW_TOL, db_tol=1e-3, margin=3.0, win_frac=1.0):
    """The dB mask share to require on interior frames of a mel chain with bank ``fb`` (F, M): ``mel_linear_bound`` fixes a
    band's dB value to ``db_tol`` where its weighted mean of P reaches t = DB_PER_REL tol max_f P / db_tol.  On a white-noise
    spectrum (exponential P, maximum ~ (ln F + 1) times the mean) a band of k effective bins ((sum w)^2 / sum w^2) averages a
    Gamma(k, 1 / k) variable, below t with probability at most (k t)^k / k!; a window of ``win_frac`` of fft_length leaves
    that share of the bins independent, so k is scaled by it (the Hann window's leakage correlates neighbouring bins even at
    full length, hence the larger default margin).  One less ``margin`` times the mean of that over
    the non-empty bands, at most KEEP_INTERIOR (which is what a bank of wide bands gets)."""
    w = torch.as_tensor(fb).detach().cpu().double().abs()
    s1, s2 = w.sum(0), (w * w).sum(0)
    k = (s1 * s1 / s2)[s1 > 0] * win_frac
    if k.numel() == 0:
        return KEEP_INTERIOR
    t = DB_PER_REL * tol / db_tol * (math.log(w.shape[0]) + 1.0)
    miss = torch.exp(k * torch.log(k * t) - torch.lgamma(k + 1)).clamp(max=1.0)
    return min(KEEP_INTERIOR, 1.0 - margin * float(miss.mean()))


def check_frames(got, ref, kind, tol, test, case, n_fft, silence=False):
    """``assert_linear`` on numpy / tensor outputs in logical layout, reported.  Every frame whose reference is exactly zero
    must come out exactly zero; ``silence``: the reference must hold at least one such frame somewhere (with 3 or more rows
    the silent row alone satisfies this: that the span frames of the other rows are silent is a property of the input,
    checked on the CPU by tests/test_frame_bounds.py).  Returns the worst ratio."""
    r = as_frames(ref, kind)
    n_silent = _n_silent(r)
    assert n_silent > 0 or not silence, '%s %r: the input was to hold a silent frame and the reference has none' % (test, case)
    worst = assert_linear(as_frames(got, kind), r, tol, '%s %r' % (test, case))
    report(test, case, n_fft, kind, worst, tol, silent=n_silent)
    return worst


def check_db(got_db, ref_lin, test, case, n_fft, tol=None, lin=None, amin=1e-7, ref=1.0, kind='db', db_tol=1e-3,
             keep=KEEP_EDGE, interior=None, keep_interior=KEEP_INTERIOR):
    """``assert_db`` on numpy / tensor outputs in (*, F, T) layout, reported.  ``lin``: a per-element linear bound in frames
    layout (``power_linear_bound``, ``mel_linear_bound``), else ``tol`` times the frame maximum.  The mask must keep ``keep``
    of the elements above the clamp over the whole tensor and ``keep_interior`` of them over the ``interior`` frames
    ((rows, frames) bool, ``interior_frames``), less two elements.  Returns the kept fraction over the interior frames (the whole tensor if none)."""
    g, r = as_frames(got_db, 'spec'), as_frames(ref_lin, 'spec')
    what = '%s %r' % (test, case)
    worst, kept, _ = assert_db(g, r, tol, db_tol, amin, ref, what, keep=keep, lin=lin)
    kept_in = None
    if interior is not None and bool(interior.any()):
        sub = None if lin is None else lin[interior][None]
        n_above = int((r[interior].abs() ** 2 > amin).sum())
        _, kept_in, _ = assert_db(g[interior][None], r[interior][None], tol, db_tol, amin, ref, what + ' (interior frames)',
                                  keep=keep_interior - 2.0 / max(n_above, 1), lin=sub)      # (two elements' grace: small tensors)
    report(test, case, n_fft, kind, worst, db_tol, kept=kept if kept_in is None else kept_in)
    return kept if kept_in is None else kept_in


def check_mel_db64(got_db, x, n, hop, fb, test, case, window=None, power=2.0, tol=2e-6, **kw):
    """dB of a mel chain of ``x`` against the float64 oracle; the mask from ``mel_linear_bound`` (POW_TOL on the power
    spectrum, ``tol`` on |X| for ``power`` 1); interior frames held to ``mel_db_keep``."""
    p = ref64(x, n, hop, window, power, **kw)
    fb = torch.as_tensor(fb).detach().cpu().double()
    lin_tol = POW_TOL if power == 2.0 else tol
    lin = mel_linear_bound(frames_of(p, 'spec'), fb, lin_tol)
    return check_db(got_db, torch_ref.apply_filterbank(p, fb), test, case, n, lin=lin,
                    interior=interior_frames(x, n, hop, kw.get('center', True)),
                    keep_interior=mel_db_keep(fb, lin_tol, win_frac=(kw.get('win_length') or n) / n))


def check_power_db64(got_db, x, n, hop, power, test, case, tol, window=None, amin=1e-7, **kw):
    """dB of |X|^power of ``x`` against the float64 oracle; the mask from ``power_linear_bound`` with the per-frame bound
    ``tol`` on |X|; interior frames held to ``power_db_keep``."""
    mag = ref64(x, n, hop, window, 1.0, **kw)
    return check_db(got_db, mag ** power, test, case, n, amin=amin,
                    lin=power_linear_bound(frames_of(mag, 'spec'), power, tol),
                    interior=interior_frames(x, n, hop, kw.get('center', True)),
                    keep_interior=power_db_keep(power, tol, mag.shape[-2]))


def check_rows(got, ref, tol, test, case, n_fft, kind='grad', silent_rows=()):
    """``assert_rows`` on (*, L) gradients, reported; ``silent_rows``: row indices whose reference must be exactly zero."""
    g = torch.as_tensor(np.asarray(got) if not isinstance(got, torch.Tensor) else got.detach().cpu()).to(torch.float64)
    r = torch.as_tensor(np.asarray(ref) if not isinstance(ref, torch.Tensor) else ref.detach().cpu()).to(torch.float64)
    g, r = g.reshape(-1, g.shape[-1]), r.reshape(-1, r.shape[-1])
    for row in silent_rows:
        assert not bool(r[row].any()), '%s %r: the reference gradient of silent row %d is not zero' % (test, case, row)
    worst = assert_rows(g, r, tol, '%s %r' % (test, case))
    report(test, case, n_fft, kind, worst, tol, silent=len(silent_rows))
    return worst
