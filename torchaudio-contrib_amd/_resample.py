"""Host tables of ``functional.resample``: the polyphase windowed-sinc bank of torchaudio's ``functional.resample``, evaluated in
float64 from the closed form and kept COMPACT — per phase only the run of taps with ``|t| < lowpass_filter_width``.

With ``orig``, ``new`` the two rates divided by their gcd, ``base = min(orig, new) * rolloff``, ``width = ceil(lpw * orig / base)``
and ``scale = base / orig``, output sample ``n = j * new + p`` is

    y[n] = sum_{d = -width}^{width + orig - 1} h(p, d) * x[j * orig + d]        (x zero outside [0, L))
    t      = base * (d / orig - p / new)
    h(p,d) = scale * sinc(pi t) * w(t)  if |t| < lpw, else 0
    w(t)   = cos^2(pi t / (2 lpw))                           'sinc_interp_hann'
    w(t)   = I0(beta * sqrt(1 - (t / lpw)^2)) / I0(beta)     'sinc_interp_kaiser'

(torchaudio clamps ``t`` to +-lpw instead, which leaves those taps at rounding noise, ~4e-17 of the window; here they are exactly
zero and are never multiplied.)  Of the ``new x (2 width + orig)`` taps only ``~2 lpw orig / base`` per phase are non-zero, and
they are contiguous in ``d`` because ``t`` is monotone in it: phase ``p`` is the run ``[off[p], off[p] + run[p])``.

Nothing here touches a device; ``_composite.resample`` (torch's ``conv1d`` with the full bank), ``_hip.polyphase`` (the gfx950
kernel with the compact one) and the layer's buffer are all built from ``bank()``."""
import math

import torch

from ._bounded import Bounded

METHODS = ('sinc_interp_hann', 'sinc_interp_kaiser')
KAISER_BETA = 14.769656459379492


class Bank(object):
    """A compact polyphase bank: ``y[j * phases + p] = sum_{k < run[p]} taps[p][k] * x[j * step + off[p] + k]``.
    ``taps`` is float64 ``(phases, K)`` with ``K = max(run)``, zero behind each phase's run; ``off`` / ``run`` are lists of ints."""
    __slots__ = ('phases', 'step', 'taps', 'off', 'run')

    def __init__(self, phases, step, taps, off, run):
        self.phases, self.step, self.taps, self.off, self.run = phases, step, taps, off, run

    @property
    def K(self):
        return int(self.taps.shape[1])


def constants(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method='sinc_interp_hann', beta=None):
    """Validate the arguments; returns ``(orig, new, lpw, rolloff, method, beta)`` with the rates reduced by their gcd and
    ``beta`` resolved (None for the Hann window).  ``ValueError`` for anything the definition does not cover."""
    for name, v in (('orig_freq', orig_freq), ('new_freq', new_freq), ('lowpass_filter_width', lowpass_filter_width)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError('resample: %s must be an int, got %r' % (name, v))
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError('resample: orig_freq and new_freq must be positive, got %d and %d' % (orig_freq, new_freq))
    if lowpass_filter_width < 1:
        raise ValueError('resample: lowpass_filter_width must be at least 1, got %d' % lowpass_filter_width)
    if isinstance(rolloff, bool) or not isinstance(rolloff, (int, float)) or not 0.0 < rolloff <= 1.0:
        raise ValueError('resample: rolloff must lie in (0, 1], got %r' % (rolloff,))
    if resampling_method not in METHODS:
        raise ValueError('resample: resampling_method must be one of %r, got %r' % (METHODS, resampling_method))
    if resampling_method == 'sinc_interp_kaiser':
        beta = KAISER_BETA if beta is None else float(beta)
    else:
        beta = None
    g = math.gcd(orig_freq, new_freq)
    return orig_freq // g, new_freq // g, lowpass_filter_width, float(rolloff), resampling_method, beta


def width_of(orig, new, lpw, rolloff):
    return int(math.ceil(lpw * orig / (min(orig, new) * rolloff)))


def out_length(length, orig, new):
    """ceil(new * length / orig)"""
    return (new * length + orig - 1) // orig


_banks = Bounded(64)


def bank(orig, new, lpw, rolloff, method, beta):
    """The forward bank of reduced rates ``orig -> new`` (``phases = new``, ``step = orig``); cached per argument tuple.
    O(new * lpw * orig / base) work and memory: the full ``new x (2 width + orig)`` bank is never formed."""
    key = (orig, new, lpw, rolloff, method, beta)
    hit = _banks.get(key)
    if hit is not None:
        return hit
    base = min(orig, new) * rolloff
    width = width_of(orig, new, lpw, rolloff)
    scale = base / orig
    p = torch.arange(new, dtype=torch.float64).unsqueeze(1)
    # candidates: |d / orig - p / new| < lpw / base, one sample of slack on either side of the real-valued interval
    reach = int(math.ceil(lpw * orig / base)) + 2
    first = torch.floor(p * orig / new).to(torch.int64) - reach                  # (new, 1)
    d = first + torch.arange(2 * reach + 2, dtype=torch.int64).unsqueeze(0)      # (new, C)
    t = base * (d.to(torch.float64) / orig - p / new)
    valid = (t.abs() < lpw) & (d >= -width) & (d < width + orig)
    safe = torch.where(t == 0, torch.ones_like(t), t)
    sinc = torch.where(t == 0, torch.ones_like(t), torch.sin(math.pi * safe) / (math.pi * safe))
    if method == 'sinc_interp_hann':
        window = torch.cos(math.pi * t / (2.0 * lpw)) ** 2
    else:
        inside = (1.0 - (t / lpw) ** 2).clamp(min=0.0)
        window = torch.special.i0(beta * torch.sqrt(inside)) / torch.special.i0(torch.tensor(beta, dtype=torch.float64))
    h = torch.where(valid, scale * sinc * window, torch.zeros_like(t))
    run = valid.sum(dim=1)
    lead = valid.to(torch.int64).argmax(dim=1)                                   # index of the first valid candidate
    K = max(int(run.max()), 1)
    cols = (lead.unsqueeze(1) + torch.arange(K).unsqueeze(0)).clamp(max=d.shape[1] - 1)
    taps = torch.gather(h, 1, cols) * (torch.arange(K).unsqueeze(0) < run.unsqueeze(1))
    off = torch.gather(d, 1, lead.unsqueeze(1)).squeeze(1)
    made = Bank(new, orig, taps.contiguous(), [int(v) for v in off], [int(v) for v in run])
    _banks[key] = made
    return made


_adjoints = Bounded(64)


def adjoint_bank(orig, new, lpw, rolloff, method, beta):
    """The bank of the gradient: ``gx[j' * orig + q] = sum_m B'[q][m] * g[j' * new + off'[q] + m]`` with ``g`` zero outside
    ``[0, L_out)`` — ``phases = orig``, ``step = new``.  It is the forward bank transposed entry by entry (tap ``(p, d)`` of the
    forward lands at ``q = d mod orig``, ``e = p - floor(d / orig) * new``), so the forward's truncation to
    ``d in [-width, width + orig)`` and ``|t| < lpw`` is kept exactly; offsets may be negative."""
    key = (orig, new, lpw, rolloff, method, beta)
    hit = _adjoints.get(key)
    if hit is not None:
        return hit
    fwd = bank(*key)
    K = fwd.K
    k = torch.arange(K, dtype=torch.int64).unsqueeze(0)
    live = k < torch.tensor(fwd.run, dtype=torch.int64).unsqueeze(1)
    d = torch.tensor(fwd.off, dtype=torch.int64).unsqueeze(1) + k               # (new, K)
    p = torch.arange(new, dtype=torch.int64).unsqueeze(1).expand_as(d)
    block = torch.div(d, orig, rounding_mode='floor')
    q = (d - block * orig)[live]
    e = (p - block * new)[live]
    w = fwd.taps[live]
    lo = torch.full((orig,), 2 ** 62, dtype=torch.int64).scatter_reduce(0, q, e, 'amin')
    hi = torch.full((orig,), -2 ** 62, dtype=torch.int64).scatter_reduce(0, q, e, 'amax')
    empty = hi < lo                                                              # (an input sample no output reads)
    lo = torch.where(empty, torch.zeros_like(lo), lo)
    run = torch.where(empty, torch.zeros_like(lo), hi - lo + 1)
    Ka = max(int(run.max()), 1)
    taps = torch.zeros(orig, Ka, dtype=torch.float64)
    taps[q, e - lo[q]] = w
    made = Bank(orig, new, taps, [int(v) for v in lo], [int(v) for v in run])
    _adjoints[key] = made
    return made


def full_bank(orig, new, lpw, rolloff, method, beta):
    """float64 ``(new, 2 width + orig)``: every tap ``h(p, d)``, ``d = -width ..``, zeros included — torchaudio's ``conv1d``
    kernel.  ``new * (2 width + orig)`` elements: the caller decides whether that is affordable."""
    b = bank(orig, new, lpw, rolloff, method, beta)
    width = width_of(orig, new, lpw, rolloff)
    full = torch.zeros(new, 2 * width + orig, dtype=torch.float64)
    k = torch.arange(b.K, dtype=torch.int64).unsqueeze(0)
    live = k < torch.tensor(b.run, dtype=torch.int64).unsqueeze(1)
    col = torch.tensor(b.off, dtype=torch.int64).unsqueeze(1) + k + width
    row = torch.arange(new, dtype=torch.int64).unsqueeze(1).expand_as(col)
    full[row[live], col[live]] = b.taps[live]
    return full


def apply_bank64(b, x, n_out):
    """float64 evaluation of a compact bank on the host, sample by sample of the run: the model of what the kernel computes
    (used by the tests to pair the forward bank with the adjoint one)."""
    x = x.to(torch.float64)
    length = x.shape[-1]
    n = torch.arange(n_out, dtype=torch.int64)
    j = torch.div(n, b.phases, rounding_mode='floor')
    p = n - j * b.phases
    start = j * b.step + torch.tensor(b.off, dtype=torch.int64)[p]
    run = torch.tensor(b.run, dtype=torch.int64)[p]
    out = torch.zeros(tuple(x.shape[:-1]) + (n_out,), dtype=torch.float64)
    for k in range(b.K):
        idx = start + k
        ok = (k < run) & (idx >= 0) & (idx < length)
        weight = torch.where(ok, b.taps[p, k], torch.zeros((), dtype=torch.float64))
        out = out + weight * x[..., idx.clamp(0, max(length - 1, 0))]
    return out
