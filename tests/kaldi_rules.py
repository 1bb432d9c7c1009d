"""Shared by tests/test_kaldi_cpu.py and tests/test_kaldi_gpu.py: the float64 reference of ``kaldi_fbank`` written from the
definition — one numpy loop per frame with ``numpy.fft.rfft``, no unfold, no matrix product over frames: it shares no structure
with the product — and the per-element rule every float32 result is held to.

Definition (W, S, N from ``sizes``; eps = 2^-23).  Frame ``t`` of a row is ``x[t S .. t S + W)`` with ``snip_edges``; otherwise it
starts at ``t S - (W // 2 - S // 2)`` on the row mirrored at both ends (``j < 0`` reads ``x[-j - 1]``, ``j >= n`` reads
``x[2 n - 1 - j]``).  Per frame: (1) subtract the mean, (2) ``e = log max(sum f^2, eps)`` (raw energy), (3) ``f[i] -= c f[i-1]``
with ``f[-1] := f[0]``, (4) window, (5) ``e`` on the windowed frame (not raw), (6) zero-pad to N, ``|rfft|`` [squared].  The bank is
triangular in mel over the bins ``k < N / 2``.  Output ``log max(spectrum . bank, eps)``, ``e`` floored at ``log energy_floor`` as
the first (HTK: last) column, column means over the frames subtracted.

The rule, u = 2^-24.  A float32 evaluation differs from this reference in two ways.

(a) Its transform, bank and square are float32: every bin of the processed frame's spectrum P is within ``FRAME_POW`` (2e-5, the
    project's per-frame tolerance for power and mel values, tests/test_gpu_parity.py) of the frame's largest bin, which the bank
    carries to ``frame_bounds.mel_linear_bound``: FRAME_POW max_k P[k] sum_k bank[b][k].

(b) The frame it transforms is not the reference's frame.  The raw samples are float32 and exact; what is rounded is
      * the mean: a float32 sum of W samples along a tree of depth d, divided by W and rounded, is off by at most
        ``delta = (d + 1) u max|x_raw|`` (each addition on a path rounds a partial sum of magnitude <= W max|x_raw| / W after
        the division).  The kernel adds 16 pair sums in a lane and log2(N / 32) <= 5 shuffle steps: d <= 21; the torch route
        accumulates in float64 and rounds once.  ``MEAN_ROUNDINGS = 22``.  An error of the mean is the SAME shift of every sample
        of the frame; pre-emphasis turns a constant shift ``delta`` into ``delta |1 - c|`` (the replicated first sample included),
        the window into ``delta |1 - c| w[i]``, the transform into ``delta |1 - c| |What[k]|`` with ``What = rfft(w, N)``: it lands
        on the lowest bins, where a row with a large offset under a small signal shows it;
      * each sample once per step: ``u |f1[i]|`` for the subtraction, ``u (|c f1[i-1]| + |f2[i]|)`` for the pre-emphasis (product
        and difference; a fused multiply-add rounds less), ``2 u |f3[i]|`` for the window (its own rounding to float32 and the
        product).  Without mean removal ``f1`` is the raw frame, so ``u |c| |x_raw|`` is the raw-sample term of that case.  These
        reach a bin through at most ``sum_i`` of their magnitudes times the window.
    Together ``|dX[k]| <= D[k] = delta |1 - c| |What[k]| + sum_i r3[i]``; then ``|d |X|^2| <= 2 |X| D + D^2`` (``|d|X|| <= D``), and
    the bank carries that to each band.

    linear bound B[b] = mel_linear_bound(P, bank, FRAME_POW)[b] + sum_k bank[b][k] (2 |X[k]| D[k] + D[k]^2)

Log output: where ``value - B > eps``, ``|got - log value| <= B / value + 4 u |log value|`` (four roundings' worth for the
logarithm itself); at least ``KEEP`` = 99 % of the elements above eps must be held this way; where ``value + B < eps`` the output
must equal ``float32(log eps)`` exactly.  Linear output (``use_log_fbank=False``): ``|got - value| <= B + u |value|``.

Energy column, the same construction on ``E = sum g^2`` (g the mean-removed frame, or the windowed one): a float32 sum of W squares
in any order is within ``(W + 2) u E``, and a per-sample perturbation p[i] (the shift ``delta`` and the roundings above) moves E by
at most ``sum 2 |g[i]| p[i] + p[i]^2``; the floor is ``max(eps, energy_floor)``.

``subtract_mean`` is checked against the unsubtracted float32 result of the same call: a float32 mean over m frames and one
subtraction stay within ``(m + 3) u max|column|``.
"""
import math

import numpy as np
import torch

import frame_bounds

U = 2.0 ** -24
EPS = 2.0 ** -23
FRAME_POW = 2e-5
MEAN_ROUNDINGS = 22
KEEP = 0.99
LOG_EPS32 = np.float32(math.log(EPS))

DEFAULTS = dict(blackman_coeff=0.42, dither=0.0, energy_floor=1.0, frame_length=25.0, frame_shift=10.0, high_freq=0.0,
                htk_compat=False, low_freq=20.0, num_mel_bins=23, preemphasis_coefficient=0.97, raw_energy=True,
                remove_dc_offset=True, round_to_power_of_two=True, sample_frequency=16000.0, snip_edges=True, subtract_mean=False,
                use_energy=False, use_log_fbank=True, use_power=True, window_type='povey')


#: the geometries of the kernel: W / S / N = 400 / 160 / 512 (4 frames per wave), 200 / 80 / 256 (8), 551 / 220 / 1024 (2, odd W),
#: an odd shift (S = 161), W = N = 512 (no zero-padding), and S = 2240: frames so far apart that a wave's four do not fit its
#: LDS area as one span and are staged one by one (the kernel's other staging path)
GEOMETRIES = [dict(), dict(sample_frequency=8000.0), dict(sample_frequency=22050.0), dict(frame_shift=10.0625),
              dict(frame_length=32.0), dict(frame_shift=140.0)]

#: every option against the defaults
OPTIONS = [dict(remove_dc_offset=False), dict(preemphasis_coefficient=0.0), dict(raw_energy=False, use_energy=True),
           dict(use_energy=True), dict(use_energy=True, htk_compat=True), dict(use_log_fbank=False), dict(use_power=False),
           dict(use_energy=True, energy_floor=0.0), dict(window_type='hanning'), dict(window_type='hamming'),
           dict(window_type='rectangular'), dict(window_type='blackman'), dict(window_type='blackman', blackman_coeff=0.3),
           dict(snip_edges=False), dict(num_mel_bins=4), dict(num_mel_bins=80), dict(num_mel_bins=128), dict(low_freq=0.0),
           dict(high_freq=-400.0)]


def ident(kw):
    return '-'.join('%s=%s' % (k, v) for k, v in kw.items()) or 'default'


def tilted(x, c):
    """``y[i] = x[i] + c y[i-1]`` in float64, rounded to float32: the inverse of the pre-emphasis, row by row"""
    y = np.array(x, dtype=np.float64)
    for i in range(1, y.shape[-1]):
        y[..., i] += c * y[..., i - 1]
    return y.astype(np.float32)


def waveform(rows, length, seed, kw=None):
    """``oracle.signals.audio_like`` rows (uniform noise, gains 2^0 .. 2^-7) with the spectral tilt of speech: de-emphasised by
    the call's own pre-emphasis coefficient, so that the processed frame's spectrum is flat.  (Pre-emphasis puts the lowest bins
    of white noise 30 dB under the highest; FRAME_POW of the frame's largest bin is then as large as the narrow lowest bands, the
    log rule cannot hold them, and the 99 % condition fails — a property of that signal, not of any code.)  With 3 or more rows
    and mean removal on, the last row is an offset of 0.5 under such a signal at an amplitude of 1e-3: the case the raw-sample
    term of the rule exists for.  (Without mean removal the offset IS the signal: its leakage buries the bands.)"""
    from oracle import signals
    c = (kw or {}).get('preemphasis_coefficient', DEFAULTS['preemphasis_coefficient'])
    x = tilted(signals.audio_like((rows, length), seed=seed), c)
    if rows >= 3 and (kw or {}).get('remove_dc_offset', True):
        ac = tilted(signals.uniform((length,), seed=seed + 100), c)
        x[rows - 1] = np.float32(0.5) + np.float32(1e-3) * (ac / np.float32(np.abs(ac).max()))
    return x


def length_for(frames, w, s, snip_edges):
    """a row length with exactly ``frames`` frames that is not on the frame grid"""
    if snip_edges:
        return w + (frames - 1) * s + (s - 1) // 2
    return frames * s + (s - 1) // 2 - s // 2 if frames * s + (s - 1) // 2 - s // 2 >= 1 else frames * s


def options(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def sizes(o):
    w = int(o['sample_frequency'] * o['frame_length'] * 0.001)
    s = int(o['sample_frequency'] * o['frame_shift'] * 0.001)
    n = w
    if o['round_to_power_of_two']:
        n = 1
        while n < w:
            n *= 2
    return w, s, n


def num_frames(length, w, s, snip_edges):
    if snip_edges:
        return 0 if length < w else 1 + (length - w) // s
    return (length + s // 2) // s


def frame_indices(length, w, s, t, snip_edges):
    """the W sample indices frame ``t`` reads, one by one"""
    start = t * s if snip_edges else t * s - (w // 2 - s // 2)
    idx = []
    for j in range(start, start + w):
        if j < 0:
            j = -j - 1
        elif j >= length:
            j = 2 * length - 1 - j
        idx.append(j)
    return idx


def window64(kind, w, a=0.42):
    out = np.empty(w, dtype=np.float64)
    for i in range(w):
        hann = 0.5 - 0.5 * math.cos(2.0 * math.pi * i / (w - 1))
        if kind == 'hanning':
            out[i] = hann
        elif kind == 'hamming':
            out[i] = 0.54 - 0.46 * math.cos(2.0 * math.pi * i / (w - 1))
        elif kind == 'povey':
            out[i] = hann ** 0.85
        elif kind == 'rectangular':
            out[i] = 1.0
        elif kind == 'blackman':
            out[i] = a - 0.5 * math.cos(2.0 * math.pi * i / (w - 1)) + (0.5 - a) * math.cos(4.0 * math.pi * i / (w - 1))
        else:
            raise ValueError(kind)
    return out


def mel(f):
    return 1127.0 * math.log(1.0 + f / 700.0)


def bank64(bins, n, sample_frequency, low, high):
    """(bins, n // 2 + 1) float64, element by element; the last column stays zero"""
    if high <= 0.0:
        high += 0.5 * sample_frequency
    delta = (mel(high) - mel(low)) / (bins + 1)
    out = np.zeros((bins, n // 2 + 1), dtype=np.float64)
    for b in range(bins):
        left, centre, right = mel(low) + b * delta, mel(low) + (b + 1) * delta, mel(low) + (b + 2) * delta
        for k in range(n // 2):
            mu = mel(k * sample_frequency / n)
            out[b, k] = max(0.0, min((mu - left) / (centre - left), (right - mu) / (right - centre)))
    return out


_bank_cache = {}


def cached_bank(o):
    w, s, n = sizes(o)
    key = (o['num_mel_bins'], n, o['sample_frequency'], o['low_freq'], o['high_freq'])
    if key not in _bank_cache:
        _bank_cache[key] = bank64(*key)
    return _bank_cache[key]


class Reference(object):
    """``out`` (rows, m, cols) float64 — the definition; ``value`` / ``bound`` (rows, m, bins): the mel value before the
    logarithm and its linear bound B; ``energy`` / ``energy_bound`` (rows, m): E and its bound; ``frames_of_sample(i)``."""


def reference(x, o):
    """``x``: float32 / float64 array (…, n).  Returns a ``Reference`` over the flattened rows."""
    a = np.asarray(x, dtype=np.float64)
    a = a.reshape(-1, a.shape[-1])
    rows, length = a.shape
    w, s, n = sizes(o)
    m = num_frames(length, w, s, o['snip_edges'])
    bins, c = o['num_mel_bins'], o['preemphasis_coefficient']
    win = window64(o['window_type'], w, o['blackman_coeff'])
    bank = cached_bank(o)
    what = np.abs(np.fft.rfft(win, n))
    r = Reference()
    r.value = np.zeros((rows, m, bins))
    r.bound = np.zeros((rows, m, bins))
    r.spec = np.zeros((rows, m, n // 2 + 1))
    r.energy = np.zeros((rows, m))
    r.energy_bound = np.zeros((rows, m))
    r.cols = bins + (1 if o['use_energy'] else 0)
    for row in range(rows):
        for t in range(m):
            f0 = a[row, frame_indices(length, w, s, t, o['snip_edges'])]
            xmax = np.abs(f0).max()
            delta, f1 = 0.0, f0
            r1 = np.zeros(w)
            if o['remove_dc_offset']:
                f1 = f0 - f0.sum() / w
                delta = MEAN_ROUNDINGS * U * xmax
                r1 = U * np.abs(f1)
            f2, r2, shift = f1, r1, delta
            if c != 0.0:
                prev = np.concatenate([f1[:1], f1[:-1]])
                f2 = f1 - c * prev
                r2 = r1 + abs(c) * np.concatenate([r1[:1], r1[:-1]]) + U * (np.abs(c * prev) + np.abs(f2))
                shift = delta * abs(1.0 - c)
            f3 = f2 * win
            r3 = win * r2 + 2.0 * U * np.abs(f3)
            g, p = (f1, delta + r1) if o['raw_energy'] else (f3, shift * win + r3)
            e = float((g * g).sum())
            r.energy[row, t] = e
            r.energy_bound[row, t] = (w + 2) * U * e + float((2.0 * np.abs(g) * p + p * p).sum())
            mag = np.abs(np.fft.rfft(np.concatenate([f3, np.zeros(n - w)])))
            d = shift * what + r3.sum()
            if o['use_power']:
                spec, dspec = mag * mag, 2.0 * mag * d + d * d
            else:
                spec, dspec = mag, d
            r.spec[row, t] = spec
            r.value[row, t] = bank @ spec
            r.bound[row, t] = bank @ dspec
    r.bound += frame_bounds.mel_linear_bound(torch.from_numpy(r.spec), torch.from_numpy(bank.T.copy()), FRAME_POW).numpy()
    with np.errstate(invalid='ignore'):
        feats = np.log(np.maximum(r.value, EPS)) if o['use_log_fbank'] else r.value.copy()
        feats = np.where(np.isnan(r.value), np.nan, feats)
        e = np.log(np.maximum(r.energy, EPS))
        if o['energy_floor'] > 0.0:
            e = np.maximum(e, math.log(o['energy_floor']))
        e = np.where(np.isnan(r.energy), np.nan, e)
    if o['use_energy']:
        feats = np.concatenate([feats, e[..., None]] if o['htk_compat'] else [e[..., None], feats], -1)
    r.unsubtracted = feats
    r.out = feats - feats.mean(1, keepdims=True) if (o['subtract_mean'] and m) else feats
    return r


def split_columns(t, o):
    """(mel columns, energy column or None) of an output (rows, m, cols)"""
    if not o['use_energy']:
        return t, None
    if o['htk_compat']:
        return t[..., :-1], t[..., -1]
    return t[..., 1:], t[..., 0]


def _log_check(got, value, bound, floor, floor_log32, what):
    """The log rule on arrays of one shape.  Returns (worst error / allowance over the held elements, kept share)."""
    assert np.isfinite(got).all(), '%s: non-finite output' % what
    above = value > floor
    held = (value - bound) > floor
    safe_value = np.where(held, value, 1.0)
    allow = bound / safe_value + 4.0 * U * np.abs(np.log(safe_value))
    err = np.abs(got - np.log(safe_value))
    ratio = np.where(held, err / np.maximum(allow, 1e-300), 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, '%s: |d log| is %.3f of its allowance at %r' % (what, worst, np.unravel_index(ratio.argmax(), ratio.shape))
    kept = float(held.sum()) / max(int(above.sum()), 1) if above.any() else 1.0
    assert kept >= KEEP, '%s: the log rule holds only %.4f of the %d elements above the floor' % (what, kept, int(above.sum()))
    deep = (value + bound) < floor
    assert (got[deep] == floor_log32).all(), '%s: %d element(s) below the floor differ from its logarithm' % (
        what, int((got[deep] != floor_log32).sum()))
    return worst, kept


def check(got, r, o, what=''):
    """``got``: the float32 result (…, m, cols) for the waveform ``r`` was made from, WITHOUT ``subtract_mean`` (see
    ``check_subtracted``).  Returns a dict of the worst ratios of error to bound."""
    g = np.asarray(got, dtype=np.float64).reshape((r.value.shape[0], r.value.shape[1], r.cols))
    mel_cols, e_col = split_columns(g, o)
    res = {}
    if o['use_log_fbank']:
        res['log'], res['kept'] = _log_check(mel_cols, r.value, r.bound, EPS, LOG_EPS32, what + ' mel')
    else:
        allow = r.bound + U * np.abs(r.value)
        ratio = np.abs(mel_cols - r.value) / np.maximum(allow, 1e-300)
        ratio = np.where((allow == 0) & (mel_cols == r.value), 0.0, ratio)
        res['linear'] = float(ratio.max()) if ratio.size else 0.0
        assert np.isfinite(mel_cols).all() and res['linear'] <= 1.0, '%s mel: the linear error is %.3f of its bound' % (what, res['linear'])
    if e_col is not None:
        floor = max(EPS, o['energy_floor']) if o['energy_floor'] > 0.0 else EPS
        res['energy'], _ = _log_check(e_col, r.energy, r.energy_bound, floor, np.float32(math.log(floor)), what + ' energy')
    return res


def check_subtracted(got_subtracted, got_plain, what=''):
    """``subtract_mean``: float32 result against the float32 result without it, less its column means in float64"""
    a = np.asarray(got_subtracted, dtype=np.float64)
    b = np.asarray(got_plain, dtype=np.float64)
    m = b.shape[-2]
    want = b - b.mean(-2, keepdims=True)
    allow = (m + 3) * U * np.abs(b).max(-2, keepdims=True)
    ratio = float((np.abs(a - want) / np.maximum(allow, 1e-300)).max()) if a.size else 0.0
    assert ratio <= 1.0, '%s: subtract_mean is %.3f of its bound off' % (what, ratio)
    return ratio


def frames_reading(length, o, sample):
    """the frames whose W samples contain ``sample``"""
    w, s, n = sizes(o)
    m = num_frames(length, w, s, o['snip_edges'])
    return [t for t in range(m) if sample in frame_indices(length, w, s, t, o['snip_edges'])]


def row_gradient(x, o, grad_out):
    """float64 gradient of ``sum(out * grad_out)`` w.r.t. the waveform ``x`` (rows, n), through torch float64 operators applied
    frame by frame to the definition above (autograd over this file's own steps, not over the product)."""
    xt = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    rows, length = xt.shape
    w, s, n = sizes(o)
    m = num_frames(length, w, s, o['snip_edges'])
    win = torch.from_numpy(window64(o['window_type'], w, o['blackman_coeff']))
    bank = torch.from_numpy(cached_bank(o))
    c = o['preemphasis_coefficient']
    g = torch.tensor(np.asarray(grad_out, dtype=np.float64)).reshape(rows, m, -1)
    total = xt.new_zeros(())
    for row in range(rows):
        for t in range(m):
            f = xt[row, torch.tensor(frame_indices(length, w, s, t, o['snip_edges']))]
            if o['remove_dc_offset']:
                f = f - f.sum() / w
            e = (f * f).sum() if o['raw_energy'] else None
            if c != 0.0:
                f = f - c * torch.cat([f[:1], f[:-1]])
            f = f * win
            if e is None:
                e = (f * f).sum()
            z = torch.fft.rfft(torch.cat([f, f.new_zeros(n - w)]))
            spec = z.real ** 2 + z.imag ** 2
            if not o['use_power']:
                spec = spec.sqrt()
            val = bank @ spec
            if o['use_log_fbank']:
                val = torch.log(torch.clamp(val, min=EPS))
            cols = [val]
            if o['use_energy']:
                le = torch.log(torch.clamp(e, min=EPS))
                if o['energy_floor'] > 0.0:
                    le = torch.clamp(le, min=math.log(o['energy_floor']))
                cols = [val, le[None]] if o['htk_compat'] else [le[None], val]
            total = total + (torch.cat(cols) * g[row, t]).sum()
    total.backward()
    return xt.grad.numpy()
