"""Shared by tests/test_loudness_cpu.py and tests/test_loudness_gpu.py: the float64 reference of ``loudness`` (ITU-R BS.1770-4 as
torchaudio evaluates it), the closed forms of the two shelf designs, the bounds every result is held to and the inputs that fix the
conditions those bounds need.  No tests in here.

Reference: the definition with ``scipy.signal.lfilter`` and ``np.clip`` as in tests/lfilter_rules.py —

    w = clip(highpass(clip(treble(x, 4 dB, 1500 Hz, Q = 1 / sqrt 2)), 38 Hz, Q = 0.5))
    E[c][k] = mean(w[c]^2 over [k step, k step + gate)),  l_k = -0.691 + 10 log10 sum_c g_c E[c][k],  g = (1, 1, 1, 1.41, 1.41)
    keep = l > -70;  gamma_r = level(mean of E over keep) - 10;  keep &= l > gamma_r;  result = level(mean of E over keep)

with ``gate = round(0.4 sr)``, ``step = round(gate / 4)`` and ``level(e) = -0.691 + 10 log10 sum_c g_c e_c``.

Bound of the float32 kernel result (csrc/loudness.hip: float64 throughout, one rounding at the end), per batch entry:

    |got - want| <= 2^-24 |want| + (10 / ln 10) rel_E

``2^-24 |want|`` is the rounding of the result to float32.  ``rel_E`` is the relative error of the gated energy under float64
arithmetic, derived — not measured — as follows (``rel_energy_error``).  Stage one's output differs from the reference by at most
``d1 = 2^-40 mass1``, the arithmetic term of ``lfilter_rules.reference`` (no float32 rounding: the value stays float64); clipping is a
contraction.  Stage two is linear, so ``d1`` reaches its output through the absolute impulse response ``|h2|`` of the whole high-pass
and its own arithmetic adds ``2^-40 mass2``: ``d2 = |h2| * d1 + 2^-40 mass2`` (a causal convolution).  A square then moves by at most
``2 |w| d2 + d2^2``, a block's mean by the mean of that, and the gated, channel-weighted energy by the same weighted sum over the
kept blocks — the SAME blocks as the reference keeps, which is what the margins below are for.  Summing ``n`` non-negative float64
terms in any order is off by at most ``(n - 1) 2^-53`` of the sum: ``(gate + blocks + 16) 2^-53`` covers the squares, the sums over
a block, over the blocks and over the channels and the divisions, and ``2^-40`` more the two ``log10`` and the offset (each a few
units of 2^-53 of a value of order ``|want| / 10``).  ``10 log10(1 + r) <= (10 / ln 10) r``, and the second-order term for negative
``r`` is far inside the ``2^-40``.

Margins: a block whose ``l_k`` lies within the arithmetic error of -70 or of ``gamma_r`` may fall on either side of a gate, and the
result then jumps.  ``margins`` returns the smallest distance of any block from either threshold; every test input has both at
1e-6 dB or more (``MARGIN``; the float64 error of an ``l_k`` is of order 1e-10 dB), asserted on the CPU by ``case`` before any
comparison.

Bound of the composite route on float32 input (``f32_bound``), derived the same way: both stage outputs are rounded to float32, so
``d1`` and ``d2`` take the WHOLE bound of ``lfilter_rules.reference`` (``2^-24 |ref| + 2^-40 mass + 2^-126``) in place of its
arithmetic term; the squares, the mean over a block (``gate`` float32 terms in whatever order torch sums them), the sums over
channels and blocks and the divisions are covered by ``(gate + blocks + 16) 2^-24`` of the energy; the two float32 ``log10`` (a few
units in the last place of a value of order ``|want| / 10``), the offset and the products by 10 by ``2^-21 (|want| + 1)``.  The
float32 inputs of the CPU tests must keep their margins above that bound (asserted there)."""
import functools
import math

import numpy as np
import scipy.signal

import lfilter_rules

WEIGHTS = (1.0, 1.0, 1.0, 1.41, 1.41)
MARGIN = 1e-6                   # dB
EPS32 = 2.0 ** -24
EPS64 = 2.0 ** -53
DB = 10.0 / math.log(10.0)
COMMON_RATES = {8000: (3200, 800), 16000: (6400, 1600), 22050: (8820, 2205), 24000: (9600, 2400), 32000: (12800, 3200),
                44100: (17640, 4410), 48000: (19200, 4800), 96000: (38400, 9600)}


def blocks(sample_rate):
    gate = int(round(0.4 * sample_rate))
    return gate, int(round(gate * 0.25))


# ----------------------------------------------------------------------------- the designs, in closed form
def _terms(sample_rate, gain, freq, q):
    w0 = 2.0 * math.pi * freq / sample_rate
    alpha = math.sin(w0) / (2.0 * q)
    big_a = math.exp(gain / 40.0 * math.log(10.0))
    return big_a, 2.0 * math.sqrt(big_a) * alpha, (big_a - 1.0) * math.cos(w0), (big_a + 1.0) * math.cos(w0)


def treble_closed_form(sample_rate, gain, freq=3000.0, q=0.707):
    a_, t1, t2, t3 = _terms(sample_rate, gain, freq, q)
    return ((a_ * ((a_ + 1) + t2 + t1), -2 * a_ * ((a_ - 1) + t3), a_ * ((a_ + 1) + t2 - t1)),
            ((a_ + 1) - t2 + t1, 2 * ((a_ - 1) - t3), (a_ + 1) - t2 - t1))


def bass_closed_form(sample_rate, gain, freq=100.0, q=0.707):
    a_, t1, t2, t3 = _terms(sample_rate, gain, freq, q)
    return ((a_ * ((a_ + 1) - t2 + t1), 2 * a_ * ((a_ - 1) - t3), a_ * ((a_ + 1) - t2 - t1)),
            ((a_ + 1) + t2 + t1, -2 * ((a_ - 1) + t3), (a_ + 1) + t2 - t1))


def highpass_closed_form(sample_rate, freq, q):
    w0 = 2.0 * math.pi * freq / sample_rate
    alpha, c = math.sin(w0) / (2.0 * q), math.cos(w0)
    return ((1 + c) / 2, -1 - c, (1 + c) / 2), (1 + alpha, -2 * c, 1 - alpha)


def k_weighting(sample_rate):
    return treble_closed_form(sample_rate, 4.0, 1500.0, 1.0 / math.sqrt(2.0)), highpass_closed_form(sample_rate, 38.0, 0.5)


# ----------------------------------------------------------------------------- the reference
def _np64(x):
    return (x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)).astype(np.float64)


def _block_means(per_sample, gate, step):
    """(…, L) -> (…, nb): the mean over [k step, k step + gate)"""
    view = np.lib.stride_tricks.sliding_window_view(per_sample, gate, axis=-1)[..., ::step, :]
    return view.mean(axis=-1)


def _level(e):
    """(…, C) -> (…)"""
    g = np.asarray(WEIGHTS[:e.shape[-1]])
    with np.errstate(divide='ignore', invalid='ignore'):
        return -0.691 + 10.0 * np.log10((g * e).sum(-1))


def _gated(energy, keep):
    """(…, C, nb), (…, nb) -> (…, C): sum_k keep_k E[c][k] / count(keep), 0 / 0 = NaN"""
    with np.errstate(divide='ignore', invalid='ignore'):
        return (keep[..., None, :] * energy).sum(-1) / np.count_nonzero(keep, axis=-1)[..., None]


def details(x, sample_rate, clip=True):
    """every intermediate of the definition on float64 ``x`` (…, C, L), as a dict"""
    x64 = _np64(x)
    gate, step = blocks(sample_rate)
    (b1, a1), (b2, a2) = k_weighting(sample_rate)
    w1 = scipy.signal.lfilter(b1, a1, x64, axis=-1)
    if clip:
        w1 = np.clip(w1, -1.0, 1.0)
    w2 = scipy.signal.lfilter(b2, a2, w1, axis=-1)
    if clip:
        w2 = np.clip(w2, -1.0, 1.0)
    energy = _block_means(w2 * w2, gate, step)                          # (…, C, nb)
    g = np.asarray(WEIGHTS[:energy.shape[-2]])
    with np.errstate(divide='ignore', invalid='ignore'):
        l = -0.691 + 10.0 * np.log10((g[:, None] * energy).sum(-2))     # (…, nb)
        keep_abs = l > -70.0
        gamma = _level(_gated(energy, keep_abs)) - 10.0
        keep = keep_abs & (l > gamma[..., None])
        value = _level(_gated(energy, keep))
    return dict(w2=w2, energy=energy, l=l, keep_abs=keep_abs, gamma=gamma, keep=keep, value=value, gate=gate, step=step)


def reference(x, sample_rate, clip=True):
    """float64 (…, C, L) -> (…)"""
    return details(x, sample_rate, clip)['value']


def margins(x, sample_rate):
    """(to -70, to gamma_r): the smallest distance in dB of any block's l_k from either threshold, over the whole batch"""
    d = details(x, sample_rate)
    l = d['l']
    with np.errstate(invalid='ignore'):
        to_abs = np.abs(l + 70.0)
        to_rel = np.abs(l - d['gamma'][..., None])
    to_rel = np.where(np.isnan(to_rel), np.inf, to_rel)                 # (no block above -70: no relative gate to miss)
    return float(to_abs.min()), float(to_rel.min())


# ----------------------------------------------------------------------------- the bounds
def rel_energy_error(x, sample_rate, rounded_stages):
    """(…): the relative error of the gated, weighted energy — see the module's docstring.  ``rounded_stages``: the stage outputs
    are rounded to float32 (the composite route on float32 input) or stay float64 (the kernel)."""
    x64 = _np64(x)
    d = details(x64, sample_rate)
    gate, step = d['gate'], d['step']
    (b1, a1), (b2, a2) = k_weighting(sample_rate)
    length = x64.shape[-1]

    def stage_error(u, b, a):
        raw, bound = lfilter_rules.reference(u, b, a, clamp=False)
        if rounded_stages:
            return raw, bound
        arith = bound - lfilter_rules.EPS32 * np.abs(raw) - lfilter_rules.TINY        # = 2^-40 mass, to 2^-52 |raw|
        return raw, np.maximum(arith, 0.0) + 2.0 ** -52 * np.abs(raw)

    raw1, d1 = stage_error(x64, b1, a1)
    raw2, own2 = stage_error(np.clip(raw1, -1.0, 1.0), b2, a2)
    impulse = np.zeros(length)
    impulse[0] = 1.0
    h2 = np.abs(scipy.signal.lfilter(b2, a2, impulse))
    d2 = lfilter_rules._causal_conv(h2, d1) + own2
    w2 = np.abs(np.clip(raw2, -1.0, 1.0))
    d_energy = _block_means(2.0 * w2 * d2 + d2 * d2, gate, step)        # (…, C, nb)
    g = np.asarray(WEIGHTS[:d_energy.shape[-2]])[:, None]
    keep = d['keep'][..., None, :]
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = (keep * g * d_energy).sum((-2, -1)) / (keep * g * d['energy']).sum((-2, -1))
    unit = lfilter_rules.EPS32 if rounded_stages else EPS64
    return rel + (gate + d['l'].shape[-1] + 16) * unit + (0.0 if rounded_stages else 2.0 ** -40)


def bound(x, sample_rate, want=None):
    """the kernel's bound per entry, in dB"""
    want = reference(x, sample_rate) if want is None else want
    return EPS32 * np.abs(want) + DB * rel_energy_error(x, sample_rate, False)


def f32_bound(x, sample_rate, want=None):
    """the bound of the composite route on float32 input per entry, in dB"""
    want = reference(x, sample_rate) if want is None else want
    return DB * rel_energy_error(x, sample_rate, True) + 2.0 ** -21 * (np.abs(want) + 1.0)


def assert_close(got, want, limit, what):
    """every entry within ``limit`` of ``want`` (NaN where ``want`` is NaN); prints and returns the worst |err| / bound"""
    g = _np64(got)
    assert g.shape == want.shape, '%s: shape %s, expected %s' % (what, g.shape, want.shape)
    assert (np.isnan(g) == np.isnan(want)).all(), '%s: NaN in %s, expected in %s' % (what, np.isnan(g), np.isnan(want))
    fin = ~np.isnan(want)
    err = np.abs(g - want)[fin]
    ratio = float((err / np.broadcast_to(limit, want.shape)[fin]).max()) if err.size else 0.0
    print('%s: worst |err| / bound = %.3g (|err| %.3g dB)' % (what, ratio, float(err.max()) if err.size else 0.0))
    assert ratio <= 1.0, '%s: worst |err| / bound = %.3g (|err| %.3g dB)' % (what, ratio, float(err.max()))
    return ratio


# ----------------------------------------------------------------------------- inputs
class Case(object):
    """an input (float32, (…, C, L)) with its reference, its kernel bound and its margins, checked"""

    def __init__(self, x, sample_rate, what, min_margin=MARGIN):
        self.x, self.sample_rate, self.what = x, sample_rate, what
        self.want = reference(x, sample_rate)
        self.bound = bound(x, sample_rate, self.want)
        self.margins = margins(x, sample_rate)
        assert min(self.margins) >= min_margin, '%s: a block lies %.3g dB from a gate' % (what, min(self.margins))
        assert np.isfinite(self.want).all() and np.isfinite(self.bound).all() and (self.bound < 1e-4).all(), (what, self.want, self.bound)


def noise(shape, sigma, seed):
    return (np.random.default_rng(seed).standard_normal(shape) * sigma).astype(np.float32)


@functools.lru_cache(maxsize=None)
def levels(sample_rate, channels, length, entries=3):
    """``entries`` batch entries of noise from sigma = 0.2 down to 0.002 (three: 0.2, 0.02, 0.002): different levels, all above the
    absolute gate, every block of an entry alike"""
    x = np.stack([noise((channels, length), 0.2 * 10.0 ** (-2.0 * e / max(entries - 1, 1)), 1000 * e + channels) for e in range(entries)])
    return Case(x, sample_rate, 'noise %d Hz, %d channels, %d samples' % (sample_rate, channels, length))


@functools.lru_cache(maxsize=None)
def three_level(sample_rate=4410, channels=2, steps=16):
    """segments of ``steps`` hops of noise at sigma = 0.1, 0.003 and 1e-5: the absolute gate removes the quiet blocks, the relative
    gate the middle ones, and the loud ones survive (asserted).  At 4410 Hz and 16 hops a segment, 21168 samples: two tiles."""
    gate, step = blocks(sample_rate)
    n = steps * step
    x = np.concatenate([noise((1, channels, n), s, 7 + i) for i, s in enumerate((0.1, 0.003, 1e-5))], axis=-1)
    case = Case(x, sample_rate, 'three levels at %d Hz' % sample_rate)
    d = details(x, sample_rate)
    by_abs = int((~d['keep_abs']).sum())
    by_rel = int((d['keep_abs'] & ~d['keep']).sum())
    assert by_abs > 0 and by_rel > 0 and int(d['keep'].sum()) > 0, (by_abs, by_rel, int(d['keep'].sum()))
    case.removed = (by_abs, by_rel, int(d['keep'].sum()))
    return case


@functools.lru_cache(maxsize=None)
def loud(sample_rate=8000, channels=2, length=3200 + 5 * 800 + 13):
    """a tone of amplitude 0.95 near 3 kHz: the shelf lifts it past 1 and the clip behind the shelf changes the result — the
    reference without the clips differs by more than 100 bounds (asserted)"""
    t = np.arange(length)
    x = np.stack([0.95 * np.sin(2.0 * math.pi * (2900.0 + 150.0 * c) / sample_rate * t + 0.3 * c) for c in range(channels)])
    case = Case(x[None].astype(np.float32), sample_rate, 'loud tone at %d Hz' % sample_rate)
    unclipped = reference(case.x, sample_rate, clip=False)
    assert (np.abs(unclipped - case.want) > 100.0 * case.bound).all(), (unclipped, case.want, case.bound)
    return case


# ----------------------------------------------------------------------------- the launcher, restated (csrc/loudness.hip)
TILE = 16384
MIN_STEP = 16
CU_COUNTS = (256, 304)
QUOTED = ('loudness.hip', (
    'constexpr int LO_C_LOG = 4;',
    'constexpr int LO_THREADS = 1024;',
    'constexpr int LO_TILE = LO_THREADS * LO_C;      // samples per tile',
    'for (long long row = blockIdx.x; row < rows; row += gridDim.x) {',
    'for (long long entry = blockIdx.x; entry < entries; entry += gridDim.x) {',
    'const long long blocks = persistent_blocks(rows, 1, (long long)device_cu_count());',
    'const long long gate_blocks = persistent_blocks(entries, 1, (long long)device_cu_count() * 8);',
))


def persistent_blocks(units, per_block, max_blocks):
    want = (units + per_block - 1) // per_block
    return max(1, min(want, max_blocks))


def grid(cus, entries, channels):
    """(workgroups of the energy kernel, of the gate kernel)"""
    return persistent_blocks(entries * channels, 1, cus), persistent_blocks(entries, 1, 8 * cus)


def wrap_rows(cus, odd=5):
    """rows that make every workgroup of the energy kernel walk its loop twice and some a third time: 2 grid + odd"""
    return 2 * cus + odd
