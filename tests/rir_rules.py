"""Rules of the ``simulate_rir_ism`` tests (tests/test_rir_cpu.py, tests/test_rir_gpu.py): a float64 restatement of the definition in
numpy, written from the definition's text and sharing no code with the package, the per-element bound every route is held to, a
float32 model of the kernel's arithmetic that shows the bound achievable without a GPU, and the case table.

Definition (``P = L // 2``).  Images: every integer vector ``X`` with ``sum |X_d| <= max_order`` in ``itertools.product`` order (the last axis
fastest); per axis ``loc = room (X + 1) - source`` where ``X`` is odd (Python ``%``), else ``room X + source``; per band ``att = prod_d tr_lo^|floor(X_d /
2)| tr_hi^|floor((X_d + 1) / 2)|`` with ``tr = sqrt(1 - absorption)`` and the walls ``[x_lo, x_hi, y_lo, y_hi, z_lo, z_hi]``.  Per (image, channel):
``dist = |loc - mic|``, ``amp = att / dist``, ``delay = dist sample_rate / sound_speed``, ``delay_i = ceil(delay)``, ``f = delay_i - delay``.  For ``m = -P … P``
and ``x = m + f``: ``amp w(x)`` is added to raw sample ``delay_i + m + P``, ``w(x) = sinc(x) (1 + cos(2 pi x / 2P)) / 2`` for ``|x| <= P``, else 0.

The bound, per output element ``t`` of band ``b`` and channel ``c``, with ``u = 2^-24``, over the images whose support ``[delay_i, delay_i + L)``
covers ``t`` (``n_t`` of them):

    BOUND = 2 ( sum_i amp_i (u (1 + 4 |w_i|) + 2^-24 |w'_i|)  +  n_t u sum_i amp_i |w_i| )

Its terms: one rounding each of the tap and of ``amp`` and the few of the tap's float32 factors (``4 |w| u``); ``f`` rounded to float32
(at most ``2^-25`` off, times the analytic derivative ``w'``, with a factor 2 of room); an absolute floor of one unit roundoff of the
image's amplitude for the window near its zero; and a float32 sum of ``n_t`` terms in any order.  The factor 2 is the margin over
what a float32 model of the recommended arithmetic reaches (0.18 – 0.84 of the bracket when the bound was set; ``model32`` below
repeats that check for the kernel as built: 0.17 – 0.46 of the bracket over the case table).  What the bound detects: dropping the two outermost taps exceeds the bracket 55 – 84 times at ``L = 81`` but
only 1.7 – 2.1 times at ``L = 255`` — under the factor 2, wrong edge taps at ``L = 255`` are therefore BELOW DETECTION; the direct float32
forms (``sinf(pi x)``, ``(1 + cos) / 2``, the tap position from a float32 delay) exceed it 3 – 72 times.
"""
import itertools
import math

import numpy as np

U = 2.0 ** -24
FILTER_TAPS, FILTER_FFT = 511, 512


def images(max_order, dims):
    r = range(-max_order, max_order + 1)
    return np.array([X for X in itertools.product(*([r] * dims)) if sum(abs(v) for v in X) <= max_order], dtype=np.int64).reshape(-1, dims)


def n_images(max_order, dims):
    return len(images(max_order, dims))


def taps(x, P):
    """``w(x)`` and ``w'(x)`` in float64"""
    x = np.asarray(x, dtype=np.float64)
    inside = np.abs(x) <= P
    sinc = np.sinc(x)
    safe = np.where(x == 0.0, 1.0, x)
    dsinc = np.where(x == 0.0, 0.0, (np.cos(np.pi * x) - sinc) / safe)
    hann = 0.5 * (1.0 + np.cos(2.0 * np.pi * x / (2.0 * P)))
    dhann = -0.5 * np.sin(np.pi * x / P) * (np.pi / P)
    return np.where(inside, sinc * hann, 0.0), np.where(inside, dsinc * hann + sinc * dhann, 0.0)


def geometry(room, source, mics, absorption, max_order, sample_rate, sound_speed):
    """one room: ``(amp (nb, I, M), delay (I, M), delay_i (I, M) int64)`` in float64 from the inputs as given (float32 values widened)"""
    room, source, mics = (np.asarray(v, dtype=np.float64) for v in (room, source, mics))
    absorption = np.asarray(absorption, dtype=np.float64)
    D = room.shape[0]
    X = images(max_order, D)
    loc = np.where(X % 2 == 1, room * (X + 1) - source, room * X + source)                     # (I, D)
    tr = np.sqrt(1.0 - absorption)                                                            # (nb, 2 D)
    e_lo, e_hi = np.abs(X // 2), np.abs((X + 1) // 2)
    att = np.ones((absorption.shape[0], X.shape[0]))
    for d in range(D):
        att = att * tr[:, None, 2 * d] ** e_lo[None, :, d] * tr[:, None, 2 * d + 1] ** e_hi[None, :, d]
    diff = loc[:, None, :] - mics[None, :, :]
    sq = diff[..., 0] * diff[..., 0]
    for d in range(1, D):
        sq = sq + diff[..., d] * diff[..., d]
    dist = np.sqrt(sq)
    with np.errstate(divide='ignore'):
        amp = att[:, :, None] / dist[None]
    delay = dist * float(sample_rate) / float(sound_speed)
    return amp, delay, np.ceil(delay).astype(np.int64)


def natural_length(rooms, sources, mics, max_order, L, sample_rate, sound_speed):
    """``max(delay_i) + L - P`` over a batch"""
    top = 0
    for r, s, m in zip(rooms, sources, mics):
        top = max(top, int(geometry(r, s, m, np.zeros((1, 2 * len(r))), max_order, sample_rate, sound_speed)[2].max()))
    return top + L - L // 2


def raw(room, source, mics, absorption, max_order, L, sample_rate, sound_speed, start, length):
    """one room → ``(raw (nb, M, length), BOUND (nb, M, length))``: samples ``[start, start + length)`` of the raw responses in float64,
    and the bound of every element"""
    P = L // 2
    amp, delay, di = geometry(room, source, mics, absorption, max_order, sample_rate, sound_speed)
    nb, I, M = amp.shape
    x = np.arange(-P, P + 1)[None, None, :] + (di - delay)[..., None]                          # (I, M, L)
    w, dw = taps(x, P)
    pos = di[..., None] + np.arange(L)[None, None, :] - start                                  # (I, M, L)
    keep = (pos >= 0) & (pos < length)
    ch = np.broadcast_to(np.arange(M)[None, :, None], pos.shape)
    out = np.zeros((nb, M, length))
    first = np.zeros((nb, M, length))
    mass = np.zeros((nb, M, length))
    count = np.zeros((M, length))
    np.add.at(count, (ch[keep], pos[keep]), 1.0)
    for b in range(nb):
        a = np.broadcast_to(amp[b][..., None], pos.shape)
        with np.errstate(invalid='ignore'):
            np.add.at(out[b], (ch[keep], pos[keep]), (a * w)[keep])
            np.add.at(first[b], (ch[keep], pos[keep]), (a * (U * (1.0 + 4.0 * np.abs(w)) + U * np.abs(dw)))[keep])
            np.add.at(mass[b], (ch[keep], pos[keep]), (a * np.abs(w))[keep])
    return out, 2.0 * (first + count[None] * U * mass)


def raw_batch(rooms, sources, mics, absorption, max_order, L, sample_rate, sound_speed, start, length):
    """a batch → ``(B, nb, M, length)`` twice; ``absorption`` is ``(nb, 2 D)`` shared or ``(B, nb, 2 D)``"""
    absorption = np.asarray(absorption, dtype=np.float64)
    got = [raw(r, s, m, absorption if absorption.ndim == 2 else absorption[i], max_order, L, sample_rate, sound_speed, start, length)
           for i, (r, s, m) in enumerate(zip(rooms, sources, mics))]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def model32(room, source, mics, absorption, max_order, L, sample_rate, sound_speed, start, length):
    """the kernel's arithmetic in numpy float32: ``f`` and ``amp`` from float64 rounded once, ``sinpi(f)`` and ``(cos, sin)(pi f / 2P)`` of the rounded ``f``; per tap ``x = m + f``,
    ``c = fma(cm, cf, -(sm sf))`` (modelled as the float32 rounding of the float64 value of the two rounded products), ``w = ((-1)^m sp) / (pi_f
    x) (c c)``, and ``out = fma(amp, w, out)`` (the float64 value rounded once) in image order"""
    f32 = np.float32
    P = L // 2
    amp, delay, di = geometry(room, source, mics, absorption, max_order, sample_rate, sound_speed)
    nb, I, M = amp.shape
    fd = di - delay
    f = fd.astype(f32)
    fr = f.astype(np.float64)                       # (everything of the ROUNDED f: x = m + f is then the x whose sine is taken)
    sp = np.where(fr == 1.0, 0.0, np.sin(np.pi * fr)).astype(f32)
    cf, sf = np.cos(np.pi * fr / (2.0 * P)).astype(f32), np.sin(np.pi * fr / (2.0 * P)).astype(f32)
    m = np.arange(-P, P + 1)
    angle = np.pi * m / (2.0 * P)
    cm, sm = np.cos(angle), np.sin(angle)
    cm[0] = cm[-1] = 0.0
    cm, sm = cm.astype(f32), sm.astype(f32)
    sg = np.where(m % 2 == 1, -1.0, 1.0).astype(f32)
    mf = m.astype(f32)
    amp32 = amp.astype(f32)
    pi_f = f32(np.pi)
    out = np.zeros((nb, M, length), dtype=f32)
    j = np.arange(L)
    for i in range(I):
        for c in range(M):
            x = mf + f[i, c]
            prod = (sm * sf[i, c]).astype(f32)
            cc = (cm.astype(np.float64) * np.float64(cf[i, c]) - prod.astype(np.float64)).astype(f32)
            with np.errstate(divide='ignore', invalid='ignore'):
                w = np.where(x == 0, f32(1.0), (sg * sp[i, c]) / (pi_f * x))
            w = np.where(x > f32(P), f32(0.0), w * (cc * cc)).astype(f32)
            pos = di[i, c] + j - start
            keep = (pos >= 0) & (pos < length)
            for b in range(nb):
                seg = out[b, c, pos[keep]].astype(np.float64)
                out[b, c, pos[keep]] = (np.float64(amp32[b, i, c]) * w[keep].astype(np.float64) + seg).astype(f32)
    return out


def direct32(room, source, mics, absorption, max_order, L, sample_rate, sound_speed, start, length):
    """the direct float32 form the bound has to refuse: delay, ``x``, ``sin(pi x) / (pi x)`` and ``(1 + cos) / 2`` all in float32"""
    f32 = np.float32
    P = L // 2
    amp, delay, di = geometry(room, source, mics, absorption, max_order, sample_rate, sound_speed)
    nb, I, M = amp.shape
    delay32 = delay.astype(f32)
    out = np.zeros((nb, M, length), dtype=f32)
    n = np.arange(L)
    for i in range(I):
        for c in range(M):
            x = ((di[i, c] + n - P).astype(f32) - delay32[i, c]).astype(f32)
            px = (f32(np.pi) * x).astype(f32)
            with np.errstate(divide='ignore', invalid='ignore'):
                sinc = np.where(x == 0, f32(1.0), np.sin(px).astype(f32) / px)
            hann = np.where(np.abs(x) <= P, f32(0.5) * (f32(1.0) + np.cos(f32(2.0 * np.pi / (2.0 * P)) * x).astype(f32)), f32(0.0))
            w = (sinc * hann).astype(f32)
            pos = di[i, c] + n - start
            keep = (pos >= 0) & (pos < length)
            for b in range(nb):
                out[b, c, pos[keep]] += (amp[b, i, c].astype(f32) * w[keep]).astype(f32)
    return out


# ----------------------------------------------------------------------------- the band filters and the multi-band result
def band_filters(centres, sample_rate):
    """``(n, 511)`` float64: the filters of the definition's step 5"""
    n = len(centres)
    v = np.arange(FILTER_FFT // 2 + 1) * (float(sample_rate) / FILTER_FFT)
    rows = []
    for b, c in enumerate(centres):
        lo = centres[0] / 2.0 if b == 0 else centres[b - 1]
        hi = float(int(sample_rate) // 2) if b == n - 1 else centres[b + 1]
        resp = np.zeros_like(v)
        for k, nu in enumerate(v):
            if lo <= nu < c:
                resp[k] = 0.5 * (1.0 + math.cos(2.0 * math.pi * nu / c))
            elif b == n - 1 and nu >= c:
                resp[k] = 1.0
            elif c <= nu < hi:
                resp[k] = 0.5 * (1.0 - math.cos(2.0 * math.pi * nu / hi))
        h = np.fft.fftshift(np.fft.irfft(resp, FILTER_FFT))[1:]
        k = np.arange(FILTER_TAPS)
        rows.append(h * (0.5 - 0.5 * np.cos(2.0 * np.pi * k / (FILTER_TAPS - 1))))
    return np.stack(rows)


def multiband(room, source, mics, absorption, centres, max_order, L, sample_rate, sound_speed, output_length):
    """one room → ``(M, output_length)`` float64: the zero-extended raw responses of every band through its filter (``'same'``), summed, cut at ``P``"""
    P = L // 2
    length = P + output_length + FILTER_TAPS // 2
    bands, _ = raw(room, source, mics, absorption, max_order, L, sample_rate, sound_speed, 0, length)
    filt = band_filters(centres, sample_rate)
    out = np.zeros((bands.shape[1], length))
    for b in range(bands.shape[0]):
        for c in range(bands.shape[1]):
            out[c] += np.convolve(bands[b, c], filt[b], mode='same')
    return out[:, P:P + output_length]


# ----------------------------------------------------------------------------- the case table
def f32(values):
    return np.asarray(values, dtype=np.float32)


ROOM_A, SOURCE_A = f32([5.3, 4.1, 3.2]), f32([2.1, 1.7, 1.4])
#: a pair 5 cm apart, one within 0.5 m of the source (its direct path arrives before sample P: the head is cut by ``start``), one far
MICS_A = f32([[3.3, 2.9, 1.1], [3.35, 2.9, 1.1], [2.3, 1.8, 1.5], [0.7, 3.6, 2.6]])
ROOM_A2, SOURCE_A2 = f32([6.1, 3.7, 2.9]), f32([4.4, 1.2, 1.9])
MICS_A2 = f32([[1.3, 2.2, 0.9], [1.3, 2.25, 0.9], [4.6, 1.3, 1.8], [5.8, 0.4, 2.7]])
ROOM_B, SOURCE_B = f32([9.7, 7.3]), f32([4.2, 3.1])
MICS_B = f32([[6.0, 5.5], [6.05, 5.5], [4.4, 3.2]])

WALLS_3D = f32([0.21, 0.34, 0.18, 0.4, 0.55, 0.12])
WALLS_2D = f32([0.25, 0.31, 0.45, 0.15])
BANDS_3D = f32([[0.21, 0.34, 0.18, 0.4, 0.55, 0.12], [0.3, 0.3, 0.25, 0.5, 0.6, 0.2], [0.45, 0.4, 0.35, 0.55, 0.7, 0.3]])
PER_ROOM_3D = f32([[[0.21, 0.34, 0.18, 0.4, 0.55, 0.12]], [[0.5, 0.1, 0.3, 0.2, 0.45, 0.6]]])
CENTRES = (500.0, 1000.0, 2000.0)


class Case(object):
    """a batch of rooms and the arguments of one call; ``absorption`` is a float, ``(2 D,)``, ``(nb, 2 D)`` or ``(B, nb, 2 D)``"""

    def __init__(self, name, rooms, sources, mics, max_order, absorption, L, sample_rate, sound_speed=343.0):
        self.name, self.rooms, self.sources, self.mics = name, np.stack(rooms), np.stack(sources), np.stack(mics)
        self.max_order, self.absorption, self.L, self.sample_rate, self.sound_speed = max_order, absorption, L, sample_rate, sound_speed
        self._cache = {}

    @property
    def dims(self):
        return self.rooms.shape[1]

    def bands(self):
        """the absorption as ``(nb, 2 D)`` or ``(B, nb, 2 D)`` float32"""
        a = self.absorption
        if isinstance(a, float):
            return np.full((1, 2 * self.dims), a, dtype=np.float32)
        return a[None] if a.ndim == 1 else a

    def natural(self):
        return natural_length(self.rooms, self.sources, self.mics, self.max_order, self.L, self.sample_rate, self.sound_speed)

    def reference(self, start, length):
        """``(raw, BOUND)`` of the batch, each ``(B, nb, M, length)``; computed once per ``(start, length)``"""
        key = (start, length)
        if key not in self._cache:
            self._cache[key] = raw_batch(self.rooms, self.sources, self.mics, self.bands(), self.max_order, self.L, self.sample_rate,
                                         self.sound_speed, start, length)
        return self._cache[key]


CASES = [
    Case('3-D order 0, float, L 81, 16 kHz', [ROOM_A], [SOURCE_A], [MICS_A], 0, 0.3, 81, 16000.0),
    Case('3-D order 1, walls, L 5, 8 kHz', [ROOM_A], [SOURCE_A], [MICS_A], 1, WALLS_3D, 5, 8000.0),
    Case('3-D order 3, three bands, L 81, 16 kHz', [ROOM_A], [SOURCE_A], [MICS_A], 3, BANDS_3D, 81, 16000.0),
    Case('3-D order 6, float, L 81, 16 kHz', [ROOM_A], [SOURCE_A], [MICS_A], 6, 0.3, 81, 16000.0),
    Case('3-D order 3, per room, L 255, 48 kHz', [ROOM_A, ROOM_A2], [SOURCE_A, SOURCE_A2], [MICS_A, MICS_A2], 3, PER_ROOM_3D, 255, 48000.0),
    Case('2-D order 6, walls, L 81, 16 kHz', [ROOM_B], [SOURCE_B], [MICS_B], 6, WALLS_2D, 81, 16000.0),
    Case('2-D order 3, float, L 255, 8 kHz', [ROOM_B], [SOURCE_B], [MICS_B[:2]], 3, 0.45, 255, 8000.0),
    Case('2-D order 1, walls, L 5, 48 kHz', [ROOM_B], [SOURCE_B], [MICS_B], 1, WALLS_2D, 5, 48000.0),
]


def excess(got, want, bound):
    """the largest ``|got - want| / BOUND`` over the elements (0 / 0 counts as 0, anything over a zero bound as inf), and where"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0.0, 0.0, err / bound)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[at]), at
