"""Portable, counter-based synthetic waveforms (TEST INFRASTRUCTURE).

``uniform(shape, seed)`` is a pure function of (flat index, seed): splitmix64 on uint64,
top 24 bits → an exact float32 in [-1, 1).  No libm, no RNG stream state, so the golden
fixtures only need to store OUTPUTS — inputs regenerate bit-identically anywhere.
"""
import numpy as np

_GOLD = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def _splitmix64(z):
    with np.errstate(over='ignore'):
        z = (z + _GOLD)
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def uniform(shape, seed=0, scale=1.0):
    """float32 array in [-scale, scale); ``scale`` should be a power of two to stay exact."""
    n = int(np.prod(shape))
    with np.errstate(over='ignore'):
        ctr = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x100000001B3)
    bits = _splitmix64(ctr) >> np.uint64(40)                  # 24 random bits
    val = bits.astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)
    return (val * np.float32(scale)).reshape(shape)


def audio_like(shape, seed=0):
    """Uniform noise with a per-row power-of-two gain (2^0 … 2^-7) so rows exercise
    different dynamic ranges (and the dB clamp) while staying exactly reproducible."""
    x = uniform(shape, seed)
    rows = x.reshape(-1, shape[-1])
    gains = (2.0 ** -(np.arange(rows.shape[0]) % 8)).astype(np.float32)
    return (rows * gains[:, None]).reshape(shape)


def gained_with_silence(shape, seed=0, n_fft=512, hop=128):
    """``uniform`` with dynamic range and silence, for per-frame checks: row r (over the flattened leading dims) scaled by
    2^-(r mod 13); in every third row (r = 0, 3, 6, ...) three spans of ``n_fft + hop`` zeros — the start of the row, mid-row
    off the hop grid, the end of the row — where the row holds them without overlap (start and end from 2 spans, the middle
    one from 3); row 1 all zeros whenever there are at least 3 rows.

    A span of ``n_fft + hop`` samples holds at least one whole frame on the hop grid (centred or not), and with both edge
    spans in place the first and last frames are silent for every pad mode (reflect, replicate and circular read only
    those spans).  A pure function of (shape, seed, n_fft, hop)."""
    x = uniform(shape, seed)
    rows = x.reshape(-1, shape[-1])
    n_rows, length = rows.shape
    rows *= (2.0 ** -(np.arange(n_rows) % 13)).astype(np.float32)[:, None]
    for r, lo, hi in silent_spans(shape, n_fft, hop):
        rows[r, lo:hi] = 0.0
    if n_rows >= 3:
        rows[1] = 0.0
    return rows.reshape(shape)


def silent_spans(shape, n_fft, hop):
    """The (row, start, stop) spans ``gained_with_silence`` zeroes (row 1 of 3 or more rows aside, which is zero whole)."""
    n_rows, length = int(np.prod(shape[:-1])), int(shape[-1])
    span = n_fft + hop
    out = []
    for r in range(0, n_rows, 3):
        if length >= 2 * span:
            out += [(r, 0, span), (r, length - span, length)]
        if length >= 3 * span:
            mid = min(max(span, length // 2 + hop // 3), length - 2 * span)
            out.append((r, mid, mid + span))
    return out


def has_silence(shape, n_fft, hop):
    """Whether ``gained_with_silence`` of this shape holds a silent row or silent spans (hence silent frames)."""
    return int(np.prod(shape[:-1])) >= 3 or int(shape[-1]) >= 2 * (n_fft + hop)
