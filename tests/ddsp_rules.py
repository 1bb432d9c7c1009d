"""References and per-element bounds of ``oscillator_bank`` / ``filter_waveform`` (tests/test_ddsp_cpu.py, tests/test_ddsp_gpu.py).

The references restate the definitions in numpy float64; the oscillator's running phase alone is carried in the 64-bit-mantissa
``numpy.longdouble`` and wrapped at every step, because an unwrapped float64 ``cumsum`` loses 2^-37 rad per step after 16384 steps
near Nyquist — more than the kernel under test."""
import numpy as np
import torch

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, 'the phase reference needs the x87 extended format'
TWO_PI_LD = 2 * LD('3.14159265358979323846264338327950288')
U24, TINY = 2.0 ** -24, 2.0 ** -126


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to('cuda')


def assert_close(got, ref, bound, what):
    """every element within its bound; returns the worst |err| / bound"""
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ratio = np.abs(got - ref) / bound
    assert np.isfinite(got).all() and ratio.max() <= 1.0, '%s: worst |err| / bound %.3g at %r' % (
        what, ratio.max(), np.unravel_index(np.argmax(ratio), ratio.shape))
    return float(ratio.max())


# ============================================================================= oscillator_bank
def phase_error(time):
    """rad, per step index.  Kernel: an increment is frac(f / sr) to 2^-63 turns (2^-60.3 rad) and integer sums add nothing, so
    phi[t] is off by (t + 1) 2^-60.3; sine and cosine are a float64 polynomial of an argument scaled by a rounded 2 pi / 2^64:
    2^-49 covers both.  Reference: the longdouble increment (2 pi f / sr, two roundings of a value below 2 pi |f| / sr <= 8 pi for
    the |f| <= 4 sr used here: 2^-59 in all) and the wrapped sum (half an ulp of a value below 4 pi: 2^-61).  Together below
    (t + 1) 2^-58 + 2^-48."""
    return (np.arange(time) + 1.0) * 2.0 ** -58 + 2.0 ** -48


def oscillator_bank(f, a, sr, reduction, g=None):
    """``f``, ``a``: float32 ``(…, T, N)``; ``g``: float32 upstream gradient of the output's shape.  Returns ``(y, bound)`` or, with
    ``g``, ``(y, bound, da, bound_da, df, bound_df)``, float64.

    Bounds.  y: the float64 products are added in float64 (N 2^-53 of the mass) and rounded to float32 once (2^-24 |y|); a phase
    error e moves a cell by |a'| e.  Per output: ``2^-24 |y| + (e[t] + N 2^-52) sum_n |a'| + 2^-126`` (over N for 'mean', per cell
    for 'none') — under the cap ``8 2^-24 sum |a'|``, asserted.  d a likewise with |g| for the mass.  d f is a float64 suffix sum
    of T terms rounded once: ``2^-24 |value| + (T 2^-53 + e[T - 1]) (2 pi / sr) sum_u |g a'|``, the mass factor asserted under the
    cap 2^-40 (it holds to T = 8000)."""
    assert np.abs(f).max(initial=0.0) <= 4 * sr
    T, N = f.shape[-2:]
    inc = np.mod(TWO_PI_LD * f.astype(LD) / LD(sr), TWO_PI_LD)
    phi = np.zeros(f.shape[:-2] + (N,), LD)
    sin, cos = np.empty(f.shape, np.float64), np.empty(f.shape, np.float64)
    for t in range(T):
        phi = phi + inc[..., t, :]
        phi = np.where(phi >= TWO_PI_LD, phi - TWO_PI_LD, phi)
        sin[..., t, :] = np.sin(phi)
        cos[..., t, :] = np.cos(phi)
    valid = np.abs(f.astype(np.float64)) < sr / 2
    ap = np.where(valid, a.astype(np.float64), 0.0)
    e = phase_error(T)[:, None]
    cells = ap * sin
    mass = np.abs(ap)
    scale = 1.0 / N if reduction == 'mean' else 1.0
    if reduction == 'none':
        y, ymass, ye = cells, mass, e
    else:
        y, ymass, ye = cells.sum(-1) * scale, mass.sum(-1) * scale, e[:, 0]
    bound = U24 * np.abs(y) + (ye + N * 2.0 ** -52) * ymass + TINY
    assert (bound <= 8 * U24 * ymass + TINY).all()
    if g is None:
        return y, bound
    gc = (g.astype(np.float64) if reduction == 'none' else g.astype(np.float64)[..., None] * scale) * np.ones(f.shape)
    da = np.where(valid, gc * sin, 0.0)
    bound_da = U24 * np.abs(da) + e * np.abs(gc) + TINY
    k = 2 * np.pi / sr
    df = k * np.flip(np.cumsum(np.flip((gc * ap * cos).astype(LD), -2), -2), -2).astype(np.float64)
    factor = T * 2.0 ** -53 + float(e[-1, 0])
    assert factor <= 2.0 ** -40
    bound_df = U24 * np.abs(df) + factor * k * np.abs(gc * ap).sum(-2, keepdims=True) + TINY
    return y, bound, da, bound_da, df, bound_df


# ============================================================================= filter_waveform
def filter_waveform(x, h, delay=-1, g=None, piece=2048, share=None):
    """``x``: float32 ``(R, T)``; ``h``: float32 ``(F, K)`` (shared) or ``(R, F, K)``; ``g``: float32 ``(R, T)``.  Returns ``(y, bound)``
    or, with ``g``, ``(y, bound, dx, bound_dx, dh, bound_dh)`` (``dh`` of ``h``'s shape: summed over the rows that share it).

    Bounds.  The kernels run one float32 fused multiply-add chain per result: ``(L + 2) 2^-24 sum |terms| + 2^-126`` with L the
    chain's roundings — K for y and d x (samples of other chunks enter as exact zeros); for d h the samples of one piece (at most
    C), then the pieces of a chunk and the R sharing rows added by ``torch.sum``: ``L = min(C, piece) + ceil(C / piece) - 1 + R - 1``,
    never more than the C R terms of the definition."""
    x64, h64 = x.astype(np.float64), h.astype(np.float64)
    R, T = x.shape
    F, K = h.shape[-2:]
    C = -(-T // F)
    s = delay if delay >= 0 else K // 2
    shared = h.ndim == 2
    y, ymass = np.zeros((R, T)), np.zeros((R, T))
    dx, dxmass = np.zeros((R, T)), np.zeros((R, T))
    dh, dhmass = np.zeros((R, F, K)), np.zeros((R, F, K))
    g64 = None if g is None else g.astype(np.float64)
    for r in range(R):
        hr = h64 if shared else h64[r]
        for m in range(T):                      # the input sample x[m] of chunk m // C reaches full[m + k]
            j = m // C
            k0, k1 = max(0, s - m), min(K, T + s - m)               # the taps k with 0 <= t = m + k - s < T
            if k0 >= k1:
                continue
            ts = slice(m + k0 - s, m + k1 - s)
            y[r, ts] += hr[j, k0:k1] * x64[r, m]
            ymass[r, ts] += np.abs(hr[j, k0:k1] * x64[r, m])
            if g64 is not None:
                dx[r, m] = (hr[j, k0:k1] * g64[r, ts]).sum()
                dxmass[r, m] = np.abs(hr[j, k0:k1] * g64[r, ts]).sum()
                dh[r, j, k0:k1] += x64[r, m] * g64[r, ts]
                dhmass[r, j, k0:k1] += np.abs(x64[r, m] * g64[r, ts])
    bound = (K + 2) * U24 * ymass + TINY
    if g is None:
        return y, bound
    bound_dx = (K + 2) * U24 * dxmass + TINY
    share = share or (R if shared else 1)          # (``share``: the rows the caller adds afterwards, for broadcast dims)
    L = min(C, piece) + -(-C // piece) - 1 + share - 1
    assert L <= C * share + 1
    if shared:
        dh, dhmass = dh.sum(0), dhmass.sum(0)
    return y, bound, dx, bound_dx, dh, (L + 2) * U24 * dhmass + TINY
