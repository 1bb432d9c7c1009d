"""The constant-Q transform of ``functional.cqt`` restated in float64 on numpy, with the per-element bound a float32 evaluation has
to meet.  The only oracle of tests/test_cqt_cpu.py and tests/test_cqt_gpu.py.

Definition: the one in ``functional.cqt``'s docstring, ``C[k, t] = sum_j x'[s_t + j - floor(N_k / 2)] conj(g_k[j])``, ``s_t = t hop``
(``center``) or ``floor(N_0 / 2) + t hop``; ``x'`` is the row mirrored once at both ends (``'reflect'``) and zero beyond.

Bound, ``u = 2^-24``: the bank is rounded once to float32 and ``n`` nonzero products are added in float32 in some order, so each of
the real and imaginary sums is off by at most ``gamma_{n+2} S``, ``S[k, t] = sum_j |x'| |g_k[j]|``, ``gamma_m = m u / (1 - m u)``,
and the complex value by ``E = sqrt(2) gamma_{n+2} S``.  ``power=1``: ``||c| - |C|| <= E`` and the epilogue ``sqrt(re re + im im)``
adds two roundings of the sum of squares (halved by the root) and a root good to 1 ulp: ``E + 4 u (|C| + E)``.  ``power=2``:
``||c|^2 - |C|^2| <= E (2 |C| + E)``, plus three roundings: ``+ 3 u (|C| + E)^2``.  A result below the smallest normal float32 may be
flushed: ``2^-126`` is added (``2^-63`` after a root of a flushed square)."""
import math

import numpy as np
import torch

U = 2.0 ** -24


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


def wavelets(sr, fmin, n_bins, B, filter_scale=1.0, gamma=0.0, norm=1, scale=True):
    """``[g_k]`` as complex128 arrays"""
    alpha = 2.0 ** (1.0 / B) - 1.0
    out = []
    for k in range(n_bins):
        f = fmin * 2.0 ** (k / B)
        N = int(math.ceil(filter_scale / alpha * sr / (f + gamma / alpha)))
        j = np.arange(N)
        g = (0.5 - 0.5 * np.cos(2 * np.pi * j / N)) * np.exp(2j * np.pi * f * (j - N // 2) / sr)
        if norm is not None:
            g = g / np.sum(np.abs(g) ** norm) ** (1.0 / norm)
        out.append(g * math.sqrt(N) if scale else g)
    return out


def cqt(x, sr, hop_length, fmin, n_bins, bins_per_octave, filter_scale=1.0, gamma=0.0, norm=1, center=True, pad_mode='reflect', scale=True, power=None):
    """``(value, bound)`` in float64 for rows ``x`` of shape ``(…, len)``: ``value`` complex ``(…, K, T)`` (real for a ``power``)"""
    x = np.asarray(x, np.float64)
    length = x.shape[-1]
    gs = wavelets(sr, fmin, n_bins, bins_per_octave, filter_scale, gamma, norm, scale)
    n0, hop = gs[0].size, hop_length
    T = 1 + length // hop if center else 1 + (length - n0) // hop
    val = np.zeros(x.shape[:-1] + (n_bins, T), np.complex128)
    bound = np.zeros(x.shape[:-1] + (n_bins, T))
    for k, g in enumerate(gs):
        i = (0 if center else n0 // 2) + hop * np.arange(T)[:, None] + np.arange(g.size)[None, :] - g.size // 2
        if center and pad_mode == 'reflect':
            i = np.where(i < 0, -i, np.where(i >= length, 2 * (length - 1) - i, i))
        inside = (i >= 0) & (i < length)
        X = np.where(inside, x[..., np.clip(i, 0, length - 1)], 0.0)                    # (…, T, N_k)
        g32 = np.conj(g).real.astype(np.float32) + 1j * np.conj(g).imag.astype(np.float32)
        with np.errstate(invalid='ignore'):
            val[..., k, :] = X @ np.conj(g)
            S = np.abs(X) @ np.abs(g)
        n = (X != 0).astype(np.float64) @ (g32 != 0).astype(np.float64) + 2
        bound[..., k, :] = math.sqrt(2) * n * U / (1 - n * U) * S
    if power is None:
        return val, bound + 2.0 ** -126
    mod = np.abs(val)
    if power == 1.0:
        return mod, bound + 4 * U * (mod + bound) + 2.0 ** -63
    return mod ** 2, bound * (2 * mod + bound) + 3 * U * (mod + bound) ** 2 + 2.0 ** -126


def signals(length, sr, hop, seed):
    """``(dense, sparse)`` float32 rows: two tones plus noise; five impulses of different amplitudes at odd positions that share no
    factor with the hop"""
    r = np.random.default_rng(seed)
    t = np.arange(length) / sr
    dense = (0.6 * np.sin(2 * np.pi * 0.031 * sr * t) + 0.3 * np.sin(2 * np.pi * 0.173 * sr * t + 1.0)
             + 0.1 * r.standard_normal(length)).astype(np.float32)
    sparse = np.zeros(length, np.float32)
    at = [p for p in (3 * length // 16 | 1, 5 * length // 16 | 1, length // 2 | 1, 11 * length // 16 | 1, length - 2 | 1)
          if p < length and math.gcd(p, hop) == 1]
    sparse[at] = np.array([1.0, -0.75, 0.5, 1.5, -1.25], np.float32)[:len(at)]
    return dense, sparse


def assert_close(got, value, bound, what):
    """every element within its bound; returns the worst ratio.  ``got``: pairs ``(…, K, T, 2)`` for a complex ``value``"""
    got = got.detach().cpu().double().numpy()
    if np.iscomplexobj(value):
        got = got[..., 0] + 1j * got[..., 1]
    assert got.shape == value.shape, '%s: shape %r, expected %r' % (what, got.shape, value.shape)
    ratio = np.abs(got - value) / bound
    assert np.all(ratio <= 1.0), '%s: |err| / bound up to %g at %r' % (what, np.nanmax(ratio), np.unravel_index(np.nanargmax(ratio), ratio.shape))
    return float(ratio.max())
