"""Shared by tests/test_convolve_cpu.py and tests/test_convolve_gpu.py: the reference (``numpy.convolve`` in float64 on the same
float32 inputs), the three crops, the five steps of the partitioned route restated in numpy (frames, kernel spectra, delay line,
kept halves), the inputs and the error measures."""
import numpy as np
import torch

from istft_rules import block_ratios        # noqa: F401  (the per-block measure: block = N / 2, neighbourhood = N)
from oracle import signals

TIGHT = 2e-6
U = 2.0 ** -24


def reference(x, h):
    """float64 full convolution per row: x (rows, L), h (rows or 1, M) -> (rows, L + M - 1)"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, np.shape(x)[-1])
    h = np.asarray(h, dtype=np.float64).reshape(-1, np.shape(h)[-1])
    return np.stack([np.convolve(x[r], h[r if h.shape[0] > 1 else 0]) for r in range(x.shape[0])])


def crop(full, x_length, y_length, mode):
    """torchaudio's rule: 'valid' keeps max - min + 1 samples, 'same' keeps x_length, both centred in the full result"""
    if mode == 'full':
        return full
    target = max(x_length, y_length) - min(x_length, y_length) + 1 if mode == 'valid' else x_length
    start = (full.shape[-1] - target) // 2
    return full[..., start:start + target]


def partitions(m, n_fft):
    return -(-m // (n_fft // 2))


def kernel_spectra(h, n_fft, dtype=np.float64):
    """H_p = rfft_N([h[p B .. (p + 1) B) | B zeros]): (P, N / 2 + 1) complex"""
    b = n_fft // 2
    p = partitions(len(h), n_fft)
    hp = np.zeros(p * b, dtype=dtype)
    hp[:len(h)] = h
    return np.stack([np.fft.rfft(np.concatenate([hp[q * b:(q + 1) * b], np.zeros(b, dtype=dtype)])) for q in range(p)])


def delay_line(X, H, conj=False):
    """Y_t = sum_{p <= min(P - 1, t)} X_{t-p} H_p: X (T, F), H (P, F)"""
    Y = np.zeros_like(X)
    Hc = np.conj(H) if conj else H
    for p in range(min(H.shape[0], X.shape[0])):
        Y[p:] += X[:X.shape[0] - p] * Hc[p]
    return Y


def overlap_save(x, h, n_fft):
    """steps 1 - 5 in float64: padded copy, frames at hop B, kernel spectra, delay line, kept second halves"""
    b = n_fft // 2
    length, m = len(x), len(h)
    t = -(-(length + m - 1) // b)
    xp = np.zeros((t + 1) * b)
    xp[b:b + length] = x
    X = np.stack([np.fft.rfft(xp[i * b:i * b + n_fft]) for i in range(t)])
    Y = delay_line(X, kernel_spectra(np.asarray(h, dtype=np.float64), n_fft))
    y = np.concatenate([np.fft.irfft(Y[i], n_fft)[b:] for i in range(t)])
    return y[:length + m - 1]


def waveform(shape, seed):
    """``signals.audio_like``; with three or more rows, row 1 is silent and row 2 sits at gain 2^-12"""
    x = np.array(signals.audio_like(shape, seed=seed), dtype=np.float32)
    rows = x.reshape(-1, shape[-1])
    if rows.shape[0] >= 3:
        rows[1] = 0.0
        rows[2] *= 2.0 ** -12
    return rows.reshape(shape)


def white_kernel(shape, seed):
    """non-decaying seeded normal noise: a dropped or shifted partition shows at full scale"""
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def rir(m, seed):
    """a decaying room impulse response: normal noise under exp(-6 n / M)"""
    return (np.random.default_rng(seed).standard_normal(m) * np.exp(-6.0 * np.arange(m) / m)).astype(np.float32)


def direct_bound(x, h):
    """(M + 2) 2^-24 (|x| * |h|), elementwise: the bound of one fused multiply-add chain of M terms"""
    m = np.shape(h)[-1]
    return (m + 2) * U * reference(np.abs(x), np.abs(h)) + 2.0 ** -126


def mac_reference(X, H, hrow, conj):
    """float64 torch tensors X (rows, T, F, 2), H (h_rows, P, F, 2), hrow: list or None -> (Y_re, Y_im, bound_re, bound_im), the
    bounds without the (2 P + 2) 2^-24 factor: sum_p |Xr||Hr| + |Xi||Hi| and its imaginary-part analogue"""
    rows, t = X.shape[0], X.shape[1]
    idx = torch.tensor(hrow if hrow is not None else [0] * rows, device=X.device)
    Hs = H[idx]
    xr, xi = X[..., 0], X[..., 1]
    out = [torch.zeros_like(xr) for _ in range(4)]
    for p in range(min(H.shape[1], t)):
        hr, hi = Hs[:, p:p + 1, :, 0], Hs[:, p:p + 1, :, 1] * (-1.0 if conj else 1.0)
        a, b = xr[:, :t - p], xi[:, :t - p]
        out[0][:, p:] += a * hr - b * hi
        out[1][:, p:] += a * hi + b * hr
        out[2][:, p:] += a.abs() * hr.abs() + b.abs() * hi.abs()
        out[3][:, p:] += a.abs() * hi.abs() + b.abs() * hr.abs()
    return out
