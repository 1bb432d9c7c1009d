"""Shared by tests/test_istft_cpu.py and tests/test_istft_gpu.py: the reference (``torch.istft`` in float64 on the CPU on the same
float32 spectrogram), the four formulas of the inverse restated in numpy, the operand rule of the frame kernels' inverse mode, the
analytic gradient recipe and the per-block error measure."""
import math

import numpy as np
import torch

from oracle import signals, torch_ref


def padded_window(window, n_fft):
    """the window zero-padded centred to fft_length, float64 numpy"""
    w = np.zeros(n_fft, dtype=np.float64)
    wl = len(window)
    off = (n_fft - wl) // 2
    w[off:off + wl] = np.asarray(window, dtype=np.float64)
    return w


def torch_istft(spec, n_fft, hop, window, center=True, normalized=False, length=None, dtype=torch.float64):
    """``torch.istft`` on the CPU in ``dtype`` on the values of ``spec`` (*, F, T, 2); window: 1-D tensor of win_length"""
    z = spec.detach().cpu().to(dtype)
    lead = tuple(z.shape[:-3])
    z = torch.view_as_complex(z.reshape((-1,) + tuple(z.shape[-3:])).contiguous())
    w = window.detach().cpu().to(dtype)
    out = torch.istft(z, n_fft, hop_length=hop, win_length=w.shape[0], window=w, center=center, normalized=normalized,
                      onesided=True, length=length, return_complex=False)
    return out.reshape(lead + (out.shape[-1],))


def c2r(h, n_fft):
    """C2R(H)[n] = H[0] + H[NC] (-1)^n + 2 Re sum_{0<k<NC} H[k] e^{+2 pi i k n / N}: the transform the frame kernels run, on the
    operands H (complex (NC + 1,)), as a plain sum"""
    nc = n_fft // 2
    n = np.arange(n_fft)
    k = np.arange(1, nc)
    mid = 2.0 * (h[1:nc, None] * np.exp(2j * np.pi * ((k[:, None] * n[None, :]) % n_fft) / n_fft)).real.sum(0)
    return h[0].real + h[nc].real * (-1.0) ** n + mid


def inverse_operands(x):
    """the inverse mode's operand rule: H[0] = Re X[0], H[NC] = Re X[NC], H[k] = X[k] (the gradient mode doubles the two ends)"""
    h = np.array(x, dtype=np.complex128)
    h[0] = h[0].real
    h[-1] = h[-1].real
    return h


def adjoint_operands(g):
    h = np.array(g, dtype=np.complex128)
    h[0] = 2.0 * h[0].real
    h[-1] = 2.0 * h[-1].real
    return h


def numpy_istft(spec, n_fft, hop, window, center=True, normalized=False, length=None):
    """the four formulas of the inverse, in float64: spec (F, T, 2) -> (samples,).  Also returns min env over the kept range."""
    z = np.asarray(spec, dtype=np.float64)
    z = z[..., 0] + 1j * z[..., 1]
    n_frames = z.shape[1]
    w = padded_window(window, n_fft)
    pad = n_fft // 2 if center else 0
    n_pos = hop * (n_frames - 1) + n_fft
    num, env = np.zeros(n_pos), np.zeros(n_pos)
    for t in range(n_frames):
        y = np.fft.irfft(z[:, t], n_fft) * (math.sqrt(n_fft) if normalized else 1.0)
        num[t * hop:t * hop + n_fft] += w * y
        env[t * hop:t * hop + n_fft] += w * w
    full = n_pos - 2 * pad
    kept = full if length is None else min(n_pos - pad, length)     # (torch.istft slices [pad, pad + length) of the positions)
    out = np.zeros(full if length is None else length)
    out[:kept] = num[pad:pad + kept] / env[pad:pad + kept]
    return out, float(env[pad:pad + kept].min())


def grad_recipe(grad_out, window, n_fft, hop, n_frames, center=True, normalized=False):
    """gradient of istft w.r.t. the spectrogram from the gradient of its output (rows, samples), float64 torch on the CPU:
    stft (center=False, same window) of grad_out / env zero-extended to the padded length, times the bin weights
    (1, 0) for the DC and Nyquist bins and 2 for the rest, times the inverse's scale.  Returns (rows, F, T, 2)."""
    go = grad_out.detach().cpu().double()
    w = torch.from_numpy(padded_window(window.detach().cpu().double().numpy(), n_fft))
    pad = n_fft // 2 if center else 0
    n_pos = hop * (n_frames - 1) + n_fft
    env = torch.zeros(n_pos, dtype=torch.float64)
    for t in range(n_frames):
        env[t * hop:t * hop + n_fft] += w * w
    kept = min(n_pos - pad, go.shape[-1])
    padded = torch.zeros(go.shape[0], n_pos, dtype=torch.float64)
    padded[:, pad:pad + kept] = go[:, :kept] / env[pad:pad + kept]
    s = torch.stft(padded, n_fft, hop_length=hop, win_length=n_fft, window=w, center=False, normalized=False, onesided=True,
                   return_complex=True)
    s = torch.view_as_real(s).clone()                                  # (rows, F, T, 2)
    scale = (math.sqrt(n_fft) if normalized else 1.0) / n_fft
    s *= 2.0 * scale
    for k in (0, n_fft // 2):
        s[:, k, :, 0] *= 0.5
        s[:, k, :, 1] = 0.0
    return s


def autograd_grad(spec, grad_out, n_fft, hop, window, center=True, normalized=False, length=None, dtype=torch.float64):
    """gradient of sum(istft(spec) * grad_out) w.r.t. spec by autograd through ``torch.istft`` on the CPU in ``dtype``"""
    z = spec.detach().cpu().to(dtype).clone().requires_grad_(True)
    out = torch_istft_graph(z, n_fft, hop, window.detach().cpu().to(dtype), center, normalized, length)
    out.backward(grad_out.detach().cpu().to(dtype).reshape(out.shape))
    return z.grad


def torch_istft_graph(z, n_fft, hop, w, center, normalized, length):
    lead = tuple(z.shape[:-3])
    zc = torch.view_as_complex(z.reshape((-1,) + tuple(z.shape[-3:])).contiguous())
    out = torch.istft(zc, n_fft, hop_length=hop, win_length=w.shape[0], window=w, center=center, normalized=normalized,
                      onesided=True, length=length, return_complex=False)
    return out.reshape(lead + (out.shape[-1],))


def block_ratios(got, ref, hop, n_fft):
    """(rows, blocks) float64: the largest error of every block of ``hop`` output samples divided by the largest reference
    magnitude over the blocks within ``fft_length`` of it — a quiet passage is held to its own scale, not to the row's.
    0 for an exactly matching silent neighbourhood, inf for a silent one that is not matched exactly, NaN propagates."""
    g = got.detach().cpu().double().reshape(-1, got.shape[-1])
    r = ref.detach().cpu().double().reshape(-1, ref.shape[-1])
    n = r.shape[1]
    n_blocks = (n + hop - 1) // hop
    fill = n_blocks * hop - n
    err = torch.nn.functional.pad((g - r).abs(), (0, fill)).reshape(-1, n_blocks, hop).amax(-1)
    mag = torch.nn.functional.pad(r.abs(), (0, fill)).reshape(-1, n_blocks, hop).amax(-1)
    reach = (n_fft + hop - 1) // hop
    scale = torch.nn.functional.max_pool1d(mag[:, None, :], 2 * reach + 1, stride=1, padding=reach)[:, 0, :]
    ratio = err / scale
    ratio = torch.where((err == 0) & (scale == 0), torch.zeros_like(ratio), ratio)
    return ratio


def consistent_spec(shape, n_fft, hop, window, seed, center=True, normalized=False, rows_special=True):
    """(waveform float32 (rows, L), float32 spectrogram (rows, F, T, 2) = the CPU stft of it).  With three or more rows, row 1
    is silent and row 2 sits at gain 2^-12."""
    x = torch.from_numpy(signals.audio_like(shape, seed=seed))
    if rows_special and shape[0] >= 3:
        x[1] = 0.0
        x[2] *= 2.0 ** -12
    mode = 'reflect' if shape[-1] > n_fft // 2 else 'constant'        # (a row of one or two hops is too short to reflect)
    z = torch_ref.stft(x, n_fft, hop, win_length=window.shape[0], window=window.cpu(), center=center, pad_mode=mode,
                       normalized=normalized)
    return x, z.float()


def random_spec(rows, n_fft, n_frames, seed):
    """a non-consistent spectrogram: seeded normal pairs (no waveform has it as its stft)"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(rows, n_fft // 2 + 1, n_frames, 2, generator=gen, dtype=torch.float32)
