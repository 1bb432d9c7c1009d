"""Shared by tests/test_stretch_cpu.py and tests/test_stretch_gpu.py: the reference chain in the oracle, the interpolated-magnitude
formula it equals, and the rule that says where the reference loses values to non-finite input."""
import math

import numpy as np
import torch

from oracle import torch_ref


def phase_advance(hop, n_freqs, dtype=torch.float32):
    return torch.linspace(0, math.pi * hop, n_freqs, dtype=dtype)[..., None]


def grid(n_frames, rate):
    """first source frame and weight of the second per output frame, as the reference's host ops round them"""
    steps = torch.arange(0, n_frames, rate)
    return steps.long().numpy(), torch.remainder(steps, torch.tensor(1.0)).numpy()


def oracle_chain(z, rate, adv, power):
    """complex_norm(phase_vocoder(z)) with the oracle's own functions; z (*, F, T, 2)"""
    return torch_ref.complex_norm(torch_ref.phase_vocoder(z, rate, adv), power)


def interpolated(mag, rate, power):
    """(alpha |X[t1]| + (1 - alpha) |X[t0]|) ** power, evaluated in the reference's order; mag (*, F, T) numpy or tensor"""
    mag = torch.as_tensor(mag)
    idx0, alpha = grid(mag.shape[-1], rate)
    padded = torch.nn.functional.pad(mag, [0, 2])
    a = torch.from_numpy(alpha).to(mag.dtype)
    out = a * padded[..., torch.from_numpy(idx0 + 1)] + (1 - a) * padded[..., torch.from_numpy(idx0)]
    return out if power == 1.0 else out.pow(power)


def lost_positions(mag, rate):
    """The position rule, in plain Python: output frame j of a bin is NaN in the reference iff a source frame among frame 0 and
    idx0[i], idx0[i] + 1 for i <= j is NaN there (i == j through the interpolation itself, i < j through the cumulative phase;
    frames past the end are zero padding, frames skipped at rate > 2 are never read); an infinite value with a finite angle only
    makes the frames interpolated from it non-finite.  mag: (F, T) numpy array of magnitudes (NaN where a component is NaN).
    Returns (nan_mask, nonfinite_mask) of shape (F, n_out)."""
    n_freqs, n_frames = mag.shape
    idx0, alpha = grid(n_frames, rate)
    n_out = len(idx0)
    nan_mask = np.zeros((n_freqs, n_out), dtype=bool)
    bad_mask = np.zeros((n_freqs, n_out), dtype=bool)
    for f in range(n_freqs):
        sticky = bool(np.isnan(mag[f, 0]))
        for j in range(n_out):
            here = [mag[f, t] for t in (idx0[j], idx0[j] + 1) if t < n_frames]
            sticky = sticky or any(np.isnan(v) for v in here)
            nan_mask[f, j] = sticky
            bad_mask[f, j] = sticky or any(np.isinf(v) for v in here)
    return nan_mask, bad_mask
