"""Host side of ``cqt``: argument checks, the wavelets of the time-domain constant-Q / variable-Q transform in float64, and the
bank arranged the way the lanes of ``tac_cqt_f32`` consume it (csrc/cqt.hip).  numpy and Python numbers only; nothing here touches
a device.

With ``B = bins_per_octave``, ``alpha = 2^(1/B) - 1``, ``Q = filter_scale / alpha``: ``f_k = fmin 2^(k/B)``, ``N_k = ceil(Q sr /
(f_k + gamma / alpha))``, ``g_k[j] = w_k[j] exp(2 pi i f_k (j - floor(N_k / 2)) / sr)`` with the periodic Hann window of ``N_k``
points, divided by its ``norm``-norm and multiplied by ``sqrt(N_k)`` where ``scale``.  What is kept is ``conj(g_k)``: the transform
is ``C[k, t] = sum_j x'[t hop + origin + e_k + j] conj(g_k[j])`` on a tap axis where every wavelet is centred at ``c0 = floor(N_0 /
2)``, ``e_k = c0 - floor(N_k / 2)``; ``x'`` is the row mirrored once at both ends (``'reflect'``) and zero beyond."""
import math

import numpy as np
import torch

from ._bounded import Bounded

PAD_MODES = ('reflect', 'constant')
GROUP_BINS = 8          # bins per group of the kernel's bank: 16 real columns (csrc/cqt.hip: CQ_GROUP_BINS)
STEP = 16               # taps per 1 KiB block of the bank (CQ_STEP)


def check(sample_rate, hop_length, fmin, n_bins, bins_per_octave, filter_scale, gamma, norm, pad_mode, power):
    """The argument errors of ``cqt``, raised before anything is built or launched."""
    for name, v in (('hop_length', hop_length), ('n_bins', n_bins), ('bins_per_octave', bins_per_octave)):
        if int(v) != v or v < 1:
            raise ValueError('cqt: %s must be a positive integer, got %r' % (name, v))
    for name, v in (('sample_rate', sample_rate), ('fmin', fmin), ('filter_scale', filter_scale)):
        if not (v > 0 and math.isfinite(v)):
            raise ValueError('cqt: %s must be positive, got %r' % (name, v))
    if not (gamma >= 0 and math.isfinite(gamma)):
        raise ValueError('cqt: gamma must not be negative, got %r' % (gamma,))
    top = fmin * 2.0 ** ((n_bins - 1) / bins_per_octave)
    if top > sample_rate / 2:
        raise ValueError('cqt: the highest bin, %g Hz, lies above Nyquist (%g Hz)' % (top, sample_rate / 2))
    if norm not in (1, 2, None):
        raise ValueError('cqt: norm must be 1, 2 or None, got %r' % (norm,))
    if pad_mode not in PAD_MODES:
        raise ValueError('cqt: pad_mode must be one of %r, got %r' % (PAD_MODES, pad_mode))
    if power not in (None, 1.0, 2.0):
        raise ValueError('cqt: power must be None, 1.0 or 2.0, got %r' % (power,))


def n_frames(length, n_max, hop_length, center, pad_mode):
    """Frames of a row of ``length`` samples; ``RuntimeError`` for a row too short to be padded or to hold one frame."""
    if center:
        if pad_mode == 'reflect' and not length > n_max // 2:
            raise RuntimeError('cqt: reflect padding by %d samples needs a row longer than that, got %d' % (n_max // 2, length))
        if length < 1:
            raise RuntimeError('cqt: an empty row has no frame')
        return 1 + length // hop_length
    if length < n_max:
        raise RuntimeError('cqt: center=False needs at least the longest wavelet, %d samples, got %d' % (n_max, length))
    return 1 + (length - n_max) // hop_length


class CqtPlan(object):
    """``lengths``: ``N_k``; ``wavelets``: ``conj(g_k)`` as complex128 arrays, normalised and scaled; ``c0``, ``n_max``; the
    kernel's operands as host tensors: ``bank`` float32 ``(blocks, 64, 4)``, ``groups`` int32 ``(G, 4)`` = (start on the tap axis,
    steps, first block, bins), ``span`` the end of group 0; ``dense()``: the ``(2 K, N_max)`` float64 matrix of the composite."""
    __slots__ = ('lengths', 'wavelets', 'c0', 'n_max', 'bank', 'groups', 'span', '_dense')

    def dense(self):
        """rows ``0 … K-1`` the real parts, ``K … 2K-1`` the imaginary parts of ``conj(g_k)``, centred in ``N_max`` taps and
        zero-filled: the kernels of the padded ``conv1d`` form (built on first use)"""
        if self._dense is None:
            K = len(self.wavelets)
            m = np.zeros((2 * K, self.n_max), np.float64)
            for k, g in enumerate(self.wavelets):
                at = self.c0 - self.lengths[k] // 2
                m[k, at:at + g.size] = g.real
                m[K + k, at:at + g.size] = g.imag
            self._dense = torch.from_numpy(m)
        return self._dense


def wavelets(sample_rate, fmin, n_bins, bins_per_octave, filter_scale, gamma, norm, scale):
    """``(N_k, conj(g_k))`` in float64"""
    alpha = 2.0 ** (1.0 / bins_per_octave) - 1.0
    Q = filter_scale / alpha
    lengths, out = [], []
    for k in range(n_bins):
        f = fmin * 2.0 ** (k / bins_per_octave)
        N = int(math.ceil(Q * sample_rate / (f + gamma / alpha)))
        j = np.arange(N, dtype=np.float64)
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * j / N)
        if norm == 1:
            w = w / np.sum(w)
        elif norm == 2:
            w = w / math.sqrt(np.sum(w * w))
        if scale:
            w = w * math.sqrt(N)
        ph = 2.0 * np.pi * f * (j - N // 2) / sample_rate
        lengths.append(N)
        out.append(w * np.cos(ph) - 1j * (w * np.sin(ph)))
    return lengths, out


def arrange(lengths, conj_g):
    """``(bank, groups, span)``: the bank in the order the lanes read it.  Lane ``(kk, i) = (lane // 16, lane % 16)`` of block
    ``s`` of a group holds column ``i`` (bin ``i // 2`` of the group, real part for even ``i``) at taps ``E + 16 s + 4 kk + m``,
    ``m = 0 … 3``: K slot ``kk`` of the ``m``-th of four back-to-back matrix instructions."""
    c0 = lengths[0] // 2
    groups, blocks = [], []
    for first in range(0, len(lengths), GROUP_BINS):
        bins = min(GROUP_BINS, len(lengths) - first)
        E = (c0 - lengths[first] // 2) // STEP * STEP
        end = max(c0 - lengths[k] // 2 + lengths[k] for k in range(first, first + bins))
        steps = -(-(end - E) // STEP)
        cols = np.zeros((2 * GROUP_BINS, steps * STEP), np.float64)
        for b in range(bins):
            k = first + b
            at = c0 - lengths[k] // 2 - E
            cols[2 * b, at:at + lengths[k]] = conj_g[k].real
            cols[2 * b + 1, at:at + lengths[k]] = conj_g[k].imag
        # (column, step, kk, m) -> (step, kk, column, m): a block is 64 lanes x 4 floats
        blocks.append(cols.reshape(2 * GROUP_BINS, steps, 4, 4).transpose(1, 2, 0, 3).reshape(steps, 64, 4))
        groups.append((E, steps, sum(g[1] for g in groups), bins))
    bank = torch.from_numpy(np.concatenate(blocks).astype(np.float32))
    return bank, torch.tensor(groups, dtype=torch.int32), groups[0][0] + STEP * groups[0][1]


def unpack(plan):
    """The float32 bank de-permuted: ``conj(g_k)`` per bin as complex64 arrays, and what lies outside every bin's own support
    (all of it has to be zero)"""
    bank, out, stray = plan.bank.numpy(), [], 0.0
    for (E, steps, first, bins), g in zip(plan.groups.tolist(), range(len(plan.groups))):
        cols = bank[first:first + steps].reshape(steps, 4, 2 * GROUP_BINS, 4).transpose(2, 0, 1, 3).reshape(2 * GROUP_BINS, steps * STEP)
        cols = cols.copy()
        for b in range(bins):
            k = g * GROUP_BINS + b
            at = plan.c0 - plan.lengths[k] // 2 - E
            out.append(cols[2 * b, at:at + plan.lengths[k]] + 1j * cols[2 * b + 1, at:at + plan.lengths[k]])
            cols[2 * b:2 * b + 2, at:at + plan.lengths[k]] = 0.0
        stray = max(stray, float(np.abs(cols).max()))
    return out, stray


_plans = Bounded(8)


def plan(sample_rate, fmin, n_bins, bins_per_octave, filter_scale, gamma, norm, scale):
    """The ``CqtPlan`` of an argument set (checked by ``check``), built once and kept."""
    key = (float(sample_rate), float(fmin), int(n_bins), int(bins_per_octave), float(filter_scale), float(gamma), norm, bool(scale))
    hit = _plans.get(key)
    if hit is None:
        with torch.inference_mode(False):
            hit = CqtPlan()
            hit.lengths, hit.wavelets = wavelets(*key)
            hit.c0, hit.n_max, hit._dense = hit.lengths[0] // 2, hit.lengths[0], None
            hit.bank, hit.groups, hit.span = arrange(hit.lengths, hit.wavelets)
        _plans[key] = hit
    return hit
