"""Shared by tests/test_pitch_shift_cpu.py and tests/test_pitch_shift_gpu.py (a plain module: no tests in here).

* ``pitch_shift`` restated from torchaudio's definition with ``torch.stft`` / ``torch.istft``, a phase vocoder on complex tensors and
  the per-sample float64 resampler of tests/resample_rules.py — it shares no code with the product's chain.  The one place it
  follows the package and not torchaudio is the dtype of the vocoder's time steps (``phase_vocoder_complex`` says why).
* the tail alone: ``resample_rules.reference`` cut or zero-padded to ``out_len``, with its bound
  ``(K_n + 2) * 2^-24 * sum |h||x|`` per element (imported, not copied); the padded tail is exact, its bound 0.
* the span a tile of the wide kernel reads, by brute force over every tile start.
* the grid of ``tac_polyphase_wide_f32`` restated from its launcher, next to the launcher's verbatim text, as tests/grid_rules.py
  does for the other persistent kernels."""
import math

import numpy as np
import torch

import resample_rules as R

WIDE_ENTRY = 'tac_polyphase_wide_f32'
LDS_ENTRY = 'tac_polyphase_f32'


# ----------------------------------------------------------------------------- rates
def rates(sample_rate, n_steps, bins_per_octave=12):
    """(rate, source, reduced pair) of torchaudio's pitch_shift"""
    rate = 2.0 ** (-float(n_steps) / bins_per_octave)
    source = int(sample_rate / rate)
    return rate, source, R.reduced(source, sample_rate)


# ----------------------------------------------------------------------------- the tail
def fit_reference(x, orig_freq, new_freq, out_len, **kw):
    """(ref, bound) of ``resample(x, orig_freq, new_freq)`` cut or zero-padded to ``out_len`` samples"""
    ref, bound = R.reference(x, orig_freq, new_freq, **kw)
    return fit(ref, out_len), fit(bound, out_len)


def fit(a, out_len):
    a = a[..., :out_len]
    if a.shape[-1] < out_len:
        a = np.concatenate([a, np.zeros(a.shape[:-1] + (out_len - a.shape[-1],))], axis=-1)
    return a


def fit_adjoint_reference(g, length, orig_freq, new_freq, **kw):
    """gradient of ``sum(fit(resample(x)) * g)`` w.r.t. ``x`` of ``length`` samples, ``g`` of any ``out_len``: what lies beyond
    ``min(n_out, out_len)`` does not count, whatever it holds"""
    n_out = R.out_length(length, *R.reduced(orig_freq, new_freq))
    g64 = R._np64(g)
    used = np.zeros(g64.shape[:-1] + (n_out,))
    m = min(n_out, g64.shape[-1])
    used[..., :m] = g64[..., :m]
    return R.adjoint_reference(used, length, orig_freq, new_freq, **kw)


# ----------------------------------------------------------------------------- the whole chain, float64
def phase_vocoder_complex(spec, rate, hop):
    """the package's ``phase_vocoder`` on a complex ``(rows, F, T)`` tensor.  Its time steps are ``torch.arange(0, T, rate)`` in the
    DEFAULT dtype, as the project it was modelled on evaluates them (torchaudio passes the spectrogram's real dtype): for a float64
    spectrogram the interpolation weights are float32 values, and that is part of the op's definition, not of its rounding."""
    n_freq, n_frames = spec.shape[-2], spec.shape[-1]
    advance = torch.linspace(0, math.pi * hop, n_freq, dtype=spec.real.dtype)[:, None]
    steps = torch.arange(0, n_frames, rate)
    alphas = steps % 1.0
    first = spec[..., :1].angle()
    spec = torch.nn.functional.pad(spec, [0, 2])
    s0 = spec.index_select(-1, steps.long())
    s1 = spec.index_select(-1, (steps + 1).long())
    phase = s1.angle() - s0.angle() - advance
    phase = phase - 2 * math.pi * torch.round(phase / (2 * math.pi))
    phase = phase + advance
    phase = torch.cat([first, phase[..., :-1]], dim=-1).cumsum(-1)
    mag = alphas * s1.abs() + (1 - alphas) * s0.abs()
    return torch.polar(mag, phase)


def stretched(x, sample_rate, n_steps, bins_per_octave=12, n_fft=512, win_length=None, hop_length=None, window=None):
    """the chain up to and including ``istft``: ``(rows, round(L / rate))`` in the dtype of ``x`` (a CPU tensor)"""
    rate, _, _ = rates(sample_rate, n_steps, bins_per_octave)
    hop = n_fft // 4 if hop_length is None else hop_length
    win_length = n_fft if win_length is None else win_length
    window = torch.hann_window(win_length, dtype=x.dtype) if window is None else window
    rows = x.reshape(-1, x.shape[-1])
    spec = torch.stft(rows, n_fft, hop_length=hop, win_length=win_length, window=window, center=True, pad_mode='reflect',
                      normalized=False, onesided=True, return_complex=True)
    return torch.istft(phase_vocoder_complex(spec, rate, hop), n_fft, hop_length=hop, win_length=win_length, window=window,
                       length=int(round(x.shape[-1] / rate)))


def pitch_shift_reference(x, sample_rate, n_steps, bins_per_octave=12, **kw):
    """float64 numpy, the shape of ``x``: torchaudio's ``pitch_shift`` from its definition"""
    x = x.to(torch.float64)
    y = stretched(x, sample_rate, n_steps, bins_per_octave, **kw)
    _, source, _ = rates(sample_rate, n_steps, bins_per_octave)
    if source == sample_rate:
        out = fit(y.numpy(), x.shape[-1])
    else:
        out, _ = fit_reference(y, source, sample_rate, x.shape[-1])
    return out.reshape(tuple(x.shape))


# ----------------------------------------------------------------------------- the span of a tile, by brute force
def brute_span(off, run, phases, step, tile):
    """the most consecutive input samples ``tile`` consecutive outputs read, counted from the first sample the FIRST of them reads,
    over every phase a tile can start at"""
    off, run = np.asarray(off, dtype=np.int64), np.asarray(run, dtype=np.int64)
    n = np.arange(phases + tile - 1)
    j, p = n // phases, n % phases
    first = j * step + off[p]
    last = first + run[p]
    if phases * tile <= 1 << 24:
        return int(max(1, max(int(last[s:s + tile].max() - first[s]) for s in range(phases))))
    best = 1                        # (the same maximum, a tile start at a time in blocks of starts: no (phases, tile) table)
    for s0 in range(0, phases, 4096):
        s1 = min(phases, s0 + 4096)
        windows = np.lib.stride_tricks.sliding_window_view(last[s0:s1 + tile - 1], tile)
        best = max(best, int((windows.max(axis=1) - first[s0:s1]).max()))
    return best


def monotone(off, phases, step):
    start = np.concatenate([np.asarray(off, dtype=np.int64), [off[0] + step]])
    return bool((np.diff(start) >= 0).all())


# ----------------------------------------------------------------------------- the grid of tac_polyphase_wide_f32
WIDE = ('resample.hip', (
    'constexpr int RSW_ROWS = 4;',
    'const int pitch = (3 + span + taps + 3) & ~3;',
    'const size_t bytes = 4 * (size_t)RSW_ROWS * (size_t)pitch;',
    'const long long tiles_per_row = (out_len + (1LL << tile_log) - 1) >> tile_log;',
    'const long long groups = (rows + RSW_ROWS - 1) / RSW_ROWS;',
    'const long long units = groups * tiles_per_row;',
    'long long per_cu = (long long)(RS_LDS_BYTES / bytes);',
    'per_cu = per_cu > 8 ? 8 : per_cu;',
    'const long long blocks = persistent_blocks(units, 1, (long long)device_cu_count() * per_cu);',
    'for (long long u = blockIdx.x; u < units; u += gridDim.x) {',
))
WIDE_ROWS = 4
LDS_BYTES = 160 * 1024
MAX_TENSOR_BYTES = 512 * 1000 * 1000            # the limit of tests/grid_rules.py


def wide_launch(cus, rows, out_len, span, taps, tile):
    """(units, grid cap) of the wide launch: a unit is a tile of ``tile`` outputs times a group of up to four rows"""
    pitch = (3 + span + taps + 3) & ~3
    per_cu = min(8, LDS_BYTES // (4 * WIDE_ROWS * pitch))
    return -(-rows // WIDE_ROWS) * -(-out_len // tile), cus * per_cu


def wrap_shape(cus, span, taps, tile, out_len):
    """rows of ``out_len`` outputs with ``units = 2 grid + r``, ``0 < r < grid``, the last row group a partial one"""
    tiles = -(-out_len // tile)
    _, grid = wide_launch(cus, 1, out_len, span, taps, tile)
    groups = -(-(2 * grid + 37) // tiles)
    rows = WIDE_ROWS * groups - 1
    units, grid = wide_launch(cus, rows, out_len, span, taps, tile)
    assert 0 < units - 2 * grid < grid, (units, grid)
    return rows
