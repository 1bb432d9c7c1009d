"""Functional API — same names, argument order, defaults and error behaviour as the reference's
``torchaudio_contrib/functional.py``.  Every function resolves its defaults and calls ONE PyTorch custom op of
the ``tac_amd`` namespace (``_ops.py``); for float32 tensors on a HIP device that op is a hand-written gfx950
kernel reached through the C ABI of ``include/tac_amd.h``.

Where the work runs (decided by the dispatcher, like for any torch op):
  * HIP device, float32 (float16 / bfloat16 widened)  → the gfx950 kernels; a missing ``libtac_amd.so`` raises.
  * CPU tensors (the reference's own test-suite, BASELINE configs[0]) → torch's CPU operators in the reference's
    operator order (``_composite.py``), so reference call sites written for the CPU keep working unchanged.
  * HIP device, float64 (the reference keeps f64 → f64) → the float64 kernels of the STFT chain and the phase vocoder
    (``_hip64.py``); float64 mu-law and HPSS → torch's operators on the device, announced.

Outputs are fresh tensors; the STFT-family results are returned as the same strided views the reference
produces (physically frame-major, logically ``(*, channel, freq, time[, 2])``).
"""
import dataclasses
import math
import warnings

import torch

from . import _composite
from . import _hip
from . import _ops
from . import _filters
from . import _kaldi
from . import _pitch
from . import _vad
from . import _rir
from . import _beamform
from . import _resample
from . import _specaug
from . import _augment
from . import _sox
from ._bounded import Bounded
from ._lazy import realize as _realize

__all__ = ['stft', 'istft', 'griffinlim', 'complex_norm', 'create_mel_filter', 'apply_filterbank', 'angle', 'magphase',
           'phase_vocoder', 'amplitude_to_db', 'db_to_amplitude', 'mu_law_encoding', 'mu_law_decoding', 'hpss',
           'create_dct', 'dct', 'resample', 'kaldi_fbank', 'kaldi_mfcc', 'kaldi_spectrogram', 'sliding_window_cmn', 'compute_deltas', 'mask_along_axis', 'mask_along_axis_iid', 'add_noise', 'speed', 'pitch_shift', 'fftconvolve', 'convolve', 'lfilter', 'sosfilt', 'tf2sos', 'filtfilt', 'biquad', 'lowpass_biquad', 'highpass_biquad', 'bandpass_biquad',
           'bandreject_biquad', 'allpass_biquad', 'equalizer_biquad', 'preemphasis', 'deemphasis', 'loudness', 'detect_pitch_frequency',
           'psd', 'mvdr_weights_souden', 'apply_beamforming', 'rtf_evd', 'rtf_power', 'mvdr_weights_rtf', 'rnnt_loss',
           'forced_align', 'merge_tokens', 'TokenSpan', 'vad', 'vad_start', 'simulate_rir_ism', 'simulate_rir_ism_batch',
           'overdrive', 'phaser', 'flanger']

_call = _ops.call


def _tensor(x, what):
    if not torch.is_tensor(x):
        raise TypeError('%s must be a torch.Tensor, got %s' % (what, type(x).__name__))
    return _realize(x)


_window_cache = Bounded(64)


def default_window(n, like):
    """periodic Hann of ``win_length`` — the constructor the reference calls (functional.py:93-97,
    layers.py:76-80), cached per (length, device, dtype) for ordinary tensors (never while tracing)."""
    dtype = like.dtype if like.dtype in (torch.float32, torch.float64) else torch.float32
    if type(like) is not torch.Tensor or torch.compiler.is_compiling():
        return torch.hann_window(n, dtype=dtype, device=like.device)
    key = (n, str(like.device), dtype)
    w = _window_cache.get(key)
    if w is None:
        # built outside inference mode whatever the caller's mode: an inference tensor in the cache could not be saved for
        # a later call's backward ("Inference tensors cannot be saved for backward")
        with torch.inference_mode(False):
            w = torch.hann_window(n, dtype=dtype, device=like.device)
        _window_cache[key] = w
    return w


def resolve_stft_args(waveforms, fft_length, hop_length, win_length, window):
    """Defaults of reference functional.py:48-49 / :86-97 and the window checks ``torch.stft`` performs."""
    n_fft = int(fft_length)
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    win_length = n_fft if win_length is None else int(win_length)
    if window is None:
        if not 0 < win_length <= max(n_fft, 1):
            raise RuntimeError('stft: expected 0 < win_length <= n_fft, got win_length=%d' % win_length)
        window = default_window(win_length, waveforms)
    else:
        if not torch.is_tensor(window) or window.dim() != 1 or window.shape[0] != win_length:
            raise RuntimeError('stft: expected a 1D window tensor of size equal to win_length=%d' % win_length)
        if window.device != waveforms.device:
            raise RuntimeError('stft: input and window must be on the same device, got %s and %s'
                               % (waveforms.device, window.device))
    return n_fft, hop, win_length, window


# ----------------------------------------------------------------------------- public API
def stft(waveforms, fft_length, hop_length=None, win_length=None, window=None,
         center=True, pad_mode='reflect', normalized=False, onesided=True):
    """Short-time Fourier transform of ``(*, channel, time)`` waveforms →
    ``(*, channel, num_freqs, time, complex=2)``  (reference: functional.py:48-113).

    ``window=None`` means a periodic Hann window of ``win_length or fft_length`` (unlike torch.stft).
    On a HIP device framing, padding (``center``/``pad_mode``), windowing and the R2C FFT run in one gfx950 kernel.
    """
    x = _tensor(waveforms, 'waveforms')
    n_fft, hop, win_length, window = resolve_stft_args(x, fft_length, hop_length, win_length, window)
    _hip.check_stft_args(x.shape, n_fft, hop, win_length, center, pad_mode)
    return _call('stft', x, window, n_fft, hop, win_length, bool(center), pad_mode, bool(normalized), bool(onesided))


def istft(complex_specgrams, fft_length, hop_length=None, win_length=None, window=None,
          center=True, normalized=False, onesided=True, length=None):
    """Inverse short-time Fourier transform of ``(*, channel, num_freqs, time, complex=2)`` spectrograms →
    ``(*, channel, samples)`` waveforms: ``torch.istft`` wrapped the way ``stft`` wraps ``torch.stft`` (leading dims
    flattened and restored; ``window=None`` means a periodic Hann window of ``win_length or fft_length``).

    ``samples`` is ``hop_length * (time - 1)`` with ``center`` (``+ fft_length`` without), or ``length`` when given (trimmed /
    zero-padded).  A window whose squared overlap-add vanishes inside the kept range raises ``RuntimeError`` as ``torch.istft``
    does (e.g. Hann with ``hop_length == fft_length``, or Hann with ``center=False``).
    On a HIP device, float32 one-sided input runs on the gfx950 kernels: one inverse real FFT per frame, then a gather
    overlap-add that divides by the window envelope.  The frame-major views ``stft`` and ``phase_vocoder`` return are read in place.
    """
    z = _tensor(complex_specgrams, 'complex_specgrams')
    if z.dim() < 3 or z.shape[-1] != 2:
        raise RuntimeError('istft: expected a tensor of shape (*, num_freqs, time, complex=2), got %s' % (tuple(z.shape),))
    if not z.is_floating_point():
        raise RuntimeError('istft: expected a floating point tensor, got %s' % z.dtype)
    if any(int(s) == 0 for s in z.shape):
        raise RuntimeError('istft: expected a non-empty tensor, got %s' % (tuple(z.shape),))
    n_fft, hop, win_length, window = resolve_stft_args(z, fft_length, hop_length, win_length, window)
    if n_fft <= 0 or hop <= 0 or hop > win_length:
        raise RuntimeError('istft: expected 0 < hop_length <= win_length <= n_fft, got n_fft=%d hop_length=%d win_length=%d'
                           % (n_fft, hop, win_length))
    n_bins = n_fft // 2 + 1 if onesided else n_fft
    if z.shape[-3] != n_bins:
        raise RuntimeError('istft: expected %d frequency bins for fft_length=%d, onesided=%s, got %d'
                           % (n_bins, n_fft, bool(onesided), z.shape[-3]))
    if length is not None:
        length = int(length)
        if length <= 0:
            raise RuntimeError('istft: expected length > 0, got %d' % length)
    return _call('istft', z, window, n_fft, hop, win_length, bool(center), bool(normalized), bool(onesided), length)


def griffinlim(specgram, window, n_fft, hop_length, win_length, power, n_iter, momentum, length, rand_init):
    """``(…, freq, time)`` real, non-negative magnitudes (``freq == n_fft // 2 + 1``) → ``(…, samples)``: torchaudio's
    ``functional.griffinlim``, phase recovery by the fast Griffin-Lim iteration.  With ``m = momentum / (1 + momentum)`` and ``S =
    specgram ** (1 / power)``: the angles start as ``1 + 0j``, or with ``rand_init`` as ``torch.rand`` complex pairs (uniform in the
    unit square, NOT normalised); ``n_iter`` times ``y = istft(S A)``, ``R = stft(y)`` (``center``, reflect padding), ``A = R - m
    Rprev``, ``A = A / (|A| + 1e-16)``; the result is ``istft(S A)``.  ``samples`` is ``hop_length * (time - 1)``, or ``length``.

    ``ValueError`` for a momentum outside ``[0, 1)``; ``TypeError`` for a non-tensor; ``RuntimeError``, before anything is
    launched, for a complex or integer ``specgram``, a wrong ``freq``, ``n_iter < 0``, ``power <= 0``, a ``length`` with ``1 +
    length // hop_length != time`` (torchaudio fails there one iteration in) and too few samples to reflect-pad; a window without
    overlap-add (NOLA) raises as ``istft`` does.

    The draw is torch's: made here with ``torch.rand`` on the tensor's device before the op, so a generator state gives what the
    composite of torch operators gives.  float32 on a HIP device: one prepare launch (csrc/griffinlim.hip: the root and the turn to
    frame-major rows, the input read where it lies), then ``istft`` and ``stft`` on the package's kernels with the projection
    between them in one elementwise launch: three launches a step at fft_length 2048 with hop 256 / 512 / 1024 (the fused
    inverse), four elsewhere.  float64, half precision, expanded strides, other fft_lengths than ``istft``'s and the backward pass take
    ``_composite.griffinlim`` (also the CPU path), announced with ``CompositeRouteWarning`` on a device."""
    if not 0 <= momentum < 1:
        raise ValueError('momentum must be in range [0, 1). Found: {}'.format(momentum))
    x = _tensor(specgram, 'specgram')
    if x.is_complex() or not x.is_floating_point():
        raise RuntimeError('griffinlim: expected a real floating point specgram, got %s' % x.dtype)
    n_fft, hop, win_length, n_iter = int(n_fft), int(hop_length), int(win_length), int(n_iter)
    if x.dim() < 2 or x.shape[-2] != n_fft // 2 + 1 or any(int(s) == 0 for s in x.shape):
        raise RuntimeError('griffinlim: expected a non-empty (*, %d, time) specgram for n_fft=%d, got %s'
                           % (n_fft // 2 + 1, n_fft, tuple(x.shape)))
    if n_iter < 0:
        raise RuntimeError('griffinlim: expected n_iter >= 0, got %d' % n_iter)
    if not power > 0:
        raise RuntimeError('griffinlim: expected power > 0, got %r' % (power,))
    if not torch.is_tensor(window) or window.dim() != 1 or window.shape[0] != win_length or window.device != x.device:
        raise RuntimeError('griffinlim: expected a 1D window tensor of size win_length=%d on %s' % (win_length, x.device))
    if n_fft <= 0 or hop <= 0 or hop > win_length or win_length > n_fft:
        raise RuntimeError('griffinlim: expected 0 < hop_length <= win_length <= n_fft, got n_fft=%d hop_length=%d win_length=%d'
                           % (n_fft, hop, win_length))
    n_frames = int(x.shape[-1])
    if length is not None:
        length = int(length)
        if length <= 0 or 1 + length // hop != n_frames:
            raise RuntimeError('griffinlim: length=%d gives %d frames of hop_length=%d where the specgram has %d'
                               % (length, 1 + length // hop if length > 0 else 0, hop, n_frames))
    samples = hop * (n_frames - 1) if length is None else length
    if samples <= 0:
        raise RuntimeError('griffinlim: %d frame(s) leave no samples' % n_frames)
    _hip.check_stft_args((samples,), n_fft, hop, win_length, True, 'reflect')
    angles0 = None
    if rand_init:
        angles0 = torch.rand(x.shape, dtype=torch.complex128 if x.dtype == torch.float64 else torch.complex64, device=x.device)
    return _call('griffinlim', x, window, angles0, n_fft, hop, win_length, float(power), n_iter,
                 float(momentum / (1 + momentum)), length)


def complex_norm(complex_tensor, power=1.0):
    """``|z|**power`` over a trailing ``complex=2`` dim (reference: functional.py:116-128)."""
    z = _tensor(complex_tensor, 'complex_tensor')
    _check_pairs(z, 'complex_norm')
    return _call('complex_norm', z, float(power))


def _hz_to_mel(hz, htk):
    hz = torch.as_tensor(hz).to(torch.get_default_dtype())
    if htk:
        return 2595. * torch.log10(torch.tensor(1., dtype=torch.get_default_dtype()) + hz / 700.)
    f_sp = 200.0 / 3
    knee_hz = 1000.0
    knee_mel = (knee_hz - 0.0) / f_sp
    step = math.log(6.4) / 27.0
    return torch.where(hz >= knee_hz, knee_mel + torch.log(hz / knee_hz) / step, (hz - 0.0) / f_sp)


def _mel_to_hz(mel, htk):
    mel = torch.as_tensor(mel).to(torch.get_default_dtype())
    if htk:
        return 700. * (10 ** (mel / 2595.) - 1.)
    f_sp = 200.0 / 3
    knee_hz = 1000.0
    knee_mel = (knee_hz - 0.0) / f_sp
    step = math.log(6.4) / 27.0
    return torch.where(mel >= knee_mel, knee_hz * torch.exp(step * (mel - knee_mel)), 0.0 + f_sp * mel)


# the reference's (private) names of the two conversions, functional.py:5-45: call sites that import them keep working
_hertz_to_mel = _hz_to_mel
_mel_to_hertz = _mel_to_hz


def create_mel_filter(num_freqs, num_mels, min_freq, max_freq, htk):
    """Dense ``(num_freqs, num_mels)`` triangular mel filterbank, Slaney (default) or HTK scale, no
    area normalisation, bin grid ``linspace(min_freq, max_freq, num_freqs)`` (reference:
    functional.py:131-169).  One-off init-time constant: evaluated with the same float32 host
    arithmetic as the reference so the matrix is bit-identical; move it with ``.cuda()``."""
    grid = torch.linspace(min_freq, max_freq, num_freqs)
    knots = _mel_to_hz(torch.linspace(_hz_to_mel(min_freq, htk), _hz_to_mel(max_freq, htk), num_mels + 2), htk)
    gap = knots[1:] - knots[:-1]
    delta = knots.unsqueeze(0) - grid.unsqueeze(1)
    lower = (-1. * delta[:, :-2]) / gap[:-1]
    upper = delta[:, 2:] / gap[1:]
    return torch.clamp(torch.min(lower, upper), min=0.)


def apply_filterbank(mag_specgrams, filterbank):
    """``(…, num_freqs, time) x (num_freqs, num_bands) → (…, num_bands, time)`` (reference:
    functional.py:172-184); on a HIP device a band-sparse streaming contraction for triangular banks, the fp32
    matrix cores for dense ones."""
    spec = _tensor(mag_specgrams, 'mag_specgrams')
    fb = _tensor(filterbank, 'filterbank')
    if fb.dim() != 2 or spec.dim() < 2 or spec.shape[-2] != fb.shape[0]:
        raise RuntimeError('apply_filterbank: size mismatch, spectrogram %s vs filterbank %s'
                           % (tuple(spec.shape), tuple(fb.shape)))
    if fb.device != spec.device:
        raise RuntimeError('apply_filterbank: spectrogram and filterbank must be on the same device')
    return _call('apply_filterbank', spec, fb)


def create_dct(num_coeffs, num_mels, norm='ortho'):
    """``(num_mels, num_coeffs)`` DCT-II matrix, float32: ``cos(pi / num_mels * (m + 0.5) * k)``, times 2 with ``norm=None``; with
    ``norm='ortho'`` column 0 times ``1/sqrt(2)`` and everything times ``sqrt(2 / num_mels)`` (torchaudio's ``create_dct``; what
    ``scipy.fft.dct(type=2, norm=norm)[..., :num_coeffs]`` multiplies by).  Evaluated in float64 and rounded once."""
    if norm is not None and norm != 'ortho':
        raise ValueError("create_dct: norm must be None or 'ortho', got %r" % (norm,))
    num_coeffs, num_mels = int(num_coeffs), int(num_mels)
    if not 1 <= num_coeffs <= num_mels:
        raise ValueError('create_dct: expected 1 <= num_coeffs <= num_mels, got num_coeffs=%d, num_mels=%d'
                         % (num_coeffs, num_mels))
    m = torch.arange(num_mels, dtype=torch.float64).unsqueeze(1)
    k = torch.arange(num_coeffs, dtype=torch.float64).unsqueeze(0)
    d = torch.cos(math.pi / num_mels * (m + 0.5) * k)
    if norm is None:
        d = d * 2.0
    else:
        d[:, 0] *= 1.0 / math.sqrt(2.0)
        d = d * math.sqrt(2.0 / num_mels)
    return d.to(torch.float32)


def dct(x, dct_matrix):
    """``(…, num_mels, time) x (num_mels, num_coeffs) → (…, num_coeffs, time)``: the matrix of ``create_dct`` (or any other)
    applied along dim −2 — behind ``Melspectrogram -> AmplitudeToDb`` these are the MFCCs.  On a HIP device one streaming
    kernel that keeps the matrix in the LDS (csrc/mfcc.hip), for matrices up to 256 x 256 with at most 32768 elements."""
    x = _tensor(x, 'x')
    mat = _tensor(dct_matrix, 'dct_matrix')
    if mat.dim() != 2 or x.dim() < 2 or x.shape[-2] != mat.shape[0]:
        raise RuntimeError('dct: size mismatch, input %s vs dct_matrix %s' % (tuple(x.shape), tuple(mat.shape)))
    if mat.device != x.device:
        raise RuntimeError('dct: input and dct_matrix must be on the same device')
    return _call('dct', x, mat)


def resample(waveforms, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method='sinc_interp_hann',
             beta=None):
    """``(…, L) → (…, ceil(new_freq * L / orig_freq))``: torchaudio's ``functional.resample`` — a polyphase windowed-sinc
    filter (Hann or Kaiser window, ``lowpass_filter_width`` zero crossings, cut-off at ``rolloff`` of the lower Nyquist rate);
    the definition is in ``_resample.py``.  Both rates are positive ints and are reduced by their gcd; equal rates return the
    input.  On a HIP device one streaming kernel that keeps the non-zero taps in the LDS (csrc/resample.hip); its gradient
    w.r.t. the waveform is the same kernel with the transposed bank."""
    x = _tensor(waveforms, 'waveforms')
    args = _resample.constants(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)
    if x.dim() < 1:
        raise RuntimeError('resample: expected a tensor of shape (…, time), got a scalar')
    if not x.is_floating_point():
        raise RuntimeError('resample: expected a floating-point waveform, got %s' % x.dtype)
    if args[0] == args[1]:
        return x
    return _call('resample', x, *args)


_phase_advances = Bounded(64)


def _phase_advance(n_fft, hop, like):
    """``linspace(0, pi * hop, n_fft // 2 + 1)[:, None]``: the expected phase advance per hop of every bin, cached like the windows"""
    if type(like) is not torch.Tensor or torch.compiler.is_compiling():
        return torch.linspace(0, math.pi * hop, n_fft // 2 + 1, dtype=like.dtype, device=like.device)[..., None]
    key = (n_fft, hop, str(like.device), like.dtype)
    pa = _phase_advances.get(key)
    if pa is None:
        with torch.inference_mode(False):
            pa = torch.linspace(0, math.pi * hop, n_fft // 2 + 1, dtype=like.dtype, device=like.device)[..., None]
        _phase_advances[key] = pa
    return pa


def pitch_shift(waveform, sample_rate, n_steps, bins_per_octave=12, n_fft=512, win_length=None, hop_length=None, window=None):
    """``(…, L) → (…, L)``: torchaudio's ``functional.pitch_shift`` — the pitch moved by ``n_steps`` of ``bins_per_octave`` to the
    octave at unchanged duration.  With ``rate = 2 ** (-n_steps / bins_per_octave)``: ``stft`` (centred, reflect padding, periodic
    Hann of ``win_length`` unless a window is given, ``hop_length = n_fft // 4``), ``phase_vocoder`` by ``rate``, ``istft`` to
    ``round(L / rate)`` samples, then ``resample`` from ``int(sample_rate / rate)`` to ``sample_rate`` cut or zero-padded to ``L``.
    Composed from the package's own ops, each with its gradient kernel; the last stage is ``tac_amd::resample_fit``: that pair
    almost never reduces (16 kHz, 4 steps: 10079 : 8000), so on a HIP device it runs on the wide polyphase kernel, which takes
    its taps from global memory and writes the ``L`` samples in the same launch (csrc/resample.hip)."""
    x = _tensor(waveform, 'waveform')
    rate, source = _augment.pitch_rates(sample_rate, n_steps, bins_per_octave)
    if x.dim() < 1:
        raise RuntimeError('pitch_shift: expected a tensor of shape (…, time), got a scalar')
    if not x.is_floating_point():
        raise RuntimeError('pitch_shift: expected a floating-point waveform, got %s' % x.dtype)
    n_fft = int(n_fft)
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    win_length = n_fft if win_length is None else int(win_length)
    length = x.shape[-1]
    rows = x.reshape(-1, length)
    spec = stft(rows, n_fft, hop, win_length, window, center=True, pad_mode='reflect', normalized=False, onesided=True)
    stretched = phase_vocoder(spec, rate, _phase_advance(n_fft, hop, spec))
    y = istft(stretched, n_fft, hop, win_length, window, length=int(round(length / rate)))
    args = _resample.constants(source, sample_rate)
    if args[0] != args[1]:                  # (equal rates, n_steps = 0: ``y`` has the L samples already)
        y = _call('resample_fit', y, *args, length)
    return y.reshape(x.shape)


def kaldi_fbank(waveforms, blackman_coeff=0.42, dither=0.0, energy_floor=1.0, frame_length=25.0, frame_shift=10.0, high_freq=0.0,
                htk_compat=False, low_freq=20.0, num_mel_bins=23, preemphasis_coefficient=0.97, raw_energy=True,
                remove_dc_offset=True, round_to_power_of_two=True, sample_frequency=16000.0, snip_edges=True, subtract_mean=False,
                use_energy=False, use_log_fbank=True, use_power=True, vtln_high=-500.0, vtln_low=100.0, vtln_warp=1.0,
                window_type='povey'):
    """``(…, time)`` → ``(…, frames, num_mel_bins [+ 1])``: Kaldi's log mel filterbank features with the keywords and defaults of
    ``torchaudio.compliance.kaldi.fbank`` (``kaldi.fbank`` is that function itself, for ``(channels, time)``), over any leading
    dimensions.  Frames of ``W = int(sample_frequency * frame_length / 1000)`` samples every ``S = int(sample_frequency *
    frame_shift / 1000)``; per frame the mean is removed, the frame pre-emphasised with its first sample replicated and
    windowed, zero-padded to the next power of two ``N``, and ``|rfft|^2`` (or ``|rfft|``) is weighted by a bank that is
    triangular in mel; the output is the natural logarithm floored at float32 epsilon, with the frame's log energy as the first
    column (the last with ``htk_compat``) when ``use_energy``.  The definition is in ``_kaldi.py``.  On a HIP device float32
    input is ONE launch from waveform rows to output rows (csrc/kaldi_fbank.hip) for ``N`` = 256 / 512 / 1024, up to 128 bins
    and ``dither == 0``; the rest, and the backward pass, take torch operators, announced.  ``vtln_warp != 1`` is not
    implemented."""
    x = _tensor(waveforms, 'waveforms')
    if x.dim() < 1:
        raise RuntimeError('kaldi_fbank: expected a tensor of shape (…, time), got a scalar')
    if not x.is_floating_point():
        raise RuntimeError('kaldi_fbank: expected a floating-point waveform, got %s' % x.dtype)
    if vtln_warp != 1.0:
        raise NotImplementedError('kaldi_fbank: vtln_warp != 1 (vocal tract length normalisation) is not implemented')
    p = _kaldi.Params(float(blackman_coeff), float(dither), float(energy_floor), float(frame_length), float(frame_shift),
                      float(high_freq), bool(htk_compat), float(low_freq), int(num_mel_bins), float(preemphasis_coefficient),
                      bool(raw_energy), bool(remove_dc_offset), bool(round_to_power_of_two), float(sample_frequency),
                      bool(snip_edges), bool(subtract_mean), bool(use_energy), bool(use_log_fbank), bool(use_power),
                      str(window_type))
    _kaldi.check(p)
    return _call('kaldi_fbank', x, *p)


#: the keywords ``kaldi_fbank`` takes behind the waveform
_KALDI_KEYWORDS = kaldi_fbank.__code__.co_varnames[1:kaldi_fbank.__code__.co_argcount]


def _kaldi_waveform(waveforms, name):
    x = _tensor(waveforms, 'waveforms')
    if x.dim() < 1:
        raise RuntimeError('%s: expected a tensor of shape (…, time), got a scalar' % name)
    if not x.is_floating_point():
        raise RuntimeError('%s: expected a floating-point waveform, got %s' % (name, x.dtype))
    return x


def kaldi_mfcc(waveforms, blackman_coeff=0.42, cepstral_lifter=22.0, dither=0.0, energy_floor=1.0, frame_length=25.0,
               frame_shift=10.0, high_freq=0.0, htk_compat=False, low_freq=20.0, num_ceps=13, num_mel_bins=23,
               preemphasis_coefficient=0.97, raw_energy=True, remove_dc_offset=True, round_to_power_of_two=True,
               sample_frequency=16000.0, snip_edges=True, subtract_mean=False, use_energy=False, vtln_high=-500.0, vtln_low=100.0,
               vtln_warp=1.0, window_type='povey'):
    """``(…, time)`` → ``(…, frames, num_ceps)``: Kaldi's mel-frequency cepstral coefficients with the keywords and defaults of
    ``torchaudio.compliance.kaldi.mfcc`` (``kaldi.mfcc`` is that function itself, for ``(channels, time)``), over any leading
    dimensions.  The log-mel rows are those of ``kaldi_fbank`` (natural logarithm of the power bank); a row times the
    orthonormal DCT-II gives ``C``, ``C[c] *= 1 + cepstral_lifter / 2 sin(pi c / cepstral_lifter)``, ``C[0]`` is the frame's log
    energy with ``use_energy``, and ``htk_compat`` moves column 0 to the end (times sqrt 2 unless it is the energy).  The
    definition is in ``_kaldi.py``.  On a HIP device float32 input is ONE launch from waveform rows to cepstra
    (csrc/kaldi_fbank.hip, the DCT as the epilogue of the ``kaldi_fbank`` launch) under ``kaldi_fbank``'s conditions and while
    the DCT table fits the launch's LDS beside the bank (about 5000 elements: 80 x 40 does, 80 x 80 does not); the rest, and
    the backward pass, take torch operators, announced.  ``num_ceps > num_mel_bins`` is a ``ValueError``; ``vtln_warp != 1``
    is not implemented."""
    x = _kaldi_waveform(waveforms, 'kaldi_mfcc')
    if vtln_warp != 1.0:
        raise NotImplementedError('kaldi_mfcc: vtln_warp != 1 (vocal tract length normalisation) is not implemented')
    p = _kaldi.MfccParams(float(blackman_coeff), float(cepstral_lifter), float(dither), float(energy_floor), float(frame_length),
                          float(frame_shift), float(high_freq), bool(htk_compat), float(low_freq), int(num_ceps),
                          int(num_mel_bins), float(preemphasis_coefficient), bool(raw_energy), bool(remove_dc_offset),
                          bool(round_to_power_of_two), float(sample_frequency), bool(snip_edges), bool(subtract_mean),
                          bool(use_energy), str(window_type))
    _kaldi.check(p, 'kaldi_mfcc')
    return _call('kaldi_mfcc', x, *p)


def kaldi_spectrogram(waveforms, blackman_coeff=0.42, dither=0.0, energy_floor=1.0, frame_length=25.0, frame_shift=10.0,
                      preemphasis_coefficient=0.97, raw_energy=True, remove_dc_offset=True, round_to_power_of_two=True,
                      sample_frequency=16000.0, snip_edges=True, subtract_mean=False, window_type='povey'):
    """``(…, time)`` → ``(…, frames, N / 2 + 1)``: Kaldi's log power spectrogram with the keywords and defaults of
    ``torchaudio.compliance.kaldi.spectrogram`` (``kaldi.spectrogram`` is that function itself, for ``(channels, time)``), over
    any leading dimensions.  Frames as in ``kaldi_fbank``; the output is ``log max(|rfft|^2, eps)`` of every bin, the Nyquist
    bin included, with the frame's log energy (floored at ``log energy_floor``) in place of the DC bin.  On a HIP device float32
    input is ONE launch (csrc/kaldi_fbank.hip, without the bank) under ``kaldi_fbank``'s conditions; the rest, and the backward
    pass, take torch operators, announced."""
    x = _kaldi_waveform(waveforms, 'kaldi_spectrogram')
    p = _kaldi.SpectrogramParams(float(blackman_coeff), float(dither), float(energy_floor), float(frame_length),
                                 float(frame_shift), float(preemphasis_coefficient), bool(raw_energy), bool(remove_dc_offset),
                                 bool(round_to_power_of_two), float(sample_frequency), bool(snip_edges), bool(subtract_mean),
                                 str(window_type))
    _kaldi.check(p, 'kaldi_spectrogram')
    return _call('kaldi_spectrogram', x, *p)


_KALDI_MFCC_KEYWORDS = kaldi_mfcc.__code__.co_varnames[1:kaldi_mfcc.__code__.co_argcount]
_KALDI_SPECTROGRAM_KEYWORDS = kaldi_spectrogram.__code__.co_varnames[1:kaldi_spectrogram.__code__.co_argcount]


def sliding_window_cmn(specgram, cmn_window=600, min_cmn_window=100, center=False, norm_vars=False):
    """``(…, T, F)`` → the same shape and dtype: torchaudio's ``functional.sliding_window_cmn`` (Kaldi's ``apply-cmvn-sliding``)
    over the layout ``kaldi_fbank`` returns, time second to last.  Frame ``t`` loses the mean of its window ``[ws, we)``: with
    ``center``, ``cmn_window`` frames around ``t`` held inside the row; otherwise the ``cmn_window`` frames before ``t`` and
    ``t`` itself (``cmn_window + 1`` frames away from the ends, as in Kaldi), grown to ``min_cmn_window`` frames at the start of
    the row.  ``norm_vars`` also divides by the window's standard deviation (0 where the window is one frame).  On a HIP device
    float32 input with positive strides — a feature or time slice as it lies — is ONE launch (csrc/cmn_deltas.hip): float64
    running sums per feature and time chunk, rounded to float32 once, where torchaudio's float32 running sums drift; its
    gradient is the same kernel's adjoint mode without ``norm_vars``.  float64, non-positive strides and the gradient with
    ``norm_vars`` take the vectorised float64 ``cumsum`` form in torch operators, announced; CPU tensors take it too.  Unlike
    torchaudio, whose running sums stay poisoned to the end of the row, a NaN or an infinity reaches exactly the frames whose
    window holds it (they are NaN) and nothing else."""
    x = _tensor(specgram, 'specgram')
    cmn_window, min_cmn_window = int(cmn_window), int(min_cmn_window)
    _composite.cmn_check(cmn_window, min_cmn_window)
    if x.dim() < 2:
        raise ValueError('sliding_window_cmn: expected a tensor of shape (…, time, features), got %d dimension(s)' % x.dim())
    if not x.is_floating_point():
        raise RuntimeError('sliding_window_cmn: expected a floating-point tensor, got %s' % x.dtype)
    return _call('sliding_window_cmn', x, cmn_window, min_cmn_window, bool(center), bool(norm_vars))


def compute_deltas(specgram, win_length=5, mode='replicate'):
    """``(…, F, T)`` → the same shape, contiguous: torchaudio's ``functional.compute_deltas``,
    ``out[…, t] = sum_{k=-n..n} k x[…, idx(t + k)] / denom`` with ``n = (win_length - 1) // 2``, ``denom = n (n + 1)(2n + 1) / 3``
    and ``idx`` the index map of ``torch.nn.functional.pad`` for ``mode``: ``'replicate'``, ``'constant'``, ``'reflect'`` (needs
    ``n < T``) or ``'circular'`` (``n <= T``).  On a HIP device float32 input with positive strides and ``win_length <= 66`` is
    ONE launch (csrc/cmn_deltas.hip) on the tensor where it lies — contiguous rows, or the transposed view ``feats.T`` of a
    ``(T, F)`` Kaldi matrix, which is turned through the LDS; the gradient is the same kernel's adjoint mode for
    ``'replicate'`` and ``'constant'``.  float64, non-positive strides, wider windows and the gradient of the other two modes
    take an index gather in torch operators, announced; CPU tensors take it too."""
    x = _tensor(specgram, 'specgram')
    if x.dim() < 1:
        raise ValueError('compute_deltas: expected a tensor of shape (…, features, time), got a scalar')
    if not x.is_floating_point():
        raise RuntimeError('compute_deltas: expected a floating-point tensor, got %s' % x.dtype)
    win_length = int(win_length)
    _composite.deltas_check(int(x.shape[-1]), win_length, mode)
    if x.dim() == 1:
        return _call('compute_deltas', x.unsqueeze(0), win_length, mode).squeeze(0)
    return _call('compute_deltas', x, win_length, mode)


def mask_along_axis_iid(specgrams, mask_param, mask_value, axis, p=1.0):
    """``(…, freq, time)`` with at least three dimensions → a new contiguous tensor of the same shape and dtype: torchaudio's
    ``functional.mask_along_axis_iid``.  Every leading index gets a span of its own on ``axis`` (``dim - 2``: frequency, ``dim - 1``:
    time): ``value = rand(lead) * mask_param``, ``min_value = rand(lead) * (n - value)``, and ``[int(min_value), int(min_value) +
    int(value))`` is set to ``mask_value`` (a number or a 0-dim tensor).  ``p < 1`` bounds ``mask_param`` by ``int(n * p)``; a
    ``mask_param`` below 1 returns the input itself.  The draws are torch's, on the input's device, and nothing waits for them: on a
    HIP device float32 input (float16 / bfloat16 widened) with positive strides is ONE launch (csrc/specaug.hip) that reads the
    spans on the device.  float64, integer dtypes and non-positive strides take sequential ``masked_fill``s in torch operators,
    announced; CPU tensors take them too."""
    x = _tensor(specgrams, 'specgrams')
    return _specaug.mask_along_axis_iid(x, int(mask_param), mask_value, axis, float(p))


def mask_along_axis(specgram, mask_param, mask_value, axis, p=1.0):
    """``(…, freq, time)`` with at least two dimensions → a new contiguous tensor of the same shape and dtype: torchaudio's
    ``functional.mask_along_axis``.  One span, drawn like ``mask_along_axis_iid``'s but with ``torch.rand(1)`` of the CPU generator,
    is shared by every leading index; ``ValueError`` if it comes out ``mask_param`` wide or wider.  The routes are those of
    ``mask_along_axis_iid``."""
    x = _tensor(specgram, 'specgram')
    return _specaug.mask_along_axis(x, int(mask_param), mask_value, axis, float(p))


def add_noise(waveform, noise, snr, lengths=None):
    """``waveform`` (…, L), ``noise`` (…, L), ``snr`` (…) in dB, ``lengths`` (…) or None → (…, L): torchaudio's ``functional.add_noise``.
    With ``m_t = t < lengths`` (every sample without ``lengths``; more than L: the whole row, 0 or less: none of it), ``E_s = sum_t
    (waveform_t m_t)^2`` and ``E_n`` likewise, ``out = waveform + sqrt(E_s / E_n) 10^(-snr / 20) noise`` at every sample, masked or not.
    The operands have the same number of leading dimensions and equal L (``ValueError`` otherwise), and the leading dimensions
    broadcast: one noise row may serve every channel, one ``snr`` every row.  On a HIP device float32 input (float16 / bfloat16
    widened) is one entry of three launches (csrc/add_noise.hip): float64 sums in a fixed order, ``scale`` rounded to float32 once,
    one fused multiply-add per output, ``snr`` and ``lengths`` read on the device; samples behind ``lengths`` are not read by the
    sums.  All three float32 gradients are the same kernels in adjoint mode.  float64, non-positive time strides and leading
    dimensions that two strides do not walk take torch operators, announced; CPU tensors take them too."""
    return _augment.add_noise(_tensor(waveform, 'waveform'), _tensor(noise, 'noise'), snr, lengths)


def speed(waveform, orig_freq, factor, lengths=None):
    """``(…, L)`` → ``((…, ceil(L * target / source)), out_lengths)``: torchaudio's ``functional.speed`` — the waveform played
    ``factor`` times faster, i.e. ``resample(waveform, source, target)`` with ``source = int(factor * orig_freq)`` and ``target =
    int(orig_freq)`` divided by their gcd (0.9 at 16 kHz: 9:10), on the ``resample`` kernel (one launch; equal rates return the
    input).  ``out_lengths`` is None without ``lengths``, else ``ceil(lengths * target / source)`` in the dtype of ``lengths``,
    computed where ``lengths`` lies.  ``ValueError`` for ``factor <= 0`` or ``int(factor * orig_freq) == 0``."""
    source, target = _augment.speed_rates(orig_freq, factor)
    return resample(waveform, source, target), _augment.speed_lengths(lengths, source, target)


_CONV_MODES = ('full', 'valid', 'same')


def _check_conv_mode(mode):
    if mode not in _CONV_MODES:
        raise ValueError('Unrecognized mode value %r. Please specify one of %s.' % (mode, list(_CONV_MODES)))


def _conv_crop(full, x_length, y_length, mode):
    """torchaudio's ``_apply_convolve_mode``: the centred crop of the full result, as a view"""
    if mode == 'full':
        return full
    target = max(x_length, y_length) - min(x_length, y_length) + 1 if mode == 'valid' else x_length
    return full.narrow(-1, (full.shape[-1] - target) // 2, target)


def fftconvolve(x, y, mode='full', n_fft=None):
    """``(*, L)``, ``(*, M)`` → ``(*, L + M - 1)`` (``'full'``), its centred crop to ``max(L, M) - min(L, M) + 1`` samples
    (``'valid'``) or to ``L`` samples (``'same'``): torchaudio's ``functional.fftconvolve`` — the convolution of ``x`` with ``y``
    along the last dimension, the leading dimensions broadcast against each other; a crop is a view of the full result.  On a HIP
    device: uniformly partitioned overlap-save on the STFT kernels with a frequency-domain delay line between them
    (csrc/fftconvolve.hip) — the error of every output block is relative to the signal around it, not to the loudest passage of
    the row — or, for one shared kernel of at most ``_hip.M_DIRECT`` taps, the polyphase kernel of ``resample`` at one phase.  The
    gradient w.r.t. ``x`` is the same route with the kernel reversed; the gradient w.r.t. ``y`` takes torch's FFT operators
    (announced).  ``n_fft`` (2048 / 4096 / 8192) forces the partitioned route at that transform length."""
    _check_conv_mode(mode)
    x, y = _tensor(x, 'x'), _tensor(y, 'y')
    if x.dim() < 1 or y.dim() < 1 or x.dim() != y.dim():
        raise ValueError('fftconvolve: x and y must have the same number of dimensions (>= 1), got %d and %d'
                         % (x.dim(), y.dim()))
    for i in range(x.dim() - 1):
        if x.shape[i] != y.shape[i] and x.shape[i] != 1 and y.shape[i] != 1:
            raise ValueError('fftconvolve: leading dimensions of x and y are not broadcastable (got %s and %s)'
                             % (tuple(x.shape), tuple(y.shape)))
    if not (x.is_floating_point() and y.is_floating_point()):
        raise RuntimeError('fftconvolve: expected floating-point tensors, got %s and %s' % (x.dtype, y.dtype))
    if n_fft is not None and n_fft not in _hip.FFTCONV_SIZES:
        raise ValueError('fftconvolve: n_fft must be one of %s, got %r' % (list(_hip.FFTCONV_SIZES), n_fft))
    full = _call('fftconvolve', x, y, int(n_fft or 0))
    return _conv_crop(full, x.shape[-1], y.shape[-1], mode)


def convolve(x, y, mode='full', n_fft=None):
    """torchaudio's ``functional.convolve``: the same function as ``fftconvolve`` here — one op, ``tac_amd::fftconvolve``, which
    picks the direct or the partitioned form by the kernel's length."""
    return fftconvolve(x, y, mode, n_fft)


def _waveform(waveforms, what):
    x = _tensor(waveforms, 'waveforms')
    if x.dim() < 1:
        raise RuntimeError('%s: expected a tensor of shape (…, time), got a scalar' % what)
    if not x.is_floating_point():
        raise RuntimeError('%s: expected a floating-point waveform, got %s' % (what, x.dtype))
    return x


def lfilter(waveforms, a_coeffs, b_coeffs, clamp=True):
    """``(…, L) → (…, L)``: torchaudio's ``functional.lfilter`` — the difference equation

        a0 y[n] = sum_k b_k x[n-k] - sum_{k>=1} a_k y[n-k]

    along the last axis with zero initial state; ``clamp`` limits the result to [-1, 1].  ``a_coeffs`` and ``b_coeffs`` are 1-D
    tensors of equal length with ``a_coeffs[0] != 0`` (``ValueError`` otherwise).  2-D coefficient banks (torchaudio's one filter
    per channel) are out of scope and raise ``ValueError`` too.

    float32 on a HIP device with at most three coefficients per side runs ONE launch of the gfx950 kernel (csrc/lfilter.hip):
    float32 loads and stores around a float64 recursion, so the result is the float64 filter rounded once.  The coefficients reach
    it as doubles (float32 tensors convert exactly; a device tensor is read back once and cached).  Its gradient w.r.t. the
    waveform is the same kernel run from the end of each row.  Higher orders, float64, non-positive strides and the gradient
    w.r.t. the coefficients take the time loop of ``_composite.lfilter`` (also the CPU path): correct and slow, announced with
    ``CompositeRouteWarning`` on a device.  The kernel route above order 2 is the cascade: ``sosfilt(x, tf2sos(b, a))``."""
    x = _waveform(waveforms, 'lfilter')
    _filters.check_coeffs(a_coeffs, b_coeffs)
    if not torch.compiler.is_compiling() and _hip.host_coeffs(a_coeffs)[0] == 0.0:
        raise ValueError('lfilter: a_coeffs[0] must not be zero')
    return _call('lfilter', x, a_coeffs, b_coeffs, bool(clamp))


def sosfilt(waveforms, sos, clamp=False):
    """``(…, L) → (…, L)``: a cascade of second-order sections along the last axis, what ``scipy.signal.sosfilt`` computes with zero
    initial state.  ``sos`` is a floating-point ``(S, 6)`` tensor with rows ``(b0, b1, b2, a0, a1, a2)`` in scipy's layout, every
    ``a0`` finite and not zero, ``S >= 1`` (``ValueError`` otherwise); it may be float64 and may live on the host.  Section
    ``s + 1`` filters the output of section ``s``; ``clamp`` limits the final result to [-1, 1].  This is the way to filters above
    order 2 — ``sosfilt(x, tf2sos(b, a))``, or a design made as sections (``scipy.signal.butter(..., output='sos')``).

    float32 on a HIP device with at most eight sections runs ONE launch of the gfx950 kernel (csrc/sosfilt.hip): the waveform is
    read once and written once as float32 and everything between the sections is float64 on chip, so the result is the float64
    cascade rounded once.  Its gradient w.r.t. the waveform is the same kernel with the sections reversed and each row walked
    from its end.  More sections, float64, non-positive strides, a section so unstable that the kernel's scan overflows, the
    gradient w.r.t. ``sos`` and double backward take ``_composite.sosfilt`` (also the CPU path): ``_composite.lfilter`` section by
    section in float64, announced with ``CompositeRouteWarning`` on a device."""
    x = _waveform(waveforms, 'sosfilt')
    _filters.check_sos(sos)
    if not torch.compiler.is_compiling():
        _filters.check_sos_values(_hip.host_sos(sos))
    return _call('sosfilt', x, sos, bool(clamp))


def _host_floats(c, name):
    if torch.is_tensor(c):
        if c.dim() != 1 or not c.is_floating_point():
            raise ValueError('tf2sos: %s must be a 1-D floating-point tensor, got %s of shape %s' % (name, c.dtype, tuple(c.shape)))
        return _hip.host_coeffs(c)
    return tuple(float(v) for v in c)


def tf2sos(b_coeffs, a_coeffs):
    """The transfer function ``b_coeffs / a_coeffs`` (1-D tensors or sequences of equal length, ``a_coeffs[0] != 0``; note the
    order, scipy's) as second-order sections for ``sosfilt``: a float64 HOST tensor of shape ``(ceil(order / 2), 6)``, computed on
    the host in float64 by scipy's ``tf2sos`` algorithm (``_filters.tf2sos``) and cached by value."""
    return _filters.tf2sos(_host_floats(b_coeffs, 'b_coeffs'), _host_floats(a_coeffs, 'a_coeffs'))


#: coefficients per side up to which ``filtfilt`` runs as two cascades of ``tf2sos``' sections (order 16: eight sections)
_FILTFILT_MAX_COEFFS = 2 * _hip.SOSFILT_MAX_SECTIONS + 1


def filtfilt(waveforms, a_coeffs, b_coeffs, clamp=True):
    """``(…, L) → (…, L)``: torchaudio's ``functional.filtfilt``, signature and semantics — ``lfilter`` forward without clamp, then
    the same filter over the time-reversed result with ``clamp``, reversed back.  The intermediate is in the input's dtype and
    there is NO edge padding: this is not scipy's ``filtfilt``.  ``a_coeffs`` / ``b_coeffs`` as for ``lfilter``.

    Up to three coefficients per side: two launches of the ``lfilter`` kernel, the second in its ``reverse`` mode (nothing is
    flipped in memory).  4 to 17 per side: ``tf2sos`` on the host values, then two launches of the ``sosfilt`` kernel, the second
    with the sections reversed and each row walked from its end.  Longer filters, coefficients that need a gradient, and
    everything ``lfilter`` itself hands to torch operators take ``_composite.lfilter`` twice, announced on a device.  The gradient
    w.r.t. the waveform follows from the two halves."""
    x = _waveform(waveforms, 'filtfilt')
    _filters.check_coeffs(a_coeffs, b_coeffs)
    n = a_coeffs.numel()
    sections = False
    if not torch.compiler.is_compiling():
        ha = _hip.host_coeffs(a_coeffs)
        if ha[0] == 0.0:
            raise ValueError('filtfilt: a_coeffs[0] must not be zero')
        sections = _hip.LFILTER_MAX_COEFFS < n <= _FILTFILT_MAX_COEFFS and not (
            torch.is_grad_enabled() and (a_coeffs.requires_grad or b_coeffs.requires_grad))
    if sections:
        sos = _filters.tf2sos(_hip.host_coeffs(b_coeffs), ha)
        return _call('sosfilt_reverse', _call('sosfilt', x, sos, False), sos, bool(clamp))
    return _call('lfilter_reverse', _call('lfilter', x, a_coeffs, b_coeffs, False), a_coeffs, b_coeffs, bool(clamp))


def overdrive(waveform, gain=20, colour=20):
    """``(…, time) → (…, time)``: torchaudio's ``functional.overdrive`` (SoX's effect).  With ``g = 10^(gain / 20)`` and
    ``c = colour / 200``: ``t = g x + c`` shaped to ``-2/3`` below -1, ``2/3`` above 1 and ``t - t^3 / 3`` between; ``v[n] = t[n] -
    t[n-1] + 0.995 v[n-1]`` from zero state; the result is ``clamp(0.5 x + 0.75 v, -1, 1)``.

    float32 on a HIP device with ``gain`` and ``colour`` in SoX's ranges (0 to 100) runs ONE launch of the gfx950 kernel
    (csrc/sox_effects.hip): float32 is read and written once around a float64 recursion on lfilter's tile walk.  Its gradient
    w.r.t. the waveform is lfilter's kernel run from the end of each row between elementwise torch operators.  Other dtypes,
    expanded views, parameters outside the ranges and CPU tensors take ``_composite.overdrive`` (elementwise operators around
    ``lfilter``), announced with ``CompositeRouteWarning`` on a device."""
    x = _waveform(waveform, 'overdrive')
    return _call('overdrive', x, float(gain), float(colour))


def phaser(waveform, sample_rate, gain_in=0.4, gain_out=0.74, delay_ms=3.0, decay=0.4, mod_speed=0.5, sinusoidal=True):
    """``(…, time) → (…, time)``: torchaudio's ``functional.phaser`` (SoX's effect).  With ``L = int(delay_ms sample_rate / 1000 +
    0.5)`` delay samples and an LFO of ``P = int(sample_rate / mod_speed + 0.5)`` integer values ``m`` in ``[1, L]`` (sine or
    triangle): ``y[n] = gain_in x[n] + decay y[n - (L - m[n mod P] + 1)]`` from zero state, and the result is
    ``clamp(gain_out y, -1, 1)``.  ``L < 1``, ``P < 1`` and ``sample_rate <= 0`` are a ``ValueError``.

    float32 on a HIP device with the parameters in SoX's ranges (``gain_in`` 0 to 1, ``delay_ms`` 0 to 5, ``decay`` 0 to 0.99,
    ``mod_speed`` 0.1 to 2) and ``L <= 1024`` runs ONE launch of the gfx950 kernel (csrc/sox_effects.hip): every sample has one
    parent, and pointer jumping in float64 over tiles held in the LDS solves the recursion in parallel.  Everything else — and the
    gradient — takes the time loop of ``_composite.phaser``, announced with ``CompositeRouteWarning`` on a device."""
    x = _waveform(waveform, 'phaser')
    return _call('phaser', x, float(sample_rate), float(gain_in), float(gain_out), float(delay_ms), float(decay), float(mod_speed),
                 bool(sinusoidal))


def flanger(waveform, sample_rate, delay=0.0, depth=2.0, regen=0.0, width=71.0, speed=0.5, phase=25.0, modulation='sinusoidal',
            interpolation='linear'):
    """``(…, channel, time) → (…, channel, time)``: torchaudio's ``functional.flanger`` (SoX's effect), at most 4 channels.  A
    delay line read at the LFO's position ``D`` (``delay`` to ``delay + depth`` ms, ``speed`` Hz, channel ``c`` shifted by
    ``c * phase`` percent of a period) with ``linear`` or ``quadratic`` interpolation; ``regen`` percent of the delayed signal is
    fed back into the line and ``width`` percent of it is mixed into the result, which is clipped to [-1, 1].  More than 4
    channels and unknown ``modulation`` / ``interpolation`` names are a ``ValueError``.

    float32 on a HIP device with the parameters in SoX's ranges (``delay`` 0 to 30, ``depth`` 0 to 10, ``regen`` -95 to 95,
    ``width`` 0 to 100, ``speed`` 0.1 to 10, ``phase`` 0 to 100) and a delay line of at most 4096 samples runs ONE launch of the
    gfx950 kernel (csrc/sox_effects.hip).  ``regen == 0`` is a streaming time-varying FIR.  Otherwise a wave walks each (entry,
    channel) row and advances ``min(64, 1 + delay in samples)`` samples per step — with ``delay = 0`` that is ONE sample per
    step, latency-bound by construction.  Everything else — and the gradient — takes the time loop of ``_composite.flanger``,
    announced with ``CompositeRouteWarning`` on a device."""
    x = _waveform(waveform, 'flanger')
    return _call('flanger', x, float(sample_rate), float(delay), float(depth), float(regen), float(width), float(speed), float(phase),
                 modulation, interpolation)


def biquad(waveforms, b0, b1, b2, a0, a1, a2):
    """torchaudio's ``functional.biquad``: ``lfilter`` with ``b = (b0, b1, b2)``, ``a = (a0, a1, a2)`` (Python numbers, kept in
    float64), clamped to [-1, 1] as ``lfilter`` is by default."""
    if float(a0) == 0.0:
        raise ValueError('biquad: a0 must not be zero')
    return lfilter(waveforms, _filters.host_tensor((a0, a1, a2)), _filters.host_tensor((b0, b1, b2)), True)


def _design(waveforms, coeffs):
    b, a = coeffs
    return biquad(waveforms, b[0], b[1], b[2], a[0], a[1], a[2])


def lowpass_biquad(waveforms, sample_rate, cutoff_freq, Q=0.707):
    """Second-order low-pass (RBJ audio-EQ cookbook), computed in float64 on the host.  With ``w0 = 2 pi cutoff_freq /
    sample_rate`` and ``alpha = sin(w0) / (2 Q)``: ``b = ((1 - cos w0) / 2, 1 - cos w0, (1 - cos w0) / 2)``,
    ``a = (1 + alpha, -2 cos w0, 1 - alpha)``."""
    return _design(waveforms, _filters.lowpass(sample_rate, cutoff_freq, Q))


def highpass_biquad(waveforms, sample_rate, cutoff_freq, Q=0.707):
    """Second-order high-pass: ``b = ((1 + cos w0) / 2, -(1 + cos w0), (1 + cos w0) / 2)``, ``a = (1 + alpha, -2 cos w0,
    1 - alpha)``; ``w0``, ``alpha`` as for ``lowpass_biquad``."""
    return _design(waveforms, _filters.highpass(sample_rate, cutoff_freq, Q))


def bandpass_biquad(waveforms, sample_rate, central_freq, Q=0.707, const_skirt_gain=False):
    """Second-order band-pass: ``b = (t, 0, -t)`` with ``t = alpha`` (0 dB peak gain) or, ``const_skirt_gain``,
    ``t = sin(w0) / 2`` (peak gain Q); ``a = (1 + alpha, -2 cos w0, 1 - alpha)``."""
    return _design(waveforms, _filters.bandpass(sample_rate, central_freq, Q, const_skirt_gain))


def bandreject_biquad(waveforms, sample_rate, central_freq, Q=0.707):
    """Second-order band-reject (notch): ``b = (1, -2 cos w0, 1)``, ``a = (1 + alpha, -2 cos w0, 1 - alpha)``."""
    return _design(waveforms, _filters.bandreject(sample_rate, central_freq, Q))


def allpass_biquad(waveforms, sample_rate, central_freq, Q=0.707):
    """Second-order all-pass: ``b = (1 - alpha, -2 cos w0, 1 + alpha)``, ``a = (1 + alpha, -2 cos w0, 1 - alpha)``."""
    return _design(waveforms, _filters.allpass(sample_rate, central_freq, Q))


def equalizer_biquad(waveforms, sample_rate, center_freq, gain, Q=0.707):
    """Peaking equalizer of ``gain`` dB at ``center_freq``: with ``A = 10^(gain / 40)``, ``b = (1 + alpha A, -2 cos w0,
    1 - alpha A)``, ``a = (1 + alpha / A, -2 cos w0, 1 - alpha / A)``."""
    return _design(waveforms, _filters.equalizer(sample_rate, center_freq, gain, Q))


def treble_biquad(waveforms, sample_rate, gain, central_freq=3000, Q=0.707):
    """High shelf (torchaudio's ``functional.treble_biquad``): ``gain`` dB above ``central_freq``.  With ``A = exp(gain / 40 ln 10)``,
    ``t1 = 2 sqrt(A) alpha``, ``t2 = (A - 1) cos w0`` and ``t3 = (A + 1) cos w0``: ``b = (A ((A + 1) + t2 + t1), -2 A ((A - 1) + t3),
    A ((A + 1) + t2 - t1))``, ``a = ((A + 1) - t2 + t1, 2 ((A - 1) - t3), (A + 1) - t2 - t1)``.  One ``lfilter`` launch."""
    return _design(waveforms, _filters.treble(sample_rate, gain, central_freq, Q))


def bass_biquad(waveforms, sample_rate, gain, central_freq=100, Q=0.707):
    """Low shelf (torchaudio's ``functional.bass_biquad``): ``gain`` dB below ``central_freq``; ``b = (A ((A + 1) - t2 + t1),
    2 A ((A - 1) - t3), A ((A + 1) - t2 - t1))``, ``a = ((A + 1) + t2 + t1, -2 ((A - 1) + t3), (A + 1) + t2 - t1)`` with the terms of
    ``treble_biquad``.  One ``lfilter`` launch."""
    return _design(waveforms, _filters.bass(sample_rate, gain, central_freq, Q))


def loudness(waveform, sample_rate):
    """``(…, channels, time)`` → ``(…)``: torchaudio's ``functional.loudness``, the gated loudness of ITU-R BS.1770-4 in LKFS.  The
    waveform passes the K-weighting (``treble_biquad(4 dB, 1500 Hz, Q = 1 / sqrt 2)``, then ``highpass_biquad(38 Hz, Q = 0.5)``, each
    clipped to [-1, 1]); the mean square of blocks of ``gate = round(0.4 sample_rate)`` samples every ``step = round(gate / 4)`` is
    summed over the channels with the weights (1, 1, 1, 1.41, 1.41) into ``l_k = -0.691 + 10 log10(.)``; blocks at or below -70 and
    blocks at or below the level of the remaining blocks' mean minus 10 are dropped, and the level of the mean of what is left is
    returned — NaN when nothing is left (silence).  ``ValueError`` for fewer than two dimensions, more than five channels, a
    non-floating dtype, a ``sample_rate`` that is not a positive int and a waveform shorter than one block.

    float32 on a HIP device (float16 / bfloat16 widened) is one entry of two launches (csrc/loudness.hip): the waveform is read
    once, both recursions, the clips, the squares and every sum are float64 and stay on chip, the gates run in a wave per entry,
    and the result is the float64 value rounded once.  float64, non-positive strides, a rate whose block is not four hops (11025 Hz:
    4410 and 1102) or whose hop is below 16 samples, and the backward pass take ``_composite.loudness`` (also the CPU path),
    announced with ``CompositeRouteWarning`` on a device."""
    x = _tensor(waveform, 'waveform')
    _filters.loudness_check(x, sample_rate)
    return _call('loudness', x, sample_rate)


def detect_pitch_frequency(waveform, sample_rate, frame_time=1e-2, win_length=30, freq_low=85, freq_high=3400):
    """``(…, time)`` → float32 ``(…, n_out)``: torchaudio's ``functional.detect_pitch_frequency``, the pitch in Hz from the normalised
    cross-correlation function and a median over time.  With ``L = ceil(sample_rate / freq_low)`` lags, frames of ``F =
    ceil(sample_rate frame_time)`` samples, ``N = ceil(time / F)`` of them and the row continued by ``L + N F - time`` zeros:
    ``nccf[t, l] = (s1 . s2) / (1e-9 + |s1|)^2 / (1e-9 + |s2|)^2`` for ``s1 = x[tF : tF + F]``, ``s2 = x[tF + l : tF + l + F]``, ``l
    = 1 … L`` (both energies, not their roots: the reference's form).  In columns ``c = l - 1`` the frame's lag is the first arg-max
    over ``[lag_min, L // 2)`` if its value exceeds 0.99 of the maximum over ``[lag_min, L)``, and the first arg-max of that range
    otherwise, ``lag_min = ceil(sample_rate / freq_high)``; an all-zero frame gets ``lag_min + 1``.  The lags get ``(win_length - 1)
    // 2`` copies of the first in front, ``out`` is ``float32(sample_rate) / float32(lower median of win_length lags)`` and ``n_out
    = N + (win_length - 1) // 2 - win_length + 1`` (``N - 15`` at the default).  The result is float32 for every input dtype and
    carries no gradient.

    ``ValueError``, before anything touches a device, for an empty search range (``lag_min >= L // 2``: ``freq_high=170`` at 16
    kHz), fewer frames than a window takes, ``win_length < 1``, a non-positive ``sample_rate``, ``frame_time``, ``freq_low`` or
    ``freq_high``, and a tensor without a time axis.

    float32 on a HIP device (float16 / bfloat16 widened) is one entry of two launches (csrc/pitch.hip): the correlations are float32
    sums in a fixed order formed in the LDS, the ``(frames, lags)`` matrix is never stored, and the median and the division are the
    second launch.  A frame whose ``F + L`` samples hold a NaN or Inf gets some lag in ``[lag_min + 1, L]`` — which one is not
    pinned, on any route — and every frame whose samples hold none is unaffected.  float64, non-positive or expanded strides,
    ``F`` / ``L`` beyond the launch's LDS plan and ``win_length`` above 64 take ``_composite.detect_pitch_frequency`` (also the CPU
    path), announced with ``CompositeRouteWarning`` on a device."""
    x = _tensor(waveform, 'waveform')
    _pitch.check(x, sample_rate, frame_time, win_length, freq_low, freq_high)
    # (detached: the op is registered without autograd and its result is piecewise constant)
    return _call('detect_pitch_frequency', x.detach(), sample_rate, float(frame_time), win_length, float(freq_low), float(freq_high))


def vad_start(waveform, sample_rate, trigger_level=7.0, trigger_time=0.25, search_time=1.0, allowed_gap=0.25, pre_trigger_time=0.0,
              boot_time=0.35, noise_up_time=0.1, noise_down_time=0.01, noise_reduction_amount=1.35, measure_freq=20.0,
              measure_duration=None, measure_smooth_time=0.4, hp_filter_freq=50.0, lp_filter_freq=6000.0, hp_lifter_freq=150.0,
              lp_lifter_freq=2000.0, joint='all'):
    """``(…, time)`` → ``(start int64, triggered bool)`` on the waveform's device: the sample at which ``vad`` would cut, and
    whether the detector triggered at all, with no host read.  The batched form torchaudio lacks: ``joint='all'`` takes every
    leading dimension as a channel of ONE group (torchaudio's grouping; 0-d results), ``'channel'`` takes axis -2 as the channels
    (results of shape ``waveform.shape[:-2]``), ``'none'`` every row on its own (``waveform.shape[:-1]``).  A group that never
    triggers gets ``start = max(0, time - keep)`` and ``triggered = False``.  The definition is ``vad``'s."""
    x = _tensor(waveform, 'waveform')
    args = _vad.resolve((trigger_level, trigger_time, search_time, allowed_gap, pre_trigger_time, boot_time, noise_up_time,
                         noise_down_time, noise_reduction_amount, measure_freq, measure_duration, measure_smooth_time, hp_filter_freq,
                         lp_filter_freq, hp_lifter_freq, lp_lifter_freq))
    _vad.check(x, sample_rate, *args)
    _vad.groups(x.shape, joint)
    # (detached: the op is registered without autograd and its result is an index)
    return _call('vad_start', x.detach(), sample_rate, *args, joint)


def vad(waveform, sample_rate, trigger_level=7.0, trigger_time=0.25, search_time=1.0, allowed_gap=0.25, pre_trigger_time=0.0,
        boot_time=0.35, noise_up_time=0.1, noise_down_time=0.01, noise_reduction_amount=1.35, measure_freq=20.0, measure_duration=None,
        measure_smooth_time=0.4, hp_filter_freq=50.0, lp_filter_freq=6000.0, hp_lifter_freq=150.0, lp_lifter_freq=2000.0):
    """``(…, time)`` → ``(…, time - start)``: torchaudio's ``functional.vad``, the SoX voice-activity detector that trims everything
    before the first speech.  As in torchaudio every leading dimension is a channel of one decision (more than two dimensions get
    its warning), and the result is the slice ``waveform[..., start:]`` — a view.

    With ``mlen = int(sample_rate (measure_duration or 2 / measure_freq) + 0.5)``, ``period = int(sample_rate / measure_freq + 0.5)``
    and ``dft`` the power of two >= max(16, mlen), frame ``t`` of a row is ``x[t period : t period + mlen]``, ``T = 1 + (time - mlen)
    // period`` of them.  Per row and spectrum bin in ``[s0, s1)`` the modulus ``|X_t|`` of the frame times ``2 / sqrt(mlen)
    hann(mlen)`` is smoothed (``S = S m + |X_t| (1 - m)``, ``m = boot / (1 + boot)`` while booting, then ``exp(-1 / (measure_smooth_time
    measure_freq))``), its power ``d = S^2`` tracked by the noise estimate ``N`` (up with ``noise_up_time``, down with
    ``noise_down_time``, equal to ``d`` while booting), ``e = sqrt(max(0, d - noise_reduction_amount N))`` windowed and transformed
    (``dft / 2`` points), and the power of its cepstrum bins ``[c0, c1)`` gives ``meas[t] = max(0, 21 + log(r / (c1 - c0)))`` (0 for
    ``r`` not above 0, a NaN included).  A row's decayed mean of the measures reaching ``trigger_level`` triggers its group at
    frame ``k``; every channel from the lowest triggering one searches back over ``n = ceil(search_time measure_freq)`` measures
    for where the speech began, ``flush`` is the furthest any of them gets, and ``start = (k - flush) period - pre``
    (``_vad.plan`` holds every integer; DESIGN §3.28 the full statement).  A group that never triggers keeps its last ``keep =
    pre + n period + mlen`` samples.

    ONE deviation from torchaudio: a negative ``start`` (``pre_trigger_time`` or the search reaching before sample 0, or a short
    input that never triggers) is clamped at 0 — the whole waveform is kept — where Python's slice would wrap around and keep
    the tail.

    ``ValueError``, before anything touches a device, for an empty spectrum or cepstrum range (``s1 <= s0``, ``c1 <= c0``), a
    non-positive ``sample_rate``, ``measure_freq`` or time constant, a non-floating tensor and a tensor without a time axis.

    float32 on a HIP device (float16 / bfloat16 widened) is three launches on the stream behind one padded copy of the rows:
    ``tac_spectrogram_f32`` for the ``|X_t|``, and the measuring and the deciding launch of csrc/vad.hip (one entry,
    ``tac_vad_start_f32``).  The length of the result depends on the data, so ``start`` is read on the host ONCE, after the third
    launch: that is the op's only synchronisation (``vad_start`` has none).  float64, expanded or non-positive strides, a ``dft``
    the spectrogram kernels do not take, bins beyond the measuring launch's plan and searches beyond 1024 measures take
    ``_composite.vad_measures`` / ``_composite.vad_start`` (also the CPU path), announced with ``CompositeRouteWarning`` on a device."""
    x = _tensor(waveform, 'waveform')
    if x.dim() > 2:
        warnings.warn('Expected input tensor dimension of 1 for single channel or 2 for multi-channel. Got %d instead. Batch '
                      'semantics is not supported. Please refer to https://github.com/pytorch/audio/issues/1348 and '
                      'https://github.com/pytorch/audio/issues/1468.' % x.dim())
    start, _ = vad_start(x, sample_rate, trigger_level, trigger_time, search_time, allowed_gap, pre_trigger_time, boot_time,
                         noise_up_time, noise_down_time, noise_reduction_amount, measure_freq, measure_duration, measure_smooth_time,
                         hp_filter_freq, lp_filter_freq, hp_lifter_freq, lp_lifter_freq, 'all')
    return x[..., int(start):]          # (the one host read)


def _simulate_rir(what, room, source, mic_array, max_order, absorption, output_length, delay_filter_length, center_frequency,
                  sound_speed, sample_rate, batch):
    room, source, mic_array = _tensor(room, 'room'), _tensor(source, 'source'), _tensor(mic_array, 'mic_array')
    D = _rir.check(room, source, mic_array, max_order, delay_filter_length, output_length, sound_speed, sample_rate, batch)
    a = _rir.absorption_of(absorption, room, D, batch)
    centres = _rir.centres_of(center_frequency, a.shape[1])
    if not batch:
        room, source, mic_array = room[None], source[None], mic_array[None]
    P, L = delay_filter_length // 2, delay_filter_length
    geometry = (max_order, L, float(sound_speed), float(sample_rate))
    if output_length is None:
        if 0 in mic_array.shape[:2]:
            output_length = L - P
        else:
            output_length = int(_call('rir_ism_span', room.detach(), source.detach(), mic_array.detach(), *geometry))    # (the one host read)
    if centres is None:
        out = _call('rir_ism', room, source, mic_array, a, max_order, P, output_length, L, float(sound_speed), float(sample_rate))[:, 0]
    else:
        raw = _call('rir_ism', room, source, mic_array, a, max_order, 0, P + output_length + _rir.FILTER_TAPS // 2, L, float(sound_speed),
                    float(sample_rate))
        filters = _rir.band_filters(centres, sample_rate, raw.device, raw.dtype)[:, None, :]                # (n_band, 1, 511)
        if batch:
            out = torch.sum(fftconvolve(raw, filters[None], mode='same'), dim=1)[..., P:P + output_length]
        else:
            out = torch.sum(fftconvolve(raw[0], filters, mode='same'), dim=0)[None, ..., P:P + output_length]
    return out if batch else out[0]


def simulate_rir_ism(room, source, mic_array, max_order, absorption, output_length=None, delay_filter_length=81, center_frequency=None,
                     sound_speed=343.0, sample_rate=16000.0):
    """``room (D,)``, ``source (D,)``, ``mic_array (M, D)``, ``D`` 2 or 3 → ``(M, output_length)``: torchaudio's
    ``prototype.functional.simulate_rir_ism``, the room impulse responses of a shoebox room by the image-source method.
    ``absorption`` is a float, ``(2 D,)`` or ``(n_band, 2 D)``, the walls as ``[x_lo, x_hi, y_lo, y_hi, z_lo, z_hi]``; more than one band
    needs ``center_frequency`` of as many entries.

    With ``P = delay_filter_length // 2`` and ``L = 2 P + 1``: every integer vector ``X`` with ``sum |X_d| <= max_order`` (in
    ``torch.cartesian_prod``'s order) is an image at ``room (X + 1) - source`` per axis where ``X`` is odd, else ``room X + source``, attenuated per
    band by ``prod_d tr_lo^|floor(X_d / 2)| tr_hi^|floor((X_d + 1) / 2)|``, ``tr = sqrt(1 - absorption)``.  For a microphone at ``dist`` it has
    ``amp = att / dist``, ``delay = dist sample_rate / sound_speed``, ``delay_i = ceil(delay)``, ``f = delay_i - delay``, and adds ``amp w(m + f)``,
    ``m = -P … P``, to sample ``delay_i + m + P`` of the raw response, ``w(x) = sinc(x) (1 + cos(2 pi x / 2P)) / 2`` for ``|x| <= P`` and 0 beyond.
    One band: the result is ``raw[P : P + output_length]`` (``None``: ``max(delay_i) + L - P`` samples, which costs the call's one host
    read; with ``output_length`` given nothing waits for the host).  Several bands: the per-band raw responses go through the band
    filters of ``_rir.band_filters`` with this package's ``fftconvolve(mode='same')``, are summed with ``torch.sum`` and cut the same way.

    TWO deviations from torchaudio: the raw responses are zero-extended, so the band filters' tails run on past the natural
    length where torchaudio cuts them; and a microphone exactly on an image gives that (room, channel) the infinities and NaNs
    of the formulas, and no other row any.

    ``ValueError`` for a room that is not 1-D with 2 or 3 entries, a source of another shape, a ``mic_array`` that is not ``(M, D)``, an even
    ``delay_filter_length``, and several bands without a ``center_frequency`` of matching length.

    float32 on a HIP device: ONE launch of csrc/rir.hip for the whole raw response (``tac_amd::rir_ism``): geometry in float64 on
    chip, float32 taps without cancellation, image-order sums in the LDS, no atomics, the same bits every run.  float64, expanded or
    non-positively strided inputs, more than 8 bands, filters beyond 255 taps, orders beyond 32 and the backward pass take
    ``_composite.rir_ism`` (float64 torch operators rounded once; also the CPU path), announced with ``CompositeRouteWarning`` on a
    device."""
    return _simulate_rir('simulate_rir_ism', room, source, mic_array, max_order, absorption, output_length, delay_filter_length,
                         center_frequency, sound_speed, sample_rate, False)


def simulate_rir_ism_batch(room, source, mic_array, max_order, absorption, output_length=None, delay_filter_length=81,
                           center_frequency=None, sound_speed=343.0, sample_rate=16000.0):
    """``room (B, D)``, ``source (B, D)``, ``mic_array (B, M, D)`` → ``(B, M, output_length)``: ``simulate_rir_ism`` for a batch of rooms in the same
    one launch — the form torchaudio lacks.  A batch of 1 gives the bits of the single call, and an entry's result does not depend
    on the rest of the batch.  ``absorption`` is a float, ``(2 D,)`` or ``(n_band, 2 D)`` shared by the batch (a 2-D tensor is always that),
    or ``(B, n_band, 2 D)`` per room (``(B, 1, 2 D)`` for one band).  ``output_length=None`` is the longest natural length of the batch."""
    return _simulate_rir('simulate_rir_ism_batch', room, source, mic_array, max_order, absorption, output_length, delay_filter_length,
                         center_frequency, sound_speed, sample_rate, True)


def psd(specgram, mask=None, normalize=True, eps=1e-10):
    """``(…, channel, freq, time)`` complex → ``(…, freq, channel, channel)``: torchaudio's ``functional.psd``, the power spectral
    density matrix ``Φ[f, c, e] = Σ_t m'[f, t] X[c, f, t] conj(X[e, f, t])`` with ``m' = 1`` without a mask, ``m`` with
    ``normalize=False`` and ``m / (Σ_t m + eps)`` otherwise.  ``mask`` is real ``(…, freq, time)``; ``ValueError`` when its shape
    does not match.  ``specgram`` is ``complex64`` (``complex64`` comes back) or the project's trailing-``2`` pairs (pairs come back).

    float32 on a HIP device with 2 to 8 channels is one entry of two launches (csrc/beamform.hip): lanes run along the bins, a lane
    keeps the Hermitian triangle of one (batch entry, bin) in registers over a piece of the frames, and the pieces are added in a
    fixed order in float64 — no ``(…, freq, time, channel, channel)`` tensor, no atomics, the same bits every run, Hermitian to the
    bit.  The frame-major views ``stft`` and ``phase_vocoder`` return are read in place.  float64, other channel counts, expanded or
    non-positive strides and the backward pass take ``_composite.psd`` (also the CPU path), announced with
    ``CompositeRouteWarning`` on a device."""
    x, was_complex = _beamform.pairs(specgram, 'specgram')
    _beamform.spec_shape(x)
    if mask is None:
        mask = _beamform.none(x)
    else:
        _beamform.check_mask(mask, x)
    return _beamform.unpairs(_call('psd', x, mask, bool(normalize), float(eps)), was_complex)


def mvdr_weights_souden(psd_s, psd_n, reference_channel, diagonal_loading=True, diag_eps=1e-7, eps=1e-8):
    """two ``(…, freq, channel, channel)`` complex PSDs → ``(…, freq, channel)`` MVDR weights by Souden's solution (torchaudio's
    ``functional.mvdr_weights_souden``): with loading ``Φn ← Φn + (diag_eps Re tr Φn + 1e-8) I``; ``N = Φn⁻¹ Φs`` by a solve;
    ``W = N / (tr N + eps)``; ``w = W[:, r]`` for an int ``r``, ``w = Σ_c W[:, c] u[c]`` for a real tensor ``u`` of shape
    ``(…, channel)`` or ``(channel,)``.

    float32 on a HIP device with 2 to 8 channels is one launch with a lane per (batch entry, bin): loading, elimination with partial
    pivoting, the complex trace, the division and the contraction run in float64 on chip from the float32 PSDs, and the result is
    rounded once.  ``u`` is read on the device."""
    s, was_complex = _beamform.pairs(psd_s, 'psd_s')
    n, _ = _beamform.pairs(psd_n, 'psd_n')
    lead, n_bins, n_ch, u, r = _beamform.check_weights_args(s, n, reference_channel)
    out = _call('mvdr_weights_souden', s, n, _beamform.none(s) if u is None else u, r, bool(diagonal_loading), float(diag_eps),
                float(eps))
    return _beamform.unpairs(out, was_complex)


def apply_beamforming(beamform_weights, specgram):
    """``(…, freq, channel)`` weights and a ``(…, channel, freq, time)`` spectrogram → ``(…, freq, time)``: ``Y[f, t] = Σ_c
    conj(w[f, c]) X[c, f, t]`` (torchaudio's ``functional.apply_beamforming``).  On a HIP device the result is the frame-major view
    ``istft`` reads without a copy; each ``X`` element is read once and each output written once."""
    w, _ = _beamform.pairs(beamform_weights, 'beamform_weights')
    x, was_complex = _beamform.pairs(specgram, 'specgram')
    _beamform.check_apply(w, x)
    return _beamform.unpairs(_call('apply_beamforming', w, x), was_complex)


def rtf_evd(psd_s):
    """``(…, freq, channel, channel)`` complex Hermitian PSD → ``(…, freq, channel)``: the relative transfer function (steering
    vector) as the eigenvector of the largest eigenvalue, at unit 2-norm (torchaudio's ``functional.rtf_evd``).

    Any unit phase of an eigenvector is an eigenvector, and the eigen-solvers do not agree on the one they return.  This package
    fixes it on every route: the component of largest modulus (the lowest index on a tie) is real and positive, its imaginary part
    exactly zero.  ``mvdr_weights_rtf`` with a reference does not depend on the phase.

    float32 on a HIP device with 2 to 8 channels is one launch with a lane per (batch entry, bin): cyclic Jacobi on the Hermitian
    matrix in float64 on chip (the lower triangle is read), which needs no spectral gap — a zero, identity or rank-one PSD gives a
    finite unit vector — rounded once.  Other inputs take ``torch.linalg.eigh`` and the same convention (``_composite.rtf_evd``)."""
    s, was_complex = _beamform.pairs(psd_s, 'psd_s')
    _beamform.psd_shape(s, 'psd_s')
    return _beamform.unpairs(_call('rtf_evd', s), was_complex)


def rtf_power(psd_s, psd_n, reference_channel, n_iter=3, diagonal_loading=True, diag_eps=1e-7):
    """two ``(…, freq, channel, channel)`` complex PSDs → ``(…, freq, channel)``: the relative transfer function by the power
    method (torchaudio's ``functional.rtf_power``).  With loading ``Φn ← Φn + (diag_eps Re tr Φn + 1e-8) I``; ``φ = Φn⁻¹ Φs`` by a
    solve; ``r = φ[:, ref]`` for an int, ``φ u`` for a real tensor ``u`` of shape ``(…, channel)`` or ``(channel,)``; for ``n_iter >=
    2``, ``r ← φ r`` ``n_iter - 2`` times and then ``r ← Φs r``; for ``n_iter == 1``, ``r ← Φn r`` with the loaded ``Φn``.  Not
    normalised.  ``ValueError`` for ``n_iter <= 0``.

    float32 on a HIP device with 2 to 8 channels and ``n_iter <= 64`` is one launch: the solve and every product in float64 on
    chip from the float32 PSDs, rounded once."""
    s, was_complex = _beamform.pairs(psd_s, 'psd_s')
    n, _ = _beamform.pairs(psd_n, 'psd_n')
    n_iter = _beamform.check_n_iter(n_iter)
    lead, n_bins, n_ch, u, r = _beamform.check_weights_args(s, n, reference_channel)
    out = _call('rtf_power', s, n, _beamform.none(s) if u is None else u, r, n_iter, bool(diagonal_loading), float(diag_eps))
    return _beamform.unpairs(out, was_complex)


def mvdr_weights_rtf(rtf, psd_n, reference_channel=None, diagonal_loading=True, diag_eps=1e-7, eps=1e-8):
    """a ``(…, freq, channel)`` relative transfer function ``d`` and a ``(…, freq, channel, channel)`` noise PSD → ``(…, freq,
    channel)`` MVDR weights (torchaudio's ``functional.mvdr_weights_rtf``): with loading ``Φn ← Φn + (diag_eps Re tr Φn + 1e-8) I``;
    ``a = Φn⁻¹ d``; ``w = a / (Re(dᴴ a) + eps)``; then ``w ← w conj(d[ref])`` for an int reference, ``w ← w Σ_c conj(d_c) u_c`` for
    a real tensor ``u``, nothing for ``None``.

    float32 on a HIP device with 2 to 8 channels is one launch, float64 on chip, rounded once."""
    d, was_complex = _beamform.pairs(rtf, 'rtf')
    n, _ = _beamform.pairs(psd_n, 'psd_n')
    lead, n_bins, n_ch, u, r = _beamform.check_rtf_weights_args(d, n, reference_channel)
    out = _call('mvdr_weights_rtf', d, n, _beamform.none(d) if u is None else u, r, bool(diagonal_loading), float(diag_eps),
                float(eps))
    return _beamform.unpairs(out, was_complex)


def rnnt_loss(logits, targets, logit_lengths, target_lengths, blank=-1, clamp=-1.0, reduction='mean', fused_log_softmax=True):
    """The transducer loss of Graves (2012) with torchaudio's ``functional.rnnt_loss`` signature, defaults and semantics.

    ``logits`` is the joint network's ``(batch, time, target + 1, class)`` output, ``targets`` ``(batch, target)`` int32 without
    blanks, ``logit_lengths`` (``Tb``) and ``target_lengths`` (``Ub``) ``(batch,)`` int32.  With ``lp = log_softmax(logits, -1)``
    (``logits`` itself for ``fused_log_softmax=False``): ``alpha[0,0] = 0``, ``alpha[t,u] = logaddexp(alpha[t-1,u] + lp[t-1,u,blank],
    alpha[t,u-1] + lp[t,u-1,targets[u-1]])`` and ``cost = -(alpha[Tb-1,Ub] + lp[Tb-1,Ub,blank])``.  A negative ``blank`` counts from
    the end.  ``reduction``: ``'none'`` gives the ``(batch,)`` costs, ``'mean'`` and ``'sum'`` a scalar, in the dtype of ``logits``.
    The gradient goes to ``logits`` alone; it is clipped to ``[-clamp, clamp]`` where ``clamp > 0`` BEFORE the incoming gradient
    (the ``1 / batch`` of ``'mean'`` included) multiplies it, as in torchaudio, and is zero for ``t >= Tb`` or ``u > Ub``.

    float32 on a HIP device whose class axis has unit stride (any positive other strides: a ``[:, :T', :U'+1]`` slice of a padded
    joint output is read in place), with ``target + 1 <= 1024`` and fewer than 2^31 lattice cells, runs csrc/rnnt.hip: forward two
    launches (one read of the valid part of the logits: the denominators and the two log-probabilities of every lattice cell;
    then alpha and beta together), backward one (a second read of the logits, one write of the gradient).  Three ``(batch, time,
    target + 1)`` arrays are kept for the backward pass — no copy of the logits and no gradient buffer.  Bit-identical from run
    to run and, for an entry, whatever else is in the batch.  Other inputs take ``_composite.rnnt_loss``, announced.

    The one deviation from torchaudio: its checks ``logit_lengths.max() == time`` and ``target_lengths.max() == target`` read
    device memory, so they are made for CPU tensors only; on a HIP device nothing waits for the host.  There an entry with ``Tb``
    outside ``[1, time]``, ``Ub`` outside ``[0, target]`` or a used target outside ``[0, class)`` gets a NaN cost and a NaN gradient
    over its own block; the other entries are unaffected and no address outside the tensors is formed."""
    if reduction not in ('none', 'mean', 'sum'):
        raise ValueError("rnnt_loss: reduction must be 'none', 'mean' or 'sum', got %r" % (reduction,))
    blank = _ops.rnnt_check(logits, targets, logit_lengths, target_lengths, int(blank))
    costs = _call('rnnt_loss', logits, targets, logit_lengths, target_lengths, blank, float(clamp), bool(fused_log_softmax))[0]
    if reduction == 'mean':
        return costs.mean()
    if reduction == 'sum':
        return costs.sum()
    return costs


def forced_align(log_probs, targets, input_lengths=None, target_lengths=None, blank=0):
    """CTC forced alignment with torchaudio's ``functional.forced_align`` signature and defaults: ``(paths, scores)``, the most
    probable frame labelling of ``log_probs`` ``(batch, time, class)`` that collapses to ``targets`` ``(batch, target)`` (int32 or
    int64, no blanks).  ``paths`` ``(batch, time)``, in the dtype of ``targets``, is the class emitted at each frame; ``scores``,
    in the dtype of ``log_probs``, is ``log_probs[b, t, paths[b, t]]`` (the same bits).  ``input_lengths`` (``Tb``) and
    ``target_lengths`` (``Lb``) are ``(batch,)`` integer tensors; ``None`` means ``time`` and ``target`` for every entry.

    Per entry there are ``2 Lb + 1`` states, even ones the blank and ``2k + 1`` ``targets[k]``.  ``alpha[0][0] = lp[0][blank]``,
    ``alpha[0][1] = lp[0][targets[0]]``, ``-inf`` elsewhere; for ``t >= 1`` with ``x0 = alpha[t-1][s]``, ``x1 = alpha[t-1][s-1]`` and
    ``x2 = alpha[t-1][s-2]`` (only for odd ``s >= 3`` whose label differs from the label before): back-pointer 2 if ``x2 > x1 and
    x2 > x0``, else 1 if ``x1 > x0 and x1 > x2``, else 0, and ``alpha[t][s] = chosen + lp[t][label(s)]``, one addition in the dtype
    of ``log_probs``.  The end state is the last blank if its alpha is greater than the last label's, else the last label; the
    back-pointers are followed down to the first frame.  Ties go to the lower back-pointer and a NaN where these comparisons
    send it.  torchaudio's moving window of states only removes states on no complete path and is not applied.

    float32 on a HIP device with positive strides (a slice of a padded model output is read in place) and ``target + 1 <= 1024``
    runs csrc/align.hip: ONE launch for the recursion, the backtrack and both outputs, a workgroup per entry; the same bits from
    run to run and whatever else is in the batch.  Other inputs take ``_composite.forced_align`` (a step of a Python loop per
    frame), announced on a HIP device.  The gradient of ``scores`` with respect to ``log_probs`` is the scatter of the incoming
    gradient at ``paths`` (torch operators); ``paths`` has none.

    Deviations from torchaudio:

    1. torchaudio refuses ``batch != 1``.  Here any ``batch >= 0`` is taken and the entries are independent; frames ``t >= Tb``
       get ``paths = blank`` and ``scores = 0``.  An empty batch launches nothing.
    2. On a HIP device nothing waits for the host: an entry that is infeasible (``Tb < Lb +`` the number of targets equal to the
       one before), has ``Tb < 1``, ``Tb > time`` or ``Lb > target``, or has the blank or an index outside ``[0, class)`` among its
       first ``Lb`` targets gets ``paths = -1`` and ``scores = NaN`` on all frames, and the other entries are unaffected.  For CPU
       tensors the same conditions raise ``ValueError`` naming the entry, as torchaudio's checks do.
    3. Dimensions, dtypes, ``blank`` in ``[0, class)``, agreeing batch sizes, one device and non-empty time and class axes are
       checked on every route and raise ``ValueError``."""
    blank = _ops.align_check(log_probs, targets, input_lengths, target_lengths, int(blank))
    return _call('forced_align', log_probs, targets, input_lengths, target_lengths, blank)


@dataclasses.dataclass
class TokenSpan:
    """A run of one token in an alignment (torchaudio's ``functional.TokenSpan``): frames ``[start, end)``, ``score`` their mean"""
    token: int
    start: int
    end: int
    score: float

    def __len__(self):
        return self.end - self.start


def merge_tokens(tokens, scores, blank=0):
    """Runs of equal tokens of a frame-level alignment as ``TokenSpan``s, blank runs dropped (torchaudio's
    ``functional.merge_tokens``): ``tokens`` and ``scores`` are 1-D and of equal length, e.g. ``paths[0]`` and ``scores[0]`` of
    ``forced_align``; a span's ``score`` is the mean of its frames' scores.  Host-side: one device-to-host copy per argument."""
    if tokens.ndim != 1 or scores.ndim != 1:
        raise ValueError('merge_tokens: `tokens` and `scores` must be 1D Tensor.')
    if len(tokens) != len(scores):
        raise ValueError('merge_tokens: `tokens` and `scores` must be the same length.')
    toks, vals = tokens.detach().cpu().tolist(), scores.detach().cpu().double().tolist()
    spans, start = [], 0
    for i in range(1, len(toks) + 1):
        if i == len(toks) or toks[i] != toks[start]:
            if toks[start] != blank:
                spans.append(TokenSpan(token=toks[start], start=start, end=i, score=sum(vals[start:i]) / (i - start)))
            start = i
    return spans


def preemphasis(waveforms, coeff=0.97):
    """``y[n] = x[n] - coeff x[n-1]``, ``y[0] = x[0]`` (torchaudio's ``functional.preemphasis``); not clamped.  The same kernel
    as ``lfilter`` with ``b = (1, -coeff)``, ``a = (1, 0)``: no recursion, one read and one write of the waveform."""
    x = _waveform(waveforms, 'preemphasis')
    return _call('lfilter', x, _filters.host_tensor((1.0, 0.0)), _filters.host_tensor((1.0, -float(coeff))), False)


def deemphasis(waveforms, coeff=0.97):
    """The inverse of ``preemphasis``: ``y[n] = x[n] + coeff y[n-1]``, i.e. ``lfilter`` with ``a = (1, -coeff)``, ``b = (1, 0)``;
    not clamped."""
    x = _waveform(waveforms, 'deemphasis')
    return _call('lfilter', x, _filters.host_tensor((1.0, -float(coeff))), _filters.host_tensor((1.0, 0.0)), False)


def _check_pairs(z, what):
    if z.dim() < 1 or z.shape[-1] != 2:
        raise RuntimeError('%s: expected a trailing dimension of size 2, got shape %s' % (what, tuple(z.shape)))


def angle(complex_tensor):
    """Phase ``atan2(im, re)`` of a ``(*, 2)`` tensor (reference: functional.py:187-191)."""
    z = _tensor(complex_tensor, 'complex_tensor')
    _check_pairs(z, 'angle')
    return _call('angle', z)


def magphase(complex_tensor, power=1.):
    """``(|z|**power, atan2(im, re))`` (reference: functional.py:194-201), both outputs from one pass over z."""
    z = _tensor(complex_tensor, 'complex_tensor')
    _check_pairs(z, 'magphase')
    return _call('magphase', z, float(power))


def phase_vocoder(complex_specgrams, rate, phase_advance):
    """Time-stretch a complex spectrogram by ``rate`` without changing pitch (reference:
    functional.py:204-274): ``(*, F, T, 2) → (*, F, ceil(T / rate), 2)``.  On a HIP device one kernel; each lane
    owns one (row, frequency) series and walks the output frames (csrc/phase_vocoder.hip)."""
    spec = _tensor(complex_specgrams, 'complex_specgrams')
    if spec.dim() < 3 or spec.shape[-1] != 2:
        raise RuntimeError('phase_vocoder: expected (*, num_freqs, time, 2), got shape %s' % (tuple(spec.shape),))
    pa = _tensor(phase_advance, 'phase_advance')
    # the reference broadcasts phase_advance against (..., num_freqs, time'): it must be (num_freqs, 1) (or a leading-1
    # variant of it) there, and every route here — HIP kernel, torch operators, fake — sees it in that one shape
    if pa.numel() != spec.shape[-3] or pa.dim() < 2 or pa.shape[-1] != 1 or pa.shape[-2] != spec.shape[-3]:
        raise RuntimeError('phase_vocoder: phase_advance must have shape (num_freqs, 1) = (%d, 1), got %s'
                           % (spec.shape[-3], tuple(pa.shape)))
    pa = pa.reshape(spec.shape[-3], 1)
    if pa.device != spec.device:
        raise RuntimeError('phase_vocoder: spectrogram and phase_advance must be on the same device')
    if not rate > 0:                 # the reference's torch.arange(0, T, rate) raises RuntimeError for such a step
        raise RuntimeError('phase_vocoder: rate must be positive, got %r' % (rate,))
    return _call('phase_vocoder', spec, pa, float(rate))


def amplitude_to_db(x, ref=1.0, amin=1e-7):
    """``10·(log10(max(x², amin)) − log10(ref))`` — the reference squares its input (functional.py:277-296)."""
    return _call('amplitude_to_db', _tensor(x, 'x'), float(ref), float(amin))


def db_to_amplitude(x, ref=1.0):
    """``(10^(x/10 + log10 ref))^0.5`` (reference: functional.py:299-314)."""
    return _call('db_to_amplitude', _tensor(x, 'x'), float(ref))


def mu_law_encoding(x, n_quantize=256):
    """mu-law companding to int64 codes (reference: functional.py:317-335).

    On a HIP device the codes are bit-exact with the reference for every input and ``n_quantize``: for 256 levels
    and ``|x| <= 1`` the kernel compares against the 255 float32 thresholds extracted from the reference
    (``_mulaw_tables.py``), everything else evaluates the closed form with the exact float32 roundings of the
    reference's CPU path (``csrc/exact_math.hpp``)."""
    return _call('mu_law_encoding', _tensor(x, 'x'), int(n_quantize))


def mu_law_decoding(x_mu, n_quantize=256, dtype=torch.get_default_dtype()):
    """mu-law expansion (reference: functional.py:338-354).  On a HIP device codes that are integers in
    ``[0, 256)`` — int64 or float-typed — with ``n_quantize == 256`` are decoded through the reference's own
    256-entry table (bit-exact); everything else evaluates the closed form in fp32 (within 1 ulp of ``exp``)."""
    return _call('mu_law_decoding', _tensor(x_mu, 'x_mu'), int(n_quantize), dtype)


def hpss(mag_specgrams, kernel_size=31, power=2.0, hard=False, mask_only=False):
    """Harmonic / percussive source separation by median filtering (reference: beta_hpss.py:35-127):
    ``(harmonic spectrogram, percussive spectrogram, harmonic mask, percussive mask)`` of a magnitude spectrogram
    ``(*, freq, time)``; with ``mask_only`` the first two are None.  ``kernel_size``: odd int, or ``(width along
    frequency of the percussive filter, width along time of the harmonic filter)`` — the reference only runs with equal
    widths (its padding and slicing mix the two up otherwise); here unequal widths do what its docstring describes.
    Hard masks are bool tensors, as in the reference.  On a HIP device one kernel (csrc/hpss.hip) for widths <= 31."""
    x = _tensor(mag_specgrams, 'mag_specgrams')
    if not isinstance(kernel_size, (tuple, int)):
        raise TypeError('kernel_size is expected to be either tuple of input, but it is: %s' % type(kernel_size))
    kf, kt = (kernel_size, kernel_size) if isinstance(kernel_size, int) else kernel_size
    if x.dim() < 2:
        raise RuntimeError('hpss: expected (*, freq, time), got shape %s' % (tuple(x.shape),))
    if kf // 2 >= x.shape[-2] or kt // 2 >= x.shape[-1]:
        raise RuntimeError('hpss: reflect padding (%d, %d) must be smaller than the spectrogram size %s'
                           % (kf // 2, kt // 2, tuple(x.shape[-2:])))
    if mask_only:                                         # (the kernels skip the two masked-spectrogram stores)
        harm = perc = None
        mask_h, mask_p = _call('hpss_masks', x, int(kf), int(kt), float(power), bool(hard))
    else:
        harm, perc, mask_h, mask_p = _call('hpss', x, int(kf), int(kt), float(power), bool(hard))
    if hard:
        mask_h, mask_p = mask_h > 0.5, mask_p > 0.5
    return harm, perc, mask_h, mask_p
