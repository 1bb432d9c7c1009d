"""Stock-torch backend of every op in ``_ops.py`` — the kernels registered for the dispatch keys the gfx950
library does not serve.

Who ends up here (``_ops.py`` decides, never silently for a float32 tensor that lives on the GPU):

  * CPU tensors.  The reference computes where its input lives (its whole test-suite is CPU-only,
    reference ``tests/test_layers.py:1-3``; BASELINE configs[0] is a CPU configuration), so a CPU tensor is
    evaluated on the CPU by torch's own operators, in the reference's operator order so the values are the
    reference's.
  * float64 tensors on either device (the reference keeps f64 -> f64, e.g. its phase-vocoder test,
    reference ``tests/test_functional.py:69-116``); the gfx950 kernels compute in float32.
  * the derivative of an op that has no hand-written backward kernel (``_ops.py`` re-evaluates the op here
    under ``torch.enable_grad`` and differentiates that).

Nothing in this file is the product's fast path and nothing in it is test infrastructure either: the tests'
checker package is never imported here; it checks this file like it checks the kernels
(``tests/test_cpu_dropin.py``).
Each function takes fully resolved arguments (the public wrappers in ``functional.py`` fill in defaults and
validate) and cites the reference lines whose operator sequence it keeps.
"""
import math

import torch
import torch.nn.functional as TF

from . import _filters
from . import _kaldi
from . import _pitch
from . import _vad
from . import _beamform
from ._bounded import Bounded

TWO_PI = 2.0 * math.pi


def stft(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided):
    """reference functional.py:89-111: fold the leading dims into the FFT batch, ``torch.stft``, unfold; the
    complex result is handed back as the trailing-2 real view the reference's era of torch produced."""
    if wave.dtype == torch.int16:                                # PCM: sample * 2^-15 (the package's convention)
        wave = wave.to(torch.float32) * (1.0 / 32768.0)
    batch_shape = wave.shape[:-1]
    rows = wave.reshape(-1, wave.shape[-1])
    z = torch.stft(rows, n_fft, hop_length=hop, win_length=win_length, window=window, center=center,
                   pad_mode=pad_mode, normalized=normalized, onesided=onesided, return_complex=True)
    pairs = torch.view_as_real(z)
    return pairs.reshape(batch_shape + pairs.shape[1:])


def istft(spec, window, n_fft, hop, win_length, center, normalized, onesided, length):
    """the inverse of ``stft`` above the way the reference would wrap it: fold the leading dims into the batch, ``torch.istft``
    on the complex view of the trailing-2 pairs, unfold."""
    batch_shape = spec.shape[:-3]
    pairs = spec.reshape((-1,) + tuple(spec.shape[-3:]))
    if pairs.stride(-1) != 1 or any(s % 2 for s in pairs.stride()[:-1]):
        pairs = pairs.contiguous()
    out = torch.istft(torch.view_as_complex(pairs), n_fft, hop_length=hop, win_length=win_length, window=window,
                      center=center, normalized=normalized, onesided=onesided, length=length, return_complex=False)
    return out.reshape(tuple(batch_shape) + out.shape[1:])


def griffinlim(specgram, window, angles0, n_fft, hop, win_length, power, n_iter, m, length):
    """torchaudio's ``functional.griffinlim`` in its operator order: ``S = specgram ** (1 / power)``, then ``n_iter`` times
    ``istft`` -> ``stft`` -> ``A = R - m Rprev`` (skipped for ``m == 0``) -> ``A / (|A| + 1e-16)``, and a last ``istft``.  ``m`` is
    ``momentum / (1 + momentum)``; ``angles0`` (complex, the caller's draw, NOT normalised) or None for ``1 + 0j``."""
    lead = tuple(specgram.shape[:-2])
    S = specgram.reshape((-1,) + tuple(specgram.shape[-2:])).pow(1.0 / power)
    A = torch.ones((), dtype=torch.complex128 if S.dtype == torch.float64 else torch.complex64, device=S.device) \
        if angles0 is None else angles0.reshape(S.shape)
    prev = None
    for _ in range(n_iter):
        y = torch.istft(S * A, n_fft, hop_length=hop, win_length=win_length, window=window, length=length)
        R = torch.stft(y, n_fft, hop_length=hop, win_length=win_length, window=window, center=True, pad_mode='reflect',
                       normalized=False, onesided=True, return_complex=True)
        A = R
        if m and prev is not None:
            A = A - prev * m
        A = A / (A.abs() + 1e-16)
        prev = R
    y = torch.istft(S * A, n_fft, hop_length=hop, win_length=win_length, window=window, length=length)
    return y.reshape(lead + tuple(y.shape[-1:]))


def complex_norm(z, power):
    """reference functional.py:126-128: 2-norm of the (re, im) pair; the exponent is a second pass."""
    length = z.norm(p=2, dim=-1)
    if power == 1.0:
        return length
    return length.pow(power)


def angle(z):
    """reference functional.py:187-191."""
    re, im = z.unbind(-1)
    return torch.atan2(im, re)


def magphase(z, power):
    """reference functional.py:194-201."""
    return complex_norm(z, power), angle(z)


def apply_filterbank(spec, bank):
    """reference functional.py:183-184: frames to the row axis, one matmul, back."""
    frames_first = spec.transpose(-1, -2)
    return (frames_first @ bank).transpose(-1, -2)


def dct(x, matrix):
    """the same shape of call for the cepstral matrix: (…, n_in, time) x (n_in, n_out) -> (…, n_out, time)."""
    return (x.transpose(-1, -2) @ matrix).transpose(-1, -2)


def resample(wave, orig, new, lowpass_filter_width, rolloff, method, beta):
    """torchaudio's ``functional.resample`` in its own operator form: the full ``(new, 1, 2 width + orig)`` bank as a ``conv1d``
    at stride ``orig`` over the input padded by ``(width, width + orig)``, the phases interleaved and cut to
    ``ceil(new * L / orig)``.  ``orig`` / ``new`` are the reduced rates (``_resample.constants``)."""
    from . import _resample as RS
    length = wave.shape[-1]
    n_out = RS.out_length(length, orig, new)
    if orig == new:
        return wave.clone()        # (an op may not return its input; ``functional.resample`` hands the input back itself)
    if length == 0:
        return wave.new_zeros(tuple(wave.shape[:-1]) + (0,))
    width = RS.width_of(orig, new, lowpass_filter_width, rolloff)
    kernel = RS.full_bank(orig, new, lowpass_filter_width, rolloff, method, beta).to(device=wave.device, dtype=wave.dtype)
    rows = wave.reshape(-1, 1, length)
    out = TF.conv1d(TF.pad(rows, (width, width + orig)), kernel.unsqueeze(1), stride=orig)     # (rows, new, L // orig + 1)
    out = out.transpose(1, 2).reshape(rows.shape[0], -1)[:, :n_out].contiguous()      # dense, like the kernel's output
    return out.reshape(tuple(wave.shape[:-1]) + (n_out,))


_compact_tables = Bounded(16)


def _compact_table(key, valid, length, device, dtype):
    """(start, ok, weight) of the first ``valid`` outputs over rows of ``length`` samples, on ``device``: int64 ``(valid,)`` first
    input sample, bool and ``dtype`` ``(K, valid)`` — tap ``k`` of output ``n`` is read (inside its phase's run and the row), and its
    value (0 where it is not)"""
    from . import _resample as RS
    hit = _compact_tables.get((key, valid, length, str(device), dtype))
    if hit is None:
        with torch.inference_mode(False):
            b = RS.bank(*key)
            n = torch.arange(valid, dtype=torch.int64)
            j = torch.div(n, b.phases, rounding_mode='floor')
            p = n - j * b.phases
            start = j * b.step + torch.tensor(b.off, dtype=torch.int64)[p]
            k = torch.arange(b.K, dtype=torch.int64).unsqueeze(1)
            idx = start.unsqueeze(0) + k
            ok = (k < torch.tensor(b.run, dtype=torch.int64)[p].unsqueeze(0)) & (idx >= 0) & (idx < length)
            weight = torch.where(ok, b.taps[p].t(), torch.zeros((), dtype=torch.float64))
            hit = (start.to(device), ok.to(device), weight.to(device=device, dtype=dtype))
        _compact_tables[(key, valid, length, str(device), dtype)] = hit
    return hit


def resample_compact(wave, orig, new, lowpass_filter_width, rolloff, method, beta, out_len):
    """``resample`` by the reduced pair cut or zero-padded to ``out_len`` samples, from the COMPACT bank: ``K`` gathers and
    multiply-adds in the tensor's dtype (``_resample.apply_bank64`` without the float64 cast), differentiable, ``O(n_out)`` memory.
    The full-bank ``conv1d`` above cannot serve the pairs this is for: its kernel is 323 MB at 10079 : 8000 and 8.2 GB at
    42763 : 48000.  Samples behind a phase's run are not multiplied (a NaN reaches what the kernels let it reach)."""
    from . import _resample as RS
    length = wave.shape[-1]
    valid = min(RS.out_length(length, orig, new), out_len)
    if orig == new:
        out = wave[..., :valid]
    else:
        out = wave.new_zeros(tuple(wave.shape[:-1]) + (valid,))
        if valid and length:
            start, ok, weight = _compact_table((orig, new, lowpass_filter_width, rolloff, method, beta), valid, length, wave.device,
                                               wave.dtype)
            zero = wave.new_zeros(())
            for k in range(weight.shape[0]):
                out = out + weight[k] * torch.where(ok[k], wave[..., (start + k).clamp(0, length - 1)], zero)
    if out_len > valid:
        return TF.pad(out, (0, out_len - valid))
    return out.clone(memory_format=torch.contiguous_format) if orig == new else out      # (an op may not return its input)


def lfilter(wave, a_coeffs, b_coeffs, clamp):
    """torchaudio's ``functional.lfilter`` from the definition, ``a0 y[n] = sum_k b_k x[n-k] - sum_{k>=1} a_k y[n-k]`` with zero
    initial state: the feed-forward part as shifted sums, the recursion as a LOOP OVER TIME in torch ops, vectorised over the
    rows.  It accumulates in float64 and rounds to the input's dtype once — a float32 recursion loses three to four digits on
    poles next to z = 1 (a 20 Hz high-pass at 48 kHz: 1.6e-3 absolute against 1.6e-7).  Correct, differentiable w.r.t. the waveform
    and both coefficient tensors, any order — and slow: two or three small torch ops per sample.  It is the CPU path and the
    announced route on a device for what the kernel does not take.  Coefficients that are exactly zero and need no gradient are
    not multiplied, so a non-finite sample reaches what the kernel lets it reach."""
    length = wave.shape[-1]
    if wave.numel() == 0:
        return torch.zeros_like(wave, memory_format=torch.contiguous_format)
    wide = torch.float64
    a = a_coeffs.to(device=wave.device, dtype=wide)
    b = b_coeffs.to(device=wave.device, dtype=wide)
    n = a.numel()
    bn, an = b / a[0], a / a[0]
    skip_b = [(not b_coeffs.requires_grad and not a_coeffs.requires_grad) and v == 0.0 for v in bn.tolist()]
    skip_a = [(not a_coeffs.requires_grad) and v == 0.0 for v in an.tolist()]
    x = wave.reshape(-1, length).to(wide)
    padded = TF.pad(x, (n - 1, 0))
    v = torch.zeros_like(x)
    for k in range(n):
        if not skip_b[k]:
            v = v + bn[k] * padded[:, n - 1 - k: n - 1 - k + length]
    if all(skip_a[1:]):
        y = v
    else:
        ys = []
        for t in range(length):
            acc = v[:, t]
            for k in range(1, min(n, t + 1)):
                if not skip_a[k]:
                    acc = acc - an[k] * ys[t - k]
            ys.append(acc)
        y = torch.stack(ys, dim=-1) if ys else v
    y = y.to(wave.dtype)
    if clamp:
        y = y.clamp(-1.0, 1.0)
    return y.reshape(wave.shape)


def sosfilt(wave, sos, clamp):
    """A cascade of second-order sections, ``sos`` of shape ``(S, 6)`` with rows ``(b0, b1, b2, a0, a1, a2)``: ``lfilter`` above
    section by section.  The signal between two sections stays float64; it is rounded to the input's dtype once, behind the last
    one, and clipped there when ``clamp``.  Differentiable w.r.t. the waveform and ``sos``, and as slow as ``lfilter``: the CPU
    path of ``tac_amd::sosfilt`` and its announced route on a device."""
    if wave.numel() == 0:
        return torch.zeros_like(wave, memory_format=torch.contiguous_format)
    y = wave.to(torch.float64)
    for s in range(sos.shape[0]):
        y = lfilter(y, sos[s, 3:], sos[s, :3], False)
    y = y.to(wave.dtype)
    if clamp:
        y = y.clamp(-1.0, 1.0)
    return y.contiguous()


def loudness(waveform, sample_rate):
    """torchaudio's ``functional.loudness`` (ITU-R BS.1770-4) in torch operators, in the input's dtype: ``(…, channels, time)`` →
    ``(…)``.  The K-weighting is this package's ``treble_biquad`` and ``highpass_biquad`` (``lfilter`` above, each clipped to [-1, 1]
    and rounded to the input's dtype), then the mean square of blocks of ``gate`` samples every ``step``, the weighted sum over
    the channels, and the two gates: ``l_k > -70`` and ``l_k >`` the level of the mean over those blocks ``- 10``.  A gated block is
    multiplied by 0, so a NaN block makes its entry NaN; no block left gives 0 / 0 = NaN.  The CPU route of ``tac_amd::loudness``
    and its announced composite route; what csrc/loudness.hip does in two launches."""
    gate, step = _filters.loudness_blocks(sample_rate)
    w = waveform
    for b, a in _filters.k_weighting(sample_rate):
        w = lfilter(w, _filters.host_tensor(a), _filters.host_tensor(b), True)
    energy = torch.square(w).unfold(-1, gate, step).mean(-1)                                    # (…, C, nb)
    g = torch.tensor(_filters.LOUDNESS_WEIGHTS[:energy.shape[-2]], dtype=energy.dtype, device=energy.device)

    def level(e):
        return -0.691 + 10.0 * torch.log10((g * e).sum(-1))

    def gated(keep):
        return (keep.unsqueeze(-2) * energy).sum(-1) / torch.count_nonzero(keep, dim=-1).unsqueeze(-1)

    l = -0.691 + 10.0 * torch.log10((g.unsqueeze(-1) * energy).sum(-2))                          # (…, nb)
    keep = l > -70.0
    gamma = level(gated(keep)) - 10.0
    keep = keep & (l > gamma.unsqueeze(-1))
    return level(gated(keep))


def pitch_nccf(waveform, geo):
    """``(rows, time)`` → ``(rows, n_frames, max_lag)``: column ``c`` holds lag ``c + 1``.  The loop over the lags of torchaudio's
    ``_compute_nccf``: ``(s1 . s2) / (1e-9 + |s1|)^2 / (1e-9 + |s2|)^2`` — both energies, not their roots."""
    frame, n_frames = geo.frame, geo.n_frames
    x = TF.pad(waveform, (0, geo.max_lag + n_frames * frame - waveform.shape[-1]))
    columns = []
    for lag in range(1, geo.max_lag + 1):
        s1 = x[..., :-lag].unfold(-1, frame, frame)[..., :n_frames, :]
        s2 = x[..., lag:].unfold(-1, frame, frame)[..., :n_frames, :]
        columns.append(((s1 * s2).sum(-1) / (1e-9 + torch.linalg.vector_norm(s1, ord=2, dim=-1)).pow(2)
                        / (1e-9 + torch.linalg.vector_norm(s2, ord=2, dim=-1)).pow(2)).unsqueeze(-1))
    return torch.cat(columns, -1)


def pitch_lags(nccf, geo):
    """``(rows, n_frames, max_lag)`` → int64 ``(rows, n_frames)``: the lag of the best column from ``lag_min`` on, or of the best
    one below ``half`` where that one exceeds 0.99 of it"""
    best = torch.max(nccf[..., geo.lag_min:], -1)
    low = torch.max(nccf[..., geo.lag_min:geo.half], -1)
    take = low[0] > 0.99 * best[0]
    return take * low[1] + ~take * best[1] + (geo.lag_min + 1)


def pitch_smooth(lags, win_length, sample_rate):
    """``(rows, n_frames)`` integer lags → float32 ``(rows, n_frames + pad - win_length + 1)``: the lower median over ``win_length``
    lags behind ``pad = (win_length - 1) // 2`` copies of the first one, then ``float32(sample_rate) / float32(lag)``"""
    pad = (win_length - 1) // 2
    if pad:
        lags = torch.cat([lags[..., :1].expand(lags.shape[:-1] + (pad,)), lags], -1)
    values = torch.median(lags.unfold(-1, win_length, 1), -1)[0]
    return torch.tensor(float(sample_rate), dtype=torch.float32, device=lags.device) / values.to(torch.float32)


def detect_pitch_frequency(waveform, sample_rate, frame_time=1e-2, win_length=30, freq_low=85, freq_high=3400):
    """torchaudio's ``functional.detect_pitch_frequency`` in torch operators: ``(…, time)`` → float32 ``(…, n_out)``.  The NCCF is
    formed in the input's dtype, lag by lag; the result is float32 whatever the input.  The CPU route of
    ``tac_amd::detect_pitch_frequency`` and its announced composite route; what csrc/pitch.hip does in two launches."""
    geo = _pitch.check(waveform, sample_rate, frame_time, win_length, freq_low, freq_high)
    rows = waveform.reshape(-1, waveform.shape[-1])
    freq = pitch_smooth(pitch_lags(pitch_nccf(rows, geo), geo), win_length, sample_rate)
    return freq.reshape(tuple(waveform.shape[:-1]) + (geo.n_out,))


def vad_measures(waveform, p):
    """``(…, time)`` → ``(…, T)``: the measures of ``vad`` for the ``_vad.Plan`` ``p`` in torch operators, vectorised over rows and
    bins with one loop over the frames.  float64 input is measured in float64, every other dtype in float32 (the windows are the
    float32 Hann values in both).  The CPU route of ``tac_amd::vad_measures`` and its announced composite route."""
    dtype = torch.float64 if waveform.dtype == torch.float64 else torch.float32
    time = waveform.shape[-1]
    n_frames = _vad.frames(time, p)
    x = waveform.reshape(-1, time).to(dtype)
    meas = x.new_zeros((x.shape[0], n_frames))
    if meas.numel() == 0:
        return meas.reshape(tuple(waveform.shape[:-1]) + (n_frames,))
    nb, nq = p.s1 - p.s0, p.c1 - p.c0
    win = torch.hann_window(p.mlen, dtype=torch.float32, device=x.device).to(dtype) * (2.0 / math.sqrt(p.mlen))
    win2 = torch.hann_window(nb, dtype=torch.float32, device=x.device).to(dtype) * (2.0 / math.sqrt(nb))
    frames = x.unfold(-1, p.mlen, p.period)[:, :n_frames]
    mag = torch.fft.rfft(frames * win, n=p.dft).abs()[..., p.s0:p.s1]                        # (rows, T, nb)
    spec = x.new_zeros((x.shape[0], nb))
    noise = x.new_zeros((x.shape[0], nb))
    buf = x.new_zeros((x.shape[0], n_frames, p.dft // 2))
    boot = 0
    for t in range(n_frames):
        m = boot / (1.0 + boot) if boot >= 0 else p.smooth
        spec = spec * m + mag[:, t] * (1.0 - m)
        d = spec * spec
        m2 = torch.zeros_like(d) if boot >= 0 else torch.where(d > noise, d.new_tensor(p.up), d.new_tensor(p.down))
        noise = noise * m2 + d * (1.0 - m2)
        buf[:, t, p.s0:p.s1] = torch.sqrt(torch.clamp(d - p.nra * noise, min=0.0)) * win2   # (clamp keeps a NaN)
        if boot >= 0:
            boot = -1 if boot == p.boot_max else boot + 1
    c = torch.fft.rfft(buf)[..., p.c0:p.c1]
    r = (c.real * c.real + c.imag * c.imag).sum(-1)
    meas = torch.where(r > 0, torch.clamp(21.0 + torch.log(r / nq), min=0.0), torch.zeros_like(r))
    return meas.reshape(tuple(waveform.shape[:-1]) + (n_frames,))


def vad_start(meas, p, time):
    """``(groups, channels, T)`` measures → ``(start int64 (groups,), triggered bool (groups,))``: the decision of ``vad`` in torch
    operators, vectorised over groups and channels, with one loop over the frames and one over the backward search; ``start`` is
    clamped at 0.  The CPU route of ``tac_amd::vad_start`` and its announced composite route."""
    groups, channels, n_frames = meas.shape
    dev = meas.device
    which = torch.arange(channels, device=dev)
    mean = meas.new_zeros((groups, channels))
    k = torch.zeros(groups, dtype=torch.int64, device=dev)
    first = torch.zeros(groups, dtype=torch.int64, device=dev)
    found = torch.zeros(groups, dtype=torch.bool, device=dev)
    for t in range(n_frames):
        mean = mean * p.trig + meas[:, :, t] * (1.0 - p.trig)
        hit = mean >= p.level
        new = hit.any(1) & ~found
        k = torch.where(new, torch.full_like(k, t), k)
        first = torch.where(new, torch.where(hit, which, channels).amin(1), first)
        found = found | new
    j_t = torch.full((groups, channels), p.n, dtype=torch.int64, device=dev)
    j_z = j_t.clone()
    for j in range(p.n if n_frames and channels else 0):
        at = k - j
        v = meas.gather(2, at.clamp(min=0)[:, None, None].expand(groups, channels, 1))[..., 0]
        v = torch.where((at >= 0)[:, None], v, torch.zeros_like(v))
        take = (v >= p.level) & (j <= j_t + p.gap)
        zero = ~take & (v == 0) & (j_t >= j_z)
        j_t = torch.where(take, torch.full_like(j_t, j), j_t)
        j_z = torch.where(take | zero, torch.full_like(j_z, j), j_z)
    flush = torch.where(which[None, :] >= first[:, None], j_z.clamp(max=p.n - 1), torch.zeros_like(j_z))
    flush = flush.amax(1) if channels else k
    start = torch.where(found, (k - flush) * p.period - p.pre, torch.full_like(k, time - p.keep))
    return start.clamp(min=0), found


def _complex(t):
    """pairs ``(…, 2)`` as a complex tensor: a view where the strides allow one (the frame-major views do)"""
    ok = t.stride(-1) == 1 and all(st % 2 == 0 for st, n in zip(t.stride()[:-1], t.shape[:-1]) if n > 1)
    return torch.view_as_complex(t if ok else t.contiguous())


def psd(specgram, mask, normalize=True, eps=1e-10):
    """torchaudio's ``functional.psd`` in torch operators, on pairs: ``(…, C, F, T, 2)`` → ``(…, F, C, C, 2)``.  The literal form:
    an einsum that materialises ``(…, F, T, C, C)``, the (normalised) mask applied to it, then the sum over time.  ``mask``:
    ``(…, F, T)`` or ``_beamform.none``."""
    x = _complex(specgram).transpose(-3, -2)                                   # (…, F, C, T)
    outer = torch.einsum('...ct,...et->...tce', x, x.conj())
    if not _beamform.absent(mask):
        if normalize:
            mask = mask / (mask.sum(dim=-1, keepdim=True) + eps)
        outer = outer * mask[..., None, None]
    return torch.view_as_real(outer.sum(dim=-3))


def mvdr_weights_souden(psd_s, psd_n, ref_vector, ref_channel, diagonal_loading=True, diag_eps=1e-7, eps=1e-8):
    """torchaudio's ``functional.mvdr_weights_souden`` on pairs: two ``(…, F, C, C, 2)`` → ``(…, F, C, 2)``.  ``ref_vector``: real
    ``(…, C)`` / ``(C,)`` or ``_beamform.none`` (then column ``ref_channel``)."""
    s, n = _complex(psd_s), _complex(psd_n)
    if diagonal_loading:
        trace = n.diagonal(dim1=-1, dim2=-2).sum(-1).real[..., None, None]
        n = n + (trace * diag_eps + 1e-8) * torch.eye(n.shape[-1], dtype=n.dtype, device=n.device)
    numerator = torch.linalg.solve(n, s)
    ws = numerator / (numerator.diagonal(dim1=-1, dim2=-2).sum(-1)[..., None, None] + eps)
    if _beamform.absent(ref_vector):
        w = ws[..., :, ref_channel]
    else:
        w = torch.einsum('...fec,...c->...fe', ws, ref_vector.to(ws.dtype))
    return torch.view_as_real(w.contiguous())


def apply_beamforming(weights, specgram):
    """torchaudio's ``functional.apply_beamforming`` on pairs: ``(…, F, C, 2)`` and ``(…, C, F, T, 2)`` → ``(…, F, T, 2)``, returned
    as the frame-major view the kernels return"""
    y = torch.einsum('...fc,...cft->...ft', _complex(weights).conj(), _complex(specgram))
    return torch.view_as_real(y.transpose(-2, -1).contiguous()).transpose(-3, -2)


def mvdr_souden(specgram, mask_s, mask_n, ref_vector, ref_channel, diagonal_loading=True, diag_eps=1e-7, eps=1e-8, psd_eps=1e-15):
    """the ``MVDR`` layer at ``solution='ref_channel'``: two normalised PSDs (``mask_n`` absent: ``1 - mask_s``), Souden weights,
    the weights applied"""
    if _beamform.absent(mask_n):
        mask_n = 1 - mask_s
    w = mvdr_weights_souden(psd(specgram, mask_s, True, psd_eps), psd(specgram, mask_n, True, psd_eps), ref_vector, ref_channel,
                            diagonal_loading, diag_eps, eps)
    return apply_beamforming(w, specgram)


def _loaded(n, diag_eps):
    trace = n.diagonal(dim1=-1, dim2=-2).sum(-1).real[..., None, None]
    return n + (trace * diag_eps + 1e-8) * torch.eye(n.shape[-1], dtype=n.dtype, device=n.device)


def lead_phase(v):
    """the phase convention of ``rtf_evd`` on a complex ``(…, C)`` vector: the component of largest modulus (lowest index on a tie)
    made real and positive, its imaginary part exactly zero"""
    mag = v.abs()
    lead = mag.argmax(dim=-1, keepdim=True)                                   # (the first of equal maxima)
    h = torch.gather(v, -1, lead)
    v = v * (h.conj() / torch.gather(mag, -1, lead))
    fixed = torch.view_as_real(v).clone()
    fixed[..., 1].scatter_(-1, lead, 0.0)
    return torch.view_as_complex(fixed)


def rtf_evd(psd_s):
    """torchaudio's ``functional.rtf_evd`` on pairs: ``(…, F, C, C, 2)`` → ``(…, F, C, 2)``, the eigenvector of the largest
    eigenvalue by ``torch.linalg.eigh`` (unit 2-norm), then ``lead_phase``"""
    _, v = torch.linalg.eigh(_complex(psd_s))
    return torch.view_as_real(lead_phase(v[..., -1]))


def rtf_power(psd_s, psd_n, ref_vector, ref_channel, n_iter=3, diagonal_loading=True, diag_eps=1e-7):
    """torchaudio's ``functional.rtf_power`` on pairs: two ``(…, F, C, C, 2)`` → ``(…, F, C, 2)``"""
    s, n = _complex(psd_s), _complex(psd_n)
    if diagonal_loading:
        n = _loaded(n, diag_eps)
    phi = torch.linalg.solve(n, s)
    if _beamform.absent(ref_vector):
        r = phi[..., ref_channel]
    else:
        r = torch.einsum('...fec,...c->...fe', phi, ref_vector.to(phi.dtype))
    r = r.unsqueeze(-1)
    if n_iter >= 2:
        for _ in range(n_iter - 2):
            r = torch.matmul(phi, r)
        r = torch.matmul(s, r)
    else:
        r = torch.matmul(n, r)
    return torch.view_as_real(r.squeeze(-1).contiguous())


def mvdr_weights_rtf(rtf, psd_n, ref_vector, ref_channel, diagonal_loading=True, diag_eps=1e-7, eps=1e-8):
    """torchaudio's ``functional.mvdr_weights_rtf`` on pairs: ``(…, F, C, 2)`` and ``(…, F, C, C, 2)`` → ``(…, F, C, 2)``.
    ``ref_vector`` absent and ``ref_channel`` -1: no reference scaling."""
    d, n = _complex(rtf), _complex(psd_n)
    if diagonal_loading:
        n = _loaded(n, diag_eps)
    numerator = torch.linalg.solve(n, d.unsqueeze(-1)).squeeze(-1)
    denominator = torch.einsum('...d,...d->...', d.conj(), numerator)
    w = numerator / (denominator.real.unsqueeze(-1) + eps)
    if not _beamform.absent(ref_vector):
        w = w * torch.einsum('...c,...c->...', d.conj(), ref_vector.to(d.dtype)[..., None, :]).unsqueeze(-1)
    elif ref_channel >= 0:
        w = w * d[..., ref_channel].conj().unsqueeze(-1)
    return torch.view_as_real(w.contiguous())


def rtf_mvdr(specgram, rtf, psd_n, ref_vector, ref_channel, diagonal_loading=True, diag_eps=1e-7, eps=1e-8):
    """the ``RTFMVDR`` layer: the RTF weights, applied"""
    return apply_beamforming(mvdr_weights_rtf(rtf, psd_n, ref_vector, ref_channel, diagonal_loading, diag_eps, eps), specgram)


def fftconvolve(x, y, n_fft=0):
    """torchaudio's ``functional.fftconvolve`` in ``'full'`` mode: the one-shot form, ``irfft(rfft(x, n) * rfft(y, n), n)`` at
    ``n = L + M - 1`` along the last dimension, the leading dimensions broadcast.  ``n_fft`` (the partition size of the gfx950
    route) has no meaning here."""
    n = x.shape[-1] + y.shape[-1] - 1
    out = torch.fft.irfft(torch.fft.rfft(x, n=n, dim=-1) * torch.fft.rfft(y, n=n, dim=-1), n=n, dim=-1)
    return out.contiguous()


def cmn_check(cmn_window, min_cmn_window):
    """The ``ValueError`` cases of ``sliding_window_cmn``'s window arguments, shared by the functional and the layer"""
    if cmn_window < 1:
        raise ValueError('sliding_window_cmn: cmn_window must be at least 1, got %d' % cmn_window)
    if min_cmn_window < 1:
        raise ValueError('sliding_window_cmn: min_cmn_window must be at least 1, got %d' % min_cmn_window)


def cmn_bounds(n_frames, cmn_window, min_cmn_window, center, device=None):
    """(ws, we): int64 ``(T,)`` tensors, the window ``[ws, we)`` of every frame of ``sliding_window_cmn`` — the closed form of
    Kaldi's step-by-step procedure (``cmn_bounds`` of csrc/cmn_deltas.hip)."""
    # a window beyond the row, or a minimum beyond twice the row, gives the bounds of that cap: no int64 sum can overflow
    cmn_window, min_cmn_window = min(cmn_window, max(n_frames, 1)), min(min_cmn_window, 2 * max(n_frames, 1))
    t = torch.arange(n_frames, dtype=torch.int64, device=device)
    if center:
        ws = (t - cmn_window // 2).clamp(min=0).clamp(max=max(n_frames - cmn_window, 0))
        we = (ws + cmn_window).clamp(max=n_frames)
    else:
        ws = (t - cmn_window).clamp(min=0)
        we = (t + 1).clamp(min=min_cmn_window)
        over = (we - n_frames).clamp(min=0)
        ws = (ws - over).clamp(min=0)
        we = we - over
    return ws, we


def sliding_window_cmn(x, cmn_window, min_cmn_window, center, norm_vars):
    """torchaudio's ``functional.sliding_window_cmn`` over ``(…, T, F)``, all frames at once: the sums of every window are
    differences of a float64 ``cumsum`` gathered at the closed-form bounds (no loop over frames, no running sum in the input's
    dtype), the subtraction and the variance are float64 and the result is rounded to the input's dtype once.  The sums run over
    the finite samples; a cumulative count of the non-finite ones makes exactly the frames whose window holds one NaN, as the
    kernel does."""
    n_frames = x.shape[-2]
    if x.numel() == 0:
        return torch.zeros_like(x, memory_format=torch.contiguous_format)
    ws, we = cmn_bounds(n_frames, cmn_window, min_cmn_window, center, x.device)
    wide = x.to(torch.float64)
    finite = torch.isfinite(wide)
    clean = torch.where(finite, wide, torch.zeros((), dtype=wide.dtype, device=x.device))

    def window_sums(v):
        c = TF.pad(v.cumsum(-2), (0, 0, 1, 0))
        return c.index_select(-2, we) - c.index_select(-2, ws)

    n = (we - ws).to(torch.float64).unsqueeze(-1)
    mean = window_sums(clean) / n
    out = clean - mean
    if norm_vars:
        # a window of one frame gives exactly 0: its variance (0) is masked BEFORE the power, so that the unselected branch
        # does not send 0 * inf = NaN into the gradient
        single = n == 1.0
        var = window_sums(clean * clean) / n - mean * mean
        var = torch.where(single, torch.ones((), dtype=wide.dtype, device=x.device), var)
        out = torch.where(single, torch.zeros((), dtype=wide.dtype, device=x.device), out * var.pow(-0.5))
    bad = window_sums((~finite).to(torch.int64)) > 0
    out = torch.where(bad, torch.full((), float('nan'), dtype=wide.dtype, device=x.device), out)
    return out.to(x.dtype).contiguous()


DELTAS_MODES = ('replicate', 'constant', 'reflect', 'circular')


def deltas_check_args(win_length, mode):
    """The ``ValueError`` cases of ``compute_deltas`` that do not depend on the input, shared by the functional and the layer"""
    if win_length < 3:
        raise ValueError('compute_deltas: win_length must be at least 3, got %d' % win_length)
    if mode not in DELTAS_MODES:
        raise ValueError('compute_deltas: mode must be one of %s, got %r' % (', '.join(DELTAS_MODES), mode))


def deltas_check(n_frames, win_length, mode):
    """The ``ValueError`` cases of ``compute_deltas``, the same on every route; returns ``n = (win_length - 1) // 2``."""
    deltas_check_args(win_length, mode)
    n = (win_length - 1) // 2
    if mode == 'reflect' and n >= n_frames:
        raise ValueError("compute_deltas: mode='reflect' needs more than n = %d frames, got %d" % (n, n_frames))
    if mode == 'circular' and n > n_frames:
        raise ValueError("compute_deltas: mode='circular' needs at least n = %d frames, got %d" % (n, n_frames))
    return n


def deltas_index(n_frames, n, mode, device=None):
    """(idx, inside): for output frame t and tap k = -n .. n the source frame of ``torch.nn.functional.pad``'s ``mode`` —
    ``(T, 2n + 1)`` int64 — and whether the tap reads the row at all (False in the zero padding of ``'constant'``)"""
    pos = torch.arange(n_frames, dtype=torch.int64, device=device).unsqueeze(-1) + \
        torch.arange(-n, n + 1, dtype=torch.int64, device=device)
    inside = (pos >= 0) & (pos < n_frames)
    if mode == 'reflect':
        idx = torch.where(pos < 0, -pos, torch.where(pos >= n_frames, 2 * (n_frames - 1) - pos, pos))
    elif mode == 'circular':
        idx = torch.remainder(pos, max(n_frames, 1))
    else:
        idx = pos.clamp(0, max(n_frames - 1, 0))
    if mode != 'constant':
        inside = torch.ones_like(inside)
    return idx, inside


def compute_deltas(x, win_length, mode):
    """torchaudio's ``functional.compute_deltas`` over ``(…, F, T)`` as an index gather: ``sum_k k x[idx(t + k)] / denom`` with
    ``idx`` the index map of ``pad``'s ``mode``, accumulated in float64 and rounded to the input's dtype once.  Contiguous."""
    n_frames = x.shape[-1]
    n = deltas_check(n_frames, win_length, mode)
    if x.numel() == 0:
        return torch.zeros_like(x, memory_format=torch.contiguous_format)
    idx, inside = deltas_index(n_frames, n, mode, x.device)
    taps = torch.arange(-n, n + 1, dtype=torch.float64, device=x.device) * inside.to(torch.float64)      # (T, 2n + 1)
    gathered = x.to(torch.float64)[..., idx]                                                            # (…, F, T, 2n + 1)
    out = (gathered * taps).sum(-1) / (n * (n + 1) * (2 * n + 1) / 3.0)
    return out.to(x.dtype).contiguous()


_kaldi_constants = Bounded(32)


def mask_spans(x, spans, k_a, value):
    """SpecAugment's masks over ``(…, A, B)`` as sequential ``masked_fill``s: span ``s`` of ``spans`` (integer ``(R, k, 2)``, ``R`` 1 or
    the number of leading indices; the first ``k_a`` along A, the rest along B) fills ``[start, end)`` of its axis with ``value``
    (a number or a 0-dim tensor).  Returns a new contiguous tensor.  The CPU route of ``tac_amd::mask_spans`` and its announced
    composite route; what csrc/specaug.hip does in one launch."""
    lead = tuple(x.shape[:-2])
    k = int(spans.shape[-2])
    out = x.contiguous()
    if k == 0 or x.numel() == 0:
        return out.clone() if out is x else out
    per_row = spans.reshape((-1, k, 2)).to(x.device)
    per_row = per_row.reshape(lead + (k, 2)) if per_row.shape[0] != 1 or not lead else per_row.reshape((1,) * len(lead) + (k, 2))
    index = (torch.arange(x.shape[-2], device=x.device).view(-1, 1), torch.arange(x.shape[-1], device=x.device).view(1, -1))
    for s in range(k):
        i = index[0 if s < k_a else 1]
        start, end = per_row[..., s, 0, None, None], per_row[..., s, 1, None, None]
        out = out.masked_fill((i >= start) & (i < end), value)
    return out


def add_noise(waveform, noise, snr, lengths=None):
    """torchaudio's ``functional.add_noise`` in torch operators, in the inputs' dtype: with ``m_t = t < lengths`` (all ones without
    ``lengths``), ``E_s = sum_t (waveform_t m_t)^2``, ``E_n = sum_t (noise_t m_t)^2``, ``scale = 10 ** ((10 (log10 E_s - log10 E_n) - snr) /
    20)`` and ``out = waveform + scale * noise`` at EVERY sample.  Leading dimensions broadcast.  The masked samples are selected out
    (``torch.where``), as the kernel leaves them unread: a NaN behind a row's length does not reach its scale.  The CPU
    route of ``tac_amd::add_noise`` and its announced composite route; what csrc/add_noise.hip does in three launches."""
    if lengths is not None:
        mask = torch.arange(waveform.shape[-1], device=waveform.device) < lengths.unsqueeze(-1)
        masked_waveform = torch.where(mask, waveform, torch.zeros((), dtype=waveform.dtype, device=waveform.device))
        masked_noise = torch.where(mask, noise, torch.zeros((), dtype=noise.dtype, device=noise.device))
    else:
        masked_waveform, masked_noise = waveform, noise
    energy_signal = (masked_waveform * masked_waveform).sum(-1)
    energy_noise = (masked_noise * masked_noise).sum(-1)
    scale = 10 ** ((10 * (torch.log10(energy_signal) - torch.log10(energy_noise)) - snr) / 20)
    return (waveform + scale.unsqueeze(-1) * noise).contiguous()


def _kaldi_tables(p, w, n, dtype, device):
    """(window (W,), bank (bins, n // 2)) of ``_kaldi`` — built in float64, rounded once — cached per argument set; no bank for
    ``SpectrogramParams``"""
    bins = getattr(p, 'num_mel_bins', None)
    band = (bins, p.sample_frequency, p.low_freq, p.high_freq) if bins is not None else None
    key = (p.window_type, p.blackman_coeff, w, n, band, dtype, str(device))
    hit = _kaldi_constants.get(key)
    if hit is None:
        with torch.inference_mode(False):
            window = _kaldi.window64(p.window_type, w, p.blackman_coeff).to(dtype).to(device)
            bank = None
            if bins is not None:
                bank = _kaldi.mel_bank64(bins, n, p.sample_frequency, p.low_freq, p.high_freq)[:, :-1]
                bank = bank.to(dtype).to(device)
        hit = _kaldi_constants[key] = (window, bank)
    return hit


def _kaldi_spectrum(work, p, w, s, n, m, window):
    """The steps ``kaldi_fbank``, ``kaldi_mfcc`` and ``kaldi_spectrogram`` share, on ``(…, time)`` with ``m >= 1`` frames:
    frames (an ``unfold`` view, or a gather through the mirrored index with ``snip_edges=False``), dither, mean removal (the
    sum accumulated in float64, rounded once), energy, pre-emphasis with the first sample replicated, window, ``rfft`` at ``N``
    points.  Returns (``|rfft|`` (…, m, n // 2 + 1), the log energy (…, m) before its floor, the floor under the logarithms)."""
    length = work.shape[-1]
    if p.snip_edges:
        frames = work.unfold(-1, w, s)
    else:
        frames = work[..., _kaldi.mirror_index(length, w, s, m).to(work.device)]
    if p.dither != 0.0:
        frames = frames + p.dither * torch.randn_like(frames)
    if p.remove_dc_offset:
        frames = frames - (frames.sum(-1, keepdim=True, dtype=torch.float64) / w).to(frames.dtype)
    floor = torch.tensor(_kaldi.EPS, dtype=work.dtype, device=work.device)

    def log_energy(f):
        return torch.maximum(f.pow(2).sum(-1), floor).log()

    energy = log_energy(frames) if p.raw_energy else None
    if p.preemphasis_coefficient != 0.0:
        frames = frames - p.preemphasis_coefficient * torch.cat([frames[..., :1], frames[..., :-1]], -1)
    frames = frames * window
    if energy is None:
        energy = log_energy(frames)
    return torch.fft.rfft(frames, n=n, dim=-1).abs(), energy, floor


def _kaldi_floored_energy(energy, p):
    if p.energy_floor > 0.0:
        energy = torch.maximum(energy, torch.tensor(math.log(p.energy_floor), dtype=energy.dtype, device=energy.device))
    return energy


def kaldi_fbank(wave, *args):
    """torchaudio's ``compliance.kaldi.fbank`` over ``(…, time)`` in torch operators, step by step as ``_kaldi`` defines it:
    the frames' spectra (``_kaldi_spectrum``), the bank over the bins below the last one, the floored logarithm, the energy
    column, the mean over frames."""
    p = _kaldi.Params(*args)
    w, s, n = _kaldi.check(p)
    work = wave if wave.dtype in (torch.float32, torch.float64) else wave.float()
    length = work.shape[-1]
    m = _kaldi.num_frames(length, w, s, p.snip_edges)
    cols = p.num_mel_bins + (1 if p.use_energy else 0)
    if m == 0 or work.numel() == 0:
        return wave.new_zeros(tuple(wave.shape[:-1]) + (m, cols))
    window, bank = _kaldi_tables(p, w, n, work.dtype, work.device)
    spec, energy, floor = _kaldi_spectrum(work, p, w, s, n, m, window)
    spec = spec[..., :n // 2]
    if p.use_power:
        spec = spec.pow(2.0)
    out = torch.matmul(spec, bank.t())
    if p.use_log_fbank:
        out = torch.maximum(out, floor).log()
    if p.use_energy:
        energy = _kaldi_floored_energy(energy, p)
        out = torch.cat([out, energy.unsqueeze(-1)] if p.htk_compat else [energy.unsqueeze(-1), out], -1)
    if p.subtract_mean:
        out = out - out.mean(dim=-2, keepdim=True)
    out = out.contiguous()
    return out if out.dtype == wave.dtype else out.to(wave.dtype)


def kaldi_mfcc(wave, *args):
    """torchaudio's ``compliance.kaldi.mfcc`` over ``(…, time)`` in torch operators: the log-mel rows as ``kaldi_fbank`` makes
    them, times ``_kaldi.mfcc_table64`` (DCT-II, lifter, HTK's sqrt 2), the energy in place of C0, the HTK column order, the
    mean over frames."""
    p = _kaldi.MfccParams(*args)
    w, s, n = _kaldi.check(p, 'kaldi_mfcc')
    work = wave if wave.dtype in (torch.float32, torch.float64) else wave.float()
    m = _kaldi.num_frames(work.shape[-1], w, s, p.snip_edges)
    if m == 0 or work.numel() == 0:
        return wave.new_zeros(tuple(wave.shape[:-1]) + (m, p.num_ceps))
    window, bank = _kaldi_tables(p, w, n, work.dtype, work.device)
    spec, energy, floor = _kaldi_spectrum(work, p, w, s, n, m, window)
    logmel = torch.maximum(torch.matmul(spec[..., :n // 2].pow(2.0), bank.t()), floor).log()
    with torch.inference_mode(False):
        table = _kaldi.mfcc_table64(p).to(work.dtype).to(work.device)
    out = torch.matmul(logmel, table)
    if p.use_energy:
        out = torch.cat([_kaldi_floored_energy(energy, p).unsqueeze(-1), out[..., 1:]], -1)
    if p.htk_compat:
        out = torch.cat([out[..., 1:], out[..., :1]], -1)
    if p.subtract_mean:
        out = out - out.mean(dim=-2, keepdim=True)
    out = out.contiguous()
    return out if out.dtype == wave.dtype else out.to(wave.dtype)


def kaldi_spectrogram(wave, *args):
    """torchaudio's ``compliance.kaldi.spectrogram`` over ``(…, time)`` in torch operators: the floored logarithm of every bin
    of the power spectrum, the Nyquist bin included, the log energy in place of the DC bin, the mean over frames."""
    p = _kaldi.SpectrogramParams(*args)
    w, s, n = _kaldi.check(p, 'kaldi_spectrogram')
    work = wave if wave.dtype in (torch.float32, torch.float64) else wave.float()
    m = _kaldi.num_frames(work.shape[-1], w, s, p.snip_edges)
    if m == 0 or work.numel() == 0:
        return wave.new_zeros(tuple(wave.shape[:-1]) + (m, n // 2 + 1))
    window, _ = _kaldi_tables(p, w, n, work.dtype, work.device)
    spec, energy, floor = _kaldi_spectrum(work, p, w, s, n, m, window)
    out = torch.maximum(spec.pow(2.0), floor).log()
    out = torch.cat([_kaldi_floored_energy(energy, p).unsqueeze(-1), out[..., 1:]], -1)
    if p.subtract_mean:
        out = out - out.mean(dim=-2, keepdim=True)
    out = out.contiguous()
    return out if out.dtype == wave.dtype else out.to(wave.dtype)


def amplitude_to_db(x, ref, amin):
    """reference functional.py:291-296: the input is squared, the square clamped, then 10·(log10 − log10 ref)."""
    floor_applied = (x ** 2.0).clamp(min=amin)
    ref_level = torch.log10(torch.tensor(ref, dtype=x.dtype, device=x.device))
    return 10.0 * (floor_applied.log10() - ref_level)


def db_to_amplitude(x, ref):
    """reference functional.py:312-314."""
    ref_level = torch.log10(torch.tensor(ref, dtype=x.dtype, device=x.device))
    return torch.pow(10.0, x / 10.0 + ref_level) ** 0.5


def spectrogram(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided, power, db, ref, amin):
    """reference layers.py:267-304 (+ :350-381 when db)."""
    out = complex_norm(stft(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided), power)
    return amplitude_to_db(out, ref, amin) if db else out


def melspectrogram(wave, window, bank, n_fft, hop, win_length, center, pad_mode, normalized, onesided, power, db,
                   ref, amin):
    """reference layers.py:307-347 (+ :350-381 when db)."""
    out = apply_filterbank(
        complex_norm(stft(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided), power), bank)
    return amplitude_to_db(out, ref, amin) if db else out


def mu_law_encoding(x, n_quantize):
    """reference functional.py:329-335."""
    if not x.is_floating_point():
        x = x.to(torch.float)
    mu = torch.tensor(n_quantize - 1, dtype=x.dtype)            # a 0-dim host tensor, as in the reference
    squashed = torch.sign(x) * torch.log1p(mu * torch.abs(x)) / torch.log1p(mu)
    return ((squashed + 1) / 2 * mu + 0.5).to(torch.int64)


def mu_law_decoding(codes, n_quantize, dtype):
    """reference functional.py:348-354."""
    if not codes.is_floating_point():
        codes = codes.to(dtype)
    mu = torch.tensor(n_quantize - 1, dtype=codes.dtype)
    unit = codes / mu * 2 - 1.
    return torch.sign(unit) * (torch.exp(torch.abs(unit) * torch.log1p(mu)) - 1.) / mu


def phase_vocoder(spec, rate, phase_advance):
    """reference functional.py:233-274: pick the two frames around every fractional time step, interpolate the
    magnitudes, accumulate the wrapped phase increments."""
    n_frames = spec.shape[-2]
    t = torch.arange(0, n_frames, rate, device=spec.device)      # default dtype, as the reference evaluates it
    frac = t % 1.0
    phase0 = angle(spec[..., :1, :])
    tail_padded = TF.pad(spec, [0, 0, 0, 2])
    left = tail_padded.index_select(-2, t.long())
    right = tail_padded.index_select(-2, (t + 1).long())
    ang_l, ang_r = angle(left), angle(right)
    len_l, len_r = left.norm(dim=-1), right.norm(dim=-1)
    step = ang_r - ang_l - phase_advance
    step = step - TWO_PI * torch.round(step / TWO_PI)
    step = step + phase_advance
    step = torch.cat([phase0, step[..., :-1]], dim=-1)
    running = step.cumsum(-1)
    length = frac * len_r + (1 - frac) * len_l
    return torch.stack([length * running.cos(), length * running.sin()], dim=-1)


def stretch_norm(mag, rate, power, db, ref, amin):
    """``complex_norm(phase_vocoder(X, rate, phase_advance), power)`` from ``mag = |X|`` alone (reference functional.py:233-274
    followed by :126-128): the vocoder returns ``(length cos phi, length sin phi)`` with ``length = frac |X[t1]| + (1 - frac) |X[t0]|``,
    whose norm is ``length`` whatever ``phi`` is — the running phase, ``phase_advance``, the wrap and the cumulative sum cancel.
    What does not cancel is how the reference loses values: a NaN component has a NaN angle, which the cumulative sum carries into
    every later frame of its bin (an infinite magnitude has a finite angle and stays where it is interpolated)."""
    n_frames = mag.shape[-1]
    t = torch.arange(0, n_frames, rate, device=mag.device)       # default dtype, as the reference evaluates it
    frac = t % 1.0
    tail_padded = TF.pad(mag, [0, 2])
    len_l = tail_padded.index_select(-1, t.long())
    len_r = tail_padded.index_select(-1, (t + 1).long())
    length = frac * len_r + (1 - frac) * len_l
    out = length if power == 1.0 else length.pow(power)
    lost = (len_l.isnan() | len_r.isnan()).cumsum(-1) > 0
    out = torch.where(lost, torch.full((), float('nan'), dtype=out.dtype, device=out.device), out)
    return amplitude_to_db(out, ref, amin) if db else out


def stretch_mel(mag, bank, rate, power, db, ref, amin):
    """``stretch_norm`` followed by reference functional.py:183-184 (+ :291-296 when db)."""
    out = apply_filterbank(stretch_norm(mag, rate, power, False, 1.0, 1e-7), bank)
    return amplitude_to_db(out, ref, amin) if db else out


def hpss(mag, kernel_f, kernel_t, power, hard):
    """reference beta_hpss.py:104-127 without its Python loops: reflect-pad both axes, running medians along frequency
    (percussive) and time (harmonic) as ``unfold(...).median``, ``pow``, soft / hard masks.  Masks come back as floats
    (the wrapper turns hard masks into bool like the reference)."""
    shape = mag.shape
    x = mag.reshape((-1, 1) + tuple(shape[-2:]))
    hf, ht = kernel_f // 2, kernel_t // 2
    padded = TF.pad(x, (ht, ht, hf, hf), mode='reflect')
    n_freqs, n_frames = shape[-2], shape[-1]
    # (an even width leaves n + 1 windows over the n + 2 (k // 2) padded positions; the reference's loops take the
    # first n, beta_hpss.py:84-91)
    perc = padded[..., ht:ht + n_frames].unfold(-2, kernel_f, 1)[..., :n_freqs, :, :].median(dim=-1).values
    harm = padded[..., hf:hf + n_freqs, :].unfold(-1, kernel_t, 1)[..., :n_frames, :].median(dim=-1).values
    if power != 1.0:
        perc, harm = perc.pow(power), harm.pow(power)
    if hard:
        mask_h, mask_p = (harm > perc).to(mag.dtype), (harm < perc).to(mag.dtype)
    else:
        eps = 1e-6
        mask_h = (harm + eps) / (harm + perc + eps)
        mask_p = (perc + eps) / (harm + perc + eps)
    mask_h, mask_p = mask_h.reshape(shape), mask_p.reshape(shape)
    return mag * mask_h, mag * mask_p, mask_h, mask_p


def melspectrogram_mulaw(codes, window, bank, n_quantize, n_fft, hop, win_length, center, pad_mode, normalized, onesided,
                         power, db, ref, amin):
    """reference functional.py:338-354 followed by layers.py:307-381: decode, then the Melspectrogram chain."""
    wave = mu_law_decoding(codes, n_quantize, torch.float32)
    return melspectrogram(wave, window, bank, n_fft, hop, win_length, center, pad_mode, normalized, onesided, power, db,
                          ref, amin)


# ----------------------------------------------------------------------------- rnnt_loss
def _rnnt_work(logits):
    return logits.float() if logits.dtype in (torch.float16, torch.bfloat16) else logits


def rnnt_valid(logits, targets, logit_lengths, target_lengths):
    """``(ok, Tb, Ub)``: which entries of the batch have ``1 <= Tb <= T``, ``0 <= Ub <= U`` and every used target inside ``[0, V)``
    — the others get a NaN cost and gradient — and the lengths clamped into those ranges, so that no index leaves the tensors.
    On the device of the inputs: nothing waits for the host."""
    B, T, U1, V = logits.shape
    U = U1 - 1
    Tb, Ub = logit_lengths.long(), target_lengths.long()
    ok = (Tb >= 1) & (Tb <= T) & (Ub >= 0) & (Ub <= U)
    if U:
        used = torch.arange(U, device=logits.device)[None, :] < Ub[:, None]
        ok = ok & ~(used & ((targets < 0) | (targets >= V))).any(dim=1)
    return ok, Tb.clamp(1, T), Ub.clamp(0, U)


def _rnnt_logaddexp(a, b):
    """``logaddexp`` from operators whose every derivative is finite at the finite "no path" value (``torch.logaddexp``'s second
    derivative is not)"""
    m = torch.maximum(a, b).detach()
    return m + torch.log(torch.exp(a - m) + torch.exp(b - m))


def _rnnt_skew(x, t_of, on):
    """``(B, T, U + 1)`` → ``(B, T + U, U + 1)`` with ``[b, d, u] = x[b, d - u, u]``, ``-1e30`` (no path) where ``d - u`` is no frame"""
    got = x.gather(1, t_of.expand(x.shape[0], -1, -1))
    return torch.where(on, got, torch.full((), -1e30, dtype=x.dtype, device=x.device))


def rnnt_loss(logits, targets, logit_lengths, target_lengths, blank, clamp, fused_log_softmax):
    """torchaudio's ``functional.rnnt_loss`` before its reduction, in torch operators: ``(costs, alphas, betas, denominators)`` of
    ``(B, T, U + 1, V)`` logits.  The recursion of Graves (2012) in log-space, one step of the Python loop per anti-diagonal
    ``t + u = d`` (``T + U`` steps for alpha and as many for beta), the whole batch at once with the lengths as masks; every step is
    a differentiable torch operator.  Cells with ``t >= Tb`` or ``u > Ub`` come back as zeros; an entry ``rnnt_valid`` refuses as
    NaN.  ``clamp`` acts on the gradient alone (``rnnt_loss_grad``)."""
    x = _rnnt_work(logits)
    B, T, U1, V = x.shape
    U, D = U1 - 1, T + U1 - 1
    dev = x.device
    # "no path" is a large finite number, not -inf: logaddexp(-inf, -inf) has a NaN derivative, and autograd visits the masked cells
    ninf = torch.full((), -1e30, dtype=x.dtype, device=dev)
    ok, Tb, Ub = rnnt_valid(x, targets, logit_lengths, target_lengths)
    denom = torch.logsumexp(x, dim=-1) if fused_log_softmax else x.new_zeros((B, T, U1))
    lpb = x[..., blank] - denom
    if U:
        lab = targets.long().clamp(0, V - 1)[:, None, :, None].expand(B, T, U, 1)
        lpl = torch.cat([x[:, :, :U].gather(-1, lab).squeeze(-1) - denom[:, :, :U], ninf.expand(B, T, 1)], dim=2)
    else:
        lpl = ninf.expand(B, T, 1)
    d_i = torch.arange(D, device=dev)[:, None]
    u_i = torch.arange(U1, device=dev)[None, :]
    t_of = d_i - u_i                                                  # (D, U1): the frame of column u on diagonal d
    on = (t_of >= 0) & (t_of < T)
    t_cl = t_of.clamp(0, T - 1)[None]
    sb, sl = _rnnt_skew(lpb, t_cl, on[None]), _rnnt_skew(lpl, t_cl, on[None])
    pad = ninf.expand(B, 1)
    # alpha does not depend on the lengths: the whole grid, read at (Tb - 1, Ub)
    row = torch.cat([x.new_zeros((B, 1)), ninf.expand(B, U)], dim=1) if U else x.new_zeros((B, 1))
    rows = [row]
    for d in range(1, D):
        up = row + sb[:, d - 1]
        left = torch.cat([pad, row[:, :-1] + sl[:, d - 1, :-1]], dim=1)
        row = torch.where(on[d][None], _rnnt_logaddexp(up, left), ninf)
        rows.append(row)
    unskew = (torch.arange(T, device=dev)[:, None] + u_i)[None].expand(B, -1, -1)
    alphas = torch.stack(rows, dim=1).gather(1, unskew)
    last = ((Tb - 1) * U1 + Ub)[:, None]
    costs = -(alphas.reshape(B, -1).gather(1, last) + lpb.reshape(B, -1).gather(1, last)).squeeze(1)
    # beta ends at (Tb - 1, Ub) of its entry
    t_b, u_b = t_of[None], u_i[None]
    corner = (t_b == (Tb - 1)[:, None, None]) & (u_b == Ub[:, None, None])
    inside = on[None] & (t_b < Tb[:, None, None]) & (u_b <= Ub[:, None, None])
    row = ninf.expand(B, U1)
    rows = [None] * D
    for d in range(D - 1, -1, -1):
        down = row + sb[:, d]
        right = torch.cat([row[:, 1:], pad], dim=1) + sl[:, d]
        row = torch.where(corner[:, d], sb[:, d], torch.where(inside[:, d], _rnnt_logaddexp(down, right), ninf))
        rows[d] = row
    betas = torch.stack(rows, dim=1).gather(1, unskew)
    t_i = torch.arange(T, device=dev)[None, :, None]
    cell = (t_i < Tb[:, None, None]) & (u_i[None] <= Ub[:, None, None])
    nan = torch.full((), float('nan'), dtype=x.dtype, device=dev)
    zero = x.new_zeros(())
    keep = ok[:, None, None]
    alphas, betas = (torch.where(keep, torch.where(cell, a, zero), nan) for a in (alphas, betas))
    denom = torch.where(cell & keep, denom, zero)
    costs = torch.where(ok, costs, nan)
    return costs.to(logits.dtype), alphas, betas, denom


def rnnt_loss_grad(logits, targets, logit_lengths, target_lengths, alphas, betas, denominators, costs, grad_costs, blank, clamp,
                   fused_log_softmax):
    """the gradient of ``rnnt_loss``'s costs with respect to the logits in closed form, from what the forward pass saved: with
    ``g = logits - denominators + alphas + costs``, ``exp(g + beta[t,u])`` minus the blank term ``exp(g + beta[t+1,u])`` (``exp(g)``
    at the last cell) and the label term ``exp(g + beta[t,u+1])``; clipped to ``[-clamp, clamp]`` where ``clamp > 0``, then times
    ``grad_costs``.  Not differentiable itself (the double backward differentiates ``rnnt_loss``)."""
    x = _rnnt_work(logits).detach()
    B, T, U1, V = x.shape
    U = U1 - 1
    dev = x.device
    ninf = torch.full((), float('-inf'), dtype=x.dtype, device=dev)
    zero = x.new_zeros(())
    ok, Tb, Ub = rnnt_valid(x, targets, logit_lengths, target_lengths)
    Tb_, Ub_ = Tb[:, None, None], Ub[:, None, None]
    t_i = torch.arange(T, device=dev)[None, :, None]
    u_i = torch.arange(U1, device=dev)[None, None, :]
    cell = (t_i < Tb_) & (u_i <= Ub_)
    alphas, betas, denominators = alphas.to(x.dtype), betas.to(x.dtype), denominators.to(x.dtype)
    c = (alphas + costs.to(x.dtype)[:, None, None]) - denominators
    below = torch.cat([betas[:, 1:], ninf.expand(B, 1, U1)], dim=1)
    sb = torch.where(t_i < Tb_ - 1, below, torch.where(u_i == Ub_, zero, ninf))
    beside = torch.cat([betas[:, :, 1:], ninf.expand(B, T, 1)], dim=2)
    sl = torch.where(u_i < Ub_, beside, ninf)
    g = x + c[..., None]
    grad = torch.exp(g + betas[..., None]) if fused_log_softmax else torch.zeros_like(x)
    grad[..., blank] -= torch.exp(g[..., blank] + sb)
    if U:
        lab = targets.long().clamp(0, V - 1)[:, None, :, None].expand(B, T, U, 1)
        grad[:, :, :U].scatter_add_(-1, lab, -torch.exp(g[:, :, :U].gather(-1, lab) + sl[:, :, :U, None]))
    grad = torch.where(cell[..., None], grad, zero)
    if clamp > 0:
        grad = grad.clamp(-clamp, clamp)
    grad = grad * grad_costs.to(x.dtype)[:, None, None, None]
    grad = torch.where(ok[:, None, None, None], grad, torch.full((), float('nan'), dtype=x.dtype, device=dev))
    return grad.to(logits.dtype)


# ----------------------------------------------------------------------------- forced_align
def align_valid(log_probs, targets, input_lengths, target_lengths, blank):
    """``(ok, Tb, Lb, lab)``: which entries have ``1 <= Tb <= T``, ``0 <= Lb <= L``, every used target inside ``[0, C)`` and not the
    blank, and ``Tb >= Lb + repeats`` — the others end as ``-1`` / NaN — with the lengths and labels clamped into their ranges, so
    that no index leaves the tensors.  On the device of the inputs: nothing waits for the host."""
    B, T, C = log_probs.shape
    L = targets.shape[1]
    dev = log_probs.device
    Tb = torch.full((B,), T, dtype=torch.long, device=dev) if input_lengths is None else input_lengths.long()
    Lb = torch.full((B,), L, dtype=torch.long, device=dev) if target_lengths is None else target_lengths.long()
    ok = (Tb >= 1) & (Tb <= T) & (Lb >= 0) & (Lb <= L)
    tg = targets.long()
    if L:
        used = torch.arange(L, device=dev)[None, :] < Lb[:, None]
        ok = ok & ~(used & ((tg < 0) | (tg >= C) | (tg == blank))).any(dim=1)
        repeats = (used[:, 1:] & (tg[:, 1:] == tg[:, :-1])).sum(dim=1)
        ok = ok & (Tb >= Lb + repeats)
    return ok, Tb.clamp(1, T), Lb.clamp(0, L), tg.clamp(0, C - 1)


def forced_align(log_probs, targets, input_lengths, target_lengths, blank):
    """torchaudio's ``functional.forced_align`` without its state window, for any batch, in torch operators: ``(paths, scores)`` of
    ``(B, T, C)`` log-probabilities.  All states and the whole batch at once, one step of the Python loop per frame for the
    recursion and one for the backtrack; the predecessor is chosen by ``torch.where`` on strict comparisons (back-pointer 2 if
    ``x2 > x1 and x2 > x0``, else 1 if ``x1 > x0 and x1 > x2``, else 0), never by a maximum, and every alpha is one addition in the
    dtype of ``log_probs``.  Frames ``t >= Tb`` come back as blank and 0; an entry ``align_valid`` refuses as ``-1`` and NaN."""
    B, T, C = log_probs.shape
    L = targets.shape[1]
    S = 2 * L + 1
    dev = log_probs.device
    ok, Tb, Lb, lab = align_valid(log_probs, targets, input_lengths, target_lengths, blank)
    ext = torch.full((B, S), blank, dtype=torch.long, device=dev)           # the label of every state
    ext[:, 1::2] = lab
    em = log_probs.detach().gather(2, ext[:, None, :].expand(B, T, S))
    ninf = torch.full((), float('-inf'), dtype=em.dtype, device=dev)
    skip = torch.zeros((B, S), dtype=torch.bool, device=dev)
    if L > 1:
        skip[:, 3::2] = lab[:, 1:] != lab[:, :-1]
    alpha = ninf.expand(B, S).clone()
    alpha[:, :2] = em[:, 0, :2]
    final = alpha
    pad1, pad2 = ninf.expand(B, 1), ninf.expand(B, 2)
    two, one, zero = (torch.full((), v, dtype=torch.long, device=dev) for v in (2, 1, 0))
    bps = [None]
    for t in range(1, T):
        x0 = alpha
        x1 = torch.cat([pad1, alpha[:, :-1]], dim=1)
        x2 = torch.where(skip, torch.cat([pad2, alpha[:, :-2]], dim=1)[:, :S], ninf)
        c2 = (x2 > x1) & (x2 > x0)
        c1 = ~c2 & (x1 > x0) & (x1 > x2)
        bps.append(torch.where(c2, two, torch.where(c1, one, zero)))
        alpha = torch.where(c2, x2, torch.where(c1, x1, x0)) + em[:, t]
        final = torch.where((Tb == t + 1)[:, None], alpha, final)
    last = (2 * Lb)[:, None]
    before = (2 * Lb - 1).clamp(min=0)[:, None]
    s = torch.where((Lb >= 1)[:, None] & ~(final.gather(1, last) > final.gather(1, before)), before, last)
    states = torch.zeros((B, T), dtype=torch.long, device=dev)
    for t in range(T - 1, -1, -1):
        inside = (Tb > t)[:, None]
        states[:, t:t + 1] = s
        if t:
            s = torch.where(inside, s - bps[t].gather(1, s), s)
    frame = torch.arange(T, device=dev)[None, :] < Tb[:, None]
    paths = torch.where(frame, ext.gather(1, states), torch.full((), blank, dtype=torch.long, device=dev))
    scores = torch.where(frame, log_probs.gather(2, paths[:, :, None]).squeeze(2), log_probs.new_zeros(()))
    keep = ok[:, None]
    paths = torch.where(keep, paths, torch.full((), -1, dtype=torch.long, device=dev)).to(targets.dtype)
    scores = torch.where(keep, scores, torch.full((), float('nan'), dtype=scores.dtype, device=dev))
    return paths, scores


# ============================================================================= rir_ism, rir_ism_span
def _rir_geometry(room, source, mic_array, max_order, sound_speed, sample_rate):
    """float64 ``(X (I, D) int64, dist (B, I, M), delay (B, I, M), di (B, I, M) float64)`` of the image sources: the definition's
    steps 1 and 2, every product and sum a torch operator of its own"""
    from . import _rir
    D = room.shape[-1]
    X = _rir.images(max_order, D, room.device).to(torch.int64)
    r, s, m = room.double()[:, None, :], source.double()[:, None, :], mic_array.double()
    Xf = X.double()[None]
    loc = torch.where((X % 2 == 1)[None], r * (Xf + 1.0) - s, r * Xf + s)                       # (B, I, D)
    diff = loc[:, :, None, :] - m[:, None, :, :]                                                # (B, I, M, D)
    sq = diff[..., 0] * diff[..., 0]
    for d in range(1, D):
        sq = sq + diff[..., d] * diff[..., d]
    dist = torch.sqrt(sq)
    delay = dist * float(sample_rate) / float(sound_speed)
    return X, dist, delay, torch.ceil(delay)


def rir_ism(room, source, mic_array, absorption, max_order, start, length, delay_filter_length, sound_speed, sample_rate):
    """``(B, D)``, ``(B, D)``, ``(B, M, D)``, ``(B or 1, n_band, 2 D)`` → ``(B, n_band, M, length)``: samples ``[start, start + length)`` of the
    raw image-source responses, the definition of ``functional.simulate_rir_ism`` in torch operators — evaluated in float64
    whatever the inputs' dtype, summed with ``index_add_`` and rounded once (float32 unless an input is float64)."""
    out_dtype = torch.float64 if torch.float64 in (room.dtype, source.dtype, mic_array.dtype, absorption.dtype) else torch.float32
    B, D = room.shape
    M = mic_array.shape[1]
    nb = absorption.shape[1]
    P, L = delay_filter_length // 2, delay_filter_length
    X, dist, delay, di = _rir_geometry(room, source, mic_array, max_order, sound_speed, sample_rate)
    tr = torch.sqrt(1.0 - absorption.double())                                                  # (B or 1, nb, 2 D)
    e_lo = torch.div(X, 2, rounding_mode='floor').abs()
    e_hi = torch.div(X + 1, 2, rounding_mode='floor').abs()
    att = None
    for d in range(D):
        term = tr[:, :, None, 2 * d] ** e_lo[None, None, :, d].double() * tr[:, :, None, 2 * d + 1] ** e_hi[None, None, :, d].double()
        att = term if att is None else att * term                                               # (B or 1, nb, I)
    amp = att[:, :, :, None] / dist[:, None, :, :]                                              # (B, nb, I, M)
    f = di - delay
    mm = torch.arange(-P, P + 1, dtype=torch.float64, device=room.device)
    x = mm + f[..., None]                                                                       # (B, I, M, L)
    if P > 0:
        hann = torch.where(x.abs() <= P, 0.5 * (1.0 + torch.cos(TWO_PI * x / (2.0 * P))), torch.zeros_like(x))
    else:
        hann = torch.ones_like(x)
    w = torch.sinc(x) * hann
    vals = amp[..., None] * w[:, None]                                                          # (B, nb, I, M, L)
    # a non-finite delay (NaN inputs) has no sample to add to: it adds nothing
    fine = torch.isfinite(di) & (di < 4.0e18)
    pos = torch.where(fine, di, torch.zeros_like(di)).to(torch.int64)[..., None] + torch.arange(L, device=room.device) - start
    keep = fine[..., None] & (pos >= 0) & (pos < length)
    pos = torch.where(keep, pos, torch.full_like(pos, length))                                  # (the dropped taps: one spare sample a row)
    rows = (torch.arange(B, device=room.device)[:, None, None, None, None] * nb
            + torch.arange(nb, device=room.device)[None, :, None, None, None]) * M + torch.arange(M, device=room.device)[None, None, None, :, None]
    index = (rows * (length + 1) + pos[:, None]).reshape(-1)
    vals = torch.where(keep[:, None].expand_as(vals), vals, torch.zeros_like(vals))
    flat = torch.zeros(B * nb * M * (length + 1), dtype=torch.float64, device=room.device)
    flat = flat.index_add(0, index, vals.reshape(-1))
    return flat.reshape(B, nb, M, length + 1)[..., :length].to(out_dtype)


def rir_ism_span(room, source, mic_array, max_order, delay_filter_length, sound_speed, sample_rate):
    """int64 scalar on the inputs' device: ``max(delay_i) + L - P`` over the batch, the natural length of the responses"""
    _, _, _, di = _rir_geometry(room, source, mic_array, max_order, sound_speed, sample_rate)
    fine = torch.isfinite(di) & (di < 4.0e18)
    top = torch.where(fine, di, torch.zeros_like(di)).max().to(torch.int64)
    return top + (delay_filter_length - delay_filter_length // 2)


# ============================================================================= SoX effects with a loop over time
def overdrive(waveform, gain, colour):
    """torchaudio's ``functional.overdrive`` in elementwise torch operators around this package's ``lfilter`` (the recursion
    ``v[n] = t[n] - t[n-1] + 0.995 v[n-1]`` is a first-order filter): ``(…, time)`` → the same, in the input's dtype.  The CPU path
    of ``tac_amd::overdrive`` and its announced route on a device; differentiable."""
    from . import _ops, _sox
    if waveform.numel() == 0:
        return torch.zeros_like(waveform, memory_format=torch.contiguous_format)
    g, c = _sox.overdrive_constants(gain, colour)
    t = waveform * g + c
    t = torch.where(t < -1.0, torch.full_like(t, -2.0 / 3.0), torch.where(t > 1.0, torch.full_like(t, 2.0 / 3.0), t - t * t * t / 3.0))
    a = torch.tensor([1.0, -0.995], dtype=torch.float64)
    b = torch.tensor([1.0, -1.0], dtype=torch.float64)
    v = _ops.call('lfilter', t, a, b, False)
    return (waveform * 0.5 + v * 0.75).clamp(-1.0, 1.0).contiguous()


def phaser(waveform, mod, L, gain_in, gain_out, decay):
    """torchaudio's ``functional.phaser`` as the recursion ``y[n] = gain_in x[n] + decay y[n - d(n)]``, ``d(n) = L - mod[n % P] + 1``
    (the closed form of its ring buffer), one column per step.  ``mod``: the LFO table as a sequence of HOST integers, so the
    loop never reads the device.  In the input's dtype; differentiable; as slow as a loop over time is."""
    if waveform.numel() == 0:
        return torch.zeros_like(waveform, memory_format=torch.contiguous_format)
    x = waveform.reshape(-1, waveform.shape[-1]) * gain_in
    period = len(mod)
    cols = []
    for n, xn in enumerate(x.unbind(-1)):
        p = n - (L - mod[n % period] + 1)
        cols.append(xn + cols[p] * decay if p >= 0 else xn)
    y = torch.stack(cols, dim=-1) * gain_out
    return y.clamp(-1.0, 1.0).reshape(waveform.shape).contiguous()


def flanger(waveform, plan):
    """torchaudio's ``functional.flanger`` from a ``_sox.FlangerPlan``: ``(…, channel, time)`` → the same.  The ring buffer is a
    list of columns ``w[i] = x[i] + fb delayed[i-1]``; the LFO values, their floors and fractions are HOST floats, so the loop
    never reads the device.  In the input's dtype; differentiable."""
    if waveform.numel() == 0:
        return torch.zeros_like(waveform, memory_format=torch.contiguous_format)
    channels, length = waveform.shape[-2], waveform.shape[-1]
    x = waveform.reshape(-1, channels, length)
    lfo = plan.lfo.tolist()
    zero = torch.zeros_like(x[..., 0])
    w, outs = [], []
    last = zero
    for i, xi in enumerate(x.unbind(-1)):
        wi = xi + last * plan.fb
        w.append(wi)
        per_channel = []
        for c in range(channels):
            d = lfo[(i + plan.phases[c]) % plan.P]
            k = int(d)
            fr = d - k

            def tap(back):      # the ring wraps: `Lb` back is the sample just written
                back = back % plan.Lb
                return w[i - back][:, c] if i - back >= 0 else zero[:, c]
            d0, d1 = tap(k), tap(k + 1)
            if plan.quadratic:
                d2 = tap(k + 2) - d0
                e1 = d1 - d0
                per_channel.append(d0 + ((d2 * 0.5 - e1) * fr + (e1 * 2.0 - d2 * 0.5)) * fr)
            else:
                per_channel.append(d0 + (d1 - d0) * fr)
        last = torch.stack(per_channel, dim=-1)
        outs.append(xi * plan.in_gain + last * plan.delay_gain)
    y = torch.stack(outs, dim=-1).clamp(-1.0, 1.0)
    return y.reshape(waveform.shape).contiguous()
