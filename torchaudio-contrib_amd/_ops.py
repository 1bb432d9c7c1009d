"""``torch.library`` registration of the path: every functional of the reference's API is one PyTorch custom op in
the ``tac_amd`` namespace, so the dispatcher, ``torch.compile`` / FakeTensor tracing, autograd and the profiler
see them by name.

    op                      CUDA (= HIP on ROCm) kernel                 CPU kernel            Meta (fake)
    tac_amd::stft           gfx950 kernels through the C ABI (_hip.py)  stock torch ops       shapes + strides
    tac_amd::spectrogram        "      (STFT + |.|^p [+ dB] fused)      (_composite.py)
    tac_amd::melspectrogram     "      (the whole chain in ONE kernel)
    tac_amd::stretch_norm       complex_norm(phase_vocoder(X)) [+ dB] from |X| alone (csrc/stretch.hip)
    tac_amd::stretch_mel            "      + apply_filterbank in the same launch
    tac_amd::dct                rows times the cepstral matrix, the step behind the mel dB rows (csrc/mfcc.hip)
    tac_amd::resample           polyphase windowed-sinc resampling of the waveform (csrc/resample.hip)
    tac_amd::resample_fit       the same cut or zero-padded to a given length, for banks beyond the LDS too: pitch_shift's tail
    tac_amd::kaldi_fbank        Kaldi log mel filterbank features: framing, FFT, mel bank and log in one launch (csrc/kaldi_fbank.hip)
    tac_amd::kaldi_mfcc         Kaldi cepstra: the same launch with the DCT, lifter and energy substitution as its epilogue
    tac_amd::kaldi_spectrogram  Kaldi log power spectrogram: the same launch, every bin's logarithm, the energy as column 0
    tac_amd::sliding_window_cmn sliding-window cepstral mean (and variance) normalisation over (…, T, F) (csrc/cmn_deltas.hip)
    tac_amd::compute_deltas     delta coefficients along time over (…, F, T) (csrc/cmn_deltas.hip)
    tac_amd::mask_spans         SpecAugment: every time and frequency mask of a call over (…, F, T) in one launch (csrc/specaug.hip)
    tac_amd::add_noise          noise mixed into (…, L) at a signal-to-noise ratio, under a length mask (csrc/add_noise.hip)
    tac_amd::loudness           ITU-R BS.1770-4 gated loudness of (…, channels, L): K-weighting, blocks and gates (csrc/loudness.hip)
    tac_amd::detect_pitch_frequency   NCCF pitch of (…, L): correlations, peak choice and median in two launches (csrc/pitch.hip)
    tac_amd::vad_measures, vad_start   the SoX voice-activity detector of (…, L): measures and trim point behind one spectrogram launch (csrc/vad.hip)
    tac_amd::rir_ism, rir_ism_span   image-source room impulse responses of a batch of rooms: raw responses in one launch, and their natural length (csrc/rir.hip)
    tac_amd::psd, mvdr_weights_souden, apply_beamforming, mvdr_souden   mask-based MVDR beamforming over (…, C, F, T) (csrc/beamform.hip)
    tac_amd::rtf_evd, rtf_power, mvdr_weights_rtf, rtf_mvdr   steering vectors from the PSDs and the MVDR solved for one (csrc/beamform.hip)
    tac_amd::rnnt_loss, rnnt_loss_grad   transducer loss over (B, T, U + 1, V) logits: costs with alpha / beta, and the gradient (csrc/rnnt.hip)
    tac_amd::forced_align       CTC Viterbi alignment of (B, T, C) log-probabilities: recursion, backtrack, paths and scores in one launch (csrc/align.hip)
    tac_amd::griffinlim         Griffin-Lim phase recovery of (…, F, T) magnitudes: prepare, then stft + inverse a step (csrc/griffinlim.hip)
    tac_amd::fftconvolve        full convolution along time by partitioned overlap-save (csrc/fftconvolve.hip)
    tac_amd::lfilter            recursive filter of order <= 2 along time: biquads, pre- / de-emphasis (csrc/lfilter.hip)
    tac_amd::sosfilt            cascade of up to 8 second-order sections along time in one launch, float64 between them (csrc/sosfilt.hip)
    tac_amd::lfilter_reverse, sosfilt_reverse   the two above run from the end of each row: filtfilt's second half (private)
    tac_amd::overdrive, phaser, flanger         the SoX effects defined by a loop over time, one launch each (csrc/sox_effects.hip)
    tac_amd::apply_filterbank, complex_norm, angle, magphase, phase_vocoder, amplitude_to_db, db_to_amplitude,
    tac_amd::mu_law_encoding, mu_law_decoding                           likewise

Routing on a HIP device: float32 (and float16/bfloat16, widened as ``torch.stft`` widens half input) always runs
the hand-written kernels and raises if ``libtac_amd.so`` is missing.  float64 runs the float64 kernels of the STFT chain
(``_hip64.py`` -> csrc/chain_f64.hip) and of the phase vocoder.  What those do not cover (float64 mu-law / HPSS) and fft
sizes outside the kernels' range are evaluated by torch's own GPU operators
(``_composite.py``) with a one-time ``CompositeRouteWarning``; ``set_strict(True)`` turns that route into an error
(the GPU parity tests run strict, so nothing they check can have come from anywhere but the HIP kernels).

Autograd: stft / spectrogram / melspectrogram / apply_filterbank / complex_norm / amplitude_to_db have hand-written
gradient kernels for the signal path (csrc/backward.hip: inverse real FFT per frame + gather overlap-add, the
filterbank GEMM with the transposed bank, elementwise adjoints; the fused ops recompute their spectrum instead of
saving it).  Gradients w.r.t. the window / filterbank, float64, CPU tensors and the remaining ops differentiate by
re-evaluating the op with torch operators under ``enable_grad``.
"""
import math
import warnings

import torch
from torch.library import Library

from . import _composite as C
from . import _filters as FL
from . import _hip as H
from . import _hip64 as H64
from . import _kaldi as K
from . import _pitch as PT
from . import _vad as VD
from . import _beamform as BF
from . import _resample as RS
from . import _sox as SX

NS = 'tac_amd'
_lib = Library(NS, 'DEF')

_strict = False
_warned = set()
#: how many op calls took the stock-torch route, per (op, reason) — introspection for tests / users
composite_calls = {}


class CompositeRouteWarning(UserWarning):
    """An op was evaluated by stock torch operators instead of the gfx950 kernels (float64 input, unsupported size)."""


_strict_backward = None        # None: follow _strict


def set_strict(flag, backward=None):
    """With strict on, a tensor on a HIP device is never handed to the stock-torch route: the call raises instead.

    That covers backward passes as well: the gradient of an op without a gradient kernel (``phase_vocoder``, ``angle``,
    ``magphase``, ``hpss``, ``db_to_amplitude``), every float64 gradient and every double backward re-evaluate the op with
    stock torch operators, so under ``set_strict(True)`` they RAISE (since round 3; earlier rounds let a backward pass through
    when its forward had run on the kernels).  ``backward=False`` keeps strictness for forward calls only — those backward
    passes then run, announced by ``CompositeRouteWarning`` and counted in ``composite_calls``; ``backward=None`` (default)
    follows ``flag``."""
    global _strict, _strict_backward
    _strict = bool(flag)
    _strict_backward = None if backward is None else bool(backward)


def strict():
    return _strict


def strict_backward():
    return _strict if _strict_backward is None else _strict_backward


def _composite_route(op, reason):
    composite_calls[(op, reason)] = composite_calls.get((op, reason), 0) + 1
    if strict_backward() if reason.startswith('backward: ') else _strict:
        raise RuntimeError('tac_amd::%s: %s is outside the gfx950 kernels and strict mode forbids the stock-torch '
                           'route' % (op, reason))
    if (op, reason) not in _warned:
        _warned.add((op, reason))
        warnings.warn('tac_amd::%s: %s — evaluated by stock torch operators on the device, not by the gfx950 '
                      'kernels' % (op, reason), CompositeRouteWarning, stacklevel=3)


_WIDEN = (torch.float16, torch.bfloat16)


def _f32(t):
    return t.float() if t.dtype in _WIDEN else t


def _hip_dtype(*tensors):
    """None when the gfx950 kernels take these tensors (float32, or half widened), else the reason they do not."""
    for t in tensors:
        if t.dtype == torch.float32 or t.dtype in _WIDEN:
            continue
        return 'dtype %s' % str(t.dtype).replace('torch.', '')
    return None


def _same_device(op, *tensors):
    dev = tensors[0].device
    for t in tensors[1:]:
        if t.device != dev:
            raise RuntimeError('tac_amd::%s: tensors are on different devices (%s and %s)' % (op, dev, t.device))


# ============================================================================= fake (meta) helpers
def _swapped(lead, tail, dtype, device, a, b):
    """empty(lead + tail).transpose(a, b): the frame-major physical layout every STFT-family kernel writes, returned
    as the logical (.., freq, time[, 2]) view — the same strides the reference's own torch ops produce."""
    return torch.empty(tuple(lead) + tuple(tail), dtype=dtype, device=device).transpose(a, b)


def _out_dtype(t):
    return torch.float32 if (t.dtype in _WIDEN or t.dtype == torch.int16) else t.dtype


def _n_frames(length, n_fft, hop, center):
    return 1 + (length + (2 * (n_fft // 2) if center else 0) - n_fft) // hop


# ============================================================================= autograd
def _plain_hip_f32(*tensors):
    return all(t is not None and type(t) is torch.Tensor and t.is_cuda and t.dtype == torch.float32 for t in tensors)


def _register_autograd(op, fn, n_tensors, hip_backward=None, n_plain=None, save_output=None):
    """Backward of ``tac_amd::<op>``.  ``hip_backward(tensors, rest, needs, grads)`` — the hand-written gradient
    kernels (csrc/backward.hip) — is used when it applies (float32 on a HIP device); it returns None otherwise and
    the op is then differentiated by re-evaluating it with differentiable torch operators (``_composite``) on the
    saved inputs.  That second route is the only one on CPU tensors; on a HIP device it is announced like every other
    use of stock torch operators there (``CompositeRouteWarning``, an error under ``set_strict(True)``, counted in
    ``composite_calls``).

    Double backward (``create_graph=True``; the reference, being stock torch operators, is twice differentiable): the
    gradient kernels produce values without a graph, so a backward pass that is itself recorded re-evaluates the op
    with torch operators on the SAVED tensors — still attached to the caller's graph — and differentiates that with
    ``create_graph=True``.

    ``n_plain``: how many of the leading tensors have to be float32 on a HIP device for the gradient kernels (all of them by
    default; ``lfilter``'s coefficient tensors may be float64 and may live on the host).  ``save_output(inputs)``: where true
    the op's output is saved too and handed to ``hip_backward`` behind the input tensors."""

    def setup_context(ctx, inputs, output):
        # an output nobody differentiated arrives in ``backward`` as None, not as a tensor of zeros: ``magphase`` with its phase
        # unused then runs the magnitude's gradient alone, like ``complex_norm`` (a zero phase gradient times an infinite component
        # was NaN where the reference, whose atan2 node never runs, gives 0), and nothing reads or fills the zeros
        ctx.set_materialize_grads(False)
        if save_output is not None and save_output(inputs):
            ctx.save_for_backward(*inputs[:n_tensors], output)
        else:
            ctx.save_for_backward(*inputs[:n_tensors])
        ctx.rest = tuple(inputs[n_tensors:])

    def backward(ctx, *grads):
        needs = ctx.needs_input_grad[:n_tensors]
        kept = ctx.saved_tensors
        saved = kept[:n_tensors]
        second_order = torch.is_grad_enabled()
        why = 'double backward (create_graph=True)' if second_order else None
        if why is None and hip_backward is not None:
            if _plain_hip_f32(*kept[n_tensors:], *saved[:n_plain]) and all(g is None or _plain_hip_f32(g) for g in grads):
                with torch.no_grad():
                    res = hip_backward(kept, ctx.rest, needs, grads)
                if res is not None:
                    return tuple(res) + (None,) * len(ctx.rest)
                why = 'this gradient has no gfx950 kernel'
            else:
                why = _hip_dtype(*[t for t in tuple(saved[:n_plain]) + tuple(grads) if t is not None]) or 'tensor subclass'
        elif why is None:
            why = 'the op has no gradient kernel'
        if any(t.is_cuda for t in saved):
            _composite_route(op, 'backward: ' + why)
        with torch.enable_grad():
            if second_order:        # keep the graph: the saved tensors are the caller's own
                ins = list(saved)
                wanted = [t for t, need in zip(ins, needs) if need and t.requires_grad]
            else:
                ins = [t.detach().requires_grad_(True) if (need and t.is_floating_point()) else t.detach()
                       for t, need in zip(saved, needs)]
                wanted = [t for t in ins if t.requires_grad]
            outs = fn(*ins, *ctx.rest)
            outs = outs if isinstance(outs, tuple) else (outs,)
            pairs = [(o, g) for o, g in zip(outs, grads) if g is not None and o.requires_grad]
            got = torch.autograd.grad([o for o, _ in pairs], wanted, [g for _, g in pairs], allow_unused=True,
                                      create_graph=second_order) if pairs and wanted else ()
        by_id = {id(t): g for t, g in zip(wanted, got)}
        result = [by_id.get(id(t)) for t in ins]
        return tuple(result) + (None,) * len(ctx.rest)

    torch.library.register_autograd('%s::%s' % (NS, op), backward, setup_context=setup_context, lib=_lib)


def _signal_path_only(needs):
    """Gradient wanted for the first tensor (waveform / spectrogram) and for none of the constant tables."""
    return bool(needs[0]) and not any(needs[1:])


def _fast_backward(needs, n_fft, onesided):
    """the fused backward kernels: gradient of the waveform only, one-sided power-of-two fft_length"""
    return _signal_path_only(needs) and H.stft_backward_supported(n_fft, onesided)


def _stft_hip_backward(saved, rest, needs, grads):
    wave, window = saved
    n_fft, hop, win_length, center, pad_mode, normalized, onesided = rest[:7]
    if grads[0] is None or not H.hip_covers_backward(n_fft):
        return None
    window = window.contiguous()
    if _fast_backward(needs, n_fft, onesided):
        return [H.stft_backward(grads[0], wave, window, n_fft, hop, win_length, center, pad_mode, normalized), None]
    return list(H.stft_backward_general(grads[0], wave, window, n_fft, hop, win_length, center, pad_mode, normalized,
                                        onesided, bool(needs[0]), bool(needs[1])))


def _spectrogram_general_backward(wave, window, geo, power, g, need_wave, need_window):
    """spectrum recomputed by the forward kernel, the norm's adjoint, then the general stft adjoint"""
    n_fft, hop, win_length, center, pad_mode, normalized, onesided = geo
    z = H.stft(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided)
    gz = H.complex_norm_backward(z, g, power)
    return H.stft_backward_general(gz, wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided,
                                   need_wave, need_window)


def _spectrogram_hip_backward(saved, rest, needs, grads):
    wave, window = saved
    n_fft, hop, win_length, center, pad_mode, normalized, onesided, power, db, ref, amin = rest
    if grads[0] is None or not H.hip_covers_backward(n_fft):
        return None
    window = window.contiguous()
    g = grads[0]
    if db:      # the |z|^power values the dB gradient needs: one fused forward launch (nothing was saved)
        g = H.amplitude_to_db_backward(H.spectrogram(wave, window, n_fft, hop, win_length, center, pad_mode, normalized,
                                                     onesided, power, False, 1.0, 1e-7), g, amin)
    if not _fast_backward(needs, n_fft, onesided):
        return list(_spectrogram_general_backward(wave, window, rest[:7], power, g, bool(needs[0]), bool(needs[1])))
    # the backward kernel transforms the frames again itself and folds the norm's adjoint into the inverse FFT's load:
    # neither the spectrum nor a gradient spectrum exists in memory (fft_length 4096: the spectrum is recomputed first)
    z = None if H.backward_recomputes_spectrum(n_fft) else \
        H.stft(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided)
    return [H.stft_backward(z, wave, window, n_fft, hop, win_length, center, pad_mode, normalized, grad_norm=g, power=power),
            None]


def _melspectrogram_hip_backward(saved, rest, needs, grads):
    wave, window, bank = saved
    n_fft, hop, win_length, center, pad_mode, normalized, onesided, power, db, ref, amin = rest
    if grads[0] is None or not H.hip_covers_backward(n_fft):
        return None
    window = window.contiguous()
    g = grads[0]
    if db:      # the mel values the dB gradient needs come from the fused forward kernel (one launch)
        mel = H.melspectrogram(wave, window, bank, n_fft, hop, win_length, center, pad_mode, normalized, onesided, power,
                               False, 1.0, 1e-7)
        g = H.amplitude_to_db_backward(mel, g, amin)
    grad_bank = None
    if needs[2]:
        grad_bank = H.filterbank_grad(H.spectrogram(wave, window, n_fft, hop, win_length, center, pad_mode, normalized,
                                                    onesided, power, False, 1.0, 1e-7), g)
    if not (needs[0] or needs[1]):
        return [None, None, grad_bank]
    if _fast_backward(needs[:2], n_fft, onesided):
        # fft_length 2048: filterbank adjoint, frame re-transform, norm adjoint, inverse FFT and overlap-add in one kernel
        gw = H.melspectrogram_backward_fused(g, wave, window, bank, n_fft, hop, win_length, center, pad_mode, normalized, power)
        if gw is not None:
            return [gw, None, grad_bank]
    gp = H.apply_filterbank_backward(g, bank)
    if not _fast_backward(needs[:2], n_fft, onesided):
        gw, gwin = _spectrogram_general_backward(wave, window, rest[:7], power, gp, bool(needs[0]), bool(needs[1]))
        return [gw, gwin, grad_bank]
    z = None if H.backward_recomputes_spectrum(n_fft) else \
        H.stft(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided)
    return [H.stft_backward(z, wave, window, n_fft, hop, win_length, center, pad_mode, normalized, grad_norm=gp, power=power),
            None, grad_bank]


def _apply_filterbank_hip_backward(saved, rest, needs, grads):
    if grads[0] is None:
        return None
    spec, bank = saved
    return [H.apply_filterbank_backward(grads[0], bank) if needs[0] else None,
            H.filterbank_grad(spec, grads[0]) if needs[1] else None]


def _complex_norm_hip_backward(saved, rest, needs, grads):
    if grads[0] is None or saved[0].shape[-1] != 2:
        return None
    return [H.complex_norm_backward(saved[0], grads[0], rest[0])]


def _amplitude_to_db_hip_backward(saved, rest, needs, grads):
    if grads[0] is None:
        return None
    return [H.amplitude_to_db_backward(saved[0], grads[0], rest[1])]


def _angle_hip_backward(saved, rest, needs, grads):
    if grads[0] is None or saved[0].shape[-1] != 2:
        return None
    return [H.magphase_backward(saved[0], None, grads[0], 1.0)]


def _magphase_hip_backward(saved, rest, needs, grads):
    if (grads[0] is None and grads[1] is None) or saved[0].shape[-1] != 2:
        return None
    return [H.magphase_backward(saved[0], grads[0], grads[1], rest[0])]


def _phase_vocoder_hip_backward(saved, rest, needs, grads):
    spec, phase_advance = saved
    if grads[0] is None or spec.shape[-1] != 2 or spec.dim() < 3:
        return None
    return [H.phase_vocoder_backward(spec, rest[0], grads[0]) if needs[0] else None,
            torch.zeros_like(phase_advance) if needs[1] else None]       # (the wrap and the advance cancel: zero, as autograd finds)


def _stretch_norm_hip_backward(saved, rest, needs, grads):
    rate, power, db, ref, amin = rest
    if grads[0] is None:
        return None
    mag, g = saved[0], grads[0]
    if db:      # the linear values the dB gradient needs: one more launch of the forward kernel (nothing was saved)
        g = H.amplitude_to_db_backward(H.stretch_norm(mag, rate, power, False, 1.0, 1e-7), g, amin)
    return [H.stretch_norm_backward(mag, rate, power, g)]


def _stretch_mel_hip_backward(saved, rest, needs, grads):
    rate, power, db, ref, amin = rest
    if grads[0] is None:
        return None
    mag, bank = saved
    g = grads[0]
    if db:
        g = H.amplitude_to_db_backward(H.stretch_mel(mag, bank, rate, power, False, 1.0, 1e-7), g, amin)
    # the bank's gradient the way apply_filterbank finds it: from the rows the bank was applied to
    grad_bank = H.filterbank_grad(H.stretch_norm(mag, rate, power, False, 1.0, 1e-7), g) if needs[1] else None
    grad_mag = H.stretch_norm_backward(mag, rate, power, H.apply_filterbank_backward(g, bank)) if needs[0] else None
    return [grad_mag, grad_bank]


def _hpss_hip_backward(saved, rest, needs, grads):
    kernel_f, kernel_t, power, hard = rest
    if all(g is None for g in grads) or not H.hpss_supported(kernel_f, kernel_t):
        return None
    gs = list(grads) if len(grads) == 4 else [None, None] + list(grads)      # (hpss_masks: the two masks only)
    if hard:
        gs[2] = gs[3] = None                                                  # boolean masks carry no gradient
    return [H.hpss_backward(saved[0], kernel_f, kernel_t, power, hard, gs)]


def _db_to_amplitude_hip_backward(saved, rest, needs, grads):
    if grads[0] is None or not rest[0] > 0.0:
        return None
    return [H.db_to_amplitude_backward(saved[0], grads[0], rest[0])]


def _istft_hip_backward(saved, rest, needs, grads):
    spec, window = saved
    n_fft, hop, win_length, center, normalized, onesided, length = rest
    if grads[0] is None or needs[1] or not onesided or not H.istft_covers(n_fft):
        return None                 # (the window's gradient: the stock-torch route, announced)
    return [H.istft_backward(grads[0], window.contiguous(), n_fft, hop, win_length, center, normalized,
                             int(spec.shape[-2])) if needs[0] else None, None]


def _dct_hip_backward(saved, rest, needs, grads):
    x, matrix = saved
    if grads[0] is None or needs[1] or not H.dct_covers(matrix.shape[0], matrix.shape[1]):
        return None                 # (the matrix's gradient: the stock-torch route, announced)
    # the same kernel with the transposed matrix; grad_out is read where it lies, whatever strides autograd gave it
    return [H.dct_rows(grads[0], matrix, transposed=True) if needs[0] else None, None]


def _resample_hip_backward(saved, rest, needs, grads):
    (wave,) = saved
    if grads[0] is None or not needs[0] or rest[0] == rest[1] or not H.resample_covers(*rest):
        return None
    # the same kernel with the transposed bank; a grad_out autograd handed over with other than unit stride is copied
    return [H.polyphase(grads[0], tuple(rest), int(wave.shape[-1]), adjoint=True)]


def _resample_fit_hip_backward(saved, rest, needs, grads):
    (wave,) = saved
    key, out_len, length = tuple(rest[:6]), rest[6], int(wave.shape[-1])
    g = grads[0]
    if g is None or not needs[0] or key[0] == key[1] or not H.resample_fit_covers(key, length, out_len):
        return None
    if any(st <= 0 for st, n in zip(g.stride(), g.shape) if n > 1):
        g = g.contiguous()                                      # (an expanded grad_out is copied)
    # the adjoint bank on the same kernel; grad_out counts as zero beyond min(n_out, out_len): the effective length is passed
    return [H.resample_fit(g, key, out_len, adjoint=True, length=length)]


def _lfilter_hip_backward_of(reverse):
    def backward(saved, rest, needs, grads):
        wave, a, b = saved[:3]
        (clamp,) = rest
        if grads[0] is None or needs[1] or needs[2]:
            return None                 # (the coefficients' gradient: the stock-torch route, announced)
        ha, hb = H.host_coeffs(a), H.host_coeffs(b)
        if not H.lfilter_covers(hb, ha):
            return None
        g = grads[0]
        if clamp:                       # the clamp passes the gradient where the saved output lies strictly inside (-1, 1)
            y = saved[3]
            g = g * ((y > -1.0) & (y < 1.0))
        # the adjoint of a causal filter is the same filter run backwards in time: the same kernel, walking each row from its end
        # (and from its start for the op that itself runs from the end)
        return [H.lfilter_rows(g, hb, ha, False, reverse=not reverse) if needs[0] else None, None, None]
    return backward


def _sosfilt_hip_backward_of(reverse):
    def backward(saved, rest, needs, grads):
        wave, sos = saved[:2]
        (clamp,) = rest
        if grads[0] is None or needs[1]:
            return None                 # (the sections' gradient: the stock-torch route, announced)
        hs = H.host_sos(sos)
        if not H.sosfilt_covers(hs):
            return None
        g = grads[0]
        if clamp:
            y = saved[2]
            g = g * ((y > -1.0) & (y < 1.0))
        # the adjoint of the cascade: its sections in reverse order, each run against time — the same kernel, ``reverse`` flipped
        return [H.sosfilt_rows(g, hs, False, reverse=not reverse) if needs[0] else None, None]
    return backward


def _overdrive_hip_backward(saved, rest, needs, grads):
    """d out / d x of ``overdrive``: the clamp's mask, the shaper's slope ``g (1 - t^2)`` inside [-1, 1] (zero outside) and, between
    them, the adjoint of ``v = lfilter(t, (1, -0.995), (1, -1))`` — lfilter's kernel run from the end of each row.  The
    elementwise steps are torch operators on the device; nothing here is the stock-torch route of the op."""
    wave, y = saved[0], saved[1]
    gain, colour = rest
    if grads[0] is None or SX.inside(SX.OVERDRIVE_RANGES, gain=gain, colour=colour) is not None:
        return None
    g, c = SX.overdrive_constants(gain, colour)
    gy = grads[0] * ((y > -1.0) & (y < 1.0))
    t = wave.double() * g + c
    slope = torch.where((t < -1.0) | (t > 1.0), torch.zeros_like(t), (1.0 - t * t) * g).float()
    gt = H.lfilter_rows(gy * 0.75, (1.0, -1.0), (1.0, -0.995), False, reverse=True)
    return [gy * 0.5 + slope * gt if needs[0] else None]


def _fftconvolve_hip_backward(saved, rest, needs, grads):
    x, y = saved
    (n_fft,) = rest
    length, m = int(x.shape[-1]), int(y.shape[-1])
    if grads[0] is None or needs[1]:
        return None                 # (the kernel's gradient: the stock-torch route, announced)
    if tuple(grads[0].shape[:-1]) != tuple(x.shape[:-1]) or not H.fftconvolve_covers(length + m - 1, m, n_fft):
        return None                 # (x itself was broadcast: its gradient is a sum over rows)
    # the same route with the kernel read from its end: samples M - 1 .. M - 1 + L of grad_out * reversed(y)
    return [H.fftconvolve(grads[0], y, n_fft, reverse=True, offset=m - 1, out_len=length), None]


def _sliding_window_cmn_hip_backward(saved, rest, needs, grads):
    cmn_window, min_cmn_window, center, norm_vars = rest
    if grads[0] is None or not needs[0] or norm_vars:
        return None                 # (the variance's gradient: the stock-torch route, announced)
    g = grads[0] if H.sliding_cmn_covers(grads[0]) else grads[0].contiguous()      # (an expanded grad_out is copied)
    # the frames whose window holds s form an interval: the same sliding sum, over g[t] / n(t)
    return [H.sliding_cmn_rows(g, cmn_window, min_cmn_window, center, False, adjoint=True)]


def _compute_deltas_hip_backward(saved, rest, needs, grads):
    win_length, mode = rest
    if grads[0] is None or not needs[0] or not H.deltas_supported(int(grads[0].shape[-1]), win_length, mode, adjoint=True):
        return None                 # ('reflect' / 'circular', a window beyond the kernel's: the stock-torch route, announced)
    g = grads[0] if H.deltas_covers(grads[0], win_length, mode, adjoint=True) else grads[0].contiguous()      # (an expanded grad_out)
    return [H.deltas_rows(g, win_length, mode, adjoint=True)]


def _mask_spans_hip_backward(saved, rest, needs, grads):
    """``saved``: the span table; ``needs``: (the input, a tensor fill).  The copy's adjoint is the copy: the same kernel on grad_out
    with zeros under the masks; what it took out is the fill's share."""
    (spans,) = saved
    k_a = rest[0]
    g = grads[0]
    if g is None or not H.mask_spans_supported(k_a, int(spans.shape[-2]) - k_a):
        return None                 # (more spans than the kernel takes: the stock-torch route, announced)
    g = g if H.mask_spans_covers(g, k_a, int(spans.shape[-2]) - k_a) else g.contiguous()      # (an expanded grad_out is copied)
    gx = H.mask_spans_rows(g, spans, k_a, None, 0.0)
    return [gx if needs[0] else None, (g - gx).sum() if needs[1] else None]


def _add_noise_lead(waveform, noise, snr, lengths):
    shapes = [tuple(waveform.shape[:-1]), tuple(noise.shape[:-1]), tuple(snr.shape)]
    if lengths is not None:
        shapes.append(tuple(lengths.shape))
    return tuple(torch.broadcast_shapes(*shapes))


def _add_noise_hip_backward(saved, rest, needs, grads):
    """``saved``: (waveform, noise, snr); ``rest``: (lengths,).  One ``tac_add_noise_grad_f32`` entry recomputes the float64 sums and
    writes the gradients over the broadcast shape; torch's ``sum`` then folds those of broadcast operands."""
    waveform, noise, snr = saved
    lengths = rest[0]
    g = grads[0]
    if g is None:
        return None
    lead = _add_noise_lead(waveform, noise, snr, lengths)
    if not H.add_noise_covers(lead, waveform, noise):
        return None                 # (the layouts the forward announced: the stock-torch route, announced again)
    g = g if H.add_noise_covers(lead, g, waveform, noise) else g.contiguous()      # (one split of the rows has to serve all three)
    got = H.add_noise_grad_rows(g, waveform, noise, snr, lengths, lead, needs)
    return [None if t is None else t.sum_to_size(ref.shape) for t, ref in zip(got, saved)]


_HIP_BACKWARD = {'overdrive': _overdrive_hip_backward, 'sliding_window_cmn': _sliding_window_cmn_hip_backward, 'compute_deltas': _compute_deltas_hip_backward,
                 'mask_spans': _mask_spans_hip_backward, 'add_noise': _add_noise_hip_backward,
                 'stft': _stft_hip_backward, 'fftconvolve': _fftconvolve_hip_backward, 'dct': _dct_hip_backward, 'resample': _resample_hip_backward, 'resample_fit': _resample_fit_hip_backward, 'lfilter': _lfilter_hip_backward_of(False), 'lfilter_reverse': _lfilter_hip_backward_of(True), 'sosfilt': _sosfilt_hip_backward_of(False), 'sosfilt_reverse': _sosfilt_hip_backward_of(True), 'istft': _istft_hip_backward, 'spectrogram': _spectrogram_hip_backward,
                 'melspectrogram': _melspectrogram_hip_backward, 'apply_filterbank': _apply_filterbank_hip_backward,
                 'complex_norm': _complex_norm_hip_backward, 'amplitude_to_db': _amplitude_to_db_hip_backward,
                 'angle': _angle_hip_backward, 'magphase': _magphase_hip_backward, 'db_to_amplitude': _db_to_amplitude_hip_backward,
                 'phase_vocoder': _phase_vocoder_hip_backward, 'stretch_norm': _stretch_norm_hip_backward,
                 'stretch_mel': _stretch_mel_hip_backward, 'hpss': _hpss_hip_backward, 'hpss_masks': _hpss_hip_backward}


#: the CUDA-key kernels by op name: `call` below invokes them directly when the dispatcher has nothing to add
cuda_kernels = {}


def call(op, *args):
    """Invoke ``tac_amd::<op>``.  In plain eager mode on HIP tensors without autograd state, tracing, dispatch modes or
    an active profiler, the dispatcher would do nothing but box the arguments twice (~11 us per call through the
    Python-kernel path) before reaching the CUDA-key kernel — so that kernel is called directly; every other situation
    (CPU tensors, autograd, torch.compile / FakeTensor, functorch, profiling) goes through the registered op."""
    if torch.compiler.is_compiling():
        return getattr(ops, op)(*args)
    grad = torch.is_grad_enabled()
    direct = not (torch._C._len_torch_dispatch_stack() or torch.autograd._profiler_enabled()
                  or torch._C._functorch.peek_interpreter_stack() is not None)
    if direct:
        for a in args:
            if isinstance(a, torch.Tensor):
                if type(a) is not torch.Tensor or not a.is_cuda or (grad and a.requires_grad):
                    direct = False
                    break
    if direct:
        return cuda_kernels[op](*args)
    return getattr(ops, op)(*args)


def _register(op, schema, cuda, cpu, fake, n_tensors, differentiable=True, **autograd_kw):
    cuda_kernels[op] = cuda
    _lib.define(op + schema)
    _lib.impl(op, cuda, 'CUDA')
    _lib.impl(op, cpu, 'CPU')
    torch.library.register_fake('%s::%s' % (NS, op), fake, lib=_lib)
    if differentiable:
        _register_autograd(op, cpu, n_tensors, _HIP_BACKWARD.get(op), **autograd_kw)


# ============================================================================= stft
_STFT_ARGS = 'int n_fft, int hop, int win_length, bool center, str pad_mode, bool normalized, bool onesided'


def _pcm(wave):
    """int16 waveforms are PCM: sample * 2^-15 (converted by a HIP kernel where the frame load cannot do it)."""
    return H.pcm16_to_f32(wave) if wave.dtype == torch.int16 else _f32(wave)


def _stft_route(op, wave, n_fft, *others):
    reason = _hip_dtype(*others) if wave.dtype == torch.int16 else _hip_dtype(wave, *others)
    if reason is None and not H.hip_covers_n_fft(n_fft):
        reason = 'fft_length %d' % n_fft
    if reason is not None:
        _composite_route(op, reason)
    return reason


def _stft_cuda(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided):
    _same_device('stft', wave, window)
    if H64.all_f64(wave, window) and H64.covers(n_fft):
        return H64.stft(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided)
    if _stft_route('stft', wave, n_fft, window) is not None:
        return C.stft(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided)
    return H.stft(_pcm(wave), _f32(window).contiguous(), n_fft, hop, win_length, center, pad_mode, normalized,
                  onesided)


def _stft_fake(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided):
    n_bins = n_fft // 2 + 1 if onesided else n_fft
    frames = _n_frames(wave.shape[-1], n_fft, hop, center)
    return _swapped(wave.shape[:-1], (frames, n_bins, 2), _out_dtype(wave), wave.device, -3, -2)


_register('stft', '(Tensor wave, Tensor window, %s) -> Tensor' % _STFT_ARGS, _stft_cuda, C.stft, _stft_fake, 2)


# ============================================================================= istft
def _istft_cuda(spec, window, n_fft, hop, win_length, center, normalized, onesided, length):
    _same_device('istft', spec, window)
    reason = _hip_dtype(spec, window)
    if reason is None and not onesided:
        reason = 'onesided=False'
    if reason is None and not H.istft_covers(n_fft):
        reason = 'fft_length %d' % n_fft
    if reason is not None:
        _composite_route('istft', reason)
        return C.istft(spec, window, n_fft, hop, win_length, center, normalized, onesided, length)
    return H.istft(_f32(spec), _f32(window).contiguous(), n_fft, hop, win_length, center, normalized, length)


def _istft_fake(spec, window, n_fft, hop, win_length, center, normalized, onesided, length):
    n_out = H.istft_full_length(spec.shape[-2], n_fft, hop, center) if length is None else length
    return torch.empty(tuple(spec.shape[:-3]) + (n_out,), dtype=_out_dtype(spec), device=spec.device)


_register('istft', '(Tensor spec, Tensor window, int n_fft, int hop, int win_length, bool center, bool normalized, '
          'bool onesided, int? length) -> Tensor', _istft_cuda, C.istft, _istft_fake, 2)


# ============================================================================= griffinlim
def _griffinlim_cuda(specgram, window, angles0, n_fft, hop, win_length, power, n_iter, m, length):
    _same_device('griffinlim', specgram, window, *(() if angles0 is None else (angles0,)))
    reason = None
    for t in (specgram, window):                # (half precision is not widened here: the iteration would run in float32)
        if reason is None and t.dtype != torch.float32:
            reason = 'dtype %s' % str(t.dtype).replace('torch.', '')
    if reason is None and angles0 is not None and angles0.dtype != torch.complex64:
        reason = 'dtype %s' % str(angles0.dtype).replace('torch.', '')
    if reason is None and not H.istft_covers(n_fft):
        reason = 'fft_length %d' % n_fft
    if reason is None and not H.griffinlim_covers(specgram, angles0):
        reason = 'expanded or non-positive strides'
    if reason is not None:
        _composite_route('griffinlim', reason)
        return C.griffinlim(specgram, window, angles0, n_fft, hop, win_length, power, n_iter, m, length)
    return H.griffinlim(specgram, window.contiguous(), angles0, n_fft, hop, win_length, power, n_iter, m, length)


def _griffinlim_fake(specgram, window, angles0, n_fft, hop, win_length, power, n_iter, m, length):
    n_out = hop * (specgram.shape[-1] - 1) if length is None else length
    return torch.empty(tuple(specgram.shape[:-2]) + (n_out,), dtype=specgram.dtype, device=specgram.device)


# (the gradient re-evaluates the listing with torch operators: announced, an error under strict unless backward=False)
_register('griffinlim', '(Tensor specgram, Tensor window, Tensor? angles0, int n_fft, int hop, int win_length, float power, '
          'int n_iter, float m, int? length) -> Tensor', _griffinlim_cuda, C.griffinlim, _griffinlim_fake, 2)


# ============================================================================= spectrogram (stft + |.|^p [+ dB])
def _spectrogram_cuda(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided, power, db, ref,
                      amin):
    _same_device('spectrogram', wave, window)
    if H64.all_f64(wave, window) and H64.covers(n_fft):
        return H64.spectrogram(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided, power, db, ref,
                               amin)
    if _stft_route('spectrogram', wave, n_fft, window) is not None:
        return C.spectrogram(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided, power, db,
                             ref, amin)
    return H.spectrogram(_pcm(wave), _f32(window).contiguous(), n_fft, hop, win_length, center, pad_mode, normalized,
                         onesided, power, db, ref, amin)


def _spectrogram_fake(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided, power, db, ref,
                      amin):
    n_bins = n_fft // 2 + 1 if onesided else n_fft
    frames = _n_frames(wave.shape[-1], n_fft, hop, center)
    return _swapped(wave.shape[:-1], (frames, n_bins), _out_dtype(wave), wave.device, -2, -1)


_register('spectrogram', '(Tensor wave, Tensor window, %s, float power, bool db, float ref, float amin) -> Tensor'
          % _STFT_ARGS, _spectrogram_cuda, C.spectrogram, _spectrogram_fake, 2)


# ============================================================================= melspectrogram (the fused chain)
def _melspectrogram_cuda(wave, window, bank, n_fft, hop, win_length, center, pad_mode, normalized, onesided, power,
                         db, ref, amin):
    _same_device('melspectrogram', wave, window, bank)
    if H64.all_f64(wave, window, bank) and H64.covers(n_fft) and bank.dim() == 2 and bank.shape[0] == (
            n_fft // 2 + 1 if onesided else n_fft):
        return H64.melspectrogram(wave, window, bank, n_fft, hop, win_length, center, pad_mode, normalized, onesided, power,
                                  db, ref, amin)
    if _stft_route('melspectrogram', wave, n_fft, window, bank) is not None:
        return C.melspectrogram(wave, window, bank, n_fft, hop, win_length, center, pad_mode, normalized, onesided,
                                power, db, ref, amin)
    window, bank = _f32(window).contiguous(), _f32(bank)
    if wave.dtype == torch.int16:                                        # PCM converted inside the frame load when one kernel covers it
        fused = H.melspectrogram_coded(wave, window, bank, n_fft, hop, win_length, center, pad_mode, normalized, onesided,
                                       power, db, ref, amin)
        if fused is not None:
            return fused
    return H.melspectrogram(_pcm(wave), window, bank, n_fft, hop, win_length, center, pad_mode, normalized, onesided,
                            power, db, ref, amin)


def _melspectrogram_fake(wave, window, bank, n_fft, hop, win_length, center, pad_mode, normalized, onesided, power,
                         db, ref, amin):
    frames = _n_frames(wave.shape[-1], n_fft, hop, center)
    return _swapped(wave.shape[:-1], (frames, bank.shape[1]), _out_dtype(wave), wave.device, -2, -1)


cuda_kernels['melspectrogram'] = _melspectrogram_cuda
_lib.define('melspectrogram(Tensor wave, Tensor window, Tensor filterbank, %s, float power, bool db, float ref, '
            'float amin) -> Tensor' % _STFT_ARGS)
_lib.impl('melspectrogram', _melspectrogram_cuda, 'CUDA')
_lib.impl('melspectrogram', C.melspectrogram, 'CPU')
torch.library.register_fake(NS + '::melspectrogram', _melspectrogram_fake, lib=_lib)
_register_autograd('melspectrogram', C.melspectrogram, 3, _melspectrogram_hip_backward)


# ============================================================================= mu-law codes -> melspectrogram
def _melspectrogram_mulaw_cuda(codes, window, bank, n_quantize, n_fft, hop, win_length, center, pad_mode, normalized,
                               onesided, power, db, ref, amin):
    _same_device('melspectrogram_mulaw', codes, window, bank)
    reason = _hip_dtype(window, bank)
    if reason is None and not H.hip_covers_n_fft(n_fft):
        reason = 'fft_length %d' % n_fft
    if reason is not None:
        _composite_route('melspectrogram_mulaw', reason)
        return C.melspectrogram_mulaw(codes, window, bank, n_quantize, n_fft, hop, win_length, center, pad_mode, normalized,
                                      onesided, power, db, ref, amin)
    window, bank = _f32(window).contiguous(), _f32(bank)
    if n_quantize == 256 and codes.dtype in (torch.uint8, torch.int64):   # decoded inside the frame load
        fused = H.melspectrogram_coded(codes, window, bank, n_fft, hop, win_length, center, pad_mode, normalized, onesided,
                                       power, db, ref, amin)
        if fused is not None:
            return fused
    wave = H.mu_law_decoding_int(codes, n_quantize) if not codes.is_floating_point() else H.mu_law_decoding_float(_f32(codes), n_quantize)
    return H.melspectrogram(wave, window, bank, n_fft, hop, win_length, center, pad_mode, normalized, onesided, power, db,
                            ref, amin)


def _melspectrogram_mulaw_fake(codes, window, bank, n_quantize, n_fft, hop, win_length, center, pad_mode, normalized,
                               onesided, power, db, ref, amin):
    frames = _n_frames(codes.shape[-1], n_fft, hop, center)
    return _swapped(codes.shape[:-1], (frames, bank.shape[1]), torch.float32, codes.device, -2, -1)


_register('melspectrogram_mulaw', '(Tensor codes, Tensor window, Tensor filterbank, int n_quantize, %s, float power, bool db, '
          'float ref, float amin) -> Tensor' % _STFT_ARGS, _melspectrogram_mulaw_cuda, C.melspectrogram_mulaw,
          _melspectrogram_mulaw_fake, 3, differentiable=False)


# ============================================================================= apply_filterbank
def _apply_filterbank_cuda(spec, bank):
    _same_device('apply_filterbank', spec, bank)
    if H64.all_f64(spec, bank) and spec.dim() >= 2 and bank.dim() == 2 and spec.shape[-2] == bank.shape[0]:
        return H64.apply_filterbank(spec, bank)
    if _hip_dtype(spec, bank) is not None:
        _composite_route('apply_filterbank', _hip_dtype(spec, bank))
        return C.apply_filterbank(spec, bank)
    out = H.apply_filterbank(_f32(spec), _f32(bank))
    return out if spec.dtype == out.dtype else out.to(spec.dtype)


def _apply_filterbank_fake(spec, bank):
    return _swapped(spec.shape[:-2], (spec.shape[-1], bank.shape[1]), spec.dtype, spec.device, -2, -1)


_register('apply_filterbank', '(Tensor spec, Tensor filterbank) -> Tensor', _apply_filterbank_cuda,
          C.apply_filterbank, _apply_filterbank_fake, 2)


# ============================================================================= dct (MFCC)
def _dct_cuda(x, matrix):
    _same_device('dct', x, matrix)
    reason = _hip_dtype(x, matrix)
    if reason is None and not H.dct_covers(matrix.shape[0], matrix.shape[1]):
        reason = 'a %d x %d matrix (beyond 256 x 256 / 32768 elements)' % tuple(matrix.shape)
    if reason is not None:
        _composite_route('dct', reason)
        return C.dct(x, matrix)
    out = H.dct_rows(_f32(x), matrix)
    return out if x.dtype == out.dtype else out.to(x.dtype)


def _dct_fake(x, matrix):
    return _swapped(x.shape[:-2], (x.shape[-1], matrix.shape[1]), x.dtype, x.device, -2, -1)


_register('dct', '(Tensor x, Tensor matrix) -> Tensor', _dct_cuda, C.dct, _dct_fake, 2)


# ============================================================================= resample
def _resample_cuda(wave, orig, new, lowpass_filter_width, rolloff, method, beta):
    key = (orig, new, lowpass_filter_width, rolloff, method, beta)
    length = wave.shape[-1]
    if orig == new or wave.numel() == 0:
        return C.resample(wave, *key)                          # the input itself / an empty output: nothing is launched
    reason = _hip_dtype(wave)
    if reason is None and not H.resample_covers(*key):
        reason = 'a polyphase bank beyond %d floats (%d -> %d)' % (H.RESAMPLE_MAX_BANK, orig, new)
    if reason is None and any(st <= 0 for st, n in zip(wave.stride(), wave.shape) if n > 1):
        reason = 'non-positive strides'
    if reason is not None:
        _composite_route('resample', reason)
        return C.resample(wave, *key)
    out = H.polyphase(_f32(wave), key, RS.out_length(length, orig, new))
    return out if wave.dtype == out.dtype else out.to(wave.dtype)


def _resample_fake(wave, orig, new, lowpass_filter_width, rolloff, method, beta):
    if orig == new:
        return wave.clone()        # (a fake kernel may not alias its input)
    return wave.new_empty(tuple(wave.shape[:-1]) + (RS.out_length(wave.shape[-1], orig, new),))


_register('resample', '(Tensor wave, int orig, int new, int lowpass_filter_width, float rolloff, str method, float? beta) '
          '-> Tensor', _resample_cuda, C.resample, _resample_fake, 1)


# ============================================================================= resample_fit
def _resample_fit_cuda(wave, orig, new, lowpass_filter_width, rolloff, method, beta, out_len):
    key = (orig, new, lowpass_filter_width, rolloff, method, beta)
    length = wave.shape[-1]
    if orig == new or wave.numel() == 0 or out_len == 0:
        return C.resample_compact(wave, *key, out_len)         # a copy / zeros: nothing is launched
    reason = _hip_dtype(wave)
    if reason is None and not H.resample_fit_covers(key, length, out_len):
        reason = 'a polyphase bank outside the LDS and the wide kernel (%d -> %d)' % (orig, new)
    if reason is None and any(st <= 0 for st, n in zip(wave.stride(), wave.shape) if n > 1):
        reason = 'non-positive strides'
    if reason is not None:
        _composite_route('resample_fit', reason)
        return C.resample_compact(wave, *key, out_len)
    out = H.resample_fit(_f32(wave), key, out_len)
    return out if wave.dtype == out.dtype else out.to(wave.dtype)


def _resample_fit_fake(wave, orig, new, lowpass_filter_width, rolloff, method, beta, out_len):
    return wave.new_empty(tuple(wave.shape[:-1]) + (out_len,))


_register('resample_fit', '(Tensor wave, int orig, int new, int lowpass_filter_width, float rolloff, str method, float? beta, '
          'int out_len) -> Tensor', _resample_fit_cuda, C.resample_compact, _resample_fit_fake, 1)


# ============================================================================= fftconvolve
def _conv_shape(x, y):
    return tuple(torch.broadcast_shapes(tuple(x.shape[:-1]), tuple(y.shape[:-1]))) + (x.shape[-1] + y.shape[-1] - 1,)


def _fftconvolve_cuda(x, y, n_fft):
    _same_device('fftconvolve', x, y)
    length, m = x.shape[-1], y.shape[-1]
    if x.numel() == 0 or y.numel() == 0:
        return x.new_zeros(_conv_shape(x, y))
    reason = _hip_dtype(x, y)
    if reason is None and any(st <= 0 for t in (x, y) for st, n in zip(t.stride(), t.shape) if n > 1):
        reason = 'non-positive strides'
    if reason is None and not H.fftconvolve_covers(length, m, n_fft):
        reason = 'a kernel of %d taps: more than %d partitions of %d samples' % (
            m, H.FFTCONV_MAX_PARTS, (n_fft or H.fftconvolve_n_fft(m)) // 2)
    if reason is not None:
        _composite_route('fftconvolve', reason)
        return C.fftconvolve(x, y, n_fft)
    out = H.fftconvolve(_f32(x), _f32(y), n_fft)
    dtype = torch.promote_types(x.dtype, y.dtype)
    return out if dtype == out.dtype else out.to(dtype)


def _fftconvolve_fake(x, y, n_fft):
    return x.new_empty(_conv_shape(x, y), dtype=torch.promote_types(x.dtype, y.dtype))


_register('fftconvolve', '(Tensor x, Tensor y, int n_fft) -> Tensor', _fftconvolve_cuda, C.fftconvolve, _fftconvolve_fake, 2)


# ============================================================================= kaldi_fbank
def _kaldi_shape(wave, p):
    w, s, n = K.sizes(p.sample_frequency, p.frame_length, p.frame_shift, p.round_to_power_of_two)
    m = K.num_frames(wave.shape[-1], w, s, p.snip_edges)
    return tuple(wave.shape[:-1]) + (m, p.num_mel_bins + (1 if p.use_energy else 0))


def _kaldi_reason(wave, p, w, n):
    """why the launch of csrc/kaldi_fbank.hip does not take this call (any of the three parameter tuples), or None"""
    reason = _hip_dtype(wave)
    if reason is None and not p.round_to_power_of_two:
        reason = 'round_to_power_of_two=False'
    if reason is None and n not in H.KALDI_SIZES:
        reason = 'a transform of %d points (the kernel takes %s)' % (n, ' / '.join(str(v) for v in H.KALDI_SIZES))
    if reason is None and getattr(p, 'num_mel_bins', 0) > H.KALDI_MAX_BINS:
        reason = '%d mel bins (the kernel takes up to %d)' % (p.num_mel_bins, H.KALDI_MAX_BINS)
    if reason is None and p.dither != 0.0:
        reason = 'dither != 0'
    if reason is None and any(st <= 0 for st, k in zip(wave.stride(), wave.shape) if k > 1):
        reason = 'non-positive strides'
    if reason is None and not p.snip_edges and wave.shape[-1] < w:
        reason = 'snip_edges=False on a waveform shorter than a frame'
    return reason


def _kaldi_fbank_cuda(wave, *args):
    p = K.Params(*args)
    w, s, n = K.check(p)
    length = wave.shape[-1]
    m = K.num_frames(length, w, s, p.snip_edges)
    if m == 0 or wave.numel() == 0:
        return wave.new_zeros(_kaldi_shape(wave, p))            # an empty output: nothing is launched
    reason = _kaldi_reason(wave, p, w, n)
    if reason is not None:
        _composite_route('kaldi_fbank', reason)
        return C.kaldi_fbank(wave, *args)
    out = H.kaldi_fbank(_f32(wave), p, w, s, n, m)
    if p.subtract_mean:
        out = out - out.mean(dim=-2, keepdim=True)
    return out if wave.dtype == out.dtype else out.to(wave.dtype)


def _kaldi_fbank_fake(wave, *args):
    return wave.new_empty(_kaldi_shape(wave, K.Params(*args)))


_register('kaldi_fbank', '(Tensor wave, %s) -> Tensor' % K.SCHEMA_ARGS, _kaldi_fbank_cuda, C.kaldi_fbank, _kaldi_fbank_fake, 1)


# ============================================================================= kaldi_mfcc, kaldi_spectrogram
def _kaldi_frames(wave, p):
    w, s, n = K.sizes(p.sample_frequency, p.frame_length, p.frame_shift, p.round_to_power_of_two)
    return K.num_frames(wave.shape[-1], w, s, p.snip_edges), n


def _kaldi_mfcc_shape(wave, p):
    return tuple(wave.shape[:-1]) + (_kaldi_frames(wave, p)[0], p.num_ceps)


def _kaldi_spectrogram_shape(wave, p):
    m, n = _kaldi_frames(wave, p)
    return tuple(wave.shape[:-1]) + (m, n // 2 + 1)


def _kaldi_mfcc_cuda(wave, *args):
    p = K.MfccParams(*args)
    w, s, n = K.check(p, 'kaldi_mfcc')
    m = K.num_frames(wave.shape[-1], w, s, p.snip_edges)
    if m == 0 or wave.numel() == 0:
        return wave.new_zeros(_kaldi_mfcc_shape(wave, p))       # an empty output: nothing is launched
    reason = _kaldi_reason(wave, p, w, n)
    if reason is None:
        limit = H.kaldi_mfcc_table_limit(p, w, n, wave.device)
        if p.num_mel_bins * p.num_ceps > limit:
            reason = 'a DCT table of %d x %d floats (the launch has room for %d)' % (p.num_mel_bins, p.num_ceps, limit)
    if reason is not None:
        _composite_route('kaldi_mfcc', reason)
        return C.kaldi_mfcc(wave, *args)
    out = H.kaldi_mfcc(_f32(wave), p, w, s, n, m)
    if p.subtract_mean:
        out = out - out.mean(dim=-2, keepdim=True)
    return out if wave.dtype == out.dtype else out.to(wave.dtype)


def _kaldi_mfcc_fake(wave, *args):
    return wave.new_empty(_kaldi_mfcc_shape(wave, K.MfccParams(*args)))


_register('kaldi_mfcc', '(Tensor wave, %s) -> Tensor' % K.MFCC_SCHEMA_ARGS, _kaldi_mfcc_cuda, C.kaldi_mfcc, _kaldi_mfcc_fake, 1)


def _kaldi_spectrogram_cuda(wave, *args):
    p = K.SpectrogramParams(*args)
    w, s, n = K.check(p, 'kaldi_spectrogram')
    m = K.num_frames(wave.shape[-1], w, s, p.snip_edges)
    if m == 0 or wave.numel() == 0:
        return wave.new_zeros(_kaldi_spectrogram_shape(wave, p))
    reason = _kaldi_reason(wave, p, w, n)
    if reason is not None:
        _composite_route('kaldi_spectrogram', reason)
        return C.kaldi_spectrogram(wave, *args)
    out = H.kaldi_spectrogram(_f32(wave), p, w, s, n, m)
    if p.subtract_mean:
        out = out - out.mean(dim=-2, keepdim=True)
    return out if wave.dtype == out.dtype else out.to(wave.dtype)


def _kaldi_spectrogram_fake(wave, *args):
    return wave.new_empty(_kaldi_spectrogram_shape(wave, K.SpectrogramParams(*args)))


_register('kaldi_spectrogram', '(Tensor wave, %s) -> Tensor' % K.SPECTROGRAM_SCHEMA_ARGS, _kaldi_spectrogram_cuda,
          C.kaldi_spectrogram, _kaldi_spectrogram_fake, 1)


# ============================================================================= sliding_window_cmn, compute_deltas
def _sliding_window_cmn_cuda(x, cmn_window, min_cmn_window, center, norm_vars):
    if x.numel() == 0:
        return torch.zeros_like(x, memory_format=torch.contiguous_format)       # an empty output: nothing is launched
    reason = _hip_dtype(x)
    if reason is None and not H.sliding_cmn_covers(x):
        reason = 'non-positive strides'
    if reason is not None:
        _composite_route('sliding_window_cmn', reason)
        return C.sliding_window_cmn(x, cmn_window, min_cmn_window, center, norm_vars)
    out = H.sliding_cmn_rows(_f32(x), cmn_window, min_cmn_window, center, norm_vars)
    return out if x.dtype == out.dtype else out.to(x.dtype)


def _same_shape_fake(x, *args):
    return x.new_empty(tuple(x.shape))


_register('sliding_window_cmn', '(Tensor x, int cmn_window, int min_cmn_window, bool center, bool norm_vars) -> Tensor',
          _sliding_window_cmn_cuda, C.sliding_window_cmn, _same_shape_fake, 1)


def _compute_deltas_cuda(x, win_length, mode):
    C.deltas_check(x.shape[-1], win_length, mode)
    if x.numel() == 0:
        return torch.zeros_like(x, memory_format=torch.contiguous_format)
    reason = _hip_dtype(x)
    if reason is None and not H.deltas_supported(int(x.shape[-1]), win_length, mode):
        reason = 'win_length %d (beyond the widest window of the kernel)' % win_length
    if reason is None and not H.deltas_covers(x, win_length, mode):
        reason = 'non-positive strides'
    if reason is not None:
        _composite_route('compute_deltas', reason)
        return C.compute_deltas(x, win_length, mode)
    out = H.deltas_rows(_f32(x), win_length, mode)
    return out if x.dtype == out.dtype else out.to(x.dtype)


def _compute_deltas_fake(x, win_length, mode):
    C.deltas_check(x.shape[-1], win_length, mode)
    return x.new_empty(tuple(x.shape))


_register('compute_deltas', '(Tensor x, int win_length, str mode) -> Tensor', _compute_deltas_cuda, C.compute_deltas,
          _compute_deltas_fake, 1)


# ============================================================================= mask_spans (SpecAugment)
def _mask_spans_check(x, spans, k_a):
    if x.dim() < 2:
        raise ValueError('mask_spans: expected a tensor of shape (…, A, B), got %d dimension(s)' % x.dim())
    if spans.dim() != 3 or spans.shape[-1] != 2 or not 0 <= k_a <= spans.shape[-2]:
        raise ValueError('mask_spans: spans must be (R, k, 2) with 0 <= k_a <= k, got %r and k_a = %d' % (tuple(spans.shape), k_a))
    rows = 1
    for n in x.shape[:-2]:
        rows *= n
    if spans.shape[-2] and spans.shape[0] != 1 and spans.shape[0] != rows:
        raise ValueError('mask_spans: spans hold %d rows, the input %d' % (spans.shape[0], rows))


def _mask_spans_cuda(x, spans, k_a, value_t, value):
    _mask_spans_check(x, spans, k_a)
    if x.numel() == 0:
        return torch.empty_like(x, memory_format=torch.contiguous_format)       # an empty output: nothing is launched
    k_b = int(spans.shape[-2]) - k_a
    reason = _hip_dtype(x)
    if reason is None and not H.mask_spans_supported(k_a, k_b):
        reason = '%d spans (beyond what one launch of the kernel takes)' % (k_a + k_b)
    if reason is None and not H.mask_spans_covers(x, k_a, k_b):
        reason = 'non-positive strides'
    if reason is not None:
        _composite_route('mask_spans', reason)
        return C.mask_spans(x, spans, k_a, value if value_t is None else value_t)
    if spans.dtype != torch.int32 or not spans.is_contiguous() or spans.device != x.device:
        spans = spans.to(device=x.device, dtype=torch.int32).contiguous()
    if value_t is not None:
        value_t = value_t.to(device=x.device, dtype=torch.float32).reshape(())
    out = H.mask_spans_rows(_f32(x), spans, k_a, value_t, value)
    return out if x.dtype == out.dtype else out.to(x.dtype)


def _mask_spans_cpu(x, spans, k_a, value_t, value):
    _mask_spans_check(x, spans, k_a)
    return C.mask_spans(x, spans, k_a, value if value_t is None else value_t)


def _mask_spans_fake(x, spans, k_a, value_t, value):
    _mask_spans_check(x, spans, k_a)
    return x.new_empty(tuple(x.shape))


def _register_mask_spans_autograd():
    """Backward of ``tac_amd::mask_spans``, whose tensor arguments do not all come first.  The gradients depend on grad_out and the
    span table alone: ``grad_x`` is grad_out with zeros under the masks, and the gradient of a tensor fill is the sum of grad_out
    under them, ``(grad_out - grad_x).sum()``.  float32 on a HIP device: the kernel (``_HIP_BACKWARD``); everything else, and every
    double backward, the same two expressions in torch operators — announced on a HIP device like every stock-torch route."""
    hip_backward = _HIP_BACKWARD['mask_spans']

    def setup_context(ctx, inputs, output):
        x, spans, k_a, value_t, value = inputs
        ctx.save_for_backward(spans)
        ctx.rest = (k_a, value)
        ctx.plain = _plain_hip_f32(x) and (value_t is None or _plain_hip_f32(value_t))
        ctx.fill = None if value_t is None else (value_t.dtype, tuple(value_t.shape), value_t.device)

    def backward(ctx, g):
        (spans,) = ctx.saved_tensors
        needs = (ctx.needs_input_grad[0], ctx.needs_input_grad[3] and ctx.fill is not None)
        second_order = torch.is_grad_enabled()
        why = 'double backward (create_graph=True)' if second_order else None
        res = None
        if why is None:
            if ctx.plain and _plain_hip_f32(g):
                with torch.no_grad():
                    res = hip_backward((spans,), ctx.rest, needs, (g,))
                why = 'this gradient has no gfx950 kernel'
            else:
                why = _hip_dtype(g) or 'tensor subclass'
        if res is None:
            if g.is_cuda:
                _composite_route('mask_spans', 'backward: ' + why)
            gx = C.mask_spans(g, spans, ctx.rest[0], 0.0)
            res = [gx if needs[0] else None, (g - gx).sum() if needs[1] else None]
        gx, gv = res
        if gv is not None:
            gv = gv.to(device=ctx.fill[2], dtype=ctx.fill[0]).reshape(ctx.fill[1])
        return gx, None, None, gv, None

    torch.library.register_autograd('%s::mask_spans' % NS, backward, setup_context=setup_context, lib=_lib)


_register('mask_spans', '(Tensor x, Tensor spans, int k_a, Tensor? value_t, float value) -> Tensor', _mask_spans_cuda, _mask_spans_cpu,
          _mask_spans_fake, 2, differentiable=False)
_register_mask_spans_autograd()


# ============================================================================= add_noise
def _add_noise_check(waveform, noise, snr, lengths):
    if not (waveform.dim() - 1 == noise.dim() - 1 == snr.dim() and (lengths is None or lengths.dim() == snr.dim())) or waveform.dim() < 1:
        raise ValueError("add_noise: the leading dimensions of waveform %r, noise %r, snr %r%s don't match"
                         % (tuple(waveform.shape), tuple(noise.shape), tuple(snr.shape),
                            '' if lengths is None else ' and lengths %r' % (tuple(lengths.shape),)))
    if waveform.shape[-1] != noise.shape[-1]:
        raise ValueError('add_noise: waveform and noise differ in length (%d and %d)' % (waveform.shape[-1], noise.shape[-1]))
    try:
        return _add_noise_lead(waveform, noise, snr, lengths)
    except RuntimeError as exc:
        raise ValueError('add_noise: the leading dimensions do not broadcast (%s)' % exc)


def _add_noise_snr(snr, dtype):
    """``snr`` in the dtype of the operands: the result has ``result_type(waveform, noise)`` on every route, the fake one included"""
    return snr if snr.dtype == dtype or not dtype.is_floating_point else snr.to(dtype)


def _add_noise_cuda(waveform, noise, snr, lengths):
    lead = _add_noise_check(waveform, noise, snr, lengths)
    _same_device('add_noise', waveform, noise, snr, *(() if lengths is None else (lengths,)))
    shape = lead + (int(waveform.shape[-1]),)
    dtype = torch.result_type(waveform, noise)
    snr = _add_noise_snr(snr, dtype)
    if 0 in shape:
        return torch.empty(shape, dtype=dtype, device=waveform.device)          # an empty output: nothing is launched
    reason = _hip_dtype(waveform, noise, snr)
    if reason is None:
        wave32, noise32 = _f32(waveform), _f32(noise)
        reason = H.add_noise_reason(lead, wave32, noise32)
    if reason is not None:
        _composite_route('add_noise', reason)
        return C.add_noise(waveform, noise, snr, lengths)
    out = H.add_noise_rows(wave32, noise32, snr, lengths, lead)
    return out if dtype == out.dtype else out.to(dtype)


def _add_noise_fake(waveform, noise, snr, lengths):
    lead = _add_noise_check(waveform, noise, snr, lengths)
    return waveform.new_empty(lead + (waveform.shape[-1],), dtype=torch.result_type(waveform, noise))


def _add_noise_cpu(waveform, noise, snr, lengths):
    _add_noise_check(waveform, noise, snr, lengths)
    return C.add_noise(waveform, noise, _add_noise_snr(snr, torch.result_type(waveform, noise)), lengths)


_register('add_noise', '(Tensor waveform, Tensor noise, Tensor snr, Tensor? lengths) -> Tensor', _add_noise_cuda, _add_noise_cpu,
          _add_noise_fake, 3)


# ============================================================================= loudness
def loudness_reason(waveform, gate, step):
    """why the two launches of csrc/loudness.hip do not take this call, or None"""
    reason = _hip_dtype(waveform)
    if reason is None and any(st <= 0 for st, n in zip(waveform.stride(), waveform.shape) if n > 1):
        reason = 'non-positive strides'
    if reason is None and gate != 4 * step:
        reason = 'a sample rate whose block of %d samples is not four hops of %d' % (gate, step)
    if reason is None and step < H.LOUDNESS_MIN_STEP:
        reason = 'a hop of %d samples (the kernel takes %d or more)' % (step, H.LOUDNESS_MIN_STEP)
    return reason


def _loudness_cuda(waveform, sample_rate):
    gate, step = FL.loudness_check(waveform, sample_rate)
    if 0 in waveform.shape[:-2]:
        return waveform.new_empty(tuple(waveform.shape[:-2]))       # an empty batch: nothing is launched
    reason = loudness_reason(waveform, gate, step)
    if reason is not None:
        _composite_route('loudness', reason)
        return C.loudness(waveform, sample_rate)
    out = H.loudness_entries(_f32(waveform), FL.k_weighting(sample_rate), gate, step)
    return out if waveform.dtype == out.dtype else out.to(waveform.dtype)


def _loudness_cpu(waveform, sample_rate):
    FL.loudness_check(waveform, sample_rate)
    if 0 in waveform.shape[:-2]:
        return waveform.new_empty(tuple(waveform.shape[:-2]))
    return C.loudness(waveform, sample_rate)


def _loudness_fake(waveform, sample_rate):
    return waveform.new_empty(tuple(waveform.shape[:-2]))


# (no gradient kernel: the backward pass re-evaluates the definition with torch operators, announced, as kaldi_fbank's does)
_register('loudness', '(Tensor waveform, int sample_rate) -> Tensor', _loudness_cuda, _loudness_cpu, _loudness_fake, 1)


# ============================================================================= detect_pitch_frequency
def pitch_reason(waveform, sample_rate, frame_time=1e-2, win_length=30, freq_low=85, freq_high=3400):
    """why the two launches of csrc/pitch.hip do not take this call, or None"""
    geo = PT.check(waveform, sample_rate, frame_time, win_length, freq_low, freq_high)
    reason = _hip_dtype(waveform)
    if reason is None and any(st <= 0 for st, n in zip(waveform.stride(), waveform.shape) if n > 1):
        reason = 'non-positive strides'
    if reason is None and (sample_rate >= 2 ** 31 or waveform.shape[-1] >= 2 ** 40):
        reason = 'a sample rate of %d over %d samples (beyond the launch\'s int32 rate and lags)' % (sample_rate, waveform.shape[-1])
    if reason is None and win_length > H.PITCH_MAX_WIN:
        reason = 'a median window of %d lags (the kernel takes %d or fewer)' % (win_length, H.PITCH_MAX_WIN)
    if reason is None and H.pitch_plan(geo.n_frames, geo.frame, geo.max_lag) is None:
        reason = 'frames of %d samples and %d lags (beyond the LDS plan of the correlation launch)' % (geo.frame, geo.max_lag)
    return reason


def _pitch_cuda(waveform, sample_rate, frame_time, win_length, freq_low, freq_high):
    geo = PT.check(waveform, sample_rate, frame_time, win_length, freq_low, freq_high)
    if 0 in waveform.shape[:-1]:
        return waveform.new_empty(tuple(waveform.shape[:-1]) + (geo.n_out,), dtype=torch.float32)     # nothing is launched
    reason = pitch_reason(waveform, sample_rate, frame_time, win_length, freq_low, freq_high)
    if reason is not None:
        _composite_route('detect_pitch_frequency', reason)
        return C.detect_pitch_frequency(waveform, sample_rate, frame_time, win_length, freq_low, freq_high)
    return H.pitch_frequency(_f32(waveform), int(sample_rate), geo.frame, geo.max_lag, geo.lag_min, win_length)


def _pitch_cpu(waveform, sample_rate, frame_time, win_length, freq_low, freq_high):
    geo = PT.check(waveform, sample_rate, frame_time, win_length, freq_low, freq_high)
    if 0 in waveform.shape[:-1]:
        return waveform.new_empty(tuple(waveform.shape[:-1]) + (geo.n_out,), dtype=torch.float32)
    return C.detect_pitch_frequency(waveform, sample_rate, frame_time, win_length, freq_low, freq_high)


def _pitch_fake(waveform, sample_rate, frame_time, win_length, freq_low, freq_high):
    geo = PT.geometry(waveform.shape[-1], sample_rate, frame_time, win_length, freq_low, freq_high)
    return waveform.new_empty(tuple(waveform.shape[:-1]) + (geo.n_out,), dtype=torch.float32)


# (no autograd: the result is piecewise constant in the waveform and carries no gradient, as torchaudio's carries none)
_register('detect_pitch_frequency', '(Tensor waveform, int sample_rate, float frame_time, int win_length, float freq_low, '
          'float freq_high) -> Tensor', _pitch_cuda, _pitch_cpu, _pitch_fake, 1, differentiable=False)


# ============================================================================= vad_measures, vad_start
_VAD_ARGS = ', '.join('float %s' % name for name in VD.ARGS)


def vad_reason(waveform, sample_rate, *args):
    """why the launches of csrc/vad.hip (behind ``tac_spectrogram_f32``) do not take this call, or None"""
    p = VD.check(waveform, sample_rate, *args)
    reason = _hip_dtype(waveform)
    if reason is None and any(st <= 0 for st, n in zip(waveform.stride(), waveform.shape) if n > 1):
        reason = 'expanded or non-positive strides'
    if reason is None and not H.vad_covers_dft(p.dft):
        reason = 'measurement windows of %d samples (a transform of %d points is none of the spectrogram kernels\')' % (p.mlen, p.dft)
    if reason is None and (p.period >= 2 ** 31 or waveform.shape[-1] >= 2 ** 40):
        reason = 'a period of %d over %d samples (beyond the launches\' int32 hop)' % (p.period, waveform.shape[-1])
    if reason is None and H.vad_limits(p) is None:
        reason = '%d spectrum and %d cepstrum bins (beyond the registers and the LDS plan of the measuring launch)' % (p.s1 - p.s0, p.c1 - p.c0)
    if reason is None and p.n > H.vad_max_search():
        reason = 'a search of %d measures (the deciding launch takes %d or fewer)' % (p.n, H.vad_max_search())
    return reason


def _vad_dtype(waveform):
    return torch.float64 if waveform.dtype == torch.float64 else torch.float32


def _vad_measures_cuda(waveform, sample_rate, *args):
    p = VD.check(waveform, sample_rate, *args)
    n_frames = VD.frames(waveform.shape[-1], p)
    if 0 in waveform.shape[:-1] or n_frames == 0:
        return waveform.new_empty(tuple(waveform.shape[:-1]) + (n_frames,), dtype=_vad_dtype(waveform))      # nothing is launched
    reason = vad_reason(waveform, sample_rate, *args)
    if reason is not None:
        _composite_route('vad_measures', reason)
        return C.vad_measures(waveform, p)
    return H.vad_measures(_f32(waveform), p)


def _vad_measures_cpu(waveform, sample_rate, *args):
    return C.vad_measures(waveform, VD.check(waveform, sample_rate, *args))


def _vad_measures_fake(waveform, sample_rate, *args):
    p = VD.plan(sample_rate, *args)
    return waveform.new_empty(tuple(waveform.shape[:-1]) + (VD.frames(waveform.shape[-1], p),), dtype=_vad_dtype(waveform))


def _vad_start_empty(waveform, p, lead, channels):
    """the result without a row to measure: no group at all, or (``joint='all'``) a group of no channel, which never triggers"""
    if 0 in lead:
        return waveform.new_empty(lead, dtype=torch.int64), waveform.new_empty(lead, dtype=torch.bool)
    return (torch.full(lead, max(waveform.shape[-1] - p.keep, 0), dtype=torch.int64, device=waveform.device),
            torch.zeros(lead, dtype=torch.bool, device=waveform.device))


def _vad_start_composite(waveform, p, lead, channels):
    meas = C.vad_measures(waveform, p)
    start, triggered = C.vad_start(meas.reshape(math.prod(lead), channels, meas.shape[-1]), p, waveform.shape[-1])
    return start.reshape(lead), triggered.reshape(lead)


def _vad_start_cuda(waveform, sample_rate, *rest):
    args, joint = rest[:-1], rest[-1]
    p = VD.check(waveform, sample_rate, *args)
    lead, channels = VD.groups(waveform.shape, joint)
    if 0 in lead or channels == 0:
        return _vad_start_empty(waveform, p, lead, channels)                  # nothing is launched
    reason = vad_reason(waveform, sample_rate, *args)
    if reason is not None:
        _composite_route('vad_start', reason)
        return _vad_start_composite(waveform, p, lead, channels)
    start, triggered = H.vad_start(_f32(waveform), p, math.prod(lead), channels)
    return start.reshape(lead), triggered.reshape(lead)


def _vad_start_cpu(waveform, sample_rate, *rest):
    args, joint = rest[:-1], rest[-1]
    p = VD.check(waveform, sample_rate, *args)
    lead, channels = VD.groups(waveform.shape, joint)
    if 0 in lead or channels == 0:
        return _vad_start_empty(waveform, p, lead, channels)
    return _vad_start_composite(waveform, p, lead, channels)


def _vad_start_fake(waveform, sample_rate, *rest):
    lead, _ = VD.groups(waveform.shape, rest[-1])
    return waveform.new_empty(lead, dtype=torch.int64), waveform.new_empty(lead, dtype=torch.bool)


# (no autograd: the measures feed a decision and the result is an index)
_register('vad_measures', '(Tensor waveform, int sample_rate, %s) -> Tensor' % _VAD_ARGS, _vad_measures_cuda, _vad_measures_cpu,
          _vad_measures_fake, 1, differentiable=False)
_register('vad_start', '(Tensor waveform, int sample_rate, %s, str joint) -> (Tensor, Tensor)' % _VAD_ARGS, _vad_start_cuda, _vad_start_cpu,
          _vad_start_fake, 1, differentiable=False)


# ============================================================================= rir_ism, rir_ism_span
_RIR_GEOMETRY = 'int max_order, int delay_filter_length, float sound_speed, float sample_rate'


def rir_reason(room, source, mic_array, absorption, max_order, delay_filter_length):
    """why the launch of csrc/rir.hip does not take this call, or None"""
    tensors = (room, source, mic_array) + (() if absorption is None else (absorption,))
    reason = None
    for t in tensors:                      # (no widening here: the geometry is read as given, and half has no room for it)
        if t.dtype != torch.float32:
            reason = 'dtype %s' % str(t.dtype).replace('torch.', '')
            break
    if reason is None and any(st <= 0 for t in tensors for st, n in zip(t.stride(), t.shape) if n > 1):
        reason = 'expanded or non-positive strides'
    _, max_bands, max_taps, top_order = H.rir_limits()
    if reason is None and absorption is not None and absorption.shape[1] > max_bands:
        reason = '%d absorption bands (the kernel takes %d or fewer)' % (absorption.shape[1], max_bands)
    if reason is None and not 3 <= delay_filter_length <= max_taps:
        reason = 'a delay filter of %d taps (the kernel takes 3 to %d)' % (delay_filter_length, max_taps)
    if reason is None and max_order > top_order:
        reason = 'max_order %d (the kernel takes %d or lower)' % (max_order, top_order)
    return reason


def _rir_out_dtype(*tensors):
    return torch.float64 if any(t.dtype == torch.float64 for t in tensors) else torch.float32


def _rir_cuda(room, source, mic_array, absorption, max_order, start, length, delay_filter_length, sound_speed, sample_rate):
    _same_device('rir_ism', room, source, mic_array, absorption)
    B, M, nb = room.shape[0], mic_array.shape[1], absorption.shape[1]
    if B == 0 or M == 0:
        return room.new_empty((B, nb, M, length), dtype=_rir_out_dtype(room, source, mic_array, absorption))     # nothing is launched
    reason = rir_reason(room, source, mic_array, absorption, max_order, delay_filter_length)
    if reason is not None:
        _composite_route('rir_ism', reason)
        return C.rir_ism(room, source, mic_array, absorption, max_order, start, length, delay_filter_length, sound_speed, sample_rate)
    return H.rir_ism(room.contiguous(), source.contiguous(), mic_array.contiguous(), absorption.contiguous(), max_order, start, length,
                     delay_filter_length, sound_speed, sample_rate)


def _rir_cpu(room, source, mic_array, absorption, max_order, start, length, delay_filter_length, sound_speed, sample_rate):
    B, M, nb = room.shape[0], mic_array.shape[1], absorption.shape[1]
    if B == 0 or M == 0:
        return room.new_empty((B, nb, M, length), dtype=_rir_out_dtype(room, source, mic_array, absorption))
    return C.rir_ism(room, source, mic_array, absorption, max_order, start, length, delay_filter_length, sound_speed, sample_rate)


def _rir_fake(room, source, mic_array, absorption, max_order, start, length, delay_filter_length, sound_speed, sample_rate):
    return room.new_empty((room.shape[0], absorption.shape[1], mic_array.shape[1], length),
                          dtype=_rir_out_dtype(room, source, mic_array, absorption))


def _rir_span_cuda(room, source, mic_array, max_order, delay_filter_length, sound_speed, sample_rate):
    _same_device('rir_ism_span', room, source, mic_array)
    reason = rir_reason(room, source, mic_array, None, 0, 3)            # (the span has no limit on order or taps)
    if reason is not None:
        _composite_route('rir_ism_span', reason)
        return C.rir_ism_span(room, source, mic_array, max_order, delay_filter_length, sound_speed, sample_rate)
    return H.rir_ism_span(room.contiguous(), source.contiguous(), mic_array.contiguous(), max_order, delay_filter_length, sound_speed,
                          sample_rate)


def _rir_span_fake(room, source, mic_array, max_order, delay_filter_length, sound_speed, sample_rate):
    return room.new_empty((), dtype=torch.int64)


# (no gradient kernel: the backward pass differentiates the definition in torch operators, announced, as loudness's does)
_register('rir_ism', '(Tensor room, Tensor source, Tensor mic_array, Tensor absorption, int max_order, int start, int length, '
          'int delay_filter_length, float sound_speed, float sample_rate) -> Tensor', _rir_cuda, _rir_cpu, _rir_fake, 4)
_register('rir_ism_span', '(Tensor room, Tensor source, Tensor mic_array, %s) -> Tensor' % _RIR_GEOMETRY, _rir_span_cuda, C.rir_ism_span,
          _rir_span_fake, 3, differentiable=False)


# ============================================================================= psd, mvdr_weights_souden, apply_beamforming, mvdr_souden
# Complex values are trailing-2 pairs here; an absent mask / reference vector is the empty tensor BF.none(like).
def beamform_reason(channels, *tensors):
    """why the kernels of csrc/beamform.hip do not take these tensors, or None"""
    tensors = [t for t in tensors if not BF.absent(t)]
    reason = _hip_dtype(*tensors)
    if reason is None and not BF.MIN_CHANNELS <= channels <= BF.MAX_CHANNELS:
        reason = '%d channels (the kernels take %d to %d)' % (channels, BF.MIN_CHANNELS, BF.MAX_CHANNELS)
    if reason is None and any(st <= 0 for t in tensors for st, n in zip(t.stride(), t.shape) if n > 1):
        reason = 'expanded or non-positive strides'
    return reason


def _bf_opt(t):
    return None if BF.absent(t) else _f32(t)


def _psd_shape(spec):
    lead, ch, F, T = BF.spec_shape(spec)
    return lead + (F, ch, ch, 2)


def _psd_cuda(spec, mask, normalize, eps):
    _same_device('psd', spec, mask)
    lead, ch, F, T = BF.spec_shape(spec)
    if 0 in spec.shape:
        return spec.new_zeros(_psd_shape(spec), dtype=_out_dtype(spec))               # nothing is launched
    reason = beamform_reason(ch, spec, mask)
    if reason is not None:
        _composite_route('psd', reason)
        return C.psd(spec, mask, normalize, eps)
    return H.psd(_f32(spec), _bf_opt(mask), normalize=normalize, eps=eps)


def _psd_fake(spec, mask, normalize, eps):
    return spec.new_empty(_psd_shape(spec), dtype=_out_dtype(spec))


_register('psd', '(Tensor specgram, Tensor mask, bool normalize, float eps) -> Tensor', _psd_cuda, C.psd, _psd_fake, 2)


def _weights_shape(psd_s):
    lead, F, ch = BF.psd_shape(psd_s)
    return lead + (F, ch, 2)


def _weights_cuda(psd_s, psd_n, ref_vector, ref_channel, diagonal_loading, diag_eps, eps):
    _same_device('mvdr_weights_souden', psd_s, psd_n, ref_vector)
    lead, F, ch = BF.psd_shape(psd_s)
    if 0 in psd_s.shape:
        return psd_s.new_zeros(_weights_shape(psd_s), dtype=_out_dtype(psd_s))
    reason = beamform_reason(ch, psd_s, psd_n)
    if reason is None and not BF.absent(ref_vector) and any(st < 0 for st in ref_vector.stride()):
        reason = 'expanded or non-positive strides'
    if reason is not None:
        _composite_route('mvdr_weights_souden', reason)
        return C.mvdr_weights_souden(psd_s, psd_n, ref_vector, ref_channel, diagonal_loading, diag_eps, eps)
    return H.mvdr_weights_souden(_f32(psd_s), _f32(psd_n), None if BF.absent(ref_vector) else ref_vector, ref_channel,
                                 diagonal_loading, diag_eps, eps)


def _weights_fake(psd_s, psd_n, ref_vector, ref_channel, diagonal_loading, diag_eps, eps):
    return psd_s.new_empty(_weights_shape(psd_s), dtype=_out_dtype(psd_s))


_register('mvdr_weights_souden', '(Tensor psd_s, Tensor psd_n, Tensor ref_vector, int ref_channel, bool diagonal_loading, '
          'float diag_eps, float eps) -> Tensor', _weights_cuda, C.mvdr_weights_souden, _weights_fake, 3)


def _apply_beamforming_cuda(weights, spec):
    _same_device('apply_beamforming', weights, spec)
    lead, ch, F, T = BF.spec_shape(spec)
    if 0 in spec.shape:
        return _swapped(lead, (T, F, 2), _out_dtype(spec), spec.device, -3, -2).zero_()
    reason = beamform_reason(ch, weights, spec)
    if reason is not None:
        _composite_route('apply_beamforming', reason)
        return C.apply_beamforming(weights, spec)
    return H.apply_beamforming(_f32(weights), _f32(spec))


def _apply_beamforming_fake(weights, spec):
    lead, ch, F, T = BF.spec_shape(spec)
    return _swapped(lead, (T, F, 2), _out_dtype(spec), spec.device, -3, -2)


_register('apply_beamforming', '(Tensor beamform_weights, Tensor specgram) -> Tensor', _apply_beamforming_cuda, C.apply_beamforming,
          _apply_beamforming_fake, 2)


def _mvdr_souden_cuda(spec, mask_s, mask_n, ref_vector, ref_channel, diagonal_loading, diag_eps, eps, psd_eps):
    _same_device('mvdr_souden', spec, mask_s, mask_n, ref_vector)
    lead, ch, F, T = BF.spec_shape(spec)
    if 0 in spec.shape:
        return _swapped(lead, (T, F, 2), _out_dtype(spec), spec.device, -3, -2).zero_()
    reason = beamform_reason(ch, spec, mask_s, mask_n)
    if reason is not None:
        _composite_route('mvdr_souden', reason)
        return C.mvdr_souden(spec, mask_s, mask_n, ref_vector, ref_channel, diagonal_loading, diag_eps, eps, psd_eps)
    return H.mvdr_souden(_f32(spec), _f32(mask_s), _bf_opt(mask_n), None if BF.absent(ref_vector) else ref_vector, ref_channel,
                         diagonal_loading, diag_eps, eps, psd_eps)[0]


def _mvdr_souden_fake(spec, mask_s, mask_n, ref_vector, ref_channel, diagonal_loading, diag_eps, eps, psd_eps):
    lead, ch, F, T = BF.spec_shape(spec)
    return _swapped(lead, (T, F, 2), _out_dtype(spec), spec.device, -3, -2)


_register('mvdr_souden', '(Tensor specgram, Tensor mask_s, Tensor mask_n, Tensor ref_vector, int ref_channel, bool diagonal_loading, '
          'float diag_eps, float eps, float psd_eps) -> Tensor', _mvdr_souden_cuda, C.mvdr_souden, _mvdr_souden_fake, 4)


# ============================================================================= rtf_evd, rtf_power, mvdr_weights_rtf, rtf_mvdr
def _ref_reason(reason, ref_vector):
    if reason is None and not BF.absent(ref_vector) and any(st < 0 for st in ref_vector.stride()):
        reason = 'expanded or non-positive strides'
    return reason


def _rtf_evd_cuda(psd_s):
    lead, F, ch = BF.psd_shape(psd_s)
    if 0 in psd_s.shape:
        return psd_s.new_zeros(_weights_shape(psd_s), dtype=_out_dtype(psd_s))
    reason = beamform_reason(ch, psd_s)
    if reason is not None:
        _composite_route('rtf_evd', reason)
        return C.rtf_evd(psd_s)
    return H.rtf_evd(_f32(psd_s))


def _rtf_evd_fake(psd_s):
    return psd_s.new_empty(_weights_shape(psd_s), dtype=_out_dtype(psd_s))


_register('rtf_evd', '(Tensor psd_s) -> Tensor', _rtf_evd_cuda, C.rtf_evd, _rtf_evd_fake, 1)


def _rtf_power_cuda(psd_s, psd_n, ref_vector, ref_channel, n_iter, diagonal_loading, diag_eps):
    _same_device('rtf_power', psd_s, psd_n, ref_vector)
    lead, F, ch = BF.psd_shape(psd_s)
    if 0 in psd_s.shape:
        return psd_s.new_zeros(_weights_shape(psd_s), dtype=_out_dtype(psd_s))
    reason = _ref_reason(beamform_reason(ch, psd_s, psd_n), ref_vector)
    if reason is None and n_iter > H.rtf_power_max_iter():
        reason = 'n_iter %d (the kernel takes up to %d)' % (n_iter, H.rtf_power_max_iter())
    if reason is not None:
        _composite_route('rtf_power', reason)
        return C.rtf_power(psd_s, psd_n, ref_vector, ref_channel, n_iter, diagonal_loading, diag_eps)
    return H.rtf_power(_f32(psd_s), _f32(psd_n), None if BF.absent(ref_vector) else ref_vector, ref_channel, n_iter,
                       diagonal_loading, diag_eps)


def _rtf_power_fake(psd_s, psd_n, ref_vector, ref_channel, n_iter, diagonal_loading, diag_eps):
    return psd_s.new_empty(_weights_shape(psd_s), dtype=_out_dtype(psd_s))


_register('rtf_power', '(Tensor psd_s, Tensor psd_n, Tensor ref_vector, int ref_channel, int n_iter, bool diagonal_loading, '
          'float diag_eps) -> Tensor', _rtf_power_cuda, C.rtf_power, _rtf_power_fake, 3)


def _weights_rtf_cuda(rtf, psd_n, ref_vector, ref_channel, diagonal_loading, diag_eps, eps):
    _same_device('mvdr_weights_rtf', rtf, psd_n, ref_vector)
    lead, F, ch = BF.psd_shape(psd_n)
    if 0 in psd_n.shape:
        return rtf.new_zeros(tuple(rtf.shape), dtype=_out_dtype(rtf))
    reason = _ref_reason(beamform_reason(ch, rtf, psd_n), ref_vector)
    if reason is not None:
        _composite_route('mvdr_weights_rtf', reason)
        return C.mvdr_weights_rtf(rtf, psd_n, ref_vector, ref_channel, diagonal_loading, diag_eps, eps)
    return H.mvdr_weights_rtf(_f32(rtf), _f32(psd_n), None if BF.absent(ref_vector) else ref_vector, ref_channel, diagonal_loading,
                              diag_eps, eps)


def _weights_rtf_fake(rtf, psd_n, ref_vector, ref_channel, diagonal_loading, diag_eps, eps):
    return rtf.new_empty(tuple(rtf.shape), dtype=_out_dtype(rtf))


_register('mvdr_weights_rtf', '(Tensor rtf, Tensor psd_n, Tensor ref_vector, int ref_channel, bool diagonal_loading, float diag_eps, '
          'float eps) -> Tensor', _weights_rtf_cuda, C.mvdr_weights_rtf, _weights_rtf_fake, 3)


def _rtf_mvdr_cuda(spec, rtf, psd_n, ref_vector, ref_channel, diagonal_loading, diag_eps, eps):
    _same_device('rtf_mvdr', spec, rtf, psd_n, ref_vector)
    lead, ch, F, T = BF.spec_shape(spec)
    if 0 in spec.shape:
        return _swapped(lead, (T, F, 2), _out_dtype(spec), spec.device, -3, -2).zero_()
    reason = _ref_reason(beamform_reason(ch, spec, rtf, psd_n), ref_vector)
    if reason is not None:
        _composite_route('rtf_mvdr', reason)
        return C.rtf_mvdr(spec, rtf, psd_n, ref_vector, ref_channel, diagonal_loading, diag_eps, eps)
    return H.rtf_mvdr(_f32(spec), _f32(rtf), _f32(psd_n), None if BF.absent(ref_vector) else ref_vector, ref_channel,
                      diagonal_loading, diag_eps, eps)[0]


def _rtf_mvdr_fake(spec, rtf, psd_n, ref_vector, ref_channel, diagonal_loading, diag_eps, eps):
    lead, ch, F, T = BF.spec_shape(spec)
    return _swapped(lead, (T, F, 2), _out_dtype(spec), spec.device, -3, -2)


_register('rtf_mvdr', '(Tensor specgram, Tensor rtf, Tensor psd_n, Tensor ref_vector, int ref_channel, bool diagonal_loading, '
          'float diag_eps, float eps) -> Tensor', _rtf_mvdr_cuda, C.rtf_mvdr, _rtf_mvdr_fake, 4)


# ============================================================================= rnnt_loss, rnnt_loss_grad
def rnnt_check(logits, targets, logit_lengths, target_lengths, blank):
    """torchaudio's argument checks of ``rnnt_loss`` that need no device memory, and for CPU tensors the two that do (the longest
    logit length is T, the longest target length is U); returns ``blank`` counted from the front.  On a HIP device the lengths
    and targets are not read on the host: an entry outside its ranges ends as NaN (``functional.rnnt_loss``)."""
    if not (isinstance(logits, torch.Tensor) and logits.is_floating_point()):
        raise ValueError('rnnt_loss: logits must be a floating-point tensor')
    for name, t, dim in (('targets', targets, 2), ('logit_lengths', logit_lengths, 1), ('target_lengths', target_lengths, 1)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise ValueError('rnnt_loss: %s must be an int32 tensor' % name)
        if t.dim() != dim:
            raise ValueError('rnnt_loss: %s must have %d dimension(s), got %d' % (name, dim, t.dim()))
    if logits.dim() != 4:
        raise ValueError('rnnt_loss: logits must be (batch, time, target + 1, class), got %d dimension(s)' % logits.dim())
    B, T, U1, V = logits.shape
    if T < 1 or U1 < 1 or V < 1:
        raise ValueError('rnnt_loss: logits of shape %r have an empty time, target or class axis' % (tuple(logits.shape),))
    if tuple(targets.shape) != (B, U1 - 1):
        raise ValueError('rnnt_loss: targets of shape %r do not match logits of shape %r: expected (%d, %d)'
                         % (tuple(targets.shape), tuple(logits.shape), B, U1 - 1))
    if logit_lengths.shape[0] != B or target_lengths.shape[0] != B:
        raise ValueError('rnnt_loss: %d logit lengths and %d target lengths for a batch of %d'
                         % (logit_lengths.shape[0], target_lengths.shape[0], B))
    if not -V <= blank < V:
        raise ValueError('rnnt_loss: blank %d is outside the %d classes' % (blank, V))
    _same_device('rnnt_loss', logits, targets, logit_lengths, target_lengths)
    if B and not logits.is_cuda and logits.device.type == 'cpu':
        if int(logit_lengths.max()) != T:
            raise ValueError('rnnt_loss: the longest logit length is %d, the time axis of the logits %d' % (int(logit_lengths.max()), T))
        if int(target_lengths.max()) != U1 - 1:
            raise ValueError('rnnt_loss: the longest target length is %d, the target axis of the logits %d + 1'
                             % (int(target_lengths.max()), U1 - 1))
    return blank + V if blank < 0 else blank


def _rnnt_work_dtype(logits):
    return torch.float64 if logits.dtype == torch.float64 else torch.float32


def rnnt_reason(logits):
    """why the launches of csrc/rnnt.hip do not take these logits, or None"""
    if logits.dtype != torch.float32:
        return 'dtype %s' % str(logits.dtype).replace('torch.', '')
    return H.rnnt_reason(logits)


def _rnnt_empty(logits):
    B, T, U1, V = logits.shape
    w = _rnnt_work_dtype(logits)
    return (logits.new_empty((B,)),) + tuple(logits.new_empty((B, T, U1), dtype=w) for _ in range(3))


def _rnnt_loss_cuda(logits, targets, logit_lengths, target_lengths, blank, clamp, fused):
    blank = rnnt_check(logits, targets, logit_lengths, target_lengths, blank)
    if logits.shape[0] == 0:
        return _rnnt_empty(logits)                                  # an empty batch: nothing is launched
    reason = rnnt_reason(logits)
    if reason is not None:
        _composite_route('rnnt_loss', reason)
        return C.rnnt_loss(logits, targets, logit_lengths, target_lengths, blank, clamp, fused)
    return H.rnnt_forward(logits, targets, logit_lengths, target_lengths, blank, fused)


def _rnnt_loss_cpu(logits, targets, logit_lengths, target_lengths, blank, clamp, fused):
    blank = rnnt_check(logits, targets, logit_lengths, target_lengths, blank)
    if logits.shape[0] == 0:
        return _rnnt_empty(logits)
    return C.rnnt_loss(logits, targets, logit_lengths, target_lengths, blank, clamp, fused)


def _rnnt_loss_fake(logits, targets, logit_lengths, target_lengths, blank, clamp, fused):
    return _rnnt_empty(logits)


def _rnnt_grad_cuda(logits, targets, logit_lengths, target_lengths, alphas, betas, denominators, costs, grad_costs, blank, clamp,
                    fused):
    if logits.numel() == 0:
        return torch.empty(tuple(logits.shape), dtype=logits.dtype, device=logits.device)
    reason = rnnt_reason(logits) or _hip_dtype(grad_costs)
    if reason is None and not _plain_hip_f32(alphas, betas, denominators, costs, grad_costs):
        reason = 'tensor subclass'
    if reason is not None:
        _composite_route('rnnt_loss', 'backward: ' + reason)
        return C.rnnt_loss_grad(logits, targets, logit_lengths, target_lengths, alphas, betas, denominators, costs, grad_costs, blank,
                                clamp, fused)
    return H.rnnt_grad(logits, targets, logit_lengths, target_lengths, alphas, betas, denominators, costs, grad_costs, blank, clamp,
                       fused)


def _rnnt_grad_fake(logits, targets, logit_lengths, target_lengths, alphas, betas, denominators, costs, grad_costs, blank, clamp,
                    fused):
    return torch.empty(tuple(logits.shape), dtype=logits.dtype, device=logits.device)


def _register_rnnt_autograd():
    """Backward of ``tac_amd::rnnt_loss``: the costs are the one differentiable output and the logits the one input with a gradient.
    What the forward pass saved — alphas, betas, denominators, costs: three ``(B, T, U + 1)`` arrays and a vector, nothing of the
    size of the logits — goes to ``tac_amd::rnnt_loss_grad``, which routes like every op (the kernel for float32 on a HIP device,
    the closed form in torch operators otherwise, announced there).  A double backward differentiates the torch-operator recursion
    on the saved logits, announced on a HIP device."""

    def setup_context(ctx, inputs, output):
        logits, targets, logit_lengths, target_lengths, blank, clamp, fused = inputs
        costs, alphas, betas, denominators = output
        ctx.mark_non_differentiable(alphas, betas, denominators)
        ctx.save_for_backward(logits, targets, logit_lengths, target_lengths, alphas, betas, denominators, costs)
        ctx.rest = (blank + logits.shape[-1] if blank < 0 else blank, clamp, fused)

    def backward(ctx, g, *unused):
        logits, targets, logit_lengths, target_lengths, alphas, betas, denominators, costs = ctx.saved_tensors
        blank, clamp, fused = ctx.rest
        if g is None or not ctx.needs_input_grad[0]:
            return (None,) * 7
        if torch.is_grad_enabled():                                 # keep the graph: the saved logits are the caller's own
            if logits.is_cuda:
                _composite_route('rnnt_loss', 'backward: double backward (create_graph=True)')
            with torch.enable_grad():
                again = C.rnnt_loss(logits, targets, logit_lengths, target_lengths, blank, clamp, fused)[0]
                (per_entry,) = torch.autograd.grad(again.sum(), logits, create_graph=True)
                if clamp > 0:
                    per_entry = per_entry.clamp(-clamp, clamp)
                grad = per_entry * g.to(per_entry.dtype)[:, None, None, None]
        else:
            grad = call('rnnt_loss_grad', logits, targets, logit_lengths, target_lengths, alphas, betas, denominators, costs, g, blank,
                        clamp, fused)
        return (grad,) + (None,) * 6

    torch.library.register_autograd('%s::rnnt_loss' % NS, backward, setup_context=setup_context, lib=_lib)


_register('rnnt_loss', '(Tensor logits, Tensor targets, Tensor logit_lengths, Tensor target_lengths, int blank, float clamp, '
          'bool fused_log_softmax) -> (Tensor, Tensor, Tensor, Tensor)', _rnnt_loss_cuda, _rnnt_loss_cpu, _rnnt_loss_fake, 1,
          differentiable=False)
_register_rnnt_autograd()
_register('rnnt_loss_grad', '(Tensor logits, Tensor targets, Tensor logit_lengths, Tensor target_lengths, Tensor alphas, Tensor betas, '
          'Tensor denominators, Tensor costs, Tensor grad_costs, int blank, float clamp, bool fused_log_softmax) -> Tensor',
          _rnnt_grad_cuda, C.rnnt_loss_grad, _rnnt_grad_fake, 1, differentiable=False)


# ============================================================================= forced_align
def align_check(log_probs, targets, input_lengths, target_lengths, blank):
    """the argument checks of ``forced_align`` that need no device memory: dimensions, dtypes, ``blank`` in ``[0, C)``, batch
    sizes, one device, no empty time or class axis.  ``ValueError`` on every route."""
    if not (isinstance(log_probs, torch.Tensor) and log_probs.is_floating_point()):
        raise ValueError('forced_align: log_probs must be a floating-point tensor')
    if not isinstance(targets, torch.Tensor) or targets.dtype not in (torch.int32, torch.int64):
        raise ValueError('forced_align: targets must be an int32 or int64 tensor')
    if log_probs.dim() != 3:
        raise ValueError('forced_align: log_probs must be (batch, time, class), got %d dimension(s)' % log_probs.dim())
    if targets.dim() != 2:
        raise ValueError('forced_align: targets must be (batch, target), got %d dimension(s)' % targets.dim())
    B, T, C = log_probs.shape
    if T < 1 or C < 1:
        raise ValueError('forced_align: log_probs of shape %r have an empty time or class axis' % (tuple(log_probs.shape),))
    if targets.shape[0] != B:
        raise ValueError('forced_align: targets for a batch of %d, log_probs for a batch of %d' % (targets.shape[0], B))
    for name, t in (('input_lengths', input_lengths), ('target_lengths', target_lengths)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError('forced_align: %s must be an integer tensor or None' % name)
        if t.dim() != 1 or t.shape[0] != B:
            raise ValueError('forced_align: %s must have shape (%d,), got %r' % (name, B, tuple(t.shape)))
        if t.device != log_probs.device:
            raise ValueError('forced_align: %s is on %s, log_probs on %s' % (name, t.device, log_probs.device))
    if targets.device != log_probs.device:
        raise ValueError('forced_align: targets are on %s, log_probs on %s' % (targets.device, log_probs.device))
    if not 0 <= blank < C:
        raise ValueError('forced_align: blank %d is outside the %d classes' % (blank, C))
    return blank


def align_check_values(log_probs, targets, input_lengths, target_lengths, blank):
    """for CPU tensors, what torchaudio's own checks refuse, by entry: lengths out of range, a blank or an out-of-range index among
    the used targets, fewer frames than targets plus repeats"""
    B, T, C = log_probs.shape
    L = targets.shape[1]
    for b in range(B):
        Tb = T if input_lengths is None else int(input_lengths[b])
        Lb = L if target_lengths is None else int(target_lengths[b])
        if not 1 <= Tb <= T:
            raise ValueError('forced_align: entry %d: input length %d is outside [1, %d]' % (b, Tb, T))
        if not 0 <= Lb <= L:
            raise ValueError('forced_align: entry %d: target length %d is outside [0, %d]' % (b, Lb, L))
        used = targets[b, :Lb].tolist()
        if any(v == blank for v in used):
            raise ValueError('forced_align: entry %d: targets must not contain the blank index %d' % (b, blank))
        if any(v < 0 or v >= C for v in used):
            raise ValueError('forced_align: entry %d: a target is outside the %d classes' % (b, C))
        repeats = sum(1 for i in range(1, Lb) if used[i] == used[i - 1])
        if Tb < Lb + repeats:
            raise ValueError('forced_align: entry %d: %d frames cannot hold %d targets with %d repeats' % (b, Tb, Lb, repeats))


def align_reason(log_probs, targets):
    """why the launch of csrc/align.hip does not take these inputs, or None"""
    if log_probs.dtype != torch.float32:
        return 'dtype %s' % str(log_probs.dtype).replace('torch.', '')
    return H.align_reason(log_probs, targets)


def _align_empty(log_probs, targets):
    B, T, C = log_probs.shape
    return (torch.empty((B, T), dtype=targets.dtype, device=log_probs.device),
            torch.empty((B, T), dtype=log_probs.dtype, device=log_probs.device))


def _align_cuda(log_probs, targets, input_lengths, target_lengths, blank):
    align_check(log_probs, targets, input_lengths, target_lengths, blank)
    if log_probs.shape[0] == 0:
        return _align_empty(log_probs, targets)                     # an empty batch: nothing is launched
    reason = align_reason(log_probs, targets)
    if reason is not None:
        _composite_route('forced_align', reason)
        return C.forced_align(log_probs, targets, input_lengths, target_lengths, blank)
    return H.forced_align(log_probs.detach(), targets, input_lengths, target_lengths, blank)


def _align_cpu(log_probs, targets, input_lengths, target_lengths, blank):
    align_check(log_probs, targets, input_lengths, target_lengths, blank)
    if log_probs.shape[0] == 0:
        return _align_empty(log_probs, targets)
    align_check_values(log_probs, targets, input_lengths, target_lengths, blank)
    paths, scores = C.forced_align(log_probs.detach(), targets, input_lengths, target_lengths, blank)
    return paths, scores


def _align_fake(log_probs, targets, input_lengths, target_lengths, blank):
    return _align_empty(log_probs, targets)


def _register_align_autograd():
    """Backward of ``tac_amd::forced_align``: ``paths`` carries no gradient, and ``scores`` is a gather of ``log_probs`` at ``paths``,
    so its gradient is a scatter of ``grad_scores`` into zeros there (frames ``t >= Tb`` and refused entries hold constants: no
    gradient).  Torch operators, announced on a HIP device like every other use of them there."""

    def setup_context(ctx, inputs, output):
        log_probs = inputs[0]
        paths, scores = output
        ctx.mark_non_differentiable(paths)
        ctx.save_for_backward(paths, inputs[2])
        ctx.like = (tuple(log_probs.shape), log_probs.dtype, log_probs.device)

    def backward(ctx, grad_paths, g):
        paths, input_lengths = ctx.saved_tensors
        shape, dtype, dev = ctx.like
        if g is None or not ctx.needs_input_grad[0]:
            return (None,) * 5
        if dev.type == 'cuda':
            _composite_route('forced_align', 'backward: the scatter of grad_scores at paths')
        live = paths >= 0
        if input_lengths is not None:
            live = live & (torch.arange(shape[1], device=dev)[None, :] < input_lengths[:, None])
        grad = torch.zeros(shape, dtype=dtype, device=dev)
        grad.scatter_(2, paths.clamp(min=0).long()[:, :, None], torch.where(live, g.to(dtype), g.new_zeros(()).to(dtype))[:, :, None])
        return (grad,) + (None,) * 4

    torch.library.register_autograd('%s::forced_align' % NS, backward, setup_context=setup_context, lib=_lib)


_register('forced_align', '(Tensor log_probs, Tensor targets, Tensor? input_lengths, Tensor? target_lengths, int blank) -> '
          '(Tensor, Tensor)', _align_cuda, _align_cpu, _align_fake, 2, differentiable=False)
_register_align_autograd()


# ============================================================================= lfilter
def _lfilter_cuda(wave, a_coeffs, b_coeffs, clamp):
    if wave.numel() == 0:
        return torch.empty_like(wave, memory_format=torch.contiguous_format)
    reason = _hip_dtype(wave)
    if reason is None and a_coeffs.numel() > H.LFILTER_MAX_COEFFS:
        reason = 'filter order %d (the kernel takes order <= 2)' % (a_coeffs.numel() - 1)
    if reason is None and any(st <= 0 for st, n in zip(wave.stride(), wave.shape) if n > 1):
        reason = 'non-positive strides'
    if reason is None:
        ha, hb = H.host_coeffs(a_coeffs), H.host_coeffs(b_coeffs)
        if not H.lfilter_covers(hb, ha):
            reason = 'a filter whose state transition over one tile overflows float64'
    if reason is not None:
        _composite_route('lfilter', reason)
        return C.lfilter(wave, a_coeffs, b_coeffs, clamp)
    out = H.lfilter_rows(_f32(wave), hb, ha, clamp)
    return out if wave.dtype == out.dtype else out.to(wave.dtype)


def _lfilter_fake(wave, a_coeffs, b_coeffs, clamp):
    return torch.empty_like(wave, memory_format=torch.contiguous_format)


# (the wave alone has to be a float32 HIP tensor for the gradient kernel; the output is saved where the clamp needs its mask)
_register('lfilter', '(Tensor wave, Tensor a_coeffs, Tensor b_coeffs, bool clamp) -> Tensor', _lfilter_cuda, C.lfilter,
          _lfilter_fake, 3, n_plain=1, save_output=lambda inputs: bool(inputs[3]))


# ============================================================================= sosfilt, and the filters run against time
def _sosfilt_reverse_cpu(wave, sos, clamp):
    return C.sosfilt(wave.flip(-1), sos.flip(0), clamp).flip(-1)


def _lfilter_reverse_cpu(wave, a_coeffs, b_coeffs, clamp):
    return C.lfilter(wave.flip(-1), a_coeffs, b_coeffs, clamp).flip(-1)


def _sosfilt_cuda_of(op, reverse, composite):
    def run(wave, sos, clamp):
        if wave.numel() == 0:
            return torch.empty_like(wave, memory_format=torch.contiguous_format)
        reason = _hip_dtype(wave)
        if reason is None and sos.shape[0] > H.SOSFILT_MAX_SECTIONS:
            reason = '%d sections (the kernel takes at most %d)' % (sos.shape[0], H.SOSFILT_MAX_SECTIONS)
        if reason is None and any(st <= 0 for st, n in zip(wave.stride(), wave.shape) if n > 1):
            reason = 'non-positive strides'
        if reason is None:
            hs = H.host_sos(sos)
            if not H.sosfilt_covers(hs):
                reason = 'a section whose state transition over one tile overflows float64'
        if reason is not None:
            _composite_route(op, reason)
            return composite(wave, sos, clamp)
        out = H.sosfilt_rows(_f32(wave), hs, clamp, reverse=reverse)
        return out if wave.dtype == out.dtype else out.to(wave.dtype)
    return run


def _lfilter_reverse_cuda(wave, a_coeffs, b_coeffs, clamp):
    """filtfilt's second half up to order 2: the lfilter kernel's ``reverse`` mode, which ``tac_amd::lfilter``'s schema does not
    expose.  (filtfilt hands over only what ``tac_amd::lfilter`` took just before; everything else is announced.)"""
    if wave.numel() == 0:
        return torch.empty_like(wave, memory_format=torch.contiguous_format)
    reason = _hip_dtype(wave)
    if reason is None and any(st <= 0 for st, n in zip(wave.stride(), wave.shape) if n > 1):
        reason = 'non-positive strides'
    if reason is None:
        ha, hb = H.host_coeffs(a_coeffs), H.host_coeffs(b_coeffs)
        if not H.lfilter_covers(hb, ha):
            reason = 'a filter outside the lfilter kernel'
    if reason is not None:
        _composite_route('lfilter_reverse', reason)
        return _lfilter_reverse_cpu(wave, a_coeffs, b_coeffs, clamp)
    out = H.lfilter_rows(_f32(wave), hb, ha, clamp, reverse=True)
    return out if wave.dtype == out.dtype else out.to(wave.dtype)


def _sosfilt_fake(wave, sos, clamp):
    return torch.empty_like(wave, memory_format=torch.contiguous_format)


# (as lfilter: the wave alone has to be a float32 HIP tensor for the gradient kernel; the output is saved for the clamp's mask.
# The two ``_reverse`` ops are private: filtfilt's second halves, the sections in reverse order and each run from the end of the row.)
_register('sosfilt', '(Tensor wave, Tensor sos, bool clamp) -> Tensor', _sosfilt_cuda_of('sosfilt', False, C.sosfilt), C.sosfilt,
          _sosfilt_fake, 2, n_plain=1, save_output=lambda inputs: bool(inputs[2]))
_register('sosfilt_reverse', '(Tensor wave, Tensor sos, bool clamp) -> Tensor',
          _sosfilt_cuda_of('sosfilt_reverse', True, _sosfilt_reverse_cpu), _sosfilt_reverse_cpu, _sosfilt_fake, 2, n_plain=1,
          save_output=lambda inputs: bool(inputs[2]))
_register('lfilter_reverse', '(Tensor wave, Tensor a_coeffs, Tensor b_coeffs, bool clamp) -> Tensor', _lfilter_reverse_cuda,
          _lfilter_reverse_cpu, _lfilter_fake, 3, n_plain=1, save_output=lambda inputs: bool(inputs[3]))


# ============================================================================= overdrive, phaser, flanger (SoX)
def _sox_layout(wave):
    """None where the SoX kernels read this tensor where it lies or after a plain copy, else the reason they do not: float32 only
    (half precision is not widened: the composites keep the input's dtype), no expanded or reversed views"""
    if wave.dtype != torch.float32:
        return 'dtype %s' % str(wave.dtype).replace('torch.', '')
    if any(st <= 0 for st, n in zip(wave.stride(), wave.shape) if n > 1):
        return 'expanded or non-positive strides'
    return None


def _overdrive_cuda(wave, gain, colour):
    if wave.numel() == 0:
        return torch.empty_like(wave, memory_format=torch.contiguous_format)
    reason = _sox_layout(wave) or SX.inside(SX.OVERDRIVE_RANGES, gain=gain, colour=colour)
    if reason is not None:
        _composite_route('overdrive', reason)
        return C.overdrive(wave, gain, colour)
    return H.overdrive_rows(wave, *SX.overdrive_constants(gain, colour))


def _phaser_cpu(wave, sample_rate, gain_in, gain_out, delay_ms, decay, mod_speed, sinusoidal):
    L, _, table = SX.phaser_plan(sample_rate, delay_ms, mod_speed, sinusoidal)
    return C.phaser(wave, table.tolist(), L, gain_in, gain_out, decay)


def _phaser_cuda(wave, sample_rate, gain_in, gain_out, delay_ms, decay, mod_speed, sinusoidal):
    if wave.numel() == 0:
        return torch.empty_like(wave, memory_format=torch.contiguous_format)
    L, P, table = SX.phaser_plan(sample_rate, delay_ms, mod_speed, sinusoidal)
    reason = _sox_layout(wave) or SX.inside(SX.PHASER_RANGES, gain_in=gain_in, delay_ms=delay_ms, decay=decay, mod_speed=mod_speed)
    if reason is None and not math.isfinite(gain_out):
        reason = 'gain_out = %r' % (gain_out,)
    if reason is None and not H.phaser_covers(L, P):
        reason = 'a delay of %d samples (the kernel holds %d)' % (L, H.PHASER_MAX_DELAY)
    if reason is not None:
        _composite_route('phaser', reason)
        return C.phaser(wave, table.tolist(), L, gain_in, gain_out, decay)
    return H.phaser_rows(wave, table, L, gain_in, gain_out, decay)


def _flanger_plan(wave, sample_rate, delay, depth, regen, width, speed, phase, modulation, interpolation):
    if wave.dim() < 2:
        raise ValueError('flanger: expected a waveform of shape (…, channel, time), got %s' % (tuple(wave.shape),))
    if wave.shape[-2] > SX.FLANGER_MAX_CHANNELS:
        raise ValueError('flanger: at most %d channels, got %d' % (SX.FLANGER_MAX_CHANNELS, wave.shape[-2]))
    return SX.flanger_plan(sample_rate, delay, depth, regen, width, speed, phase, modulation, interpolation, wave.shape[-2])


def _flanger_cpu(wave, sample_rate, delay, depth, regen, width, speed, phase, modulation, interpolation):
    return C.flanger(wave, _flanger_plan(wave, sample_rate, delay, depth, regen, width, speed, phase, modulation, interpolation))


def _flanger_cuda(wave, sample_rate, delay, depth, regen, width, speed, phase, modulation, interpolation):
    plan = _flanger_plan(wave, sample_rate, delay, depth, regen, width, speed, phase, modulation, interpolation)
    if wave.numel() == 0:
        return torch.empty_like(wave, memory_format=torch.contiguous_format)
    reason = _sox_layout(wave) or SX.inside(SX.FLANGER_RANGES, delay=delay, depth=depth, regen=regen, width=width, speed=speed,
                                            phase=phase)
    if reason is None and not H.flanger_covers(plan, wave.shape[-2]):
        reason = 'a delay line of %d samples (the kernel holds %d)' % (plan.Lb, H.FLANGER_MAX_DELAY)
    if reason is not None:
        _composite_route('flanger', reason)
        return C.flanger(wave, plan)
    return H.flanger_rows(wave, plan)


def _sox_fake(wave, *args):
    return torch.empty_like(wave, memory_format=torch.contiguous_format)


# (overdrive's gradient is elementwise torch around lfilter's reverse launch, and needs the output for the clamp's mask; phaser and
# flanger have no gradient kernel: their backward re-evaluates the composites, announced)
_register('overdrive', '(Tensor waveform, float gain, float colour) -> Tensor', _overdrive_cuda, C.overdrive, _sox_fake, 1,
          save_output=lambda inputs: True)
_register('phaser', '(Tensor waveform, float sample_rate, float gain_in, float gain_out, float delay_ms, float decay, float mod_speed, '
          'bool sinusoidal) -> Tensor', _phaser_cuda, _phaser_cpu, _sox_fake, 1)
_register('flanger', '(Tensor waveform, float sample_rate, float delay, float depth, float regen, float width, float speed, float phase, '
          'str modulation, str interpolation) -> Tensor', _flanger_cuda, _flanger_cpu, _sox_fake, 1)


# ============================================================================= complex pairs
def _pairwise_cuda(op, hip_fn, composite_fn):
    def run(z, *args):
        if z.dtype == torch.float64 and z.dim() >= 1 and z.shape[-1] == 2:
            return getattr(H64, op)(z, *args)
        reason = _hip_dtype(z)
        if reason is not None:
            _composite_route(op, reason)
            return composite_fn(z, *args)
        out = hip_fn(_f32(z), *args)
        if z.dtype in _WIDEN:
            out = tuple(o.to(z.dtype) for o in out) if isinstance(out, tuple) else out.to(z.dtype)
        return out
    return run


def _pair_meta(z):
    """Layout of a per-pair result: the kernels keep the (dense) storage order of their input, halved."""
    if z.stride(-1) == 1 and H.is_dense(z) and not any(s % 2 for s, n in zip(z.stride()[:-1], z.shape[:-1]) if n > 1):
        return torch.empty_strided(z.shape[:-1], tuple(s // 2 for s in z.stride()[:-1]), dtype=z.dtype, device=z.device)
    return torch.empty(z.shape[:-1], dtype=z.dtype, device=z.device)


def _like_meta(x, dtype=None):
    return torch.empty_like(x, dtype=dtype) if H.is_dense(x) else torch.empty(x.shape, dtype=dtype or x.dtype,
                                                                              device=x.device)


def _complex_norm_fake(z, power):
    return _pair_meta(z)


_register('complex_norm', '(Tensor z, float power) -> Tensor', _pairwise_cuda('complex_norm', H.complex_norm,
                                                                               C.complex_norm),
          C.complex_norm, _complex_norm_fake, 1)
_register('angle', '(Tensor z) -> Tensor', _pairwise_cuda('angle', H.angle, C.angle), C.angle, _pair_meta, 1)
_register('magphase', '(Tensor z, float power) -> (Tensor, Tensor)', _pairwise_cuda('magphase', H.magphase, C.magphase),
          C.magphase, lambda z, power: (_pair_meta(z), _pair_meta(z)), 1)


# ============================================================================= phase vocoder
def _phase_vocoder_cuda(spec, phase_advance, rate):
    _same_device('phase_vocoder', spec, phase_advance)
    if spec.dtype == torch.float64 and phase_advance.is_floating_point():
        return H.phase_vocoder(spec, rate, phase_advance)          # the float64 kernel (reference's own test dtype)
    reason = _hip_dtype(spec, phase_advance)
    if reason is not None:
        _composite_route('phase_vocoder', reason)
        return C.phase_vocoder(spec, rate, phase_advance)
    out = H.phase_vocoder(_f32(spec), rate, _f32(phase_advance))
    return out if spec.dtype == out.dtype else out.to(spec.dtype)


def _phase_vocoder_cpu(spec, phase_advance, rate):
    return C.phase_vocoder(spec, rate, phase_advance)


def _phase_vocoder_fake(spec, phase_advance, rate):
    n_out = H.phase_vocoder_out_frames(spec.shape[-2], rate)
    return _swapped(spec.shape[:-3], (n_out, spec.shape[-3], 2), spec.dtype, spec.device, -3, -2)


_register('phase_vocoder', '(Tensor spec, Tensor phase_advance, float rate) -> Tensor', _phase_vocoder_cuda,
          _phase_vocoder_cpu, _phase_vocoder_fake, 2)


# ============================================================================= stretch on magnitudes
def _stretch_norm_cuda(mag, rate, power, db, ref, amin):
    reason = _hip_dtype(mag)            # (float64 included: a float64 kernel of this op is not written)
    if reason is not None:
        _composite_route('stretch_norm', reason)
        return C.stretch_norm(mag, rate, power, db, ref, amin)
    out = H.stretch_norm(_f32(mag), rate, power, db, ref, amin)
    return out if mag.dtype == out.dtype else out.to(mag.dtype)


def _stretch_norm_fake(mag, rate, power, db, ref, amin):
    n_out = H.phase_vocoder_out_frames(mag.shape[-1], rate)
    return _swapped(mag.shape[:-2], (n_out, mag.shape[-2]), mag.dtype, mag.device, -2, -1)


_register('stretch_norm', '(Tensor mag, float rate, float power, bool db, float ref, float amin) -> Tensor', _stretch_norm_cuda,
          C.stretch_norm, _stretch_norm_fake, 1)


def _stretch_mel_cuda(mag, bank, rate, power, db, ref, amin):
    _same_device('stretch_mel', mag, bank)
    reason = _hip_dtype(mag, bank)
    if reason is not None:
        _composite_route('stretch_mel', reason)
        return C.stretch_mel(mag, bank, rate, power, db, ref, amin)
    out = H.stretch_mel(_f32(mag), _f32(bank), rate, power, db, ref, amin)
    return out if mag.dtype == out.dtype else out.to(mag.dtype)


def _stretch_mel_fake(mag, bank, rate, power, db, ref, amin):
    n_out = H.phase_vocoder_out_frames(mag.shape[-1], rate)
    return _swapped(mag.shape[:-2], (n_out, bank.shape[1]), mag.dtype, mag.device, -2, -1)


_register('stretch_mel', '(Tensor mag, Tensor filterbank, float rate, float power, bool db, float ref, float amin) -> Tensor',
          _stretch_mel_cuda, C.stretch_mel, _stretch_mel_fake, 2)


# ============================================================================= dB
def _unary_cuda(op, hip_fn, composite_fn):
    def run(x, *args):
        if x.dtype == torch.float64:
            return getattr(H64, op)(x, *args)
        reason = _hip_dtype(x)
        if reason is not None:
            _composite_route(op, reason)
            return composite_fn(x, *args)
        out = hip_fn(_f32(x), *args)
        return out if x.dtype == out.dtype else out.to(x.dtype)
    return run


_register('amplitude_to_db', '(Tensor x, float ref, float amin) -> Tensor',
          _unary_cuda('amplitude_to_db', H.amplitude_to_db, C.amplitude_to_db), C.amplitude_to_db,
          lambda x, ref, amin: _like_meta(x), 1)
_register('db_to_amplitude', '(Tensor x, float ref) -> Tensor',
          _unary_cuda('db_to_amplitude', H.db_to_amplitude, C.db_to_amplitude), C.db_to_amplitude,
          lambda x, ref: _like_meta(x), 1)


# ============================================================================= mu-law
def _mu_law_encoding_cuda(x, n_quantize):
    if not x.is_floating_point():
        x = x.to(torch.float)                              # reference functional.py:329-330
    if x.dtype == torch.float64:
        return H.mu_law_encoding_f64(x, n_quantize)        # the formula in double, like the reference's CPU path on double input
    reason = _hip_dtype(x)
    if reason is not None:
        _composite_route('mu_law_encoding', reason)
        return C.mu_law_encoding(x, n_quantize)
    return H.mu_law_encoding(_f32(x), n_quantize)


_register('mu_law_encoding', '(Tensor x, int n_quantize) -> Tensor', _mu_law_encoding_cuda, C.mu_law_encoding,
          lambda x, n_quantize: torch.empty(x.shape, dtype=torch.int64, device=x.device), 1, differentiable=False)


def _mu_law_decoding_cuda(codes, n_quantize, dtype):
    if not codes.is_floating_point():
        if dtype == torch.float32:
            return H.mu_law_decoding_int(codes, n_quantize)
        if dtype in _WIDEN:
            return H.mu_law_decoding_int(codes, n_quantize).to(dtype)
        if dtype == torch.float64:
            return H.mu_law_decoding_f64(codes.to(torch.int64), n_quantize)
        _composite_route('mu_law_decoding', 'dtype %s' % str(dtype).replace('torch.', ''))
        return C.mu_law_decoding(codes, n_quantize, dtype)
    if codes.dtype == torch.float64:
        return H.mu_law_decoding_f64(codes, n_quantize)
    reason = _hip_dtype(codes)
    if reason is not None:
        _composite_route('mu_law_decoding', reason)
        return C.mu_law_decoding(codes, n_quantize, dtype)
    out = H.mu_law_decoding_float(_f32(codes), n_quantize)
    return out if codes.dtype == out.dtype else out.to(codes.dtype)


def _mu_law_decoding_fake(codes, n_quantize, dtype):
    if codes.is_floating_point():
        return _like_meta(codes)
    return torch.empty(codes.shape, dtype=dtype, device=codes.device)


_register('mu_law_decoding', '(Tensor codes, int n_quantize, ScalarType dtype) -> Tensor', _mu_law_decoding_cuda,
          C.mu_law_decoding, _mu_law_decoding_fake, 1)

# ============================================================================= hpss
def _hpss_cuda(mag, kernel_f, kernel_t, power, hard):
    reason = _hip_dtype(mag)
    if reason is None and not H.hpss_supported(kernel_f, kernel_t):
        reason = 'kernel_size (%d, %d)' % (kernel_f, kernel_t)
    if reason is not None:
        _composite_route('hpss', reason)
        return C.hpss(mag, kernel_f, kernel_t, power, hard)
    outs = H.hpss(_f32(mag), kernel_f, kernel_t, power, hard)
    return outs if mag.dtype == torch.float32 else tuple(o.to(mag.dtype) for o in outs)


_register('hpss', '(Tensor mag, int kernel_f, int kernel_t, float power, bool hard) -> (Tensor, Tensor, Tensor, Tensor)',
          _hpss_cuda, C.hpss, lambda mag, kernel_f, kernel_t, power, hard: tuple(_like_meta(mag) for _ in range(4)), 1)

def _hpss_masks_cuda(mag, kernel_f, kernel_t, power, hard):
    reason = _hip_dtype(mag)
    if reason is None and not H.hpss_supported(kernel_f, kernel_t):
        reason = 'kernel_size (%d, %d)' % (kernel_f, kernel_t)
    if reason is not None:
        _composite_route('hpss', reason)
        return C.hpss(mag, kernel_f, kernel_t, power, hard)[2:]
    outs = H.hpss(_f32(mag), kernel_f, kernel_t, power, hard, masks_only=True)
    return outs if mag.dtype == torch.float32 else tuple(o.to(mag.dtype) for o in outs)


_register('hpss_masks', '(Tensor mag, int kernel_f, int kernel_t, float power, bool hard) -> (Tensor, Tensor)',
          _hpss_masks_cuda, lambda mag, kernel_f, kernel_t, power, hard: C.hpss(mag, kernel_f, kernel_t, power, hard)[2:],
          lambda mag, kernel_f, kernel_t, power, hard: tuple(_like_meta(mag) for _ in range(2)), 1)

ops = getattr(torch.ops, NS)
