"""Layer API — the ``nn.Module`` surface of the reference's ``torchaudio_contrib/layers.py``
(same class names, constructor signatures, attributes, buffers, ``__repr__`` strings and
exceptions), backed by the gfx950 kernels in ``csrc/``.

Chains of these layers fuse automatically: ``STFT`` hands a deferred result to ``ComplexNorm`` →
``ApplyFilterbank`` → ``AmplitudeToDb`` (see ``_lazy.py``), so
``nn.Sequential(*Melspectrogram(...), AmplitudeToDb())`` — the reference's own idiom — is a single
kernel launch that reads the waveform once and writes only the mel-dB tensor.
"""
import math

import torch
import torch.nn as nn

from . import functional as F
from . import _composite
from . import _filters
from . import _hip
from . import _lazy
from . import _ops
from . import _pitch
from . import _vad
from . import _beamform
from . import _resample
from . import _specaug
from . import _augment
from ._bounded import Bounded
from ._lazy import DeferredSpectral, DeferredWave, can_defer, can_defer_codes, lazy_fusion_enabled, realize


class _ModuleNoStateBuffers(nn.Module):
    """Module whose buffers (window, filterbank, phase_advance) are derived constants: they follow
    ``.to()/.cuda()`` but never enter ``state_dict()`` and are ignored when loading one
    (contract of reference layers.py:11-32; ``state_dict()`` of a whole pipeline is empty)."""

    def state_dict(self, *args, **kwargs):
        prefix = kwargs.get('prefix', args[1] if len(args) > 1 else '')
        full = super(_ModuleNoStateBuffers, self).state_dict(*args, **kwargs)
        for name in self._buffers:
            full.pop(prefix + name, None)
        return full

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        kept, self._buffers = self._buffers, {}
        try:
            return super(_ModuleNoStateBuffers, self)._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        finally:
            self._buffers = kept


class STFT(_ModuleNoStateBuffers):
    """Short-time Fourier transform layer: ``(*, channel, time)`` → ``(*, channel, num_freqs, time, 2)``.

    Arguments and defaults are those of the reference (layers.py:35-109): ``hop_length`` defaults to
    ``fft_length // 4``, ``win_length`` to ``fft_length``, ``window`` to a periodic Hann window of
    ``win_length``; ``center``/``pad_mode``/``normalized``/``onesided`` as in ``torch.stft``.
    """

    def __init__(self, fft_length, hop_length=None, win_length=None,
                 window=None, center=True, pad_mode='reflect',
                 normalized=False, onesided=True):
        super(STFT, self).__init__()
        self.fft_length = fft_length
        self.hop_length = hop_length
        self.win_length = win_length
        self.center = center
        self.pad_mode = pad_mode
        self.normalized = normalized
        self.onesided = onesided
        if window is None:
            window = torch.hann_window(fft_length if win_length is None else win_length)
        self.register_buffer('window', window)

    def forward(self, waveforms):
        if torch.is_tensor(waveforms) and can_defer(waveforms, self.window):
            # validate now, so errors surface here; the launch itself waits for the rest of the chain (_lazy.py).  The
            # resolved arguments and the recipe's shapes depend on the input's shape only: remembered per shape, so that a
            # repeated call neither re-validates nor re-derives them (the attributes are read on every call: changing one
            # is seen)
            key = (waveforms.shape, self.fft_length, self.hop_length, self.win_length, self.center, self.pad_mode,
                   self.normalized, self.onesided, id(self.window))
            hit = self.__dict__.get('_recipes')
            if hit is None:
                hit = self.__dict__['_recipes'] = Bounded(32)
            tmpl = hit.get(key)
            if tmpl is None or tmpl[0] is not self.window:
                n_fft, hop, win_length, window = F.resolve_stft_args(waveforms, self.fft_length, self.hop_length,
                                                                     self.win_length, self.window)
                _hip.check_stft_args(waveforms.shape, n_fft, hop, win_length, self.center, self.pad_mode)
                if window is self.window:
                    tmpl = hit[key] = (window, DeferredSpectral.template(
                        waveforms.shape, n_fft, hop, win_length, bool(self.center), self.pad_mode, bool(self.normalized),
                        bool(self.onesided)))
                else:       # (a window resolve_stft_args had to build or move: not remembered)
                    d = DeferredSpectral.from_stft(waveforms, window, n_fft, hop, win_length, bool(self.center),
                                                   self.pad_mode, bool(self.normalized), bool(self.onesided))
                    return d.realize() if _lazy.ends_chain(self) else d
            d = DeferredSpectral.from_template(waveforms, tmpl[0], tmpl[1])
            return d.realize() if _lazy.ends_chain(self) else d        # (the last layer of a user's nn.Sequential: an ordinary tensor)
        return F.stft(waveforms, self.fft_length, self.hop_length, self.win_length, self.window, self.center,
                      self.pad_mode, self.normalized, self.onesided)

    def __repr__(self):
        head = '(fft_length={}, hop_length={}, win_length={})'.format(
            self.fft_length, self.hop_length, self.win_length)
        tail = '(center={}, pad_mode={}, normalized={}, onesided={})'.format(
            self.center, self.pad_mode, self.normalized, self.onesided)
        return self.__class__.__name__ + head + tail


class ISTFT(_ModuleNoStateBuffers):
    """Inverse short-time Fourier transform layer: ``(*, channel, num_freqs, time, 2)`` → ``(*, channel, samples)``.

    Mirrors ``STFT``: ``hop_length`` defaults to ``fft_length // 4``, ``win_length`` to ``fft_length``, ``window`` to a periodic
    Hann window of ``win_length`` (a buffer that follows ``.to()`` and stays out of ``state_dict()``);
    ``center``/``normalized``/``onesided`` as in ``torch.istft``.  ``forward(complex_specgrams, length=None)``.
    """

    def __init__(self, fft_length, hop_length=None, win_length=None,
                 window=None, center=True, normalized=False, onesided=True):
        super(ISTFT, self).__init__()
        self.fft_length = fft_length
        self.hop_length = hop_length
        self.win_length = win_length
        self.center = center
        self.normalized = normalized
        self.onesided = onesided
        if window is None:
            window = torch.hann_window(fft_length if win_length is None else win_length)
        self.register_buffer('window', window)

    def forward(self, complex_specgrams, length=None):
        return F.istft(complex_specgrams, self.fft_length, self.hop_length, self.win_length, self.window, self.center,
                       self.normalized, self.onesided, length)

    def __repr__(self):
        head = '(fft_length={}, hop_length={}, win_length={})'.format(
            self.fft_length, self.hop_length, self.win_length)
        tail = '(center={}, normalized={}, onesided={})'.format(self.center, self.normalized, self.onesided)
        return self.__class__.__name__ + head + tail


class GriffinLim(_ModuleNoStateBuffers):
    """``functional.griffinlim`` as a layer (torchaudio's ``transforms.GriffinLim``, its argument order and defaults):
    ``forward(specgram)`` maps ``(…, n_fft // 2 + 1, time)`` magnitudes (to the ``power``) to the ``(…, samples)`` waveform.
    ``win_length`` defaults to ``n_fft``, ``hop_length`` to ``win_length // 2``; the window ``window_fn(win_length, **wkwargs)`` is a
    buffer that follows ``.to()`` and stays out of ``state_dict()``."""

    def __init__(self, n_fft=400, n_iter=32, win_length=None, hop_length=None, window_fn=torch.hann_window, power=2.0,
                 wkwargs=None, momentum=0.99, length=None, rand_init=True):
        super(GriffinLim, self).__init__()
        if not 0 <= momentum < 1:
            raise ValueError('momentum must be in range [0, 1). Found: {}'.format(momentum))
        self.n_fft = n_fft
        self.n_iter = n_iter
        self.win_length = win_length if win_length is not None else n_fft
        self.hop_length = hop_length if hop_length is not None else self.win_length // 2
        self.register_buffer('window', window_fn(self.win_length) if wkwargs is None else window_fn(self.win_length, **wkwargs))
        self.length = length
        self.power = power
        self.momentum = momentum
        self.rand_init = rand_init

    def forward(self, specgram):
        return F.griffinlim(specgram, self.window, self.n_fft, self.hop_length, self.win_length, self.power, self.n_iter,
                            self.momentum, self.length, self.rand_init)

    def __repr__(self):
        return self.__class__.__name__ + '(n_fft={}, n_iter={}, win_length={}, hop_length={}, power={}, momentum={}, length={}, ' \
            'rand_init={})'.format(self.n_fft, self.n_iter, self.win_length, self.hop_length, self.power, self.momentum,
                                   self.length, self.rand_init)


class ComplexNorm(nn.Module):
    """``|z| ** power`` over the trailing complex dim (reference layers.py:112-135)."""

    def __init__(self, power=1.0):
        super(ComplexNorm, self).__init__()
        self.power = power

    def forward(self, complex_tensor):
        if isinstance(complex_tensor, DeferredSpectral) and complex_tensor.pending() \
                and complex_tensor._stage == 'stft':
            d = complex_tensor.with_norm(self.power)
            return d.realize() if _lazy.ends_chain(self) else d
        return F.complex_norm(complex_tensor, self.power)

    def __repr__(self):
        return self.__class__.__name__ + '(power={})'.format(self.power)


class ApplyFilterbank(_ModuleNoStateBuffers):
    """Multiply the frequency axis by a ``(num_freqs, num_bands)`` matrix held as the non-persistent
    buffer ``filterbank`` (reference layers.py:138-155)."""

    def __init__(self, filterbank):
        super(ApplyFilterbank, self).__init__()
        self.register_buffer('filterbank', filterbank)

    def forward(self, mag_specgrams):
        x = mag_specgrams
        fb = self.filterbank
        # (the recipe's own record of bins / device: attribute access on the wrapper goes through __torch_function__)
        if isinstance(x, DeferredSpectral) and x.pending() and x._stage == 'spec' \
                and fb.dim() == 2 and fb.shape[0] == x._src.n_bins and fb.device == x._src.wave.device \
                and fb.dtype == torch.float32 and not (fb.requires_grad and torch.is_grad_enabled()):
            d = x.with_filterbank(fb)
            return d.realize() if _lazy.ends_chain(self) else d
        return F.apply_filterbank(x, fb)


class Filterbank(object):
    """Abstract provider of a filterbank matrix (reference layers.py:158-167)."""

    def __init__(self):
        super(Filterbank, self).__init__()

    def get_filterbank(self):
        raise NotImplementedError


class MelFilterbank(Filterbank):
    """Mel filterbank provider (reference layers.py:170-212): ``max_freq`` defaults to
    ``sample_rate // 2``; one of the two must be given."""

    def __init__(self, num_freqs=1025, num_mels=128,
                 min_freq=0.0, max_freq=None, sample_rate=None, htk=False):
        super(MelFilterbank, self).__init__()
        if sample_rate is None and max_freq is None:
            raise ValueError('Either max_freq or sample_rate should be specified.'
                             ', but both are None.')
        self.num_freqs = num_freqs
        self.num_mels = num_mels
        self.min_freq = min_freq
        self.max_freq = max_freq if max_freq else sample_rate // 2
        self.htk = htk

    def get_filterbank(self):
        return F.create_mel_filter(num_freqs=self.num_freqs, num_mels=self.num_mels,
                                   min_freq=self.min_freq, max_freq=self.max_freq, htk=self.htk)

    def __repr__(self):
        # string kept byte-for-byte (typo and bracket order included): it is visible API
        a = '(num_freqs={}, snum_mels={}'.format(self.num_freqs, self.num_mels)
        b = ', min_freq={}, max_freq={})'.format(self.min_freq, self.max_freq)
        c = ', htk={}'.format(self.htk)
        return self.__class__.__name__ + a + b + c


class TimeStretch(_ModuleNoStateBuffers):
    """Phase-vocoder time stretch of a complex spectrogram (reference layers.py:215-264).  Handed a deferred STFT it records
    the rate in the recipe: behind ``ComplexNorm`` the phases cancel, and ``STFT -> TimeStretch -> ComplexNorm [-> ApplyFilterbank]
    [-> AmplitudeToDb]`` runs on magnitudes alone (``_lazy.py``, csrc/stretch.hip); anything else that takes the stretched result
    gets the STFT kernel followed by the phase-vocoder kernel.  A realised tensor is stretched at once."""

    def __init__(self, hop_length, num_freqs, fixed_rate=None):
        super(TimeStretch, self).__init__()
        self.fixed_rate = fixed_rate
        self.register_buffer('phase_advance',
                             torch.linspace(0, math.pi * hop_length, num_freqs)[..., None])

    def forward(self, complex_specgrams, overriding_rate=None):
        rate = self.fixed_rate if overriding_rate is None else overriding_rate
        if rate is None:
            raise ValueError("If no fixed_rate is specified"
                             ", must pass a valid rate to the forward method.")
        if rate == 1.0:
            return complex_specgrams
        x, pa = complex_specgrams, self.phase_advance
        if isinstance(x, DeferredSpectral) and x.pending() and x._stage == 'stft' and x._stretch is None \
                and isinstance(rate, (int, float)) and rate > 0 and type(pa) is torch.Tensor and pa.dtype == torch.float32 \
                and pa.device == x._src.wave.device and pa.dim() >= 2 and pa.shape[-1] == 1 and pa.shape[-2] == x._src.n_bins \
                and pa.numel() == x._src.n_bins and not (pa.requires_grad and torch.is_grad_enabled()) and _hip.finite_table(pa):
            # (phase_advance cancels behind ComplexNorm, but a non-finite one poisons the reference: that case, like every
            # argument F.phase_vocoder would refuse, takes the ordinary route below)
            d = x.with_stretch(float(rate), pa)
            return d.realize() if _lazy.ends_chain(self) else d
        return F.phase_vocoder(x, rate, pa)

    def __repr__(self):
        return self.__class__.__name__ + '(fixed_rate={})'.format(self.fixed_rate)


class _FusedSequential(nn.Sequential):
    """``nn.Sequential`` returned by the factories: children stay individually usable and ``*``-unpackable; a
    whole-chain call is ONE ``tac_amd::spectrogram`` / ``tac_amd::melspectrogram`` op (one kernel on a HIP device,
    differentiable, traceable by ``torch.compile``) and returns an ordinary tensor."""
    _tac_realizes = True            # (_lazy.ends_chain: this container launches what its children deferred by itself)

    def forward(self, input):
        kids = list(self._modules.values())
        if lazy_fusion_enabled() and torch.is_tensor(input) and 2 <= len(kids) <= 3 and type(kids[0]) is STFT and type(kids[1]) is ComplexNorm \
                and (len(kids) == 2 or type(kids[2]) is ApplyFilterbank):
            st = kids[0]
            x = realize(input)
            n_fft, hop, win_length, window = F.resolve_stft_args(x, st.fft_length, st.hop_length, st.win_length,
                                                                 st.window)
            _hip.check_stft_args(x.shape, n_fft, hop, win_length, st.center, st.pad_mode)
            args = (n_fft, hop, win_length, bool(st.center), st.pad_mode, bool(st.normalized), bool(st.onesided),
                    float(kids[1].power), False, 1.0, 1e-7)
            if len(kids) == 2:
                return F._call('spectrogram', x, window, *args)
            fb = kids[2].filterbank
            if fb.dim() == 2 and fb.shape[0] == (n_fft // 2 + 1 if st.onesided else n_fft) and fb.device == x.device:
                return F._call('melspectrogram', x, window, fb, *args)
        return realize(super(_FusedSequential, self).forward(input))


def Spectrogram(fft_length, hop_length=None, win_length=None,
                window=None, center=True, pad_mode='reflect',
                normalized=False, onesided=True, power=1.):
    """``Sequential(STFT(...), ComplexNorm(power))`` (reference layers.py:267-304); evaluated as one
    FFT kernel with the magnitude/power taken in its epilogue."""
    return _FusedSequential(
        STFT(fft_length, hop_length, win_length, window, center, pad_mode, normalized, onesided),
        ComplexNorm(power))


def Melspectrogram(num_mels=128, sample_rate=22050, min_freq=0.0, max_freq=None, num_freqs=None,
                   htk=False, mel_filterbank=None, **kwargs):
    """``Sequential(STFT, ComplexNorm(2.), ApplyFilterbank(mel))`` (reference layers.py:307-347).

    As in the reference, ``num_freqs`` is ignored and recomputed from ``kwargs['fft_length']``
    (1025 when absent), ``mel_filterbank`` may name a custom ``MelFilterbank``-like class, and the
    remaining ``kwargs`` go to ``Spectrogram`` (so omitting ``fft_length`` is a ``TypeError``)."""
    fft_length = kwargs.get('fft_length', None)
    num_freqs = fft_length // 2 + 1 if fft_length else 1025
    provider = MelFilterbank if mel_filterbank is None else mel_filterbank
    matrix = provider(num_mels=num_mels, sample_rate=sample_rate, min_freq=min_freq,
                      max_freq=max_freq, num_freqs=num_freqs, htk=htk).get_filterbank()
    return _FusedSequential(*Spectrogram(power=2., **kwargs), ApplyFilterbank(matrix))


class AmplitudeToDb(_ModuleNoStateBuffers):
    """``10·(log10(max(x², amin)) − log10(ref))`` (reference layers.py:350-381); fused into the
    producing kernel's epilogue when the input is a deferred spectrogram / mel-spectrogram."""

    def __init__(self, ref=1.0, amin=1e-7):
        super(AmplitudeToDb, self).__init__()
        self.ref = ref
        self.amin = amin
        assert ref > amin, "Reference value is expected to be bigger than amin, but I have" \
                           "ref:{} and amin:{}".format(ref, amin)

    def forward(self, x):
        if isinstance(x, DeferredSpectral) and x.pending() and x._stage in ('spec', 'mel'):
            # terminal stage: nothing can fuse behind the dB epilogue, so the fused kernel is launched now, on the
            # stream of the STFT call, and the caller gets an ordinary tensor
            return x.realize(db=(self.ref, self.amin))
        return F.amplitude_to_db(x, ref=self.ref, amin=self.amin)

    def __repr__(self):
        return self.__class__.__name__ + '(ref={}, amin={})'.format(self.ref, self.amin)


class DCT(_ModuleNoStateBuffers):
    """Multiply the band axis of ``(…, num_mels, time)`` by a ``(num_mels, num_coeffs)`` matrix held as the non-persistent
    buffer ``dct_matrix`` (``functional.create_dct``): ``(…, num_coeffs, time)``."""

    def __init__(self, dct_matrix):
        super(DCT, self).__init__()
        self.register_buffer('dct_matrix', dct_matrix)

    def forward(self, x):
        return F.dct(x, self.dct_matrix)

    def __repr__(self):
        return self.__class__.__name__ + '(num_mels={}, num_coeffs={})'.format(*self.dct_matrix.shape)


def MFCC(num_coeffs=40, norm='ortho', ref=1.0, amin=1e-7, **melkwargs):
    """``Sequential(*Melspectrogram(**melkwargs), AmplitudeToDb(ref, amin), DCT(create_dct(num_coeffs, num_mels, norm)))``:
    mel-frequency cepstral coefficients ``(*, channel, num_coeffs, time)`` of this package's mel dB values (``AmplitudeToDb``
    squares its input, as the reference's does; no ``top_db``, no ``log_mels``).  On a HIP device two launches: the fused
    Melspectrogram + dB kernel, then the DCT kernel.  The children stay individually usable."""
    num_mels = melkwargs.get('num_mels', 128)
    return nn.Sequential(*Melspectrogram(**melkwargs), AmplitudeToDb(ref, amin),
                         DCT(F.create_dct(num_coeffs, num_mels, norm)))


class Resample(_ModuleNoStateBuffers):
    """``functional.resample`` as a layer: ``(…, time)`` → ``(…, ceil(new_freq * time / orig_freq))``.  The compact polyphase
    bank — float32 ``(new, K)``, row ``p`` the taps of phase ``p`` from its first non-zero one — is the non-persistent buffer
    ``bank`` (a derived constant: it follows ``.to()`` and stays out of ``state_dict()``; the kernel's own copy is cached per
    argument tuple and device)."""

    def __init__(self, orig_freq=16000, new_freq=16000, lowpass_filter_width=6, rolloff=0.99,
                 resampling_method='sinc_interp_hann', beta=None):
        super(Resample, self).__init__()
        self.orig_freq = orig_freq
        self.new_freq = new_freq
        self.lowpass_filter_width = lowpass_filter_width
        self.rolloff = rolloff
        self.resampling_method = resampling_method
        self.beta = beta
        args = _resample.constants(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)
        self.register_buffer('bank', _resample.bank(*args).taps.to(torch.float32))

    def forward(self, waveforms):
        return F.resample(waveforms, self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff,
                          self.resampling_method, self.beta)

    def __repr__(self):
        return self.__class__.__name__ + '(orig_freq={}, new_freq={}, lowpass_filter_width={}, rolloff={}, resampling_method={}, beta={})'.format(
            self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff, self.resampling_method, self.beta)


class PitchShift(_ModuleNoStateBuffers):
    """``functional.pitch_shift`` as a layer (torchaudio's ``transforms.PitchShift``): ``(…, time)`` → ``(…, time)``, the pitch
    moved by ``n_steps`` of ``bins_per_octave`` to the octave.  The window ``window_fn(win_length, **wkwargs)`` is a non-persistent
    buffer; the compact polyphase banks of the last stage (forward and gradient) and their tile plans are built here, once."""

    def __init__(self, sample_rate, n_steps, bins_per_octave=12, n_fft=512, win_length=None, hop_length=None,
                 window_fn=torch.hann_window, wkwargs=None):
        super(PitchShift, self).__init__()
        self.sample_rate = sample_rate
        self.n_steps = n_steps
        self.bins_per_octave = bins_per_octave
        self.n_fft = n_fft
        self.win_length = win_length if win_length is not None else n_fft
        self.hop_length = hop_length if hop_length is not None else self.n_fft // 4
        self.register_buffer('window', window_fn(self.win_length) if wkwargs is None else window_fn(self.win_length, **wkwargs))
        _, source = _augment.pitch_rates(sample_rate, n_steps, bins_per_octave, 'PitchShift')
        args = _resample.constants(source, sample_rate)
        if args[0] != args[1]:
            from . import _hip
            _hip.resample_wide_plan(_resample.bank(*args))
            _hip.resample_wide_plan(_resample.adjoint_bank(*args))

    def forward(self, waveform):
        return F.pitch_shift(waveform, self.sample_rate, self.n_steps, self.bins_per_octave, self.n_fft, self.win_length,
                             self.hop_length, self.window)

    def __repr__(self):
        return self.__class__.__name__ + '(sample_rate={}, n_steps={}, bins_per_octave={}, n_fft={}, win_length={}, hop_length={})'.format(
            self.sample_rate, self.n_steps, self.bins_per_octave, self.n_fft, self.win_length, self.hop_length)


class LFilter(_ModuleNoStateBuffers):
    """``functional.lfilter`` as a layer: ``(…, time)`` → ``(…, time)``.  The two 1-D coefficient tensors are the non-persistent
    buffers ``a_coeffs`` / ``b_coeffs`` (kept in float64 unless given otherwise; they follow ``.to()`` — a change of dtype rounds
    them like any buffer — and stay out of ``state_dict()``)."""

    def __init__(self, a_coeffs, b_coeffs, clamp=True):
        super(LFilter, self).__init__()
        a = torch.as_tensor(a_coeffs, dtype=None if torch.is_tensor(a_coeffs) else torch.float64)
        b = torch.as_tensor(b_coeffs, dtype=None if torch.is_tensor(b_coeffs) else torch.float64)
        _filters.check_coeffs(a, b)
        if _hip.host_coeffs(a)[0] == 0.0:
            raise ValueError('lfilter: a_coeffs[0] must not be zero')
        self.clamp = bool(clamp)
        self.register_buffer('a_coeffs', a.detach().clone())
        self.register_buffer('b_coeffs', b.detach().clone())

    def forward(self, waveforms):
        return _ops.call('lfilter', F._waveform(waveforms, 'lfilter'), self.a_coeffs, self.b_coeffs, self.clamp)

    def __repr__(self):
        return self.__class__.__name__ + '(order={}, clamp={})'.format(self.a_coeffs.numel() - 1, self.clamp)


class SosFilt(_ModuleNoStateBuffers):
    """``functional.sosfilt`` as a layer: ``(…, time)`` → ``(…, time)``.  The ``(S, 6)`` sections are the non-persistent buffer
    ``sos`` (kept in float64 unless given otherwise; it follows ``.to()`` and stays out of ``state_dict()``, as ``LFilter``'s
    coefficients do)."""

    def __init__(self, sos, clamp=False):
        super(SosFilt, self).__init__()
        s = torch.as_tensor(sos, dtype=None if torch.is_tensor(sos) else torch.float64)
        _filters.check_sos(s)
        _filters.check_sos_values(_hip.host_sos(s))
        self.clamp = bool(clamp)
        self.register_buffer('sos', s.detach().clone())

    def forward(self, waveforms):
        return _ops.call('sosfilt', F._waveform(waveforms, 'sosfilt'), self.sos, self.clamp)

    def __repr__(self):
        return self.__class__.__name__ + '(sections={}, clamp={})'.format(self.sos.shape[0], self.clamp)


class Overdrive(nn.Module):
    """``functional.overdrive`` as a layer: ``(…, time)`` → ``(…, time)``.  No buffers."""

    def __init__(self, gain=20, colour=20):
        super(Overdrive, self).__init__()
        self.gain, self.colour = float(gain), float(colour)

    def forward(self, waveform):
        return F.overdrive(waveform, self.gain, self.colour)

    def __repr__(self):
        return self.__class__.__name__ + '(gain={}, colour={})'.format(self.gain, self.colour)


class Phaser(nn.Module):
    """``functional.phaser`` as a layer: ``(…, time)`` → ``(…, time)``.  No buffers: the LFO table is kept by value on the host
    and per device."""

    def __init__(self, sample_rate, gain_in=0.4, gain_out=0.74, delay_ms=3.0, decay=0.4, mod_speed=0.5, sinusoidal=True):
        super(Phaser, self).__init__()
        self.args = (float(sample_rate), float(gain_in), float(gain_out), float(delay_ms), float(decay), float(mod_speed),
                     bool(sinusoidal))
        F._sox.phaser_plan(self.args[0], self.args[3], self.args[5], self.args[6])      # (argument errors at construction)

    def forward(self, waveform):
        return F.phaser(waveform, *self.args)

    def __repr__(self):
        return self.__class__.__name__ + '(sample_rate={}, gain_in={}, gain_out={}, delay_ms={}, decay={}, mod_speed={}, sinusoidal={})'.format(*self.args)


class Flanger(nn.Module):
    """``functional.flanger`` as a layer: ``(…, channel, time)`` → ``(…, channel, time)``.  No buffers."""

    def __init__(self, sample_rate, delay=0.0, depth=2.0, regen=0.0, width=71.0, speed=0.5, phase=25.0, modulation='sinusoidal',
                 interpolation='linear'):
        super(Flanger, self).__init__()
        self.args = (float(sample_rate), float(delay), float(depth), float(regen), float(width), float(speed), float(phase),
                     modulation, interpolation)
        F._sox.flanger_plan(*self.args, 1)                                              # (argument errors at construction)

    def forward(self, waveform):
        return F.flanger(waveform, *self.args)

    def __repr__(self):
        return self.__class__.__name__ + '(sample_rate={}, delay={}, depth={}, regen={}, width={}, speed={}, phase={}, modulation={!r}, interpolation={!r})'.format(*self.args)


class Preemphasis(_ModuleNoStateBuffers):
    """``functional.preemphasis`` as a layer: ``y[n] = x[n] - coeff x[n-1]``.  No buffers: ``coeff`` is a Python float, and the
    two float64 host tensors the op takes are plain attributes (they stay float64 on the host whatever ``.to()`` is given)."""

    def __init__(self, coeff=0.97):
        super(Preemphasis, self).__init__()
        self.coeff = float(coeff)
        self._a, self._b = _filters.host_tensor((1.0, 0.0)), _filters.host_tensor((1.0, -self.coeff))

    def forward(self, waveforms):
        return _ops.call('lfilter', F._waveform(waveforms, 'preemphasis'), self._a, self._b, False)

    def __repr__(self):
        return self.__class__.__name__ + '(coeff={})'.format(self.coeff)


class Deemphasis(_ModuleNoStateBuffers):
    """``functional.deemphasis`` as a layer: ``y[n] = x[n] + coeff y[n-1]``.  No buffers, as ``Preemphasis``."""

    def __init__(self, coeff=0.97):
        super(Deemphasis, self).__init__()
        self.coeff = float(coeff)
        self._a, self._b = _filters.host_tensor((1.0, -self.coeff)), _filters.host_tensor((1.0, 0.0))

    def forward(self, waveforms):
        return _ops.call('lfilter', F._waveform(waveforms, 'deemphasis'), self._a, self._b, False)

    def __repr__(self):
        return self.__class__.__name__ + '(coeff={})'.format(self.coeff)


class KaldiFbank(_ModuleNoStateBuffers):
    """``functional.kaldi_fbank`` as a layer: ``(…, time)`` → ``(…, frames, num_mel_bins [+ 1])``, with the keywords and
    defaults of ``torchaudio.compliance.kaldi.fbank`` (less ``channel`` and ``min_duration``, which belong to ``kaldi.fbank``).
    No buffers: the window and the packed bank are cached per argument set and device."""

    def __init__(self, **kwargs):
        super(KaldiFbank, self).__init__()
        unknown = sorted(set(kwargs) - set(F._KALDI_KEYWORDS))
        if unknown:
            raise TypeError('KaldiFbank: unexpected keyword(s) %s' % ', '.join(unknown))
        self.options = dict(kwargs)
        F.kaldi_fbank(torch.zeros(0), **self.options)          # argument errors surface here, not in the first forward

    def forward(self, waveforms):
        return F.kaldi_fbank(waveforms, **self.options)

    def __repr__(self):
        return self.__class__.__name__ + '(' + ', '.join('{}={!r}'.format(k, v) for k, v in self.options.items()) + ')'


class _KaldiFeature(_ModuleNoStateBuffers):
    """a ``functional.kaldi_*`` function as a layer: keywords checked and argument errors raised at construction"""
    _function, _keywords = None, ()

    def __init__(self, **kwargs):
        super(_KaldiFeature, self).__init__()
        unknown = sorted(set(kwargs) - set(self._keywords))
        if unknown:
            raise TypeError('%s: unexpected keyword(s) %s' % (self.__class__.__name__, ', '.join(unknown)))
        self.options = dict(kwargs)
        type(self)._function(torch.zeros(0), **self.options)   # argument errors surface here, not in the first forward

    def forward(self, waveforms):
        return type(self)._function(waveforms, **self.options)

    def __repr__(self):
        return self.__class__.__name__ + '(' + ', '.join('{}={!r}'.format(k, v) for k, v in self.options.items()) + ')'


class KaldiMfcc(_KaldiFeature):
    """``functional.kaldi_mfcc`` as a layer: ``(…, time)`` → ``(…, frames, num_ceps)``, with the keywords and defaults of
    ``torchaudio.compliance.kaldi.mfcc`` (less ``channel`` and ``min_duration``, which belong to ``kaldi.mfcc``).  No buffers:
    the window, the packed bank and the DCT table are cached per argument set and device."""
    _function, _keywords = staticmethod(F.kaldi_mfcc), F._KALDI_MFCC_KEYWORDS


class KaldiSpectrogram(_KaldiFeature):
    """``functional.kaldi_spectrogram`` as a layer: ``(…, time)`` → ``(…, frames, N / 2 + 1)``, with the keywords and defaults
    of ``torchaudio.compliance.kaldi.spectrogram`` (less ``channel`` and ``min_duration``).  No buffers."""
    _function, _keywords = staticmethod(F.kaldi_spectrogram), F._KALDI_SPECTROGRAM_KEYWORDS


class SlidingWindowCmn(_ModuleNoStateBuffers):
    """``functional.sliding_window_cmn`` as a layer (torchaudio's ``transforms.SlidingWindowCmn``): ``(…, T, F)`` → the same
    shape.  No buffers."""

    def __init__(self, cmn_window=600, min_cmn_window=100, center=False, norm_vars=False):
        super(SlidingWindowCmn, self).__init__()
        self.cmn_window, self.min_cmn_window = int(cmn_window), int(min_cmn_window)
        self.center, self.norm_vars = bool(center), bool(norm_vars)
        _composite.cmn_check(self.cmn_window, self.min_cmn_window)          # argument errors surface here, not in the first forward

    def forward(self, specgram):
        return F.sliding_window_cmn(specgram, self.cmn_window, self.min_cmn_window, self.center, self.norm_vars)

    def __repr__(self):
        return self.__class__.__name__ + '(cmn_window={}, min_cmn_window={}, center={}, norm_vars={})'.format(
            self.cmn_window, self.min_cmn_window, self.center, self.norm_vars)


class ComputeDeltas(_ModuleNoStateBuffers):
    """``functional.compute_deltas`` as a layer (torchaudio's ``transforms.ComputeDeltas``): ``(…, F, T)`` → the same shape.
    No buffers."""

    def __init__(self, win_length=5, mode='replicate'):
        super(ComputeDeltas, self).__init__()
        self.win_length, self.mode = int(win_length), mode
        _composite.deltas_check_args(self.win_length, mode)                 # argument errors surface here, not in the first forward

    def forward(self, specgram):
        return F.compute_deltas(specgram, self.win_length, self.mode)

    def __repr__(self):
        return self.__class__.__name__ + '(win_length={}, mode={!r})'.format(self.win_length, self.mode)


class _AxisMasking(_ModuleNoStateBuffers):
    """One mask along the time or the frequency axis of ``(…, freq, time)`` (torchaudio's ``transforms._AxisMasking``): a span per
    leading index with ``iid_masks`` on an input of three or more dimensions, one shared span otherwise.  No buffers."""
    _from_end = 1                      # the axis, counted from the end

    def __init__(self, mask_param, iid_masks=False, p=1.0):
        super(_AxisMasking, self).__init__()
        self.mask_param, self.iid_masks, self.p = int(mask_param), bool(iid_masks), float(p)
        _specaug.check_p(self.__class__.__name__, self.p)                   # argument errors surface here, not in the first forward

    def forward(self, specgram, mask_value=0.0):
        x = realize(specgram)
        name = self.__class__.__name__
        if self.iid_masks and x.dim() >= 3:
            return _specaug.mask_along_axis_iid(x, self.mask_param, mask_value, x.dim() - self._from_end, self.p, name)
        return _specaug.mask_along_axis(x, self.mask_param, mask_value, x.dim() - self._from_end, self.p, name)

    def __repr__(self):
        return self.__class__.__name__ + '(mask_param={}, iid_masks={}, p={})'.format(self.mask_param, self.iid_masks, self.p)


class TimeMasking(_AxisMasking):
    """torchaudio's ``transforms.TimeMasking``: ``forward(specgram, mask_value=0.0)`` masks up to ``time_mask_param`` frames (at most
    the share ``p`` of them) of ``(…, freq, time)``: one launch on a HIP device (``functional.mask_along_axis[_iid]``)."""
    _from_end = 1

    def __init__(self, time_mask_param, iid_masks=False, p=1.0):
        super(TimeMasking, self).__init__(time_mask_param, iid_masks, p)


class FrequencyMasking(_AxisMasking):
    """torchaudio's ``transforms.FrequencyMasking``: ``forward(specgram, mask_value=0.0)`` masks up to ``freq_mask_param`` bins of
    ``(…, freq, time)``: one launch on a HIP device."""
    _from_end = 2

    def __init__(self, freq_mask_param, iid_masks=False):
        super(FrequencyMasking, self).__init__(freq_mask_param, iid_masks, 1.0)


class SpecAugment(_ModuleNoStateBuffers):
    """torchaudio's ``transforms.SpecAugment`` over ``(…, freq, time)``: ``n_time_masks`` time masks of up to ``time_mask_param`` frames
    (at most the share ``p`` of them), then ``n_freq_masks`` frequency masks of up to ``freq_mask_param`` bins, filled with 0
    (``zero_masking``) or with the input's mean, taken once before any mask; a span per leading index with ``iid_masks`` on three
    or more dimensions.  The draws are made in the order of the sequential ``mask_along_axis[_iid]`` calls, so a generator state
    gives what those give; ALL masks are then applied by one ``tac_amd::mask_spans`` call — on a HIP device one launch
    (csrc/specaug.hip) beside torch's ``mean``, whose result the kernel reads on the device.  No buffers."""

    def __init__(self, n_time_masks, time_mask_param, n_freq_masks, freq_mask_param, iid_masks=True, p=1.0, zero_masking=False):
        super(SpecAugment, self).__init__()
        self.n_time_masks, self.time_mask_param = int(n_time_masks), int(time_mask_param)
        self.n_freq_masks, self.freq_mask_param = int(n_freq_masks), int(freq_mask_param)
        self.iid_masks, self.p, self.zero_masking = bool(iid_masks), float(p), bool(zero_masking)
        _specaug.check_p('SpecAugment', self.p)

    def forward(self, specgram):
        return _specaug.spec_augment(realize(specgram), self.n_time_masks, self.time_mask_param, self.n_freq_masks,
                                     self.freq_mask_param, self.iid_masks, self.p, self.zero_masking)

    def __repr__(self):
        return ('SpecAugment(n_time_masks={}, time_mask_param={}, n_freq_masks={}, freq_mask_param={}, iid_masks={}, p={}, '
                'zero_masking={})').format(self.n_time_masks, self.time_mask_param, self.n_freq_masks, self.freq_mask_param,
                                           self.iid_masks, self.p, self.zero_masking)


class AddNoise(_ModuleNoStateBuffers):
    """``functional.add_noise`` as a layer (torchaudio's ``transforms.AddNoise``): ``forward(waveform, noise, snr, lengths=None)``.  No
    buffers."""

    def forward(self, waveform, noise, snr, lengths=None):
        return _augment.add_noise(realize(waveform), realize(noise), snr, lengths, 'AddNoise')


class Loudness(_ModuleNoStateBuffers):
    """``functional.loudness`` as a layer (torchaudio's ``transforms.Loudness``): ``forward(waveform)`` maps ``(…, channels, time)``
    to the ``(…)`` loudness in LKFS at ``sample_rate``.  No buffers."""

    def __init__(self, sample_rate):
        super(Loudness, self).__init__()
        if isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or sample_rate <= 0:
            raise ValueError('Loudness: sample_rate must be a positive int, got %r' % (sample_rate,))
        self.sample_rate = sample_rate

    def forward(self, waveform):
        return F.loudness(waveform, self.sample_rate)

    def __repr__(self):
        return self.__class__.__name__ + '(sample_rate={})'.format(self.sample_rate)


class PitchFrequency(_ModuleNoStateBuffers):
    """``functional.detect_pitch_frequency`` as a layer: ``forward(waveform)`` maps ``(…, time)`` to the float32 ``(…, n_out)`` pitch
    in Hz.  No buffers."""

    def __init__(self, sample_rate, frame_time=1e-2, win_length=30, freq_low=85, freq_high=3400):
        super(PitchFrequency, self).__init__()
        _pitch.geometry(2 ** 40, sample_rate, frame_time, win_length, freq_low, freq_high)    # (every error but a short waveform's)
        self.sample_rate, self.frame_time, self.win_length = sample_rate, frame_time, win_length
        self.freq_low, self.freq_high = freq_low, freq_high

    def forward(self, waveform):
        return F.detect_pitch_frequency(waveform, self.sample_rate, self.frame_time, self.win_length, self.freq_low, self.freq_high)

    def __repr__(self):
        return self.__class__.__name__ + '(sample_rate={}, frame_time={}, win_length={}, freq_low={}, freq_high={})'.format(
            self.sample_rate, self.frame_time, self.win_length, self.freq_low, self.freq_high)


class Vad(_ModuleNoStateBuffers):
    """``functional.vad`` as a layer (torchaudio's ``transforms.Vad``, its constructor): ``forward(waveform)`` maps ``(…, time)`` to
    ``(…, time - start)``, everything before the first speech trimmed.  No buffers."""

    def __init__(self, sample_rate, trigger_level=7.0, trigger_time=0.25, search_time=1.0, allowed_gap=0.25, pre_trigger_time=0.0,
                 boot_time=0.35, noise_up_time=0.1, noise_down_time=0.01, noise_reduction_amount=1.35, measure_freq=20.0,
                 measure_duration=None, measure_smooth_time=0.4, hp_filter_freq=50.0, lp_filter_freq=6000.0, hp_lifter_freq=150.0,
                 lp_lifter_freq=2000.0):
        super(Vad, self).__init__()
        self.sample_rate = sample_rate
        self.args = (trigger_level, trigger_time, search_time, allowed_gap, pre_trigger_time, boot_time, noise_up_time, noise_down_time,
                     noise_reduction_amount, measure_freq, measure_duration, measure_smooth_time, hp_filter_freq, lp_filter_freq,
                     hp_lifter_freq, lp_lifter_freq)
        _vad.plan(sample_rate, *_vad.resolve(self.args))                  # (every error but the tensor's)
        for name, value in zip(_vad.ARGS, self.args):
            setattr(self, name, value)

    def forward(self, waveform):
        return F.vad(waveform, self.sample_rate, *self.args)

    def __repr__(self):
        return self.__class__.__name__ + '(sample_rate={}, {})'.format(
            self.sample_rate, ', '.join('{}={}'.format(name, value) for name, value in zip(_vad.ARGS, self.args)))


class SimulateRirIsm(_ModuleNoStateBuffers):
    """``functional.simulate_rir_ism`` / ``simulate_rir_ism_batch`` as a layer: ``forward(room, source, mic_array)`` maps a room ``(D,)`` to
    ``(M, output_length)`` and a batch of rooms ``(B, D)`` to ``(B, M, output_length)``.  No buffers."""

    def __init__(self, max_order, absorption, output_length=None, delay_filter_length=81, center_frequency=None, sound_speed=343.0,
                 sample_rate=16000.0):
        super(SimulateRirIsm, self).__init__()
        if isinstance(delay_filter_length, bool) or not isinstance(delay_filter_length, int) or delay_filter_length % 2 != 1:
            raise ValueError('SimulateRirIsm: delay_filter_length must be odd, got %r' % (delay_filter_length,))
        self.max_order, self.absorption, self.output_length = max_order, absorption, output_length
        self.delay_filter_length, self.center_frequency = delay_filter_length, center_frequency
        self.sound_speed, self.sample_rate = sound_speed, sample_rate

    def forward(self, room, source, mic_array):
        fn = F.simulate_rir_ism_batch if room.dim() == 2 else F.simulate_rir_ism
        return fn(room, source, mic_array, self.max_order, self.absorption, self.output_length, self.delay_filter_length,
                  self.center_frequency, self.sound_speed, self.sample_rate)

    def __repr__(self):
        return self.__class__.__name__ + '(max_order={}, output_length={}, delay_filter_length={}, sound_speed={}, sample_rate={})'.format(
            self.max_order, self.output_length, self.delay_filter_length, self.sound_speed, self.sample_rate)


class PSD(_ModuleNoStateBuffers):
    """``functional.psd`` as a layer (torchaudio's ``transforms.PSD``): ``forward(specgram, mask=None)`` maps ``(…, channel, freq,
    time)`` to ``(…, freq, channel, channel)``.  With ``multi_mask`` the mask is ``(…, channel, freq, time)`` and is averaged over
    the channels first.  No buffers."""

    def __init__(self, multi_mask=False, normalize=True, eps=1e-15):
        super(PSD, self).__init__()
        self.multi_mask, self.normalize, self.eps = bool(multi_mask), bool(normalize), float(eps)

    def forward(self, specgram, mask=None):
        if mask is not None and self.multi_mask:
            _beamform.check_mask(mask, _beamform.pairs(specgram, 'specgram')[0], multi=True)
            mask = mask.mean(dim=-3)
        return F.psd(specgram, mask, self.normalize, self.eps)

    def __repr__(self):
        return self.__class__.__name__ + '(multi_mask={}, normalize={}, eps={})'.format(self.multi_mask, self.normalize, self.eps)


class SoudenMVDR(_ModuleNoStateBuffers):
    """torchaudio's ``transforms.SoudenMVDR``: ``forward(specgram, psd_s, psd_n, reference_channel, diagonal_loading=True,
    diag_eps=1e-7, eps=1e-8)`` computes the Souden weights from the two PSDs and applies them: ``(…, channel, freq, time)`` →
    ``(…, freq, time)``.  Two launches on a HIP device.  No buffers."""

    def forward(self, specgram, psd_s, psd_n, reference_channel, diagonal_loading=True, diag_eps=1e-7, eps=1e-8):
        w = F.mvdr_weights_souden(psd_s, psd_n, reference_channel, diagonal_loading, diag_eps, eps)
        return F.apply_beamforming(w, specgram)


class RTFMVDR(_ModuleNoStateBuffers):
    """torchaudio's ``transforms.RTFMVDR``: ``forward(specgram, rtf, psd_n, reference_channel, diagonal_loading=True, diag_eps=1e-7,
    eps=1e-8)`` computes ``functional.mvdr_weights_rtf`` from the relative transfer function and the noise PSD and applies the
    weights: ``(…, channel, freq, time)`` → ``(…, freq, time)``.  On a HIP device ONE entry of two launches, the result the
    frame-major view ``istft`` reads in place.  ``PSD → rtf_evd / rtf_power → RTFMVDR`` is the steering-vector beamformer.  No
    buffers."""

    def forward(self, specgram, rtf, psd_n, reference_channel, diagonal_loading=True, diag_eps=1e-7, eps=1e-8):
        x, was_complex = _beamform.pairs(specgram, 'specgram')
        d, _ = _beamform.pairs(rtf, 'rtf')
        n, _ = _beamform.pairs(psd_n, 'psd_n')
        lead, n_ch, n_bins, n_frames = _beamform.spec_shape(x)
        _beamform.check_apply(d, x)
        _, _, _, u, r = _beamform.check_rtf_weights_args(d, n, reference_channel)
        out = _ops.call('rtf_mvdr', x, d, n, _beamform.none(x) if u is None else u, r, bool(diagonal_loading), float(diag_eps),
                        float(eps))
        return _beamform.unpairs(out, was_complex)


class RNNTLoss(_ModuleNoStateBuffers):
    """torchaudio's ``transforms.RNNTLoss``: ``forward(logits, targets, logit_lengths, target_lengths)`` is ``functional.rnnt_loss``
    with the ``blank``, ``clamp``, ``reduction`` and ``fused_log_softmax`` of the constructor.  No buffers, no parameters."""

    def __init__(self, blank=-1, clamp=-1.0, reduction='mean', fused_log_softmax=True):
        super(RNNTLoss, self).__init__()
        if reduction not in ('none', 'mean', 'sum'):
            raise ValueError("RNNTLoss: reduction must be 'none', 'mean' or 'sum', got %r" % (reduction,))
        self.blank = blank
        self.clamp = clamp
        self.reduction = reduction
        self.fused_log_softmax = fused_log_softmax

    def forward(self, logits, targets, logit_lengths, target_lengths):
        return F.rnnt_loss(logits, targets, logit_lengths, target_lengths, self.blank, self.clamp, self.reduction,
                           self.fused_log_softmax)


class MVDR(_ModuleNoStateBuffers):
    """torchaudio's mask-based ``transforms.MVDR`` at ``solution='ref_channel'``: ``forward(specgram, mask_s, mask_n=None)`` maps a
    ``(…, channel, freq, time)`` spectrogram and real ``(…, freq, time)`` masks (``(…, channel, freq, time)`` with ``multi_mask``,
    averaged over the channels) to the enhanced ``(…, freq, time)``; ``mask_n=None`` means ``1 - mask_s``.  The PSDs are those of
    ``PSD(multi_mask, normalize=True, eps=1e-15)``, the weights Souden's at ``ref_channel``.  On a HIP device one entry of three
    launches: both PSDs from ONE pass over the spectrogram (the complement formed in the kernel), the float64 solve, the weights
    applied; the result is the frame-major view ``istft`` reads in place.  ``solution='stv_evd'`` / ``'stv_power'`` and
    ``online=True`` raise ``NotImplementedError``.  No buffers."""

    def __init__(self, ref_channel=0, solution='ref_channel', multi_mask=False, diag_loading=True, diag_eps=1e-7, online=False):
        super(MVDR, self).__init__()
        if solution != 'ref_channel':
            raise NotImplementedError('MVDR: solution=%r is not implemented (only \'ref_channel\', Souden\'s, is)' % (solution,))
        if online:
            raise NotImplementedError('MVDR: online=True is not implemented')
        if isinstance(ref_channel, bool) or not isinstance(ref_channel, int):
            raise TypeError('MVDR: ref_channel must be an int, got %s' % type(ref_channel).__name__)
        self.ref_channel, self.solution, self.multi_mask = ref_channel, solution, bool(multi_mask)
        self.diag_loading, self.diag_eps, self.online = bool(diag_loading), float(diag_eps), False

    def forward(self, specgram, mask_s, mask_n=None):
        x, was_complex = _beamform.pairs(specgram, 'specgram')
        lead, n_ch, n_bins, n_frames = _beamform.spec_shape(x)
        if not -n_ch <= self.ref_channel < n_ch:
            raise ValueError('MVDR: ref_channel %d is out of range for %d channels' % (self.ref_channel, n_ch))
        masks = []
        for name, mask in (('mask_s', mask_s), ('mask_n', mask_n)):
            if mask is None and name == 'mask_n':
                masks.append(_beamform.none(x))
                continue
            _beamform.check_mask(mask, x, name, multi=self.multi_mask)
            masks.append(mask.mean(dim=-3) if self.multi_mask else mask)
        out = _ops.call('mvdr_souden', x, masks[0], masks[1], _beamform.none(x), self.ref_channel % n_ch, self.diag_loading,
                        self.diag_eps, 1e-8, 1e-15)
        return _beamform.unpairs(out, was_complex)

    def __repr__(self):
        return self.__class__.__name__ + '(ref_channel={}, solution={!r}, multi_mask={}, diag_loading={}, diag_eps={})'.format(
            self.ref_channel, self.solution, self.multi_mask, self.diag_loading, self.diag_eps)


class Speed(_ModuleNoStateBuffers):
    """``functional.speed`` as a layer (torchaudio's ``transforms.Speed``): ``forward(waveform, lengths=None)`` returns ``(waveform
    played factor times faster, its valid lengths or None)``.  It holds the ``Resample`` layer of the reduced pair ``int(factor *
    orig_freq) : int(orig_freq)``, whose bank is built once, here."""

    def __init__(self, orig_freq, factor):
        super(Speed, self).__init__()
        self.orig_freq, self.factor = orig_freq, factor
        self.source_sample_rate, self.target_sample_rate = _augment.speed_rates(orig_freq, factor, 'Speed')
        self.resampler = Resample(orig_freq=self.source_sample_rate, new_freq=self.target_sample_rate)

    def forward(self, waveform, lengths=None):
        return self.resampler(waveform), _augment.speed_lengths(lengths, self.source_sample_rate, self.target_sample_rate)

    def __repr__(self):
        return self.__class__.__name__ + '(orig_freq={}, factor={})'.format(self.orig_freq, self.factor)


class SpeedPerturbation(_ModuleNoStateBuffers):
    """torchaudio's ``transforms.SpeedPerturbation``: ``forward(waveform, lengths=None)`` draws one of ``factors`` —
    ``int(torch.randint(len(factors), ()))`` from the CPU generator, once per call and before anything else, also where the factor
    drawn is 1.0 — and applies that ``Speed``."""

    def __init__(self, orig_freq, factors):
        super(SpeedPerturbation, self).__init__()
        factors = list(factors)
        if not factors:
            raise ValueError('SpeedPerturbation: factors must not be empty')
        self.orig_freq, self.factors = orig_freq, factors
        self.speeders = nn.ModuleList([Speed(orig_freq, factor) for factor in factors])

    def forward(self, waveform, lengths=None):
        index = int(torch.randint(len(self.speeders), ()))
        return self.speeders[index](waveform, lengths)

    def __repr__(self):
        return self.__class__.__name__ + '(orig_freq={}, factors={})'.format(self.orig_freq, self.factors)


class FFTConvolve(_ModuleNoStateBuffers):
    """``functional.fftconvolve`` as a layer (torchaudio's ``transforms.FFTConvolve``): ``forward(x, y)`` with ``mode`` one of
    ``'full'``, ``'valid'``, ``'same'``."""

    def __init__(self, mode='full'):
        super(FFTConvolve, self).__init__()
        F._check_conv_mode(mode)
        self.mode = mode

    def forward(self, x, y):
        return F.fftconvolve(x, y, self.mode)

    def __repr__(self):
        return self.__class__.__name__ + '(mode={!r})'.format(self.mode)


class Convolve(FFTConvolve):
    """``functional.convolve`` as a layer (torchaudio's ``transforms.Convolve``)."""

    def forward(self, x, y):
        return F.convolve(x, y, self.mode)


class DbToAmplitude(_ModuleNoStateBuffers):
    """Inverse of ``AmplitudeToDb`` (reference layers.py:384-412)."""

    def __init__(self, ref=1.0):
        super(DbToAmplitude, self).__init__()
        self.ref = ref

    def forward(self, x):
        return F.db_to_amplitude(x, ref=self.ref)

    def __repr__(self):
        return self.__class__.__name__ + '(ref={})'.format(self.ref)


class MuLawEncoding(_ModuleNoStateBuffers):
    """mu-law companding to int64 codes (reference layers.py:415-440)."""

    def __init__(self, n_quantize=256):
        super(MuLawEncoding, self).__init__()
        self.n_quantize = n_quantize

    def forward(self, x):
        return F.mu_law_encoding(x, self.n_quantize)

    def __repr__(self):
        return self.__class__.__name__ + '(n_quantize={})'.format(self.n_quantize)


class MuLawDecoding(_ModuleNoStateBuffers):
    """mu-law expansion; like the reference (layers.py:443-467) always decodes to the default dtype."""

    def __init__(self, n_quantize=256):
        super(MuLawDecoding, self).__init__()
        self.n_quantize = n_quantize

    def forward(self, x_mu):
        if torch.is_tensor(x_mu) and self.n_quantize == 256 and can_defer_codes(x_mu) \
                and torch.get_default_dtype() == torch.float32:
            # an STFT layer behind this one decodes the codes inside its frame load; anything else decodes now
            return DeferredWave(x_mu, self.n_quantize)
        return F.mu_law_decoding(x_mu, self.n_quantize)

    def __repr__(self):
        return self.__class__.__name__ + '(n_quantize={})'.format(self.n_quantize)


class HPSS(nn.Module):
    """Harmonic / percussive separation layer (reference beta_hpss.py:12-32): wraps ``functional.hpss``."""

    def __init__(self, kernel_size=31, power=2.0, hard=False, mask_only=False):
        super(HPSS, self).__init__()
        self.kernel_size = kernel_size
        self.power = power
        self.hard = hard
        self.mask_only = mask_only

    def forward(self, mag_specgrams):
        return F.hpss(mag_specgrams, self.kernel_size, self.power, self.hard, self.mask_only)

    def __repr__(self):
        return self.__class__.__name__ + '(kernel_size={}, power={}, hard={}, mask_only={})'.format(
            self.kernel_size, self.power, self.hard, self.mask_only)
