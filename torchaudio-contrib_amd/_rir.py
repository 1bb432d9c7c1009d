"""Tables and argument checks of ``simulate_rir_ism`` (shared by ``functional``, ``layers``, ``_ops``, ``_hip`` and ``_composite``): the
image offsets of an order, the windowed-sinc tap table of a filter length and the band filters of a set of centre frequencies."""
import math

import torch

from ._bounded import Bounded

#: the band filters: taps, and the transform they are sampled on
FILTER_TAPS = 511
FILTER_FFT = 512

_image_tables = Bounded(32)
_tap_tables = Bounded(32)
_band_filters = Bounded(32)


def n_images(max_order, dims):
    """how many integer vectors of ``dims`` entries have ``sum |X_d| <= max_order``"""
    n = max_order
    return 2 * n * n + 2 * n + 1 if dims == 2 else (4 * n * n * n + 6 * n * n + 8 * n + 3) // 3


def images(max_order, dims, device='cpu'):
    """int8 ``(n_images, dims)`` on ``device`` (int16 beyond order 127, which only the composite takes): every integer vector ``X`` of ``{-max_order … max_order}^dims`` with ``sum |X_d| <= max_order``,
    in ``torch.cartesian_prod``'s order (the last axis fastest); built on the host once per (order, dims, device)"""
    key = (max_order, dims, str(device))
    hit = _image_tables.get(key)
    if hit is None:
        with torch.inference_mode(False):
            r = torch.arange(-max_order, max_order + 1, dtype=torch.int64)
            X = torch.cartesian_prod(*([r] * dims)).reshape(-1, dims)
            hit = X[X.abs().sum(-1) <= max_order].to(torch.int8 if max_order <= 127 else torch.int16).contiguous().to(device)
        _image_tables[key] = hit
    return hit


def shell(max_order, dims, device='cpu'):
    """the images with ``sum |X_d| >= max_order - 1``: the farthest image of any microphone is one of them.  An image further in has the
    neighbour ``X ± 2 e_d`` of the same parity inside the order — its location is the image's moved by two room lengths along axis ``d`` —
    and the sign that moves it away from the microphone along that axis makes the distance larger."""
    key = ('shell', max_order, dims, str(device))
    hit = _image_tables.get(key)
    if hit is None:
        with torch.inference_mode(False):
            X = images(max_order, dims)
            hit = X[X.long().abs().sum(-1) >= max_order - 1].contiguous().to(device)
        _image_tables[key] = hit
    return hit


def tap_table(filter_length, device):
    """float32 ``(filter_length, 2)`` on ``device``: ``cos`` and ``sin`` of ``pi m / 2P`` for ``m = -P … P``, float64 values rounded once"""
    key = (filter_length, str(device))
    hit = _tap_tables.get(key)
    if hit is None:
        with torch.inference_mode(False):
            P = filter_length // 2
            angle = torch.arange(-P, P + 1, dtype=torch.float64) * (math.pi / (2.0 * P))
            tab = torch.stack([torch.cos(angle), torch.sin(angle)], -1)
            tab[0, 0] = tab[-1, 0] = 0.0            # (the window's zeros at m = -P and P, exactly)
            hit = tab.to(torch.float32).to(device)
        _tap_tables[key] = hit
    return hit


def band_edges(centres, sample_rate):
    """``[(lo, centre, hi)]`` per band: ``[c_0 / 2, c_1]``, ``[c_{b-1}, c_{b+1}]``, … , ``[c_{n-2}, sample_rate // 2]``"""
    n = len(centres)
    out = []
    for b, c in enumerate(centres):
        lo = centres[0] / 2.0 if b == 0 else centres[b - 1]
        hi = float(int(sample_rate) // 2) if b == n - 1 else centres[b + 1]
        out.append((lo, c, hi))
    return out


def band_filters(centres, sample_rate, device='cpu', dtype=torch.float32):
    """``(n_band, 511)`` on ``device``: the linear-phase band filters of the centre frequencies ``centres`` (a tuple of floats, two or
    more).  On the 257 frequencies ``k sample_rate / 512`` band ``b`` of edges ``(lo, c, hi)`` has the response ``(1 + cos(2 pi v / c)) / 2`` for
    ``lo <= v < c`` and ``(1 - cos(2 pi v / hi)) / 2`` for ``c <= v < hi`` (the last band: 1 for ``v >= c``), 0 elsewhere; the filter is
    ``fftshift(irfft(response, 512))[1:]`` times the symmetric 511-point Hann window.  Computed in float64 on the host and rounded once."""
    key = (tuple(centres), float(sample_rate), str(device), dtype)
    hit = _band_filters.get(key)
    if hit is None:
        with torch.inference_mode(False):
            v = torch.arange(FILTER_FFT // 2 + 1, dtype=torch.float64) * (float(sample_rate) / FILTER_FFT)
            rows = []
            edges = band_edges(centres, sample_rate)
            for b, (lo, c, hi) in enumerate(edges):
                rise = 0.5 * (1.0 + torch.cos(2.0 * math.pi * v / c))
                fall = torch.ones_like(v) if b == len(edges) - 1 else 0.5 * (1.0 - torch.cos(2.0 * math.pi * v / hi))
                upper = (v >= c) if b == len(edges) - 1 else (v >= c) & (v < hi)
                rows.append(torch.where((v >= lo) & (v < c), rise, torch.where(upper, fall, torch.zeros_like(v))))
            taps = torch.fft.fftshift(torch.fft.irfft(torch.stack(rows), FILTER_FFT), dim=-1)[:, 1:]
            taps = taps * torch.hann_window(FILTER_TAPS, periodic=False, dtype=torch.float64)
            hit = taps.to(dtype).to(device)
        _band_filters[key] = hit
    return hit


def centres_of(center_frequency, n_band):
    """the centre frequencies as a tuple of floats (a tensor is read on the host), checked against the bands of ``absorption``"""
    if n_band == 1:
        return None
    if center_frequency is None:
        raise ValueError('simulate_rir_ism: center_frequency must be given when absorption has %d bands' % n_band)
    values = center_frequency.detach().reshape(-1).tolist() if torch.is_tensor(center_frequency) else list(center_frequency)
    if len(values) != n_band:
        raise ValueError('simulate_rir_ism: center_frequency has %d entries for %d absorption bands' % (len(values), n_band))
    values = tuple(float(c) for c in values)
    if not all(c > 0 and math.isfinite(c) for c in values) or any(b <= a for a, b in zip(values, values[1:])):
        raise ValueError('simulate_rir_ism: center_frequency must be positive and increasing, got %r' % (values,))
    return values


def check(room, source, mic_array, max_order, delay_filter_length, output_length, sound_speed, sample_rate, batch):
    """torchaudio's checks of the three tensors and the filter length (``ValueError``), for the single or the batch form; the number of
    axes ``D``"""
    lead = 1 if batch else 0
    what = 'simulate_rir_ism_batch' if batch else 'simulate_rir_ism'
    if room.dim() != lead + 1 or room.shape[-1] not in (2, 3):
        raise ValueError('%s: room must be a %d-D tensor with 2 or 3 entries%s, got shape %s'
                         % (what, lead + 1, ' a room' if batch else '', tuple(room.shape)))
    D = room.shape[-1]
    if tuple(source.shape) != tuple(room.shape):
        raise ValueError('%s: source must have the shape of room %s, got %s' % (what, tuple(room.shape), tuple(source.shape)))
    if mic_array.dim() != lead + 2 or mic_array.shape[-1] != D or (batch and mic_array.shape[0] != room.shape[0]):
        raise ValueError('%s: mic_array must be %s with D = %d, got shape %s'
                         % (what, '(B, M, D)' if batch else '(M, D)', D, tuple(mic_array.shape)))
    if not (room.is_floating_point() and source.is_floating_point() and mic_array.is_floating_point()):
        raise ValueError('%s: room, source and mic_array must be floating-point tensors' % what)
    if isinstance(max_order, bool) or not isinstance(max_order, int) or max_order < 0:
        raise ValueError('%s: max_order must be a non-negative int, got %r' % (what, max_order))
    if isinstance(delay_filter_length, bool) or not isinstance(delay_filter_length, int) or delay_filter_length < 1 or delay_filter_length % 2 != 1:
        raise ValueError('%s: delay_filter_length must be odd, got %r' % (what, delay_filter_length))
    if output_length is not None and (isinstance(output_length, bool) or not isinstance(output_length, int) or output_length < 1):
        raise ValueError('%s: output_length must be a positive int or None, got %r' % (what, output_length))
    for name, v in (('sound_speed', sound_speed), ('sample_rate', sample_rate)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (0 < v < math.inf):
            raise ValueError('%s: %s must be a positive finite number, got %r' % (what, name, v))
    return D


def absorption_of(absorption, room, D, batch):
    """``absorption`` as ``(B or 1, n_band, 2 D)`` of the room's dtype on its device: a float, ``(2 D,)``, ``(n_band, 2 D)`` (shared by a
    batch) or, for the batch form, ``(B, n_band, 2 D)``"""
    what = 'simulate_rir_ism_batch' if batch else 'simulate_rir_ism'
    if not torch.is_tensor(absorption):
        if isinstance(absorption, bool) or not isinstance(absorption, (int, float)):
            raise ValueError('%s: absorption must be a float or a tensor, got %r' % (what, type(absorption).__name__))
        return torch.full((1, 1, 2 * D), float(absorption), dtype=room.dtype, device=room.device)
    a = absorption
    if a.dim() < 1 or a.dim() > (3 if batch else 2) or a.shape[-1] != 2 * D or (a.dim() == 3 and a.shape[0] != room.shape[0]):
        raise ValueError('%s: absorption must be a float, (%d,), (n_band, %d)%s, got shape %s'
                         % (what, 2 * D, 2 * D, ' or (B, n_band, %d)' % (2 * D) if batch else '', tuple(a.shape)))
    if not a.is_floating_point():
        raise ValueError('%s: absorption must be a floating-point tensor' % what)
    a = a.reshape((1,) * (3 - a.dim()) + tuple(a.shape))
    if a.shape[1] < 1:
        raise ValueError('%s: absorption has no band' % what)
    return a.to(device=room.device, dtype=torch.promote_types(a.dtype, room.dtype) if a.dtype == torch.float64 else room.dtype)
