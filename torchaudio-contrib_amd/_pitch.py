"""Frame geometry and argument checks of ``detect_pitch_frequency`` (host arithmetic only; shared by ``functional``, ``layers``,
``_ops`` and ``_composite``)."""
import math
from collections import namedtuple

Geometry = namedtuple('Geometry', 'frame max_lag lag_min half n_frames pad n_out')


def _positive(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 < v < math.inf:
        raise ValueError('detect_pitch_frequency: %s must be a positive finite number, got %r' % (name, v))


def geometry(time, sample_rate, frame_time, win_length, freq_low, freq_high):
    """``Geometry`` of a row of ``time`` samples: ``frame = ceil(sample_rate frame_time)`` samples a frame, lags ``1 .. max_lag =
    ceil(sample_rate / freq_low)``, the search from column ``lag_min = ceil(sample_rate / freq_high)`` to ``max_lag`` and to ``half =
    max_lag // 2``, ``n_frames = ceil(time / frame)``, ``pad = (win_length - 1) // 2`` copies of the first lag in front of the
    median and ``n_out = n_frames + pad - win_length + 1`` outputs.  ``ValueError`` for arguments the definition has no answer to."""
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or sample_rate <= 0:
        raise ValueError('detect_pitch_frequency: sample_rate must be a positive int, got %r' % (sample_rate,))
    for name, v in (('frame_time', frame_time), ('freq_low', freq_low), ('freq_high', freq_high)):
        _positive(name, v)
    if isinstance(win_length, bool) or not isinstance(win_length, int) or win_length < 1:
        raise ValueError('detect_pitch_frequency: win_length must be an int of 1 or more, got %r' % (win_length,))
    if time < 1:
        raise ValueError('detect_pitch_frequency: the waveform has no samples')
    frame = int(math.ceil(sample_rate * frame_time))
    max_lag = int(math.ceil(sample_rate / freq_low))
    lag_min = int(math.ceil(sample_rate / freq_high))
    half = max_lag // 2
    if lag_min >= half:
        raise ValueError('detect_pitch_frequency: no lag to search: columns [%d, %d) at sample_rate %r, freq_low %r, freq_high %r'
                         % (lag_min, half, sample_rate, freq_low, freq_high))
    n_frames = -(-time // frame)
    pad = (win_length - 1) // 2
    n_out = n_frames + pad - win_length + 1
    if n_out < 1:
        raise ValueError('detect_pitch_frequency: %d frames of %d samples are fewer than a median window of %d takes (%d with its '
                         'padding)' % (n_frames, frame, win_length, n_frames + pad))
    return Geometry(frame, max_lag, lag_min, half, n_frames, pad, n_out)


def check(waveform, sample_rate, frame_time, win_length, freq_low, freq_high):
    """``geometry`` of ``waveform`` ``(…, time)``; ``ValueError`` also for a tensor without a time axis or of a non-floating dtype"""
    if waveform.dim() < 1:
        raise ValueError('detect_pitch_frequency: waveform must be (…, time), got a tensor without dimensions')
    if not waveform.is_floating_point():
        raise ValueError('detect_pitch_frequency: waveform must be a floating-point tensor, got %s' % waveform.dtype)
    return geometry(waveform.shape[-1], sample_rate, frame_time, win_length, freq_low, freq_high)
