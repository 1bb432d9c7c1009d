"""Host side of the SoX effects (``overdrive``, ``phaser``, ``flanger``): argument checks, the derived integers and the LFO tables.

Everything here is numpy float64 and Python numbers; the formulas are torchaudio's (``functional/filtering.py``,
``_generate_wave_table``).  A table is built once per parameter set and kept (``Bounded``); its device copy hangs on the host
tensor through ``_hip.cached_on``."""
import math

import numpy as np
import torch

from ._bounded import Bounded

SINE, TRIANGLE = 'SINE', 'TRIANGLE'
INT, FLOAT = 'INT', 'FLOAT'

#: SoX's parameter ranges: inside them (and float32 on a HIP device) the gfx950 kernels run, outside the announced composites
OVERDRIVE_RANGES = {'gain': (0.0, 100.0), 'colour': (0.0, 100.0)}
PHASER_RANGES = {'gain_in': (0.0, 1.0), 'delay_ms': (0.0, 5.0), 'decay': (0.0, 0.99), 'mod_speed': (0.1, 2.0)}
FLANGER_RANGES = {'delay': (0.0, 30.0), 'depth': (0.0, 10.0), 'regen': (-95.0, 95.0), 'width': (0.0, 100.0), 'speed': (0.1, 10.0),
                  'phase': (0.0, 100.0)}
FLANGER_MAX_CHANNELS = 4
#: slots per step of the flanger's feedback path: the lanes of a wave (csrc/sox_effects.hip: FL_MAX_BLOCK)
FLANGER_MAX_BLOCK = 64


def wave_table(kind, data_type, n, lo, hi, phase):
    """torchaudio's ``_generate_wave_table`` in numpy float64: ``n`` samples of one LFO period between ``lo`` and ``hi``, starting
    at ``phase`` radians; ``INT`` rounds half away from zero to int32, ``FLOAT`` rounds to float32."""
    off = int(phase / math.pi / 2 * n + 0.5)
    p = (np.arange(n, dtype=np.int64) + off) % n
    if kind == SINE:
        d = (np.sin(p.astype(np.float64) / n * 2 * np.pi) + 1) / 2
    elif kind == TRIANGLE:
        d = p.astype(np.float64) * 2 / n
        v = (4 * p) // n
        d = np.where(v == 0, d + 0.5, np.where(v == 3, d - 1.5, 1.5 - d))
    else:
        raise ValueError('wave_table: kind %r' % (kind,))
    d = d * (hi - lo) + lo
    if data_type == INT:
        return np.where(d < 0, d - 0.5, d + 0.5).astype(np.int32)
    if data_type == FLOAT:
        return d.astype(np.float32)
    raise ValueError('wave_table: data type %r' % (data_type,))


def inside(ranges, **values):
    """None when every value lies inside its SoX range, else the reason for the composite route"""
    for name, v in values.items():
        lo, hi = ranges[name]
        if not (lo <= v <= hi):                 # (a NaN is outside)
            return '%s = %r outside [%g, %g]' % (name, v, lo, hi)
    return None


def overdrive_constants(gain, colour):
    """``(g, c)``: the linear gain and the offset"""
    return math.exp(gain * math.log(10) / 20.0), colour / 200.0


_plans = Bounded(64)


def _kept(key, build):
    hit = _plans.get(key)
    if hit is None:
        with torch.inference_mode(False):
            hit = build()
        _plans[key] = hit
    return hit


def phaser_plan(sample_rate, delay_ms, mod_speed, sinusoidal):
    """``(L, P, table)``: the delay in samples, the LFO period and the int32 host tensor of ``P`` modulation values in ``[1, L]``.
    ``ValueError`` where torchaudio would divide by zero."""
    sample_rate, delay_ms, mod_speed = float(sample_rate), float(delay_ms), float(mod_speed)
    if not sample_rate > 0 or not math.isfinite(sample_rate):
        raise ValueError('phaser: sample_rate must be positive, got %r' % sample_rate)
    if not mod_speed > 0 or not math.isfinite(mod_speed) or not math.isfinite(delay_ms):
        raise ValueError('phaser: mod_speed must be positive and delay_ms finite, got %r and %r' % (mod_speed, delay_ms))
    L = int(delay_ms * 0.001 * sample_rate + 0.5)
    P = int(sample_rate / mod_speed + 0.5)
    if L < 1 or P < 1:
        raise ValueError('phaser: delay_ms %r at %r Hz is %d samples and the LFO period %d: both must be at least 1'
                         % (delay_ms, sample_rate, L, P))
    if P >= 2 ** 31 or L >= 2 ** 31:
        raise ValueError('phaser: the LFO period %d or the delay %d does not fit 32 bits' % (P, L))

    def build():
        m = wave_table(SINE if sinusoidal else TRIANGLE, INT, P, 1.0, float(L), math.pi / 2)
        return L, P, torch.from_numpy(m)
    return _kept(('phaser', sample_rate, delay_ms, mod_speed, bool(sinusoidal)), build)


class FlangerPlan(object):
    __slots__ = ('fb', 'in_gain', 'delay_gain', 'Lb', 'P', 'tmin', 'W', 'lfo', 'phases', 'quadratic')


def flanger_plan(sample_rate, delay, depth, regen, width, speed, phase, modulation, interpolation, channels):
    """The constants of torchaudio's ``flanger`` — feedback, gains, the delay line ``Lb``, the LFO period ``P``, its lowest delay
    ``tmin``, the slots per step ``W = min(64, 1 + tmin)``, the per-channel LFO phases — and the float32 host LFO table, kept by
    value.  ``ValueError`` for unknown names and where torchaudio would divide by zero."""
    if modulation not in ('sinusoidal', 'triangular'):
        raise ValueError("flanger: modulation must be 'sinusoidal' or 'triangular', got %r" % (modulation,))
    if interpolation not in ('linear', 'quadratic'):
        raise ValueError("flanger: interpolation must be 'linear' or 'quadratic', got %r" % (interpolation,))
    sample_rate, delay, depth, regen, width, speed, phase = (float(v) for v in (sample_rate, delay, depth, regen, width, speed, phase))
    if not sample_rate > 0 or not math.isfinite(sample_rate):
        raise ValueError('flanger: sample_rate must be positive, got %r' % sample_rate)
    if not speed > 0 or not all(math.isfinite(v) for v in (delay, depth, regen, width, speed, phase)):
        raise ValueError('flanger: speed must be positive and every parameter finite')
    if delay < 0 or depth < 0 or phase < 0 or width <= -100.0:
        raise ValueError('flanger: delay, depth and phase must not be negative and width must exceed -100')

    def build():
        q = FlangerPlan()
        q.fb = regen / 100.0
        dg = width / 100.0
        q.in_gain = 1.0 / (1.0 + dg)
        q.delay_gain = dg / (1.0 + dg) * (1.0 - abs(q.fb))
        q.Lb = int((delay + depth) / 1000.0 * sample_rate + 0.5) + 2
        q.P = int(sample_rate / speed)
        if q.P < 1:
            raise ValueError('flanger: the LFO period int(%r / %r) must be at least 1' % (sample_rate, speed))
        if q.P >= 2 ** 30 or q.Lb >= 2 ** 30:
            raise ValueError('flanger: the LFO period %d or the delay line %d is too long' % (q.P, q.Lb))
        q.tmin = int(math.floor(delay / 1000.0 * sample_rate + 0.5))
        q.W = min(FLANGER_MAX_BLOCK, 1 + q.tmin)
        q.lfo = torch.from_numpy(wave_table(SINE if modulation == 'sinusoidal' else TRIANGLE, FLOAT, q.P, float(q.tmin),
                                            q.Lb - 2.0, 3 * math.pi / 2))
        q.phases = tuple(int(c * q.P * phase / 100.0 + 0.5) for c in range(max(1, channels)))
        q.quadratic = interpolation == 'quadratic'
        return q
    return _kept(('flanger', sample_rate, delay, depth, regen, width, speed, phase, modulation, interpolation, int(channels)), build)
