"""Plan and argument checks of ``vad`` (host arithmetic only; shared by ``functional``, ``layers``, ``_ops``, ``_hip`` and
``_composite``): torchaudio's SoX voice-activity detector restated as a table of integers and four decay factors."""
import math
from collections import namedtuple

#: torchaudio's argument names behind ``(waveform, sample_rate)``, in its order, and their defaults
ARGS = ('trigger_level', 'trigger_time', 'search_time', 'allowed_gap', 'pre_trigger_time', 'boot_time', 'noise_up_time',
        'noise_down_time', 'noise_reduction_amount', 'measure_freq', 'measure_duration', 'measure_smooth_time', 'hp_filter_freq',
        'lp_filter_freq', 'hp_lifter_freq', 'lp_lifter_freq')
DEFAULTS = (7.0, 0.25, 1.0, 0.25, 0.0, 0.35, 0.1, 0.01, 1.35, 20.0, None, 0.4, 50.0, 6000.0, 150.0, 2000.0)
JOINT = ('all', 'channel', 'none')

Plan = namedtuple('Plan', 'rate mlen dft period n gap pre keep s0 s1 c0 c1 up down smooth trig boot_max level nra')


def _number(name, v, positive):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not (0 < v if positive else 0 <= v) or not v < math.inf:
        raise ValueError('vad: %s must be a %s finite number, got %r' % (name, 'positive' if positive else 'non-negative', v))


def resolve(args):
    """the sixteen arguments as floats, ``measure_duration=None`` as ``2 / measure_freq``: what the ops take"""
    if len(args) != len(ARGS):
        raise TypeError('vad: expected %d arguments behind sample_rate, got %d' % (len(ARGS), len(args)))
    a = dict(zip(ARGS, args))
    _number('measure_freq', a['measure_freq'], True)
    if a['measure_duration'] is None:
        a['measure_duration'] = 2.0 / a['measure_freq']
    for name in ARGS:
        v = a[name]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError('vad: %s must be a finite number, got %r' % (name, v))
    return tuple(float(a[name]) for name in ARGS)


def plan(sample_rate, *args):
    """``Plan`` of the sixteen resolved arguments at ``sample_rate``: ``mlen`` samples a measurement window every ``period`` samples
    in a ``dft``-point transform, spectrum bins ``[s0, s1)``, cepstrum bins ``[c0, c1)`` of the ``dft / 2``-point transform, the
    decay factors ``exp(-1 / (t measure_freq))``, ``boot_max`` (frames ``0 … boot_max`` boot the noise estimate), a backward search of
    ``n`` measures with gaps of ``gap``, ``pre`` samples kept before the trigger and ``keep = pre + n period + mlen`` samples of an
    input that never triggers.  ``ValueError`` for arguments the definition has no answer to."""
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or sample_rate <= 0:
        raise ValueError('vad: sample_rate must be a positive int, got %r' % (sample_rate,))
    a = dict(zip(ARGS, resolve(args)))
    for name in ('trigger_time', 'search_time', 'noise_up_time', 'noise_down_time', 'measure_freq', 'measure_duration',
                 'measure_smooth_time', 'hp_filter_freq', 'lp_filter_freq', 'hp_lifter_freq', 'lp_lifter_freq'):
        _number(name, a[name], True)
    for name in ('allowed_gap', 'pre_trigger_time', 'boot_time'):
        _number(name, a[name], False)
    rate, freq = sample_rate, a['measure_freq']
    mlen = int(rate * a['measure_duration'] + 0.5)
    period = int(rate / freq + 0.5)
    if mlen < 1 or period < 1:
        raise ValueError('vad: a measurement window of %d samples every %d samples at sample_rate %d' % (mlen, period, rate))
    dft = 16
    while dft < mlen:
        dft *= 2
    n = int(math.ceil(a['search_time'] * freq))
    gap = int(a['allowed_gap'] * freq + 0.5)
    pre = int(a['pre_trigger_time'] * rate + 0.5)
    s0 = max(int(a['hp_filter_freq'] / rate * dft + 0.5), 1)
    s1 = min(int(a['lp_filter_freq'] / rate * dft + 0.5), dft // 2)
    c0 = int(math.ceil(rate * 0.5 / a['lp_lifter_freq']))
    c1 = min(int(math.floor(rate * 0.5 / a['hp_lifter_freq'])), dft // 4)
    if s1 <= s0:
        raise ValueError('vad: no spectrum bin to measure: [%d, %d) of %d at sample_rate %d, hp_filter_freq %r, lp_filter_freq %r'
                         % (s0, s1, dft, rate, a['hp_filter_freq'], a['lp_filter_freq']))
    if c1 <= c0:
        raise ValueError('vad: no cepstrum bin to measure: [%d, %d) at sample_rate %d, hp_lifter_freq %r, lp_lifter_freq %r'
                         % (c0, c1, rate, a['hp_lifter_freq'], a['lp_lifter_freq']))
    decay = [math.exp(-1.0 / (a[name] * freq)) for name in ('noise_up_time', 'noise_down_time', 'measure_smooth_time', 'trigger_time')]
    return Plan(rate, mlen, dft, period, n, gap, pre, pre + n * period + mlen, s0, s1, c0, c1, decay[0], decay[1], decay[2], decay[3],
                int(a['boot_time'] * freq - 0.5), a['trigger_level'], a['noise_reduction_amount'])


def frames(time, p):
    """measurement windows of a row of ``time`` samples: ``1 + (time - mlen) // period``, 0 for a row shorter than one"""
    return 0 if time < p.mlen else 1 + (time - p.mlen) // p.period


def check(waveform, sample_rate, *args):
    """``plan`` for ``waveform`` ``(…, time)``; ``ValueError`` also for a tensor without a time axis or of a non-floating dtype"""
    if waveform.dim() < 1:
        raise ValueError('vad: waveform must be (…, time), got a tensor without dimensions')
    if not waveform.is_floating_point():
        raise ValueError('vad: waveform must be a floating-point tensor, got %s' % waveform.dtype)
    return plan(sample_rate, *args)


def groups(shape, joint):
    """``(lead, channels)``: the shape of the result and the rows that decide together, for a waveform of ``shape`` — ``'all'``:
    every leading dimension is a channel of one group (torchaudio); ``'channel'``: axis -2; ``'none'``: every row on its own"""
    if joint not in JOINT:
        raise ValueError('vad_start: joint must be one of %r, got %r' % (JOINT, joint))
    lead = tuple(int(s) for s in shape[:-1])
    if joint == 'all':
        return (), int(math.prod(lead))
    if joint == 'channel':
        if len(lead) < 1:
            raise ValueError("vad_start: joint='channel' needs a waveform of (…, channel, time), got %d dimension" % len(shape))
        return lead[:-1], lead[-1]
    return lead, 1
