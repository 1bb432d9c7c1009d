"""Shared by tests/test_vad_cpu.py and tests/test_vad_gpu.py (a plain module: no tests in here): the definition of ``vad`` restated,
the signals, the bound ``DELTA`` and the decision-stability rule.

The restatement (``measures``) follows the issue's definition in vectorised torch, in float64 or float32, and returns the measures,
``raw = 21 + log(r / (c1 - c0))`` before the clamp (``-inf`` where ``r`` is not above 0) and ``r``.  ``decide`` is the decision over
one group of rows as plain Python loops over the definition's steps.

Signals (``signal``): every row is 0.01 Gaussian noise plus a voiced burst of 19 harmonics (f0 120 / 160 / 200 Hz, amplitude 0.3)
switched on at 0.9 / 1.1 / 1.3 s for 0.8 s; rows are 2.5 s + 37 samples long; a case is ``(2, 3, time)`` at 8, 16, 22.05, 44.1 or
48 kHz (``dft`` 1024, 2048, 4096, 8192, 8192; ``period`` 1103, odd, at 22.05 kHz; ``T`` 48 or 49).

``DELTA`` — what a measures array may differ by from the float64 restatement of the same float32 samples — is 4 times the largest
deviation, over every (row, frame) of the case table (the two level-dependence gains included), of the FLOAT32 restatement from
the float64 one: the yardstick is the definition's own float32 evaluation with torch's CPU transforms, never a kernel, and the
factor 4 (the margin ``griffinlim`` gets) allows another, equally valid float32 summation order in the two transforms.  The CPU
test prints it: 3.29e-4 (largest deviation 8.24e-5, at the gain 64 case) on the development host and 6.07e-4 on the MI355X host,
whose torch CPU transforms round differently; the kernels' largest deviation from the float64 measures was 2.03e-4 (8 kHz).

A group is STABLE when, in float64, every ``|mean_r - level|`` up to the trigger frame (every frame, for a group that never
triggers) exceeds ``DELTA``, and every measure the backward search consults has ``|raw - level| > DELTA`` and ``|raw| > DELTA``
(``raw = -inf`` for ``r`` not above 0 satisfies both).  Then every evaluation within ``DELTA`` of the float64 measures takes the same
``(k, i*, flush, start)``.  The table may hold no unstable group (``UNSTABLE_CAP`` = 0)."""
import functools
import math
from collections import namedtuple

import torch

RATES = (8000, 16000, 22050, 44100, 48000)
DFT = {8000: 1024, 16000: 2048, 22050: 4096, 44100: 8192, 48000: 8192}
GAINS = (2.0 ** -6, 2.0 ** 6)
SECONDS, EXTRA = 2.5, 37
F0 = (120.0, 160.0, 200.0)
ONSET = (0.9, 1.1, 1.3)
BURST, HARMONICS, AMPLITUDE, NOISE = 0.8, 19, 0.3, 0.01
FACTOR = 4.0
UNSTABLE_CAP = 0

NAMES = ('trigger_level', 'trigger_time', 'search_time', 'allowed_gap', 'pre_trigger_time', 'boot_time', 'noise_up_time',
         'noise_down_time', 'noise_reduction_amount', 'measure_freq', 'measure_duration', 'measure_smooth_time', 'hp_filter_freq',
         'lp_filter_freq', 'hp_lifter_freq', 'lp_lifter_freq')
DEFAULTS = dict(zip(NAMES, (7.0, 0.25, 1.0, 0.25, 0.0, 0.35, 0.1, 0.01, 1.35, 20.0, None, 0.4, 50.0, 6000.0, 150.0, 2000.0)))

Plan = namedtuple('Plan', 'rate mlen dft period n gap pre keep s0 s1 c0 c1 up down smooth trig boot_max level nra')
Measures = namedtuple('Measures', 'meas raw r')
Decision = namedtuple('Decision', 'k first flush start triggered')
Verdict = namedtuple('Verdict', 'decision stable margin_mean margin_level margin_zero')


def plan(rate, **kw):
    """the issue's plan table, restated"""
    a = dict(DEFAULTS, **kw)
    freq = a['measure_freq']
    mlen = int(rate * (a['measure_duration'] or 2.0 / freq) + 0.5)
    dft = 16
    while dft < mlen:
        dft *= 2
    period = int(rate / freq + 0.5)
    n = int(math.ceil(a['search_time'] * freq))
    pre = int(a['pre_trigger_time'] * rate + 0.5)
    decay = [math.exp(-1.0 / (a[t] * freq)) for t in ('noise_up_time', 'noise_down_time', 'measure_smooth_time', 'trigger_time')]
    return Plan(rate, mlen, dft, period, n, int(a['allowed_gap'] * freq + 0.5), pre, pre + n * period + mlen,
                max(int(a['hp_filter_freq'] / rate * dft + 0.5), 1), min(int(a['lp_filter_freq'] / rate * dft + 0.5), dft // 2),
                int(math.ceil(rate * 0.5 / a['lp_lifter_freq'])), min(int(math.floor(rate * 0.5 / a['hp_lifter_freq'])), dft // 4),
                decay[0], decay[1], decay[2], decay[3], int(a['boot_time'] * freq - 0.5), a['trigger_level'], a['noise_reduction_amount'])


def arguments(**kw):
    """the sixteen arguments in torchaudio's order, for a call"""
    a = dict(DEFAULTS, **kw)
    return tuple(a[name] for name in NAMES)


def n_frames(time, p):
    return 0 if time < p.mlen else 1 + (time - p.mlen) // p.period


def row(rate, which, seed, seconds=SECONDS, extra=EXTRA):
    """one row: noise plus the burst of voice ``which`` (0, 1, 2), float32"""
    n = int(seconds * rate) + extra
    gen = torch.Generator().manual_seed(1000 * seed + which)
    t = torch.arange(n, dtype=torch.float64) / rate
    x = NOISE * torch.randn(n, generator=gen, dtype=torch.float64)
    gate = ((t >= ONSET[which]) & (t < ONSET[which] + BURST)).to(torch.float64)
    voiced = sum(torch.sin(2.0 * math.pi * F0[which] * h * t) for h in range(1, HARMONICS + 1))
    return (x + AMPLITUDE * gate * voiced).to(torch.float32)


SEEDS = {8000: (11, 18), 16000: (3, 4), 22050: (5, 6), 44100: (7, 8), 48000: (9, 10)}


@functools.lru_cache(maxsize=None)
def signal(rate):
    """``(2, 3, time)`` float32: two groups of the three voices, with their own noise"""
    return torch.stack([torch.stack([row(rate, which, seed) for which in range(3)]) for seed in SEEDS[rate]])


def measures(x, p, dtype):
    """the definition's measures of ``x`` ``(…, time)`` in ``dtype``: ``Measures(meas, raw, r)``, each ``(…, T)``"""
    lead, time = tuple(x.shape[:-1]), x.shape[-1]
    rows = x.reshape(-1, time).to(dtype)
    frames_n = n_frames(time, p)
    nb, nq = p.s1 - p.s0, p.c1 - p.c0
    if frames_n == 0 or rows.shape[0] == 0:
        empty = rows.new_zeros(lead + (frames_n,))
        return Measures(empty, empty.clone(), empty.clone())
    starts = torch.arange(frames_n) * p.period
    frames = rows[:, starts[:, None] + torch.arange(p.mlen)[None, :]]                       # (rows, T, mlen)
    window = (2.0 / math.sqrt(p.mlen)) * torch.hann_window(p.mlen, dtype=torch.float32).to(dtype)
    spectrum = torch.fft.rfft(frames * window, n=p.dft, dim=-1).abs()[..., p.s0:p.s1]
    lifter = (2.0 / math.sqrt(nb)) * torch.hann_window(nb, dtype=torch.float32).to(dtype)
    smoothed = torch.zeros(rows.shape[0], nb, dtype=dtype)
    noise = torch.zeros(rows.shape[0], nb, dtype=dtype)
    e = torch.zeros(rows.shape[0], frames_n, p.dft // 2, dtype=dtype)
    up, down = torch.tensor(p.up, dtype=dtype), torch.tensor(p.down, dtype=dtype)
    boot = 0
    for t in range(frames_n):
        m = boot / (1.0 + boot) if boot >= 0 else p.smooth
        smoothed = smoothed * m + spectrum[:, t] * (1.0 - m)
        d = smoothed ** 2
        m2 = torch.zeros_like(d) if boot >= 0 else torch.where(d > noise, up, down)
        noise = noise * m2 + d * (1.0 - m2)
        e[:, t, p.s0:p.s1] = torch.sqrt(torch.clamp(d - p.nra * noise, min=0.0)) * lifter
        if boot >= 0:
            boot = -1 if boot == p.boot_max else boot + 1
    c = torch.fft.rfft(e, dim=-1)[..., p.c0:p.c1]
    r = (c.real ** 2 + c.imag ** 2).sum(-1)
    positive = r > 0
    raw = torch.where(positive, 21.0 + torch.log(torch.where(positive, r, torch.ones_like(r)) / nq), torch.full_like(r, -math.inf))
    meas = torch.clamp(raw, min=0.0)
    shape = lead + (frames_n,)
    return Measures(meas.reshape(shape), raw.reshape(shape), r.reshape(shape))


def means(meas, p):
    """the decayed means ``(C, T)`` of a group's measures ``(C, T)``"""
    out = torch.zeros_like(meas)
    mean = torch.zeros(meas.shape[0], dtype=meas.dtype)
    for k in range(meas.shape[1]):
        mean = mean * p.trig + meas[:, k] * (1.0 - p.trig)
        out[:, k] = mean
    return out


def search(meas_row, k, p):
    """``jZ`` of one row's backward search from frame ``k``, and the frames it consulted"""
    j_t = j_z = p.n
    seen = []
    for j in range(p.n):
        v = float(meas_row[k - j]) if k - j >= 0 else 0.0
        if k - j >= 0:
            seen.append(k - j)
        if v >= p.level and j <= j_t + p.gap:
            j_z = j_t = j
        elif v == 0 and j_t >= j_z:
            j_z = j
    return j_z, seen


def decide(meas, p, time):
    """``Decision`` of one group: ``meas`` is ``(C, T)``, its rows the channels in order"""
    mean = means(meas, p)
    hit = mean >= p.level
    frames = hit.any(0).nonzero()
    if frames.numel() == 0:
        return Decision(None, None, None, max(time - p.keep, 0), False)
    k = int(frames[0])
    first = int(hit[:, k].nonzero()[0])
    flush = 0
    for i in range(first, meas.shape[0]):
        j_z, _ = search(meas[i], k, p)
        flush = min(max(flush, min(p.n - 1, j_z)), p.n)
    return Decision(k, first, flush, max((k - flush) * p.period - p.pre, 0), True)


def judge(m64, p, time, delta):
    """``Verdict`` of one group from its float64 ``Measures`` ``(C, T)``"""
    decision = decide(m64.meas, p, time)
    mean = means(m64.meas, p)
    upto = mean.shape[1] if not decision.triggered else decision.k + 1
    margin_mean = float((mean[:, :upto] - p.level).abs().min()) if upto and mean.shape[0] else math.inf
    margin_level = margin_zero = math.inf
    if decision.triggered:
        for i in range(decision.first, m64.meas.shape[0]):
            _, seen = search(m64.meas[i], decision.k, p)
            raw = m64.raw[i, seen]
            margin_level = min(margin_level, float((raw - p.level).abs().min()))
            margin_zero = min(margin_zero, float(raw.abs().min()))
    stable = margin_mean > delta and margin_level > delta and margin_zero > delta
    return Verdict(decision, stable, margin_mean, margin_level, margin_zero)


Case = namedtuple('Case', 'x plan m64 m32')


@functools.lru_cache(maxsize=None)
def case(rate, gain=1.0):
    """the ``(2, 3, time)`` signal of ``rate`` times ``gain`` with its float64 and float32 restatements, computed once"""
    x = signal(rate) * gain
    p = plan(rate)
    return Case(x, p, measures(x, p, torch.float64), measures(x, p, torch.float32))


def table():
    """every case ``DELTA`` is taken over"""
    return [case(rate) for rate in RATES] + [case(16000, gain) for gain in GAINS]


@functools.lru_cache(maxsize=None)
def delta():
    """``(DELTA, the largest float32 deviation)`` over the case table"""
    worst = max(float((c.m32.meas.double() - c.m64.meas).abs().max()) for c in table())
    return FACTOR * worst, worst


def groupings(m, joint):
    """the groups ``(C, T)`` of a ``(2, 3, T)`` array under ``joint``, in the order of the flattened result"""
    if joint == 'all':
        return [m.reshape(-1, m.shape[-1])]
    if joint == 'channel':
        return [m[b] for b in range(m.shape[0])]
    return [m[b, c:c + 1] for b in range(m.shape[0]) for c in range(m.shape[1])]


def group_measures(m, joint):
    return [Measures(a, b, c) for a, b, c in zip(groupings(m.meas, joint), groupings(m.raw, joint), groupings(m.r, joint))]


def verdicts(c, joint):
    """the ``Verdict`` of every group of a case under ``joint``"""
    return [judge(g, c.plan, c.x.shape[-1], delta()[0]) for g in group_measures(c.m64, joint)]


def assert_measures(got, c, what):
    """``got`` ``(…, T)`` within ``DELTA`` of the float64 restatement at every (row, frame); returns the largest deviation"""
    bound = delta()[0]
    assert tuple(got.shape) == tuple(c.m64.meas.shape), (what, tuple(got.shape))
    err = (got.detach().cpu().double() - c.m64.meas).abs()
    assert bool(torch.isfinite(err).all()), what
    worst = float(err.max()) if err.numel() else 0.0
    print('%s: largest deviation from the float64 measures %.3g (DELTA %.3g)' % (what, worst, bound))
    assert worst <= bound, '%s: %.3g beyond DELTA %.3g at %r' % (what, worst, bound, (err == err.max()).nonzero()[0].tolist())
    return worst


def assert_starts(start, triggered, c, joint, what):
    """the device results against the float64 decisions of every (stable) group"""
    vs = verdicts(c, joint)
    assert all(v.stable for v in vs), what
    want_start = torch.tensor([v.decision.start for v in vs])
    want_trig = torch.tensor([v.decision.triggered for v in vs])
    assert start.dtype == torch.int64 and triggered.dtype == torch.bool, what
    assert torch.equal(start.detach().cpu().reshape(-1), want_start), (what, start, want_start)
    assert torch.equal(triggered.detach().cpu().reshape(-1), want_trig), (what, triggered, want_trig)


# ----------------------------------------------------------------------------- launch 2's grid (csrc/vad.hip)
VAD_LAUNCH = ('vad.hip', (
    'constexpr int VD_PER_CU = 2;',
    'persistent_blocks(rows, 1, (long long)device_cu_count() * VD_PER_CU)',
    'for (long long row = blockIdx.x; row < A.rows; row += gridDim.x) {',
))
VAD_PER_CU = 2


def measure_grid(cus, rows):
    """(work, grid) of ``tac_vad_measures_f32``: a unit is a row"""
    return rows, max(1, min(rows, cus * VAD_PER_CU))
