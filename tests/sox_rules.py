"""Shared by tests/test_sox_cpu.py and tests/test_sox_gpu.py: the SoX effects ``overdrive``, ``phaser`` and ``flanger`` restated in
numpy, the bound every float32 result is held to, and input makers.  No tests in here.

References: the LITERAL loops of torchaudio's ``functional/filtering.py`` (ring buffers and all) in float64, vectorised over rows;
the same loops in float32 are what torchaudio computes on float32 input.  The closed form of the phaser and the blocked form of
the flanger, which the kernels rest on, are restated next to them and tested against the literal ones.

Bounds, per element, derived as ``lfilter_rules`` derives its own.  The kernels read float32, keep every state in float64 and round
the result once, so

    |got - ref| <= 2^-24 |raw| + 2^-40 mass + 2^-126

with ``raw`` the unclamped float64 result (clipping is a contraction, so both sides are compared after it under the same bound),
``2^-126`` for flushed denormals and ``mass`` the magnitude every float64 rounding acts on, carried to the output by the SAME
recursion run on absolute values — every product and sum at sample ``m`` is rounded at 2^-53 of its magnitude and reaches sample
``n`` through the recursion's own (absolute) gains; 2^-40 leaves 2^13 for the operation counts (a few per sample, the
``log2(tile)`` levels of a scan or of pointer jumping, and the up to 4096 factors a jumped coefficient is a product of):

    overdrive   inner[n] = |g x[n]| + |c| + |t[n]| + |t[n-1]| + |v[n]|,   M[n] = inner[n] + 0.995 M[n-1],
                mass = 0.5 |x| + 0.75 M + |raw|
    phaser      inner[n] = gain_in |x[n]| + decay |y[n-d]| + |y[n]|,      M[n] = inner[n] + decay M[n-d],   mass = gain_out M
    flanger     Mdl[i] = the taps' magnitudes as the interpolation formula combines them (2 |w0| + |w1| linear,
                5 |w0| + 3 |w1| + |w2| quadratic),  Ew[i] = 2^-40 (|x[i]| + |fb| Mdl[i-1]) + |fb| Edl[i-1],
                Edl[i] = 2^-40 Mdl[i] + sum_j |weight_j| Ew[i-k-j];   the bound is
                2^-24 |raw| + delay_gain Edl + 2^-40 (in_gain |x| + delay_gain Mdl + |raw|) + 2^-126
                (the kernel's FIR path, ``fb == 0``, computes in float64 as well, so the same rule holds with ``Ew`` = 2^-40 |x|).

float32 arithmetic (the CPU route of the ops in float32, and the float32 literal loops) is held to the same rule with 2^-24 in
place of 2^-53 and a factor ``OPS32 = 16`` for the operations per sample in place of the 2^13: ``bound32``, first-order in 2^-24
and doubled for that reason."""
import math

import numpy as np
import torch

import lfilter_rules as L

EPS32, EPS_ARITH, TINY = L.EPS32, L.EPS_ARITH, L.TINY
OPS32 = 16
assert_close = L.assert_close
_np64 = L._np64

SINE, TRIANGLE, INT, FLOAT = 'SINE', 'TRIANGLE', 'INT', 'FLOAT'


# ----------------------------------------------------------------------------- the LFO table
def wave_table(kind, data_type, n, lo, hi, phase):
    off = int(phase / math.pi / 2 * n + 0.5)
    p = (np.arange(n, dtype=np.int64) + off) % n
    if kind == SINE:
        d = (np.sin(p.astype(np.float64) / n * 2 * np.pi) + 1) / 2
    else:
        assert kind == TRIANGLE
        d = p.astype(np.float64) * 2 / n
        v = (4 * p) // n
        d = np.select([v == 0, v == 3], [d + 0.5, d - 1.5], 1.5 - d)
    d = d * (hi - lo) + lo
    if data_type == INT:
        return np.trunc(np.where(d < 0, d - 0.5, d + 0.5)).astype(np.int32)
    assert data_type == FLOAT
    return d.astype(np.float32)


# ----------------------------------------------------------------------------- inputs
def waveform(shape, seed, scale=1.0):
    """``lfilter_rules.waveform`` (randn with a stretch of zeros and one at 1e-30), scaled"""
    return (np.float32(scale) * L.waveform(shape, seed)).astype(np.float32)


def _bound(raw, mass):
    return EPS32 * np.abs(raw) + EPS_ARITH * mass + TINY


def bound32(mass):
    return 2.0 * OPS32 * EPS32 * mass + TINY


# ----------------------------------------------------------------------------- overdrive
def overdrive_constants(gain, colour):
    return math.exp(gain * math.log(10) / 20.0), colour / 200.0


def overdrive_literal(x, gain, colour, dtype=np.float64):
    """``(raw, t, v)``: the unclamped result, the shaped signal and the recursion's state, in ``dtype``"""
    g, c = (dtype(v) for v in overdrive_constants(gain, colour))
    x = np.asarray(x).astype(dtype)
    flat = x.reshape(-1, x.shape[-1])
    t = flat * g + c
    t = np.where(t < -1, dtype(-2.0 / 3.0), np.where(t > 1, dtype(2.0 / 3.0), t - t * t * t / dtype(3.0))).astype(dtype)
    v = np.zeros_like(t)
    last_in = np.zeros(flat.shape[0], dtype)
    last_out = np.zeros(flat.shape[0], dtype)
    for i in range(flat.shape[1]):
        last_out = t[:, i] - last_in + dtype(0.995) * last_out
        last_in = t[:, i]
        v[:, i] = last_out
    raw = flat * dtype(0.5) + v * dtype(0.75)
    return raw.reshape(x.shape), t.reshape(x.shape), v.reshape(x.shape)


def _first_order_mass(inner, a):
    m = np.empty_like(inner)
    acc = np.zeros(inner.shape[:-1])
    for i in range(inner.shape[-1]):
        acc = inner[..., i] + a * acc
        m[..., i] = acc
    return m


def overdrive(x, gain, colour):
    """``(ref, bound, mass)``: float64, clipped to [-1, 1]"""
    g, c = overdrive_constants(gain, colour)
    raw, t, v = overdrive_literal(x, gain, colour)
    ax = np.abs(_np64(x))
    tp = np.concatenate([np.zeros_like(t[..., :1]), np.abs(t[..., :-1])], axis=-1)
    inner = g * ax + abs(c) + np.abs(t) + tp + np.abs(v)
    mass = 0.5 * ax + 0.75 * _first_order_mass(inner, 0.995) + np.abs(raw)
    return np.clip(raw, -1.0, 1.0), _bound(raw, mass), mass


def overdrive_gradient(x, gy, gain, colour):
    """``(grad, mass, raw)``: the float64 gradient of ``sum(overdrive(x) * gy)`` w.r.t. ``x``, the magnitude its float32 steps act
    on (for ``bound32``) and the unclamped forward result (the caller leaves out the elements where rounding decides the clamp).
    out = clamp(0.5 x + 0.75 v), v = F t, t = shape(g x + c): grad = 0.5 m + g (1 - t_lin^2) [|t_lin| <= 1] F^T (0.75 m), m = gy
    where the unclamped result lies strictly inside (-1, 1)."""
    g, c = overdrive_constants(gain, colour)
    x64, gy64 = _np64(x), _np64(gy)
    raw, _, _ = overdrive_literal(x64, gain, colour)
    m = gy64 * (np.abs(raw) < 1.0)

    def adjoint(u):            # F^T: q[n] = u[n] + 0.995 q[n+1];  result q[n] - q[n+1]
        q = _first_order_mass(u[..., ::-1], 0.995)[..., ::-1]
        nxt = np.concatenate([q[..., 1:], np.zeros_like(q[..., :1])], axis=-1)
        return q - nxt, q + nxt
    ft, ft_mag = adjoint(0.75 * m)
    _, ft_abs = adjoint(0.75 * np.abs(m))
    tl = g * x64 + c
    slope = np.where(np.abs(tl) <= 1.0, g * (1.0 - tl * tl), 0.0)
    grad = 0.5 * m + slope * ft
    mass = 0.5 * np.abs(m) + (np.abs(slope) + g) * ft_abs
    return grad, mass, raw


# ----------------------------------------------------------------------------- phaser
def phaser_plan(sample_rate, delay_ms, mod_speed, sinusoidal):
    L_ = int(delay_ms * 0.001 * sample_rate + 0.5)
    P = int(sample_rate / mod_speed + 0.5)
    return L_, P, wave_table(SINE if sinusoidal else TRIANGLE, INT, P, 1.0, float(L_), math.pi / 2)


def phaser_literal(x, sample_rate, gain_in=0.4, gain_out=0.74, delay_ms=3.0, decay=0.4, mod_speed=0.5, sinusoidal=True,
                   dtype=np.float64):
    """torchaudio's loop over a ring of ``L`` samples: ``y`` before ``gain_out`` and the clamp, in ``dtype``"""
    L_, P, m = phaser_plan(sample_rate, delay_ms, mod_speed, sinusoidal)
    x = np.asarray(x).astype(dtype)
    flat = x.reshape(-1, x.shape[-1])
    buf = np.zeros((flat.shape[0], L_), dtype)
    y = np.empty_like(flat)
    delay_pos = mod_pos = 0
    gi, dc = dtype(gain_in), dtype(decay)
    for i in range(flat.shape[1]):
        idx = int((delay_pos + m[mod_pos]) % L_)
        mod_pos = (mod_pos + 1) % P
        delay_pos = (delay_pos + 1) % L_
        temp = flat[:, i] * gi + buf[:, idx]
        buf[:, delay_pos] = temp * dc
        y[:, i] = temp
    return y.reshape(x.shape)


def phaser_closed(x, sample_rate, gain_in=0.4, gain_out=0.74, delay_ms=3.0, decay=0.4, mod_speed=0.5, sinusoidal=True,
                  inner=None):
    """``y[n] = gain_in x[n] + decay y[n - d(n)]``, ``d(n) = L - m[n mod P] + 1``, zero before the row; with ``inner`` given the
    same recursion on it instead of on ``gain_in x`` (the bound's mass)"""
    L_, P, m = phaser_plan(sample_rate, delay_ms, mod_speed, sinusoidal)
    x64 = _np64(x)
    flat = (gain_in * x64 if inner is None else inner).reshape(-1, x64.shape[-1])
    y = np.zeros_like(flat)
    for n in range(flat.shape[1]):
        p = n - (L_ - int(m[n % P]) + 1)
        y[:, n] = flat[:, n] + (decay * y[:, p] if p >= 0 else 0.0)
    return y.reshape(x64.shape)


def phaser_parents(length, sample_rate, delay_ms, mod_speed, sinusoidal):
    L_, P, m = phaser_plan(sample_rate, delay_ms, mod_speed, sinusoidal)
    n = np.arange(length)
    return n - (L_ - m[n % P].astype(np.int64) + 1)


def phaser_jumped(x, sample_rate, gain_in=0.4, gain_out=0.74, delay_ms=3.0, decay=0.4, mod_speed=0.5, sinusoidal=True):
    """Pointer jumping over (value, coefficient, parent) triples over the whole row: ``(y, rounds)``"""
    x64 = _np64(x)
    flat = x64.reshape(-1, x64.shape[-1])
    val = gain_in * flat
    par = phaser_parents(flat.shape[1], sample_rate, delay_ms, mod_speed, sinusoidal)
    coef = np.full(flat.shape[1], float(decay))
    rounds = 0
    while (par >= 0).any():
        live = par >= 0
        p = np.where(live, par, 0)
        val = val + np.where(live, coef * val[:, p], 0.0)
        coef = np.where(live, coef * coef[p], coef)
        par = np.where(live, par[p], par)
        rounds += 1
    return val.reshape(x64.shape), rounds


def phaser(x, sample_rate, gain_in=0.4, gain_out=0.74, delay_ms=3.0, decay=0.4, mod_speed=0.5, sinusoidal=True):
    """``(ref, bound, mass)``: float64, clipped to [-1, 1]"""
    args = (sample_rate, gain_in, gain_out, delay_ms, decay, mod_speed, sinusoidal)
    y = phaser_literal(x, *args)
    par = phaser_parents(y.shape[-1], sample_rate, delay_ms, mod_speed, sinusoidal)
    yp = np.where(par >= 0, np.abs(y[..., np.maximum(par, 0)]), 0.0)
    inner = gain_in * np.abs(_np64(x)) + decay * yp + np.abs(y)
    mass = abs(gain_out) * phaser_closed(x, *args, inner=inner)
    raw = gain_out * y
    return np.clip(raw, -1.0, 1.0), _bound(raw, mass), mass


# ----------------------------------------------------------------------------- flanger
class FlangerPlan(object):
    pass


def flanger_plan(sample_rate, delay=0.0, depth=2.0, regen=0.0, width=71.0, speed=0.5, phase=25.0, modulation='sinusoidal',
                 interpolation='linear', channels=1):
    q = FlangerPlan()
    q.fb = regen / 100.0
    dg = width / 100.0
    q.in_gain = 1.0 / (1.0 + dg)
    q.delay_gain = dg / (1.0 + dg) * (1.0 - abs(q.fb))
    q.Lb = int((delay + depth) / 1000.0 * sample_rate + 0.5) + 2
    q.P = int(sample_rate / speed)
    q.tmin = int(math.floor(delay / 1000.0 * sample_rate + 0.5))
    q.lfo = wave_table(SINE if modulation == 'sinusoidal' else TRIANGLE, FLOAT, q.P, float(q.tmin), q.Lb - 2.0, 3 * math.pi / 2)
    q.phases = np.array([int(c * q.P * phase / 100.0 + 0.5) for c in range(channels)], dtype=np.int64)
    q.quadratic = interpolation == 'quadratic'
    return q


def _interpolate(d0, d1, d2, fr, quadratic, two=2.0, half=0.5):
    if not quadratic:
        return d0 + (d1 - d0) * fr
    d2 = d2 - d0
    e1 = d1 - d0
    return d0 + ((d2 * half - e1) * fr + (e1 * two - d2 * half)) * fr


def flanger_literal(x, plan, dtype=np.float64):
    """torchaudio's loop over a ring of ``Lb`` samples per (entry, channel): ``(raw, w, delayed)`` in ``dtype``, ``x`` of shape
    ``(…, C, T)`` with ``C == len(plan.phases)``"""
    x = np.asarray(x).astype(dtype)
    C, T = x.shape[-2], x.shape[-1]
    assert C == len(plan.phases)
    flat = x.reshape(-1, C, T)
    E = flat.shape[0]
    buf = np.zeros((E, C, plan.Lb), dtype)
    last = np.zeros((E, C), dtype)
    raw, ws, dls = np.empty_like(flat), np.empty_like(flat), np.empty_like(flat)
    fb, ig, dgain = dtype(plan.fb), dtype(plan.in_gain), dtype(plan.delay_gain)
    pos = lfo_pos = 0
    ch = np.arange(C)
    for i in range(T):
        pos = (pos + plan.Lb - 1) % plan.Lb
        D = plan.lfo[(lfo_pos + plan.phases) % plan.P]
        k = np.floor(D).astype(np.int64)
        fr = (D - k).astype(dtype)
        buf[:, :, pos] = flat[:, :, i] + fb * last
        ws[:, :, i] = buf[:, :, pos]
        d0 = buf[:, ch, (pos + k) % plan.Lb]
        d1 = buf[:, ch, (pos + k + 1) % plan.Lb]
        d2 = buf[:, ch, (pos + k + 2) % plan.Lb] if plan.quadratic else None
        last = _interpolate(d0, d1, d2, fr, plan.quadratic, dtype(2.0), dtype(0.5)).astype(dtype)
        dls[:, :, i] = last
        raw[:, :, i] = flat[:, :, i] * ig + last * dgain
        lfo_pos = (lfo_pos + 1) % plan.P
    return raw.reshape(x.shape), ws.reshape(x.shape), dls.reshape(x.shape)


def _taps(arr, i, k, Lb, ch, count):
    """``arr[..., c, i - k_c - j]`` for j < count, zero before the row — and zero for the tap ``k + 2 == Lb``, the ring's wrap
    onto the sample being written, whose weight is exactly zero (``fr == 0``)"""
    out = []
    for j in range(count):
        at = i - k - j
        ok = (at >= 0) & (k + j < Lb)
        out.append(np.where(ok, arr[:, ch, np.maximum(at, 0)], 0.0))
    return out


def flanger_blocked(x, plan, W):
    """The form the feedback kernel runs, in float64: blocks of ``W`` slots; for every slot ``i`` of a block first
    ``delayed[i-1]`` — from ``w`` BEFORE the block only, asserted — then the block's ``w[i] = x[i] + fb delayed[i-1]``.
    Returns ``raw``."""
    x64 = _np64(x)
    C, T = x64.shape[-2], x64.shape[-1]
    flat = x64.reshape(-1, C, T)
    w = np.full_like(flat, np.nan)                       # (a read of a slot not yet computed would poison the result)
    dl = np.zeros_like(flat)
    ch = np.arange(C)
    w[:, :, 0] = flat[:, :, 0]
    s = 1
    while s <= T:
        block = range(s, min(s + W, T + 1))
        for i in block:
            D = plan.lfo[(i - 1 + plan.phases) % plan.P]
            k = np.floor(D).astype(np.int64)
            fr = (D - k).astype(np.float64)
            count = 3 if plan.quadratic else 2
            for j in range(count):
                at = i - 1 - k - j
                assert ((at < s) | (k + j >= plan.Lb)).all(), 'slot %d of the block at %d reads w[%s]' % (i, s, at)
            taps = _taps(w, i - 1, k, plan.Lb, ch, count)
            dl[:, :, i - 1] = _interpolate(taps[0], taps[1], taps[2] if plan.quadratic else None, fr, plan.quadratic)
        for i in block:
            if i < T:
                w[:, :, i] = flat[:, :, i] + plan.fb * dl[:, :, i - 1]
        s += W
    raw = flat * plan.in_gain + dl * plan.delay_gain
    return raw.reshape(x64.shape)


def flanger(x, plan):
    """``(ref, bound, mass)``: float64, clipped to [-1, 1]"""
    x64 = _np64(x)
    raw, w, dl = flanger_literal(x64, plan)
    C, T = x64.shape[-2], x64.shape[-1]
    aw = np.abs(w).reshape(-1, C, T)
    ax = np.abs(x64).reshape(-1, C, T)
    ch = np.arange(C)
    Ew, Edl, Mdl = np.zeros_like(aw), np.zeros_like(aw), np.zeros_like(aw)
    afb = abs(plan.fb)
    count = 3 if plan.quadratic else 2
    for i in range(T):
        D = plan.lfo[(i + plan.phases) % plan.P]
        k = np.floor(D).astype(np.int64)
        fr = (D - k).astype(np.float64)
        Ew[:, :, i] = EPS_ARITH * (ax[:, :, i] + (afb * Mdl[:, :, i - 1] if i else 0.0)) + (afb * Edl[:, :, i - 1] if i else 0.0)
        m = _taps(aw, i, k, plan.Lb, ch, count)
        e = _taps(Ew, i, k, plan.Lb, ch, count)
        if plan.quadratic:
            Mdl[:, :, i] = 5.0 * m[0] + 3.0 * m[1] + m[2]
            wt = (np.abs(1.0 - 1.5 * fr + 0.5 * fr * fr), np.abs(2.0 * fr - fr * fr), np.abs(0.5 * fr * fr - 0.5 * fr))
        else:
            Mdl[:, :, i] = 2.0 * m[0] + m[1]
            wt = (np.abs(1.0 - fr), np.abs(fr))
        Edl[:, :, i] = EPS_ARITH * Mdl[:, :, i] + sum(wj * ej for wj, ej in zip(wt, e))
    Edl, Mdl = Edl.reshape(x64.shape), Mdl.reshape(x64.shape)
    static = plan.in_gain * np.abs(x64) + plan.delay_gain * Mdl + np.abs(raw)
    bound = EPS32 * np.abs(raw) + plan.delay_gain * Edl + EPS_ARITH * static + TINY
    mass = static + plan.delay_gain * Edl / EPS_ARITH
    return np.clip(raw, -1.0, 1.0), bound, mass


def dev(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to('cuda')
