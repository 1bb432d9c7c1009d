"""Shared by tests/test_pitch_cpu.py and tests/test_pitch_gpu.py (a plain module: no tests in here): ``detect_pitch_frequency`` restated
literally from torchaudio 2.x with its loop over the lags, the signals and case tables of the tests, and the rule that says which
frames a float32 kernel has to decide exactly as the float64 restatement does.

The definition
--------------
``L = ceil(rate / freq_low)``, ``F = ceil(rate frame_time)``, ``N = ceil(time / F)``, the row continued by zeros to ``L + N F``;
``nccf[t, c] = (s1 . s2) / (1e-9 + |s1|)^2 / (1e-9 + |s2|)^2`` for lag ``c + 1``; the frame's column is the first arg-max over
``[lag_min, L // 2)`` if its value exceeds 0.99 of the maximum over ``[lag_min, L)`` and that range's first arg-max otherwise; its lag
is the column + 1; the lags get ``(win_length - 1) // 2`` copies of the first in front, the lower median over ``win_length`` of them
is taken and ``float32(rate) / float32(lag)`` comes out.

The decision-stability rule
---------------------------
The kernel (csrc/pitch.hip) forms ``num = s1 . s2`` as a float32 sum of ``F`` float32 products in some fixed order, takes ``|s2|^2``
from a float64 prefix of squares rounded to float32, and compares ``num / (1e-9 + sqrt(|s2|^2))^2`` between the lags of a frame
(the factor of ``s1`` is common to them).  With ``u = 2^-24``:

* a float32 dot product of ``F`` terms, in any order and with or without fused multiply-adds, is within ``gamma_F sum |x_i y_i|`` of the
  exact one, ``gamma_F = F u / (1 - F u)`` (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1), and ``sum |x_i y_i| <=
  |s1| |s2|`` (Cauchy-Schwarz).  Divided by the two denominators that is ``gamma_F |s1| |s2| / ((1e-9 + |s1|)^2 (1e-9 + |s2|)^2)`` of
  the value: the issue's ``c F 2^-24 / (|s1| |s2|)`` with ``c = 1 / (1 - F u)``, exact where an energy is 0;
* the denominator costs 7 roundings at most on the value (the energy to float32: 1; its root halves that and adds 1; the sum with
  1e-9: 1; the square doubles and adds 1; the division: 1), the product with the float32 0.99 one more: ``8 u |value|``;
* the difference of two float64 prefix values over a span of at most ``n`` samples of the row is within ``2 n 2^-53`` of the row's
  whole energy: ``2 n 2^-53 E_row / |s2|^2`` of the value (it matters only where a frame is 2^-25 of its row).

``delta[t, c]`` is the sum of the three.  A frame is STABLE when, in float64, the maximum of each range stays the maximum after every
column moved by its ``delta`` (``v[m] - delta[m] > v[c] + delta[c]`` for all other ``c`` of the range) and ``|v[ch] - 0.99 v[cb]| >
delta[ch] + 0.99 delta[cb]``: then every evaluation within the bound takes the same lag, and the kernel has to.  An all-zero frame
has every value 0 and takes ``lag_min + 1`` by the first-index rule.  Every other frame is UNSTABLE; what a kernel gives there must
still be a near-maximum: a lag of the searched range whose float64 value is within twice the bounds of ``v[cb]``, or — below ``half`` —
of ``v[ch]``.  No frame goes unchecked, and at most ``UNSTABLE_CAP`` of a case's non-silent frames may be unstable (asserted for the
restatement alone in tests/test_pitch_cpu.py).
"""
import math
from collections import namedtuple

import torch

U = 2.0 ** -24
UNSTABLE_CAP = 0.10
MAX_WIN = 64                              # the longest median window the second launch takes (csrc/pitch.hip: PT_MAX_WIN)
LDS_PER_CU, LDS_PLAN = 160 * 1024, 64 * 1024

Geo = namedtuple('Geo', 'F L lag_min half N pad n_out')


def ceil_div(a, b):
    return -(-a // b)


def geometry(time, rate, frame_time=1e-2, win_length=30, freq_low=85, freq_high=3400):
    F = int(math.ceil(rate * frame_time))
    L = int(math.ceil(rate / freq_low))
    lag_min = int(math.ceil(rate / freq_high))
    N = ceil_div(time, F)
    pad = (win_length - 1) // 2
    return Geo(F, L, lag_min, L // 2, N, pad, N + pad - win_length + 1)


# ----------------------------------------------------------------------------- the literal restatement
def nccf_of(x, geo):
    """``(rows, time)`` → ``(rows, N, L)`` in the dtype of ``x``: the loop over the lags"""
    x = torch.nn.functional.pad(x, (0, geo.L + geo.N * geo.F - x.shape[-1]))
    out = []
    for lag in range(1, geo.L + 1):
        s1 = x[..., :-lag].unfold(-1, geo.F, geo.F)[..., :geo.N, :]
        s2 = x[..., lag:].unfold(-1, geo.F, geo.F)[..., :geo.N, :]
        frames = ((s1 * s2).sum(-1) / (1e-9 + torch.linalg.vector_norm(s1, ord=2, dim=-1)).pow(2)
                  / (1e-9 + torch.linalg.vector_norm(s2, ord=2, dim=-1)).pow(2))
        out.append(frames.unsqueeze(-1))
    return torch.cat(out, -1)


def lags_of(nccf, geo):
    """``(rows, N, L)`` → int64 ``(rows, N)`` lags (CPU torch's ``max`` returns the first index on ties)"""
    best = torch.max(nccf[..., geo.lag_min:], -1)
    low = torch.max(nccf[..., geo.lag_min:geo.half], -1)
    mask = low[0] > 0.99 * best[0]
    return mask * low[1] + ~mask * best[1] + geo.lag_min + 1


def smooth(lags, win_length, rate):
    """integer ``(rows, N)`` → float32 ``(rows, n_out)``: front replication, ``torch.median`` (the lower one), one float32 division"""
    pad = (win_length - 1) // 2
    lags = lags.to(torch.int64)
    if pad:
        lags = torch.cat([lags[..., :1]] * pad + [lags], -1)
    med = torch.median(lags.unfold(-1, win_length, 1), -1)[0]
    return torch.tensor(float(rate), dtype=torch.float32, device=lags.device) / med.to(torch.float32)


def restatement(x, rate, frame_time=1e-2, win_length=30, freq_low=85, freq_high=3400):
    """``(…, time)`` → float32 ``(…, n_out)``, the NCCF in the dtype of ``x``"""
    geo = geometry(x.shape[-1], rate, frame_time, win_length, freq_low, freq_high)
    rows = x.reshape(-1, x.shape[-1])
    return smooth(lags_of(nccf_of(rows, geo), geo), win_length, rate).reshape(tuple(x.shape[:-1]) + (geo.n_out,))


# ----------------------------------------------------------------------------- the stability rule
Verdict = namedtuple('Verdict', 'geo v delta lags stable silent unstable_share')


def deltas(x64, v, geo):
    """``(rows, N, L)`` float64: how far a float32 evaluation of column ``c`` of frame ``t`` may lie from ``v`` (module docstring)"""
    rows, time = x64.shape
    xp = torch.nn.functional.pad(x64, (0, geo.L + geo.N * geo.F - time))
    sq = torch.cat([torch.zeros(rows, 1, dtype=torch.float64), torch.cumsum(xp * xp, -1)], -1)
    starts = torch.arange(geo.N) * geo.F
    e1 = sq[:, starts + geo.F] - sq[:, starts]                                          # (rows, N)
    at = starts.unsqueeze(-1) + torch.arange(1, geo.L + 1)                              # (N, L): the first sample of s2
    e2 = sq[:, at + geo.F] - sq[:, at]                                                  # (rows, N, L)
    n1, n2 = e1.clamp_min(0).sqrt().unsqueeze(-1), e2.clamp_min(0).sqrt()
    gamma = geo.F * U / (1.0 - geo.F * U)
    dot = gamma * n1 * n2 / ((1e-9 + n1) ** 2 * (1e-9 + n2) ** 2)
    span = 32 * geo.F + geo.L                                                            # the longest span of one prefix
    prefix = 2.0 * span * 2.0 ** -53 * sq[:, -1].reshape(rows, 1, 1) / e2.clamp_min(1e-300)
    return dot + (8.0 * U + torch.where(e2 > 0, prefix, torch.zeros_like(prefix))) * v.abs()


def judge(x, rate, frame_time=1e-2, freq_low=85, freq_high=3400):
    """The float64 restatement of ``x`` ``(rows, time)`` (float32 samples, widened) and the verdict on every frame: ``lags`` int64
    ``(rows, N)``, ``stable`` and ``silent`` bool ``(rows, N)``"""
    x64 = x.detach().cpu().to(torch.float64)
    geo = geometry(x64.shape[-1], rate, frame_time, 1, freq_low, freq_high)
    v = nccf_of(x64, geo)
    delta = deltas(x64, v, geo)
    lags = lags_of(v, geo)
    xp = torch.nn.functional.pad(x64, (0, geo.N * geo.F - x64.shape[-1]))
    silent = (xp.reshape(x64.shape[0], geo.N, geo.F) == 0).all(-1)
    ok = torch.ones_like(silent)
    peak = {}
    for name, hi in (('b', geo.L), ('h', geo.half)):
        vv, dd = v[..., geo.lag_min:hi], delta[..., geo.lag_min:hi]
        m = vv.argmax(-1, keepdim=True)
        floor = vv.gather(-1, m) - dd.gather(-1, m)
        others = (vv + dd).scatter(-1, m, -math.inf)
        ok &= (floor > others.amax(-1, keepdim=True)).squeeze(-1) if hi - geo.lag_min > 1 else True
        peak[name] = (vv.gather(-1, m).squeeze(-1), dd.gather(-1, m).squeeze(-1))
    (vb, db), (vh, dh) = peak['b'], peak['h']
    ok &= (vh - 0.99 * vb).abs() > dh + 0.99 * db
    stable = ok & ~silent
    share = float((~stable & ~silent).sum()) / max(1, int((~silent).sum()))
    return Verdict(geo, v, delta, lags, stable, silent, share)


def assert_lags(got, verdict, what, frames=None):
    """``got``: integer ``(rows, N)`` lags of a kernel for the signal of ``verdict``.  Stable frames exactly, silent frames ``lag_min +
    1``, every other frame a near-maximum.  ``frames``: a bool mask of the frames to hold (default: all).  Returns the number of
    frames that differ from the restatement (all of them unstable)."""
    geo, v, delta = verdict.geo, verdict.v, verdict.delta
    got = got.detach().cpu().to(torch.int64)
    assert tuple(got.shape) == tuple(verdict.lags.shape), '%s: lags of shape %r, expected %r' % (what, tuple(got.shape), tuple(verdict.lags.shape))
    held = torch.ones_like(verdict.silent) if frames is None else frames
    in_range = (got >= geo.lag_min + 1) & (got <= geo.L)
    assert bool(in_range[held].all()), '%s: lags outside [%d, %d]: %r' % (what, geo.lag_min + 1, geo.L, got[held & ~in_range][:8])
    wrong = held & verdict.stable & (got != verdict.lags)
    assert not bool(wrong.any()), '%s: %d stable frames differ, first (row, frame) %r: got %r, want %r' % (
        what, int(wrong.sum()), wrong.nonzero()[0].tolist(), got[wrong][:4].tolist(), verdict.lags[wrong][:4].tolist())
    quiet = held & verdict.silent & (got != geo.lag_min + 1)
    assert not bool(quiet.any()), '%s: %d all-zero frames without lag_min + 1 = %d' % (what, int(quiet.sum()), geo.lag_min + 1)
    rest = held & ~verdict.stable & ~verdict.silent
    col = (got - 1).clamp(0, geo.L - 1).unsqueeze(-1)
    vg, dg = v.gather(-1, col).squeeze(-1), delta.gather(-1, col).squeeze(-1)
    near = torch.zeros_like(rest)
    for hi in (geo.L, geo.half):
        vv = v[..., geo.lag_min:hi]
        m = vv.argmax(-1, keepdim=True)
        top, dt = vv.gather(-1, m).squeeze(-1), delta[..., geo.lag_min:hi].gather(-1, m).squeeze(-1)
        near |= (got - 1 < hi) & (vg >= top - 2.0 * (dg + dt))
    far = rest & ~near
    assert not bool(far.any()), '%s: %d unstable frames whose lag is no near-maximum, first (row, frame) %r' % (
        what, int(far.sum()), far.nonzero()[0].tolist())
    return int((held & (got != verdict.lags)).sum())


# ----------------------------------------------------------------------------- signals and case tables
#: rate -> (F, L) at the default arguments
RATES = {8000: (80, 95), 16000: (160, 189), 44100: (441, 519), 48000: (480, 565)}

#: (rate, frame_time, freq_low, freq_high): variants that move lag_min, half and F; the second one's F = 150 is no multiple of 4
VARIANTS = ((16000, 1e-2, 60, 2000), (8000, 0.01875, 85, 1000), (16000, 0.0075, 120, 3400), (8000, 0.0123, 50, 400))


def glide(rate, rows=6, seed=5, seconds=0.62, extra=37):
    """float32 ``(rows, int(seconds rate) + extra)``: four harmonics of a fundamental that glides between 95 and 440 Hz (each row its
    own end points), 1 % white noise, a leading ninth of exact zeros.  The length is no multiple of ``F``."""
    gen = torch.Generator().manual_seed(seed * 1000003 + rate)
    time = int(seconds * rate) + extra
    t = torch.arange(time, dtype=torch.float64) / rate
    out = torch.zeros(rows, time, dtype=torch.float64)
    for r in range(rows):
        f0, f1 = (95.0 + 345.0 * torch.rand(2, generator=gen, dtype=torch.float64)).tolist()
        if r == 0:
            f0, f1 = 95.0, 440.0
        freq = f0 + (f1 - f0) * t / t[-1]
        phase = 2.0 * math.pi * torch.cumsum(freq, 0) / rate
        amps = 0.1 + 0.4 * torch.rand(4, generator=gen, dtype=torch.float64)
        for k in range(4):
            out[r] += amps[k] * torch.sin((k + 1) * phase + 2.0 * math.pi * float(torch.rand(1, generator=gen, dtype=torch.float64)))
        out[r] *= 0.5 / out[r].abs().max()
        out[r] += 0.01 * 0.5 * torch.randn(time, generator=gen, dtype=torch.float64)
    out[:, :time // 9] = 0.0
    return out.to(torch.float32)


def tone(rate, freq, time, harmonics=3):
    """a harmonic tone whose period is a whole number of samples: every frame's lag is ``rate / freq``"""
    t = torch.arange(time, dtype=torch.float64) / rate
    return sum(torch.sin(2.0 * math.pi * (k + 1) * freq * t) / (k + 1) for k in range(harmonics)).to(torch.float32)


def lag_table(rows, n, lo, hi, seed):
    """int32 ``(rows, n)`` lags in ``[lo, hi]``: row 0 random, row 1 in constant runs, row 2 constant, the others random walks"""
    gen = torch.Generator().manual_seed(seed)
    out = torch.randint(lo, hi + 1, (rows, n), generator=gen, dtype=torch.int64)
    if rows > 1:
        out[1] = out[1][torch.arange(n) // 7 * 7 % n]
    if rows > 2:
        out[2] = out[2, 0]
    for r in range(3, rows):
        out[r] = (lo + torch.cumsum(torch.randint(-2, 3, (n,), generator=gen), 0).abs() % (hi - lo + 1))
    return out.to(torch.int32)


# ----------------------------------------------------------------------------- the first launch's plan and grid, restated
def plan(n_frames, F, L):
    """``(G, NH, LDS bytes)`` of ``pitch_plan`` (csrc/pitch.hip): tasks of two blocks of four lags, ``G`` frames a workgroup with the
    best use of its 256 lanes that fits ``LDS_PLAN``; None where one frame does not fit"""
    nh = (L // 4 + 1 + 1) // 2
    best, best_use, best_bytes = 0, 0.0, 0
    for g in range(1, min(32, n_frames) + 1):
        tasks = g * nh
        nbytes = 8 * (g * F + L + 1) + 4 * ((g * F + 8 * nh + 8 + 3) // 4 * 4) + 16 * tasks + 32
        if tasks > 1024 or nbytes > LDS_PLAN:
            break
        use = tasks / (ceil_div(tasks, 256) * 256.0)
        if use > best_use + 1e-9:
            best, best_use, best_bytes = g, use, nbytes
    return (best, nh, best_bytes) if best else None


def lags_grid(cus, rows, n_frames, F, L):
    """``(units, grid)`` of the first launch: a unit is a group of ``G`` frames of one row, the grid ``cus`` times the workgroups a
    CU's LDS holds, 8 at the most"""
    g, _, nbytes = plan(n_frames, F, L)
    return rows * ceil_div(n_frames, g), cus * min(8, LDS_PER_CU // nbytes)
