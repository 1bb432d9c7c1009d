"""Shared by tests/test_griffinlim_cpu.py and tests/test_griffinlim_gpu.py: the definition of ``griffinlim`` in torch CPU operators,
the one-step formula in float64 with its per-element bound, the bounds of the prepare launch, the two error measures and the inputs.

Definition (torchaudio's ``functional.griffinlim``; ``m = momentum / (1 + momentum)``)::

    S = specgram.reshape(-1, freq, time) ** (1 / power);  A = angles0 or ones (1 + 0j);  Rprev = 0
    n_iter times:  y = istft(S * A);  R = stft(y);  A = R - m * Rprev (skipped when m == 0);  A = A / (abs(A) + 1e-16);  Rprev = R
    y = istft(S * A)

Float32 and float64 runs of this drift apart as the iterations go (a bin near zero has an arbitrary phase after the division), so
the 32-iteration waveform is held to what the float32 CPU run itself reaches against the float64 one (test 4 of the GPU file),
and what is held tightly is one step and the driver's bookkeeping.

One step, ``X = M A / (|A| + 1e-16)`` with ``A = R - m Rprev`` — ``update_bound``, from the operations of ``gl_project``
(csrc/griffinlim_project.hpp), ``u = 2^-24`` per rounded operation, no library call:

  * ``a_c = fmaf(-m, p_c, r_c)``: ONE rounding of the exact difference (the product inside an fma is not rounded), so what a
    separate product and difference would lose to cancellation, ``u (|R| + m |Rprev|)``, is ``u |a_c|`` here; for the pair,
    ``|dA| <= u |A|``.  The map ``A -> A / (|A| + e)`` has a derivative of norm at most ``2 / (|A| + e)``: the rounding of A moves
    each component of X by at most ``2 u M |A| / (|A| + e)`` — carried as an absolute term, the same for both components.
  * the scaling by a power of two is exact; ``t = s_im^2`` (u), ``n2 = fmaf(s_re, s_re, t)`` (u): ``n2`` carries 2 u, the root
    halves that and adds u: ``n`` carries 2 u; ``d = n + e'`` adds u: 3 u; ``q_c = s_c / d``: 4 u; ``x_c = M q_c``: 5 u of ``|want_c|``.
  * the smaller component may fall below 2^-126 after the scaling and lose bits there: ``2^-149`` of a quotient, ``M 2^-148`` with
    room; and a floor of ``TINY = K_LIB`` subnormal spacings, as in tests/elementwise_rules.py.

Both terms get the factor ``1 + 2^-10`` for what the first-order count leaves out.  The bound is never fitted to an output.
``m`` and 1e-16 enter the reference as the float32 values the entry point holds.
"""
import math

import numpy as np
import torch

from oracle import signals

import elementwise_rules as ER

U = 2.0 ** -24
TINY = ER.TINY[ER.F32]
LIB = ER.LIB
EPS32 = float(np.float32(1e-16))
SLACK = 1.0 + 2.0 ** -10

#: the geometries of the GPU tests: tag -> (n_fft, hop, win_length, user window, rows, frames, power)
GENERAL = {
    '256/64': (256, 64, 256, False, 3, 40, 2.0),
    '400/160': (400, 160, 400, False, 2, 30, 1.0),
    '512/128 win 400 user': (512, 128, 400, True, 3, 31, 2.0),
    '960/240': (960, 240, 960, False, 2, 20, 0.7),
}
AT_2048 = {
    '2048/512': (2048, 512, 2048, False, 3, 24, 2.0),
    '2048/256': (2048, 256, 2048, False, 2, 57, 2.0),
    '2048/1024': (2048, 1024, 2048, False, 2, 17, 1.0),
}
CASES = dict(GENERAL, **AT_2048)
#: seed offsets of the inputs.  tests/test_griffinlim_cpu.py holds every case's rows to conditions stated on torch's CPU operators
#: alone (float32 within 1e-4 of float64 at n_iter <= 4): the first noise row tried at 2048/1024 holds a bin so close to zero
#: that its phase flips between the two precisions by the fourth step (2.7e-4), the next one does not (1.0e-5)
SEEDS = {'2048/1024': 1}


def momentum_m(momentum):
    return momentum / (1 + momentum)


# ----------------------------------------------------------------------------- inputs
def window_of(case):
    n_fft, hop, wl, user = case[:4]
    w = torch.hann_window(wl, dtype=torch.float32)
    if user:
        gen = torch.Generator().manual_seed(wl + hop)
        w = (w * 0.75 + 0.25 + 0.05 * torch.rand(wl, generator=gen)).float()
    return w


def waves(rows, length, seed):
    """float32 ``(rows, length)``: row 0 a decaying chirp plus noise, the others noise; with three or more rows, row 1 is silent
    and row 2 at gain 2^-12"""
    noise = torch.from_numpy(signals.uniform((rows, length), seed=seed)).double()
    n = torch.arange(length, dtype=torch.float64)
    t = n / length
    chirp = torch.exp(-3.0 * t) * torch.sin(2.0 * math.pi * (0.01 + 0.10 * t) * n)
    x = 0.5 * noise
    x[0] = chirp + 0.05 * noise[0]
    if rows >= 3:
        x[1] = 0.0
        x[2] *= 2.0 ** -12
    return x.float()


def torch_stft(y, n_fft, hop, window):
    return torch.stft(y, n_fft, hop_length=hop, win_length=window.shape[0], window=window, center=True, pad_mode='reflect',
                      normalized=False, onesided=True, return_complex=True)


_inputs = {}


def case_input(tag, seed=0):
    """``(window, specgram (rows, F, T) float32 = |stft|^power of the case's rows)``, computed once"""
    key = (tag, seed)
    if key not in _inputs:
        n_fft, hop, wl, user, rows, frames, power = CASES[tag]
        w = window_of(CASES[tag])
        x = waves(rows, hop * (frames - 1), 900 + seed + SEEDS.get(tag, 0) + n_fft + hop)
        mag = torch_stft(x, n_fft, hop, w).abs()
        spec = mag if power == 1.0 else mag.pow(power)
        assert spec.shape == (rows, n_fft // 2 + 1, frames)
        _inputs[key] = (w, spec.contiguous())
    return _inputs[key]


def seeded_angles(shape, seed, dtype=torch.complex64):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(shape, dtype=dtype, generator=gen)


# ----------------------------------------------------------------------------- the definition
def reference(S, window, n_fft, hop, win_length, power, n_iter, momentum, length, angles0, dtype):
    """the listing above in torch CPU operators in ``dtype`` (float32 or float64) on the values of ``S`` (…, F, T)"""
    cdtype = torch.complex128 if dtype == torch.float64 else torch.complex64
    spec = S.detach().cpu().to(dtype)
    w = window.detach().cpu().to(dtype)
    assert w.shape[0] == win_length
    m = momentum_m(momentum)
    lead = tuple(spec.shape[:-2])
    s = spec.reshape((-1,) + tuple(spec.shape[-2:])).pow(1.0 / power)
    a = torch.ones(s.shape, dtype=cdtype) if angles0 is None else angles0.detach().cpu().to(cdtype).reshape(s.shape)
    prev = torch.zeros((), dtype=cdtype)
    for _ in range(n_iter):
        y = torch.istft(s * a, n_fft, hop_length=hop, win_length=win_length, window=w, length=length)
        r = torch_stft(y, n_fft, hop, w)
        a = r
        if m:
            a = a - prev * m
        a = a / (a.abs() + 1e-16)
        prev = r
    y = torch.istft(s * a, n_fft, hop_length=hop, win_length=win_length, window=w, length=length)
    return y.reshape(lead + tuple(y.shape[-1:]))


# ----------------------------------------------------------------------------- one step
def _c(t):
    """(…, 2) real pairs or a complex tensor -> complex128 on the CPU"""
    t = t.detach().cpu()
    return (t if t.is_complex() else torch.view_as_complex(t.double().contiguous())).to(torch.complex128)


def update_reference(r, rprev, mag, m):
    """``M (R - m Rprev) / (|R - m Rprev| + 1e-16)`` in float64 as ``(…, 2)`` pairs; ``m`` and 1e-16 as the float32 values held"""
    a = _c(r)
    if rprev is not None and m != 0.0:
        a = a - float(np.float32(m)) * _c(rprev)
    x = mag.detach().cpu().double() * a / (a.abs() + EPS32)
    return torch.view_as_real(x)


def update_bound(r, rprev, mag, m):
    """per component of ``update_reference``'s result: see the module docstring"""
    a = _c(r)
    if rprev is not None and m != 0.0:
        a = a - float(np.float32(m)) * _c(rprev)
    mg = mag.detach().cpu().double().abs()
    f = a.abs() / (a.abs() + EPS32)
    want = torch.view_as_real(mg * a / (a.abs() + EPS32)).abs()
    return SLACK * (5.0 * U * want + (2.0 * U * mg * f)[..., None]) + (mg * 2.0 ** -148)[..., None] + TINY


def fractions(got, want, bound):
    got = got.detach().cpu().double()
    frac = (got - want).abs() / bound
    return torch.where(torch.isfinite(got), frac, torch.full_like(frac, math.inf))


# ----------------------------------------------------------------------------- the prepare launch
def root_param(power):
    """the exponent the entry point holds: float32(1 / float32(power))"""
    return float(np.float32(1.0 / float(np.float32(power))))


def prepare_reference(spec, angles0, power):
    """``(M (rows, T, F), X0 (rows, T, F, 2))`` float64 of ``spec`` (rows, F, T)"""
    s = spec.detach().cpu().double().transpose(1, 2)
    mag = s if power == 1.0 else (s.sqrt() if power == 2.0 else s.pow(root_param(power)))
    a = torch.ones((), dtype=torch.complex128) if angles0 is None else _c(angles0).transpose(1, 2)
    return mag.contiguous(), torch.view_as_real((mag * a).contiguous())


def prepare_bounds(mag64, x064, power, with_angles):
    """M: the bound of its one operation (none: exact; ``sqrtf``: u; ``powf``: LIB u, the exponent being the value held); X0 one
    rounding more where it is a product, the same where it is a copy; the TINY floor"""
    rel = 0.0 if power == 1.0 else (U if power == 2.0 else LIB * U)
    return rel * mag64.abs() + TINY, (rel + (U if with_angles else 0.0)) * SLACK * x064.abs() + TINY


# ----------------------------------------------------------------------------- error measures
def _norms(z):
    return z.abs().pow(2).sum((-2, -1)).sqrt()


def linear_magnitude(spec, power):
    return spec.detach().cpu().double().pow(1.0 / power)


def E(y, y_ref, s_lin, n_fft, hop, window):
    """per row ``|| STFT64(y - y_ref) ||_F / || S ||_F``, S the linear magnitude (rows, F, T); 0 for an exactly matching silent row.
    By the reverse triangle inequality ``|conv(y) - conv(y_ref)| <= E``."""
    d = y.detach().cpu().double() - y_ref.detach().cpu().double()
    num = _norms(torch_stft(d.reshape(-1, d.shape[-1]), n_fft, hop, window.detach().cpu().double()))
    den = _norms(s_lin.reshape((-1,) + tuple(s_lin.shape[-2:])))
    return torch.where((num == 0) & (den == 0), torch.zeros_like(num), num / den)


def conv(y, s_lin, n_fft, hop, window):
    """per row ``|| |STFT64(y)| - S ||_F / || S ||_F``: the spectral convergence; 0 for a silent row reproduced exactly"""
    y = y.detach().cpu().double()
    s = s_lin.reshape((-1,) + tuple(s_lin.shape[-2:]))
    num = _norms(torch_stft(y.reshape(-1, y.shape[-1]), n_fft, hop, window.detach().cpu().double()).abs() - s)
    den = _norms(s)
    return torch.where((num == 0) & (den == 0), torch.zeros_like(num), num / den)


def row_max_rel(y, y_ref):
    """per row ``max |y - y_ref| / max |y_ref|``; 0 for an exactly matching silent row"""
    y, r = y.detach().cpu().double(), y_ref.detach().cpu().double()
    y, r = y.reshape(-1, y.shape[-1]), r.reshape(-1, r.shape[-1])
    num, den = (y - r).abs().amax(-1), r.abs().amax(-1)
    return torch.where((num == 0) & (den == 0), torch.zeros_like(num), num / den)


# ----------------------------------------------------------------------------- the update's grid
UPDATE_THREADS, UPDATE_BLOCKS_PER_CU = 256, 4


def update_launch(cus, n_bins):
    """``tac_griffinlim_update_f32``: (workgroups an unbounded grid would have, the launcher's cap); a thread owns two bins"""
    return ((n_bins + 1) // 2 + UPDATE_THREADS - 1) // UPDATE_THREADS, UPDATE_BLOCKS_PER_CU * cus
