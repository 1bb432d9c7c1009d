"""References, per-element bounds, input generators and ``assert_*`` helpers of the elementwise kernels and their gradients
(tests/test_elementwise_cpu.py, test_elementwise_gpu.py): ``complex_norm``, ``angle`` / ``magphase``, ``amplitude_to_db``,
``db_to_amplitude`` (csrc/elementwise.hip, the float64 forms in csrc/chain_f64.hip) and the four kernels of csrc/backward.hip.

Reference.  The documented formulas (oracle/torch_ref.py) evaluated one precision up on the SAME inputs: float64 torch operators
for the float32 kernels, gradients by float64 autograd of those formulas; ``numpy.longdouble`` (>= 63 mantissa bits, asserted by
``longdouble_ok``) for the float64 kernels.  Parameters enter the reference as the values the entry points hold: ``power`` and
``amin`` rounded to the kernel's type, ``log10(ref)`` as the value of that type the entry point computes on the host.  The clamp of
``amplitude_to_db`` is decided, as the formula decides it in the kernel's type, on the ROUNDED square ``fl(x * x) >= amin``.

Bounds (derived here from the operations each kernel performs, never fitted to an output).  ``u`` is the unit roundoff of the
kernel's type (2^-24, 2^-53).  A correctly rounded operation (``* + /``, ``sqrt``, an ``fma``) adds ``u`` relative to its result;
a library call (``powf``, ``atan2f``, ``log10f``, ``exp2f`` and their double forms) adds ``K_LIB = 4`` ulps = ``LIB = 8 u`` relative
to its result — a condition set for these kernels (the customary ceiling of a library function that is no fast approximation), not
a measurement; an error already in an argument is carried on by the function's condition number.

  |z|^p        ``s = re^2 + im^2``: 2 u (product and sum; less where the compiler contracts).  ``sqrt`` halves that and adds u:
               ``m`` carries 2 u.  p = 2 returns ``s`` (2 u), p = 1 returns ``m`` (2 u), any other p ``powf(m, p)``:
               ``(2 |p| + LIB) u``.
  atan2        exact inputs, one library call: ``LIB u |want|``.
  to dB        ``sigma = max(fl(x^2), amin)`` carries u, which ``log10`` turns into ``u / ln 10`` absolute; the call itself adds
               ``LIB u |log10 sigma|``, the subtraction ``u |log10 sigma - log10 ref|``, ``log10 ref`` was rounded once on the host
               (``u |log10 ref|``; this also covers a last-bit difference between two hosts' ``log10f``) and the product by 10
               rounds the result:  ``10 (u / ln 10 + LIB u |log10 sigma| + u |log10 sigma - log10 ref| + u |log10 ref|) + u |want|``.
  from dB      float32 (``exp2f(e * c)``, ``e = x / 10 + log10 ref``, ``c = fl(log2(10) / 2)``): the quotient and the sum put
               ``(|x| / 10 + |e|) u`` on ``e``; the rounding of ``c`` and of the product ``2 u |e c|``; ``exp2`` turns an absolute
               error d of its argument into ``ln 2 * d`` relative, and ``ln 2 * c = ln 10 / 2``:
               ``(ln 10 / 2) (|x| / 10 + 3 |e|) u + LIB u``, relative.
               float64 (``sqrt(pow(10, e))``): ``ln 10 (|x| / 10 + |e|) u + LIB u`` after ``pow``, halved by the root, plus u:
               ``(ln 10 / 2) (|x| / 10 + |e|) u + (LIB / 2 + 1) u``.
  d|z|^p       ``z * (f * g)`` with ``f = p |z|^(p-2)`` (``norm_pow_grad``, fft_core.hpp): p = 2: ``f = 2`` exactly; p = 1:
               ``1 / sqrtf(s)``: u (half of s's 2 u) + u + u = 3 u; other p: ``p * powf(sqrtf(s), fl(p - 2))``: the base's 2 u
               times ``|p - 2|``, the exponent's own rounding ``u |p - 2|`` times its condition ``|ln m|``, ``LIB u`` for the
               call and u for the product: ``(2 |p - 2| + |p - 2| |ln m| + LIB + 1) u``.  The scale by the incoming gradient
               and the product with the component add 2 u.  Everything is a product, so the bound is relative per component.
  d atan2      ``f = g / s`` (s: 2 u, the quotient u), times the component (u): 4 u of the phase term B; added to the magnitude
               term A (bound above) by a last rounded operation: ``bound(A) + 4 u |B| + u |A + B|``.
  d to dB      ``g * (c / x)`` where ``fl(x^2) >= amin``: the constant, the quotient, the product: 3 u; an exact 0 elsewhere.
  d from dB    ``g * (k * y)``, y the forward value re-evaluated: the forward bound + 3 u.

Every bound gets a floor of ``K_LIB`` subnormal spacings (``TINY``), so that exact zeros compare and a result in the subnormal
range, where one ulp is the fixed spacing, is still held to K_LIB ulps.  A value whose reference rounds to infinity may be
infinite; one within its bound of the largest finite number may be either.

Intended deviations from the float32 torch evaluation (``DEVIATIONS``): the edge table's expectation for a row is what the formula
gives in float32 torch on the CPU, forward and autograd, compared by class (NaN, +inf, -inf, zero with its sign, finite) and, where
finite, by the bound above.  Each entry of ``DEVIATIONS`` names the rows where the kernels are meant to differ, with the reason.
"""
import math

import numpy as np
import torch

K_LIB = 4
LIB = 2.0 * K_LIB                      # a library call, in units of u
LN10 = math.log(10.0)
UNIT = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
TINY = {np.dtype(np.float32): K_LIB * 2.0 ** -149, np.dtype(np.float64): K_LIB * 2.0 ** -1074}
F32, F64 = np.dtype(np.float32), np.dtype(np.float64)

POWERS = (1.0, 2.0, 0.5, 0.7, 3.0)
DB_CASES = ((1.0, 1e-7), (2.0, 1e-5), (0.03, 1e-10), (1.0, 1e-30))
#: a fifth case whose ``amin`` IS the rounded square of a float32, so that ``fl(x^2) == amin`` occurs whatever the four above allow
DB_EQUALITY_CASE = (1.0, float(np.float32(np.float32(3.1622776e-3) * np.float32(3.1622776e-3))))
UNDB_REFS = (1.0, 3.5, 1e-3)
PAIR_BINADES = tuple(range(-50, 61))
DB_BINADES = tuple(range(-40, 41))
PAIRS_PER_BINADE, DB_PER_BINADE = 96, 128
N_PAIRS = len(PAIR_BINADES) * PAIRS_PER_BINADE           # 10656 = 3 * 37 * 96
N_DB = len(DB_BINADES) * DB_PER_BINADE                   # 10368 = 3 * 27 * 128
PAIR_SHAPE, DB_SHAPE = (3, 37, 96), (3, 27, 128)
AXIS_SHARE = LOPSIDED_SHARE = 1.0 / 8.0

DEVIATIONS = {
    'gradient zero sign':
        'a gradient that is zero is compared without its sign: -0 and +0 are the same step, and the sign torch returns there '
        'comes from which mask or product made the zero (0 * 2x, a masked_fill), not from the function',
    'norm gradient, power 2':
        '|z|^2 = re^2 + im^2 is a polynomial and its gradient 2 z g needs no norm: the kernel returns that product for every z, '
        'where torch\'s norm-then-pow chain forms inf * 0 once the square overflows or a component is infinite',
    'norm gradient where s == 0':
        'where fl(re^2 + im^2) is 0 (z = 0, or |z| below 2^-75) the forward value is the constant 0 and so is its gradient; torch '
        'returns that 0 for powers 1, 2 and 3 and forms 0 * inf = NaN for the others',
    'norm gradient where s overflows, power above 2':
        'with fl(re^2 + im^2) = inf the kernel evaluates p |z|^(p-2) z g with |z| = inf, which is the rounding of the true '
        'gradient (it is beyond float32 there) component by component; torch\'s chain forms inf * 0',
    'phase gradient where s overflows':
        'with fl(re^2 + im^2) = inf and finite components torch returns g z / inf = 0, as the kernel does, unless its own product '
        'g * component overflows first and makes inf * 0; the kernel divides g by s before it multiplies, so it returns the 0 there too',
    'dB gradient at infinity':
        '20 / (ln 10 x) tends to 0 as x tends to +-inf and the kernel returns that limit; torch multiplies d log / d(x^2) = 0 by '
        'd(x^2) / dx = inf',
    'dB gradient where x^2 overflows':
        'the closed form 20 g / (ln 10 x) never squares x, so it stays the correctly rounded gradient for |x| > 1.8e19 where '
        'torch, whose x^2 is inf, returns 0',
    'dB gradient where x^2 underflows and amin is 0':
        'likewise for |x| < 2^-75 when nothing floors the square: the closed form is finite and right, torch divides by fl(x^2) = 0',
    'dB gradient at x == 0 with amin 0':
        '20 g / (ln 10 x) at x = +-0 is the one-sided limit, an infinity with the signs of x and g; torch forms inf * 0',
    'from dB beyond 10^+-38':
        'the kernel raises 2 to (x / 10 + log10 ref) log2(10) / 2 and never forms 10^y before the root, so value and gradient stay '
        'finite and correctly rounded for |x / 10 + log10 ref| up to 76 (45 on the subnormal side) where torch\'s 10^y is already '
        'inf or 0; there both are held to the float64 value rounded to float32',
}


def longdouble_ok():
    return np.finfo(np.longdouble).nmant >= 63


def _hi(dtype):
    return np.float64 if np.dtype(dtype) == F32 else np.longdouble


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def host_log10(ref, dtype=F32):
    """``log10(ref)`` as the entry point computes it: in the kernel's type, on the host"""
    return float(np.log10(np.dtype(dtype).type(ref)))


def as_param(v, dtype=F32):
    return float(np.dtype(dtype).type(v))


# ----------------------------------------------------------------------------- generators (deterministic)
def _torch_dtype(dtype):
    return torch.float32 if np.dtype(dtype) == F32 else torch.float64


def _mantissas(n, gen, dtype):
    m = 1.0 + torch.rand(n, generator=gen, dtype=torch.float64)
    return m.to(_torch_dtype(dtype)).double().clamp(max=2.0 - 2.0 ** -23)


def pair_sweep(dtype=F32, seed=0):
    """``(N_PAIRS, 2)``: magnitudes ``m 2^k`` for every k of PAIR_BINADES (element i has k = PAIR_BINADES[i % 111]), uniform
    phases; every eighth pair (i % 8 == 0) on an axis (+re, -re, +im, -im in turn), every eighth (i % 8 == 1) with components
    exactly 2^30 apart (either way round, all four sign pairs).  8 and 111 are coprime: every binade gets every kind."""
    g = torch.Generator().manual_seed(1000 + seed)
    i = torch.arange(N_PAIRS)
    mag = torch.ldexp(_mantissas(N_PAIRS, g, dtype), (i % len(PAIR_BINADES)) + PAIR_BINADES[0])
    theta = 2.0 * math.pi * torch.rand(N_PAIRS, generator=g, dtype=torch.float64)
    re, im = mag * torch.cos(theta), mag * torch.sin(theta)
    kind, turn = i % 8, (i // 8) % 4
    zero = torch.zeros_like(mag)
    axis = kind == 0
    re = torch.where(axis, torch.where(turn == 0, mag, torch.where(turn == 1, -mag, zero)), re)
    im = torch.where(axis, torch.where(turn == 2, mag, torch.where(turn == 3, -mag, zero)), im)
    lop = kind == 1
    sa = torch.where((i // 16) % 2 == 0, 1.0, -1.0).double()
    sb = torch.where((i // 32) % 2 == 0, 1.0, -1.0).double()
    big, small = sa * mag, sb * mag * 2.0 ** -30
    re = torch.where(lop, torch.where(turn % 2 == 0, big, small), re)
    im = torch.where(lop, torch.where(turn % 2 == 0, small, big), im)
    return torch.stack([re, im], dim=-1).to(_torch_dtype(dtype))


def clamp_neighbours(amin, dtype=F32):
    """the 18 values within +-4 spacings of ``sqrt(amin)`` (both signs), in the kernel's type"""
    ty = np.dtype(dtype).type
    r = np.sqrt(ty(amin))
    vals = [r]
    lo = hi = r
    for _ in range(4):
        lo, hi = np.nextafter(lo, ty(0)), np.nextafter(hi, ty(np.inf))
        vals += [lo, hi]
    vals = np.array(sorted(vals), dtype=dtype)
    return np.concatenate([vals, -vals])


def clamp_sides(x, amin):
    """``(below, equal, above)`` counts of ``fl(x^2)`` against ``amin`` in x's own type"""
    x = _np(x)
    sq = x * x
    a = x.dtype.type(amin)
    return int((sq < a).sum()), int((sq == a).sum()), int((sq > a).sum())


def db_sweep(amin, dtype=F32, seed=0):
    """``(N_DB + 18,)``: ``+-m 2^k`` for every k of DB_BINADES, then ``clamp_neighbours(amin)``"""
    g = torch.Generator().manual_seed(2000 + seed)
    i = torch.arange(N_DB)
    x = torch.ldexp(_mantissas(N_DB, g, dtype), (i % len(DB_BINADES)) + DB_BINADES[0])
    x = torch.where(torch.rand(N_DB, generator=g) < 0.5, x, -x).to(_torch_dtype(dtype))
    return torch.cat([x, torch.from_numpy(clamp_neighbours(amin, dtype))])


def undb_sweep(dtype=F32, seed=0):
    """``(N_DB,)`` uniform in +-300 dB"""
    g = torch.Generator().manual_seed(3000 + seed)
    return ((torch.rand(N_DB, generator=g, dtype=torch.float64) * 2.0 - 1.0) * 300.0).to(_torch_dtype(dtype))


def grad_weights(n, seed=0):
    """an incoming gradient of both signs, magnitudes in [0.5, 2): float32 ``(n,)``"""
    g = torch.Generator().manual_seed(4000 + seed)
    w = 0.5 + 1.5 * torch.rand(n, generator=g)
    return torch.where(torch.rand(n, generator=g) < 0.5, w, -w)


def binades(mag):
    """the set of ``floor(log2 |v|)`` over the non-zero values"""
    mag = _np(mag).astype(np.float64)
    return set(np.floor(np.log2(np.abs(mag[mag != 0]))).astype(int).tolist())


# ----------------------------------------------------------------------------- edge tables (float32)
_INF, _NAN = float('inf'), float('nan')
_SPECIAL = (0.0, -0.0, _INF, -_INF, _NAN)


def pair_edges():
    """``(rows, 2)`` float32: +-0, +-inf, NaN in either slot against each other and against finite values; |z| above 1.9e19
    (``s`` overflows), below 2^-75 (``s`` is 0), subnormal components"""
    rows = [(a, b) for a in _SPECIAL for b in _SPECIAL]
    for a in _SPECIAL:
        for b in (1.0, -1.5):
            rows += [(a, b), (b, a)]
    rows += [(3e19, 1e19), (-2e19, 2e19), (2e19, -3e19), (3e38, 1e38), (-1e30, -3e19)]
    rows += [(2.0 ** -76, 2.0 ** -77), (-2.0 ** -80, 2.0 ** -90), (2.0 ** -100, -2.0 ** -76)]
    rows += [(1e-40, 1e-41), (-1e-42, 1e-39), (1e-40, 1.0), (1.0, -1e-40), (1e-40, 0.0), (-0.0, 1e-45)]
    return torch.tensor(rows, dtype=torch.float32)


DB_EDGE_X = (0.0, -0.0, 1e-40, -1e-42, _INF, -_INF, _NAN, 3e19, -2e19, 1e-30, -1e-30, 1.0, -2.0, 1e-4)
DB_EDGE_AMIN = (1e-7, 1e-42, 0.0)
DB_EDGE_REF = (1.0, 2.0)
UNDB_EDGE_X = (400.0, -400.0, 800.0, -800.0, _INF, -_INF, _NAN, 0.0, -0.0, 1e-40, 25.0, -371.5)
UNDB_EDGE_REF = (1.0, 3.5)


# ----------------------------------------------------------------------------- references
def _power(p, dtype=F32):
    return as_param(p, dtype)


def t_norm(z, p):
    """torch, in z's dtype: sqrt(re^2 + im^2) ** p"""
    s = z[..., 0] * z[..., 0] + z[..., 1] * z[..., 1]
    if p == 2.0:
        return s
    return s.sqrt() if p == 1.0 else s.sqrt().pow(p)


def t_angle(z):
    return torch.atan2(z[..., 1], z[..., 0])


def t_passes(x32, amin):
    """where ``fl(x^2) >= amin`` in float32 (NaN: False)"""
    return (x32.double() * x32.double()).float() >= as_param(amin)


def t_to_db(x64, passes, ref, amin):
    sq = x64 * x64
    sigma = torch.where(passes | sq.isnan(), sq, torch.full_like(sq, as_param(amin)))
    return 10.0 * (torch.log10(sigma) - host_log10(ref))


def t_from_db(x64, ref):
    return torch.pow(10.0, x64 / 10.0 + host_log10(ref)).pow(0.5)


def n_forward(op, x, *params):
    """numpy reference of a forward op one precision above x's: 'norm' (p), 'angle', 'to_db' (ref, amin), 'from_db' (ref)"""
    x = _np(x)
    hi = _hi(x.dtype)
    with np.errstate(all='ignore'):
        if op in ('norm', 'angle'):
            re, im = x[..., 0].astype(hi), x[..., 1].astype(hi)
            if op == 'angle':
                return np.arctan2(im, re)
            s = re * re + im * im
            p = _power(params[0], x.dtype)
            return s if p == 2.0 else (np.sqrt(s) if p == 1.0 else np.power(np.sqrt(s), hi(p)))
        xh = x.astype(hi)
        if op == 'to_db':
            ref, amin = params
            a = x.dtype.type(amin)
            sigma = np.where((x * x >= a) | np.isnan(x), xh * xh, hi(a))
            return hi(10) * (np.log10(sigma) - hi(host_log10(ref, x.dtype)))
        if op == 'from_db':
            return np.sqrt(np.power(hi(10), xh / hi(10) + hi(host_log10(params[0], x.dtype))))
    raise ValueError(op)


def forward_bound(op, x, want, *params):
    """the per-element bound of a forward op, in the precision of ``want``"""
    x = _np(x)
    hi, u, tiny = _hi(x.dtype), UNIT[x.dtype], TINY[x.dtype]
    with np.errstate(all='ignore'):
        if op == 'norm':
            p = _power(params[0], x.dtype)
            rel = 2.0 * u if p in (1.0, 2.0) else (2.0 * abs(p) + LIB) * u
            b = rel * np.abs(want)
        elif op == 'angle':
            b = LIB * u * np.abs(want)
        elif op == 'to_db':
            ref, amin = params
            a = x.dtype.type(amin)
            xh = x.astype(hi)
            L = np.log10(np.where(x * x >= a, xh * xh, hi(a)))
            l = hi(host_log10(ref, x.dtype))
            b = 10.0 * (u / LN10 + LIB * u * np.abs(L) + u * np.abs(L - l) + u * abs(l)) + u * np.abs(want)
        elif op == 'from_db':
            xh = x.astype(hi)
            e = xh / 10 + hi(host_log10(params[0], x.dtype))
            if x.dtype == F32:
                rel = (LN10 / 2.0) * (np.abs(xh) / 10 + 3 * np.abs(e)) * u + LIB * u
            else:
                rel = (LN10 / 2.0) * (np.abs(xh) / 10 + np.abs(e)) * u + (LIB / 2.0 + 1.0) * u
            b = rel * np.abs(want)
        else:
            raise ValueError(op)
    return np.where(np.isfinite(b), b, 0).astype(hi) + hi(tiny)


_cache = {}


def cached(key, build):
    """a reference computed once per ``key`` and left unchanged"""
    if key is None:
        return build()
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def norm_factor_rel(z64, p):
    """relative error of ``f = p |z|^(p-2)`` as ``norm_pow_grad`` forms it, per pair, in units of 1 (float32)"""
    u = UNIT[F32]
    p = _power(p)
    if p == 2.0:
        return torch.zeros(z64.shape[:-1], dtype=torch.float64)
    if p == 1.0:
        return torch.full(z64.shape[:-1], 3.0 * u, dtype=torch.float64)
    lnm = t_norm(z64, 1.0).log().abs()
    lnm = torch.where(torch.isfinite(lnm), lnm, torch.zeros_like(lnm))
    return (2.0 * abs(p - 2.0) + abs(p - 2.0) * lnm + LIB + 1.0) * u


def grad_reference(op, x, g, *params, second=None):
    """``(want, bound)`` float64 numpy of a backward kernel on float32 ``x`` and incoming gradient(s): float64 autograd of the
    formula.  'norm' (p): g (n,); 'magphase' (p): g for the magnitude, ``second`` for the phase, either may be None;
    'to_db' (ref, amin); 'from_db' (ref)."""
    u, tiny = UNIT[F32], TINY[F32]
    x64 = x.detach().cpu().double().requires_grad_(True)
    d = lambda t: None if t is None else t.detach().cpu().double()
    g, second = d(g), d(second)
    if op in ('norm', 'magphase'):
        p = _power(params[0])
        A = torch.zeros_like(x64)
        B = torch.zeros_like(x64)
        if g is not None:
            (A,) = torch.autograd.grad(t_norm(x64, p), x64, g)
        if second is not None:
            (B,) = torch.autograd.grad(t_angle(x64), x64, second)
        want = A + B
        rel = norm_factor_rel(x64.detach(), p)[..., None] + 2.0 * u
        bound = rel * A.abs() + 4.0 * u * B.abs() + (u * want.abs() if second is not None else 0.0)
    elif op == 'to_db':
        ref, amin = params
        (want,) = torch.autograd.grad(t_to_db(x64, t_passes(x.detach().cpu(), amin), ref, amin), x64, g)
        bound = 3.0 * u * want.abs()
    elif op == 'from_db':
        y = t_from_db(x64, params[0])
        (want,) = torch.autograd.grad(y, x64, g)
        e = x64.detach() / 10.0 + host_log10(params[0])
        rel = (LN10 / 2.0) * (x64.detach().abs() / 10.0 + 3.0 * e.abs()) * u + LIB * u
        bound = (rel + 3.0 * u) * want.abs()
    else:
        raise ValueError(op)
    bound = torch.where(torch.isfinite(bound), bound, torch.zeros_like(bound)) + tiny
    return want.numpy(), bound.numpy()


# ----------------------------------------------------------------------------- the comparison
def fractions(got, want, bound):
    """per element ``|got - want| / bound``; 0 where both are NaN or the same infinity, or where ``got`` is the infinity ``want``
    rounds to (or reaches within its bound); inf where the classes differ"""
    got, want, bound = _np(got), np.asarray(want), np.asarray(bound)
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    hi = want.dtype.type
    gh = got.astype(want.dtype)
    fmax = hi(np.finfo(got.dtype).max)
    with np.errstate(all='ignore'):
        frac = np.abs(gh - want) / bound
        nan_w, nan_g, inf_w, inf_g = np.isnan(want), np.isnan(gh), np.isinf(want), np.isinf(gh)
        same_inf = inf_w & (gh == want)
        rounds_up = inf_g & ~inf_w & ~nan_w & (np.sign(gh) == np.sign(want)) & (np.abs(want) + bound >= fmax)
        frac = np.where((nan_w & nan_g) | same_inf | rounds_up, 0.0, frac)
        frac = np.where((nan_w ^ nan_g) | (inf_w & ~same_inf) | (inf_g & ~inf_w & ~rounds_up), np.inf, frac)
    return np.where(np.isnan(frac), np.inf, frac).astype(np.float64)


def assert_held(got, want, bound, what):
    """every element inside its bound; prints and returns the worst error as a fraction of its bound"""
    frac = fractions(got, want, bound).reshape(-1)
    at = int(frac.argmax())
    worst = float(frac[at])
    print('%s: worst error %.3f of its bound' % (what, worst))
    assert worst <= 1.0, '%s: element %d is %.3f of its bound off: got %r, want %r, bound %r' % (
        what, at, worst, _np(got).reshape(-1)[at], np.asarray(want).reshape(-1)[at], np.asarray(bound).reshape(-1)[at])
    return worst


def forward_reference(op, x, *params, key=None):
    """``(want, bound)`` of a forward op, computed once per ``key``"""
    def build():
        want = n_forward(op, x, *params)
        return want, forward_bound(op, x, want, *params)
    return cached(key, build)


def tiled(pair, n):
    """``(want, bound)`` of the base input repeated to ``n`` leading entries (the second-trip cases fill their input this way)"""
    def rep(a):
        return a[np.arange(n) % a.shape[0]]
    return rep(pair[0]), rep(pair[1])


def assert_forward(op, got, x, *params, what='', key=None):
    """``got`` (any layout, the logical order of ``x``) against the reference of forward op ``op`` on ``x``"""
    want, bound = forward_reference(op, x, *params, key=key)
    return assert_held(_np(got).reshape(want.shape), want, bound, what or op)


def assert_grad(op, got, x, g, *params, second=None, what='', key=None):
    want, bound = cached(key, lambda: grad_reference(op, x, g, *params, second=second))
    return assert_held(_np(got).reshape(want.shape), want, bound, what or ('d ' + op))


# ----------------------------------------------------------------------------- the edge table's expectation
def classes(v, signed_zero=True):
    """0 NaN, 1 +inf, 2 -inf, 3 +0, 4 -0 (3 when ``signed_zero`` is off), 5 finite"""
    v = _np(v)
    c = np.full(v.shape, 5, dtype=np.int64)
    c[np.isnan(v)] = 0
    c[np.isposinf(v)] = 1
    c[np.isneginf(v)] = 2
    zero = v == 0
    c[zero] = np.where(np.signbit(v[zero]) & signed_zero, 4, 3)
    return c


def _oracle_f32(op, x, *params):
    """the formula in float32 torch on the CPU, as oracle/torch_ref.py states it"""
    if op == 'norm':
        m = torch.norm(x, 2, -1)
        return m if params[0] == 1.0 else m.pow(params[0])
    if op == 'angle':
        return torch.atan2(x[..., 1], x[..., 0])
    if op == 'to_db':
        ref, amin = params
        return 10.0 * (torch.log10(torch.clamp(x.pow(2.0), min=amin)) - torch.log10(torch.tensor(ref, dtype=x.dtype)))
    if op == 'from_db':
        return torch.pow(10.0, x / 10.0 + torch.log10(torch.tensor(params[0], dtype=x.dtype))).pow(0.5)
    raise ValueError(op)


def _round32(a):
    with np.errstate(all='ignore'):
        return np.asarray(a, dtype=np.float64).astype(np.float32)


def edge_expectation(op, x, *params, g=None):
    """``(expect float32, used)`` for the rows ``x`` (float32, CPU): the float32 torch evaluation, forward (``g`` None) or autograd
    with incoming gradient ``g``, with the rows of every applicable entry of DEVIATIONS replaced; ``used`` maps the names of the
    deviations that replaced something to their row counts."""
    x = x.detach().cpu()
    used = {}

    def replace(expect, rows, values, name):
        rows = np.asarray(rows)
        if rows.any():
            used[name] = int(rows.sum())
            expect = np.where(rows, _round32(values), expect)
        return expect

    with np.errstate(all='ignore'):
        if op == 'from_db':
            x64 = x.double()
            e = (x64 / 10.0 + host_log10(params[0])).numpy()
            y = np.power(10.0, e / 2.0)
            far = (np.abs(e) > 37.9) & ~np.isnan(e)
            if g is None:
                return replace(_oracle_f32(op, x, *params).numpy(), far, y, 'from dB beyond 10^+-38'), used
            xr = x.clone().requires_grad_(True)
            (expect,) = torch.autograd.grad(_oracle_f32(op, xr, *params), xr, g)
            return replace(expect.numpy(), far, g.double().numpy() * y * (LN10 / 20.0), 'from dB beyond 10^+-38'), used
        if g is None:
            return _oracle_f32(op, x, *params).numpy(), used
        xr = x.clone().requires_grad_(True)
        (expect,) = torch.autograd.grad(_oracle_f32(op, xr, *params), xr, g)
        expect = expect.numpy()
        g64 = g.double().numpy()
        if op == 'norm':
            p = _power(params[0])
            z = x.double().numpy()
            s32 = (x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]).numpy()         # float32, as the kernel forms it
            if p == 2.0:
                expect = replace(expect, np.ones(z.shape, dtype=bool), 2.0 * z * g64[..., None], 'norm gradient, power 2')
            elif p != 1.0:
                rows = np.broadcast_to((s32 == 0)[..., None], z.shape)
                expect = replace(expect, rows & np.isnan(expect), np.zeros(z.shape), 'norm gradient where s == 0')
                if p > 2.0:
                    rows = np.broadcast_to(np.isposinf(s32)[..., None], z.shape)
                    closed = (p * np.power(np.sqrt(s32.astype(np.float64)), p - 2.0) * g64)[..., None] * z
                    expect = replace(expect, rows, closed, 'norm gradient where s overflows, power above 2')
        elif op == 'angle':
            s32 = (x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]).numpy()
            rows = np.broadcast_to((np.isposinf(s32) & np.isfinite(x.numpy()).all(-1))[..., None], expect.shape)
            expect = replace(expect, rows & np.isnan(expect), np.zeros(expect.shape), 'phase gradient where s overflows')
        elif op == 'to_db':
            ref, amin = params
            xv = x.numpy()
            x64 = xv.astype(np.float64)
            sq32 = xv * xv
            closed = g64 * (20.0 / LN10) / x64
            floor0 = as_param(amin) == 0.0
            expect = replace(expect, np.isinf(xv), np.zeros(xv.shape), 'dB gradient at infinity')
            expect = replace(expect, np.isposinf(sq32) & np.isfinite(xv), closed, 'dB gradient where x^2 overflows')
            if floor0:
                expect = replace(expect, (sq32 == 0) & (xv != 0), closed, 'dB gradient where x^2 underflows and amin is 0')
                expect = replace(expect, xv == 0, closed, 'dB gradient at x == 0 with amin 0')
        return expect, used


def assert_edges(op, got, x, *params, g=None, what=''):
    """``got`` against the edge table's expectation: by class (zero signs only forward: 'gradient zero sign'), and where both are
    finite and non-zero against the float64 reference within the core bound.  Returns the deviations used."""
    expect, used = edge_expectation(op, x, *params, g=g)
    got = _np(got).reshape(expect.shape)
    signed = g is None
    cg, ce = classes(got, signed), classes(expect, signed)
    bad = np.argwhere(cg != ce)
    assert not len(bad), '%s: row %r of %r: got %r, expected %r (inputs %r)' % (
        what or op, tuple(bad[0]), params, got[tuple(bad[0])], expect[tuple(bad[0])], _np(x)[bad[0][0]])
    finite = (cg == 5)
    if finite.any():
        if g is None:
            want = n_forward(op, x, *params)
            bound = forward_bound(op, x, want, *params)
        elif op == 'angle':
            want, bound = grad_reference('magphase', x, None, 1.0, second=g)
        else:
            want, bound = grad_reference(op, x, g, *params)
        # where the float32 chain of the expectation has itself left the reference (a deviation replaced the row, or the reference
        # is not finite) the row is held to the expectation's own rounding
        ref_ok = np.isfinite(want) & (want != 0)
        frac = fractions(got, np.where(ref_ok, want, expect.astype(np.float64)), bound)
        frac = np.where(finite, frac, 0.0)
        at = np.unravel_index(int(frac.argmax()), frac.shape)
        print('%s %r: finite rows worst %.3f of the bound; deviations %r' % (what or op, params, float(frac[at]), used))
        assert float(frac[at]) <= 1.0, (what or op, params, at, got[at], want[at], bound[at])
    return used
