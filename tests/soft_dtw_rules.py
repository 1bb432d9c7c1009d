"""The float64 reference of ``soft_dtw`` and the bounds its float32 kernels are held to (tests/test_soft_dtw_gpu.py).

Reference: the recursion of the issue in float64 (numpy, an anti-diagonal at a time), fed the SAME float32 inputs widened; ``Q`` is the
recursion on the entry flipped in both axes, ``E`` and the gradients come from the closed forms.

Bounds (derived here from the instruction sequence of csrc/soft_dtw.hip, never fitted to its output).  ``EPS = 2^-24`` is half a
float32 spacing relative to a value.  ``softmin`` is a convex combination of its arguments, so it hands their errors on with weights
that sum to 1: the error of a cell of ``R`` is at most the sum of the local errors along ONE path to it, and a path to
``(Nb, Mb)`` has at most ``Nb + Mb - 1`` cells.  A cell commits:

  1. its cost, ``D`` times ``t = x - y`` (one rounding), ``t * t`` (one) and the addition to the running sum (one, of a partial sum
     ``<= delta``): ``(D + 2) EPS dmax`` to first order, ``dmax`` the largest cost of the entry;
  2. ``softmin``: the differences ``m - v`` (a rounding each) times the rounded ``1 / gamma`` give the exponent ``a <= 0`` to a
     relative ``3 EPS``, which moves ``e^a`` by at most ``3 EPS |a| e^a <= 1.2 EPS``; the fast ``exp`` adds a relative ``2^-22`` of a
     value ``<= 1``: ``5.2 EPS`` a term, ``15.6 EPS`` for the three; the two additions of a sum in ``[1, 3]`` add ``6 EPS``; all
     of it is divided by the sum ``>= 1`` inside the logarithm; the fast ``log`` of ``[1, 3]`` adds ``2^-23 = 2 EPS`` and the product
     with ``gamma`` ``1.1 EPS``: below ``25 EPS gamma``, counted as ``K_SOFT = 32``;
  3. ``m - gamma log(..)`` and the addition of the cost: a rounding each at magnitude ``<= rmax``, the largest finite ``|R|`` or
     ``|Q|`` of the float64 lattice.

``local = (D + 2) EPS dmax + 2 EPS rmax + 32 EPS gamma`` and ``bound_R = (Nb + Mb - 1) local`` holds for every cell of ``R`` and
``Q`` and for the value.  The exponent of ``E`` carries the errors of ``R``, ``Q`` and the value (``3 bound_R``), of the cost and of
the three subtractions at magnitude ``<= 2 rmax`` (``3 local`` covers them): ``t = 3 (bound_R + local) / gamma``, so
``|dE| <= E expm1(t) + 2^-21`` (the fast ``exp`` of a value ``<= 1`` and the rounding of its exponent).  A gradient element is
``2 w sum_j E[i][j] (x[i][d] - y[j][d])``, evaluated as ``x sum E - sum E y`` with ``Mb`` sequential additions in the row sum, ``Mb``
matrix-pipe accumulations and three closing roundings: ``(Mb + 4) EPS`` relative to ``sum_j E (|x| + |y|)``.  Hence
``2 |w| sum_j (E (expm1(t) + (Mb + 4) EPS) + 2^-21) (|x[i][d]| + |y[j][d]|)`` per element, and the same over ``i`` for ``y``.
"""
import numpy as np
import torch

EPS = 2.0 ** -24
K_SOFT = 32


def make_case(B, N, M, D, seed=0):
    """seeded float32 ``x (B, N, D)`` and ``y (B, M, D)`` on the host: ``y`` is noise around half of ``x`` resampled to ``M`` rows"""
    g = torch.Generator().manual_seed(1000 * seed + 131 * N + 17 * M + D)
    x = torch.randn((B, N, D), generator=g)
    rows = torch.linspace(0, N - 1, M).round().long()
    return x, 0.5 * x[:, rows] + 0.5 * torch.randn((B, M, D), generator=g)


def recursion(delta, gamma):
    """float64 ``R (n, m)`` of the costs ``delta``"""
    n, m = delta.shape
    R = np.full((n + 1, m + 1), np.inf)
    R[0, 0] = 0.0
    for k in range(n + m - 1):
        i = np.arange(max(0, k - m + 1), min(n - 1, k) + 1)
        j = k - i
        a, b, c = R[i, j + 1], R[i + 1, j], R[i, j]
        lo = np.minimum(np.minimum(a, b), c)
        R[i + 1, j + 1] = delta[i, j] + lo - gamma * np.log(np.exp((lo - a) / gamma) + np.exp((lo - b) / gamma) + np.exp((lo - c) / gamma))
    return R[1:, 1:]


class Reference(object):
    """values ``(B,)``, ``E (B, N, M)``, the gradients of ``sum_b w_b value[b]`` and the bounds of each, padded with zeros"""

    def __init__(self, x, y, gamma, xl=None, yl=None, w=None):
        B, N, D = x.shape
        M = y.shape[1]
        xl = [N] * B if xl is None else [int(v) for v in xl]
        yl = [M] * B if yl is None else [int(v) for v in yl]
        self.w = np.ones(B) if w is None else w.double().numpy()
        self.value, self.value_bound = np.zeros(B), np.zeros(B)
        self.E, self.E_bound = np.zeros((B, N, M)), np.zeros((B, N, M))
        self.gx, self.gx_bound, self.gy, self.gy_bound = (np.zeros(s) for s in ((B, N, D), (B, N, D), (B, M, D), (B, M, D)))
        with np.errstate(over='ignore'):
            for b in range(B):
                n, m = xl[b], yl[b]
                xb, yb = x[b, :n].double().numpy(), y[b, :m].double().numpy()
                delta = ((xb[:, None, :] - yb[None, :, :]) ** 2).sum(-1)
                R = recursion(delta, gamma)
                Q = recursion(delta[::-1, ::-1], gamma)[::-1, ::-1]
                E = np.exp(-(R + Q - delta - R[-1, -1]) / gamma)
                local = EPS * ((D + 2) * delta.max() + 2 * max(np.abs(R).max(), np.abs(Q).max()) + K_SOFT * gamma)
                bound_r = (n + m - 1) * local
                t = min(3 * (bound_r + local) / gamma, 60.0)        # (beyond, the bound says nothing: kept finite so that 0 * it is 0)
                self.value[b], self.value_bound[b] = R[-1, -1], bound_r
                self.E[b, :n, :m], self.E_bound[b, :n, :m] = E, E * np.expm1(t) + 2.0 ** -21
                for own, other, e, grad, bound in ((xb, yb, E, self.gx, self.gx_bound), (yb, xb, E.T, self.gy, self.gy_bound)):
                    k = len(own)
                    grad[b, :k] = 2 * self.w[b] * (own * e.sum(1, keepdims=True) - e @ other)
                    slack = e * (np.expm1(t) + (len(other) + 4) * EPS) + 2.0 ** -21
                    bound[b, :k] = 2 * abs(self.w[b]) * (np.abs(own) * slack.sum(1, keepdims=True) + slack @ np.abs(other))


_references = {}


def reference(key, *args, **kw):
    """the ``Reference`` of a case, computed once per ``key`` and left unchanged"""
    if key not in _references:
        _references[key] = Reference(*args, **kw)
    return _references[key]


def assert_within(got, want, bound, what):
    """``got`` within ``bound`` of ``want`` elementwise (all three numpy-shaped alike); prints the worst fraction of the bound"""
    got = got.detach().cpu().double().numpy()
    assert got.shape == want.shape and np.isfinite(got).all(), (what, got.shape, want.shape)
    exact = bound == 0
    assert np.array_equal(got[exact], want[exact]), what             # (padding: exactly zero)
    frac = float((np.abs(got - want)[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0
    print('%s: worst error %.3g of its bound' % (what, frac))
    assert frac <= 1.0, (what, frac)
