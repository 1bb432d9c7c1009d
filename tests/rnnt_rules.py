"""The float64 reference of ``rnnt_loss`` and the bounds its float32 kernels are held to (tests/test_rnnt_cpu.py, test_rnnt_gpu.py).

Reference: the recursion of Graves (2012) as torchaudio documents it, per batch entry on that entry's own ``(Tb, Ub + 1)`` lattice, in
float64 torch operators, one anti-diagonal per step — fed the SAME float32 logits as the code under test.  The gradient is float64
autograd of that recursion; the closed expression the kernels implement is evaluated beside it (``closed_gradient``) and
tests/test_rnnt_cpu.py holds the two together.

Bounds (derived here, never fitted to a kernel's output).  Unit: ``ulp = 2^-24 * A_b``, half a float32 spacing at the largest
magnitude the entry's lattice holds — ``A_b`` is the largest finite ``|alpha|``, ``|beta|`` or ``|denominator|`` of the entry in this
reference.  ``logaddexp(x, y)`` has partial derivatives ``(p, 1 - p)``: it hands its inputs' errors on with weights that sum to 1,
so the error of a lattice cell is at most the error of ONE chain of steps leading to it, and a chain to the cost has ``Tb + Ub + 1``
steps (``Tb - 1 + Ub`` cells after the first, the closing blank, and one for the first cell's own inputs).  A step commits these
roundings, each at most one unit because each rounds a value of magnitude ``<= A_b`` to nearest (half a spacing is ``<= 2^-24 |x|``):

  1. the denominator the step's log-probability was made with (its sum and its logarithm, rounded at magnitude ``|denominator|``);
  2. ``logit - denominator``;
  3. the sum ``alpha + lp``;
  4. the ``logaddexp``: ``max + log1p(exp(-|difference|))``, whose last addition rounds at magnitude ``|alpha|`` (the correction term
     is at most ``log 2`` and its own error a fraction of a unit wherever ``A_b >= 1``).

Hence ``K_STEP = 4`` and ``E_b = (Tb + Ub + 1) * 4 * 2^-24 * A_b``.  A gradient element is a difference of two terms in ``[0, 1]``
(``exp(g + beta[t,u])`` and one of the blank / label terms) whose exponents carry at most three such errors (alpha, beta, cost), so
it is held to ``4 E_b + 2^-23`` before the ``grad_costs`` scale: ``exp`` of an exponent off by ``3 E_b`` is off by ``3 E_b`` of a
value ``<= 1`` to first order, the fourth ``E_b`` covers the second order and the exponent's own sums, and ``2^-23`` the rounding of
the two terms and their difference.  Clipping is 1-Lipschitz, so a clamp does not widen the bound.
"""
import math

import torch

K_STEP = 4
EPS = 2.0 ** -24

#: (B, T, U, V) with ragged lengths; the first entry is always full length (torchaudio's CPU checks ask for that)
SHAPES = ((3, 7, 4, 6), (2, 70, 66, 29), (2, 5, 0, 3))


def make_case(B, T, U, V, blank=-1, seed=0, scale=1.0, full=False):
    """``(logits float32 (B, T, U + 1, V), targets int32 (B, U), logit_lengths, target_lengths)`` on the host.  Entry 0 has the full
    lengths, the others run down to 60 % of them (never below one frame); the targets avoid ``blank`` and repeat labels (every
    second target equals its left neighbour where the class count allows nothing else or by construction)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * T + U + V)
    logits = torch.randn((B, T, U + 1, V), generator=g, dtype=torch.float32) * scale
    b = blank + V if blank < 0 else blank
    classes = torch.tensor([v for v in range(V) if v != b], dtype=torch.int32)
    targets = classes[torch.randint(0, V - 1, (B, U), generator=g)]
    if U > 1:
        targets[:, 1::2] = targets[:, 0::2][:, :targets[:, 1::2].shape[1]].clone()    # repeated labels: (0, 1), (2, 3), …
    share = [1.0] + [1.0 - 0.4 * (i + 1) / max(B - 1, 1) for i in range(B - 1)]
    if full:
        share = [1.0] * B
    logit_lengths = torch.tensor([max(1, int(math.ceil(T * s))) for s in share], dtype=torch.int32)
    target_lengths = torch.tensor([int(U * s) for s in share], dtype=torch.int32)
    return logits, targets.to(torch.int32).contiguous(), logit_lengths, target_lengths


def _log_probs(x, labels, blank, fused):
    """``(denominator, lp_blank (Tb, Ub + 1), lp_label (Tb, Ub))`` of one entry's float64 logits ``(Tb, Ub + 1, V)``"""
    denom = torch.logsumexp(x, dim=-1) if fused else torch.zeros(x.shape[:2], dtype=x.dtype)
    lpb = x[..., blank] - denom
    Ub = x.shape[1] - 1
    if Ub:
        idx = labels.long()[None, :, None].expand(x.shape[0], Ub, 1)
        lpl = x[:, :Ub].gather(-1, idx).squeeze(-1) - denom[:, :Ub]
    else:
        lpl = x.new_zeros((x.shape[0], 0))
    return denom, lpb, lpl


def _alpha(lpb, lpl):
    Tb, U1 = lpb.shape
    rows = {(0, 0): lpb.new_zeros(())}
    for d in range(1, Tb + U1 - 1):
        for u in range(max(0, d - Tb + 1), min(U1 - 1, d) + 1):
            t = d - u
            terms = []
            if t > 0:
                terms.append(rows[(t - 1, u)] + lpb[t - 1, u])
            if u > 0:
                terms.append(rows[(t, u - 1)] + lpl[t, u - 1])
            rows[(t, u)] = terms[0] if len(terms) == 1 else torch.logaddexp(terms[0], terms[1])
    return torch.stack([torch.stack([rows[(t, u)] for u in range(U1)]) for t in range(Tb)])


def _beta(lpb, lpl):
    Tb, U1 = lpb.shape
    rows = {(Tb - 1, U1 - 1): lpb[Tb - 1, U1 - 1]}
    for d in range(Tb + U1 - 3, -1, -1):
        for u in range(max(0, d - Tb + 1), min(U1 - 1, d) + 1):
            t = d - u
            terms = []
            if t < Tb - 1:
                terms.append(rows[(t + 1, u)] + lpb[t, u])
            if u < U1 - 1:
                terms.append(rows[(t, u + 1)] + lpl[t, u])
            rows[(t, u)] = terms[0] if len(terms) == 1 else torch.logaddexp(terms[0], terms[1])
    return torch.stack([torch.stack([rows[(t, u)] for u in range(U1)]) for t in range(Tb)])


def closed_gradient(x, labels, blank, fused, alpha, beta, denom, cost):
    """the closed expression csrc/rnnt.hip implements, on one entry, float64: the gradient of ``cost`` by ``x``"""
    Tb, U1, V = x.shape
    ninf = float('-inf')
    g = x - denom[..., None] + alpha[..., None] + cost
    grad = torch.exp(g + beta[..., None]) if fused else torch.zeros_like(x)
    below = torch.full((Tb, U1), ninf, dtype=x.dtype)
    below[:-1] = beta[1:]
    below[Tb - 1, U1 - 1] = 0.0
    grad[..., blank] -= torch.exp(g[..., blank] + below)
    for u in range(U1 - 1):
        grad[:, u, int(labels[u])] -= torch.exp(g[:, u, int(labels[u])] + beta[:, u + 1])
    return grad


class Reference(object):
    """costs, alphas, betas, denominators ``(zeros outside an entry's lattice)``, the autograd gradient of ``sum_b costs[b]`` and the
    closed one, all float64, and the bounds ``cost_bound (B,)`` and ``grad_bound (B,)`` (per element, before ``grad_costs``)"""

    def __init__(self, logits, targets, logit_lengths, target_lengths, blank=-1, fused=True):
        B, T, U1, V = logits.shape
        blank = blank + V if blank < 0 else blank
        self.costs = torch.zeros(B, dtype=torch.float64)
        self.alphas, self.betas, self.denoms = (torch.zeros((B, T, U1), dtype=torch.float64) for _ in range(3))
        self.grad, self.grad_closed = (torch.zeros((B, T, U1, V), dtype=torch.float64) for _ in range(2))
        self.cost_bound, self.grad_bound, self.beta_cost = (torch.zeros(B, dtype=torch.float64) for _ in range(3))
        for b in range(B):
            Tb, Ub = int(logit_lengths[b]), int(target_lengths[b])
            x = logits[b, :Tb, :Ub + 1].double().clone().requires_grad_(True)
            labels = targets[b, :Ub]
            denom, lpb, lpl = _log_probs(x, labels, blank, fused)
            alpha, beta = _alpha(lpb, lpl), _beta(lpb, lpl)
            cost = -(alpha[Tb - 1, Ub] + lpb[Tb - 1, Ub])
            (grad,) = torch.autograd.grad(cost, x)
            with torch.no_grad():
                self.costs[b] = cost
                self.beta_cost[b] = -beta[0, 0]
                self.alphas[b, :Tb, :Ub + 1], self.betas[b, :Tb, :Ub + 1], self.denoms[b, :Tb, :Ub + 1] = alpha, beta, denom
                self.grad[b, :Tb, :Ub + 1] = grad
                self.grad_closed[b, :Tb, :Ub + 1] = closed_gradient(x.detach(), labels, blank, fused, alpha, beta, denom, cost)
                mags = torch.cat([alpha.abs().flatten(), beta.abs().flatten(), denom.abs().flatten()])
                a_b = float(mags[torch.isfinite(mags)].max())
                self.cost_bound[b] = (Tb + Ub + 1) * K_STEP * EPS * a_b
                self.grad_bound[b] = 4.0 * self.cost_bound[b] + 2.0 ** -23


_references = {}


def reference(key, logits, targets, logit_lengths, target_lengths, blank=-1, fused=True):
    """the ``Reference`` of a case, computed once per ``key`` and left unchanged"""
    if key not in _references:
        _references[key] = Reference(logits, targets, logit_lengths, target_lengths, blank, fused)
    return _references[key]


def assert_costs(got, ref, what):
    """``got (B,)`` against the reference within ``E_b``; returns the worst error as a fraction of its bound"""
    got = got.detach().cpu().double()
    assert not got.isnan().any(), (what, got)
    frac = ((got - ref.costs).abs() / ref.cost_bound).max().item()
    print('%s: worst cost error %.3f of its bound' % (what, frac))
    assert frac <= 1.0, (what, frac, got, ref.costs)
    return frac


def assert_grad(got, ref, what, grad_costs=None, clamp=-1.0):
    """``got (B, T, U + 1, V)`` against ``clip(reference gradient) * grad_costs`` within ``(4 E_b + 2^-23) |grad_costs[b]|``; exact
    zeros outside each entry's lattice are part of the reference"""
    got = got.detach().cpu().double()
    assert not got.isnan().any(), what
    want = ref.grad.clamp(-clamp, clamp) if clamp > 0 else ref.grad
    scale = torch.ones(got.shape[0], dtype=torch.float64) if grad_costs is None else grad_costs.detach().cpu().double()
    want = want * scale[:, None, None, None]
    bound = (ref.grad_bound * scale.abs())[:, None, None, None]
    frac = ((got - want).abs() / bound).max().item()
    print('%s: worst gradient error %.3f of its bound' % (what, frac))
    assert frac <= 1.0, (what, frac)
    return frac
