"""The float64 reference of ``ctc_loss`` and the bounds its float32 kernels are held to (tests/test_ctc_loss_gpu.py).

Reference: ``torch.nn.functional.ctc_loss`` on the CPU in float64, fed the SAME float32 ``log_probs`` widened; its autograd gives the
gradient in the convention the kernels implement.

Bounds (derived here, never fitted to a kernel's output).  Unit: ``u = 2^-24 * A_b``, half a float32 spacing at the largest finite
``|alpha|`` or ``|beta|`` of the entry's float64 lattice (recomputed below; ``A_b`` is floored at 3, see item 3).  A ``logsumexp`` hands its inputs'
errors on with weights that sum to 1, so a cell's error is at most that of ONE chain of steps, and a chain to the cost has ``Tb``
steps plus the closing ``logaddexp``: ``Tb + 1``.  A step of csrc/ctc_loss.hip is ``m + log(sum_i exp(x_i - m)) + lp`` with up to
three ``x_i``, the exponentials and the logarithm by the hardware's fast instructions.  It commits:

  1. the differences ``x_i - m`` and the fast ``exp`` of each: a relative ``2^-22`` of terms whose sum is the argument of the log, i.e.
     at most ``2^-22`` absolute in the result;
  2. the two additions of the sum: a relative ``2^-24`` each of a sum in ``[1, 3]``, together ``2^-23`` absolute in its logarithm;
  3. the fast ``log`` of a value in ``[1, 3]``: ``2^-23`` absolute;
  4. the addition ``m + log(..)``, rounded at magnitude ``<= A_b``: one unit;
  5. the addition of the emission, likewise one unit.

Items 1 to 3 are ``2^-21 = 8 * 2^-24`` absolute at most whatever the magnitudes; they are counted as three units, which covers them
for ``A_b >= 8 / 3``, and ``A_b`` is floored at 3 so that it always does.  So ``K_STEP = 5`` and ``E_b = (Tb + 1) * 5 * 2^-24 * A_b``.

A gradient element is ``exp(lp) - exp(ab + cost - lp)``, two terms in ``[0, 1]`` (the second is the posterior of the class at the
frame).  The exponent of the second carries the errors of an alpha and a beta (whose chains together have ``Tb + 1`` steps: ``E_b``), of
the cost (``E_b``) and of the fixed-order group sum and the two additions around it (a chain of a few roundings at magnitude
``<= 2 A_b``, covered by a third ``E_b`` since ``Tb + 1 >= 2``); ``exp`` of an exponent off by ``3 E_b`` is off by ``3 E_b`` of a value
``<= 1`` to first order, a fourth ``E_b`` covers the second order, and ``2^-21`` the two fast exponentials (``2^-22`` of a value
``<= 1`` each) with the rounding of the difference.  Hence ``4 E_b + 2^-21`` per element, before the ``grad_out`` scale.
"""
import torch

K_STEP = 5
EPS = 2.0 ** -24
INF = float('inf')


def make_case(T, N, C, S, blank=0, seed=0, labels=None):
    """``(log_probs float32 (T, N, C), targets int64 (N, S), input_lengths, target_lengths int64 (N,))`` on the host: ``log_softmax``
    of seeded normals; entry 0 has all ``T`` frames, the others run down to 60 %; the targets avoid ``blank``, come from the first
    ``labels`` other classes (all by default) and repeat their left neighbour at every fourth place.  Every entry takes as many
    of its ``S`` targets as leave ``Tb >= Lb + repeats + 2`` (``Tb >= Lb + repeats`` where ``Tb < 3``)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * T + S + C)
    lp = torch.log_softmax(torch.randn((T, N, C), generator=g), -1)
    classes = torch.tensor([c for c in range(C) if c != blank][:labels])
    targets = classes[torch.randint(0, len(classes), (N, S), generator=g)]
    if S > 1:
        targets[:, 1::4] = targets[:, 0::4][:, :targets[:, 1::4].shape[1]].clone()
    il, tl = [], []
    for b in range(N):
        Tb = max(1, -(-T * (10 * max(N - 1, 1) - 4 * b) // (10 * max(N - 1, 1))))
        Lb = S
        while Lb and Lb + int((targets[b, 1:Lb] == targets[b, :Lb - 1]).sum()) + (2 if Tb >= 3 else 0) > Tb:
            Lb -= 1
        il.append(Tb), tl.append(Lb)
    return lp, targets, torch.tensor(il), torch.tensor(tl)


def lattice(lp, labels, blank):
    """float64 alphas ``(Tb, 2 Lb + 1)`` of one entry's ``lp (Tb, C)``; the betas are the alphas of the reversed entry, reversed"""
    ext = torch.full((2 * len(labels) + 1,), blank, dtype=torch.long)
    ext[1::2] = labels
    e = lp[:, ext]
    skip = torch.zeros(len(ext), dtype=torch.bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    ninf = e.new_full((2,), -INF)
    a = e.new_full((len(ext),), -INF)
    a[:2] = e[0, :2]
    rows = [a]
    for t in range(1, len(e)):
        one, two = torch.cat([ninf[:1], a[:-1]]), torch.where(skip, torch.cat([ninf, a[:-2]])[:len(a)], ninf[0])
        a = torch.logsumexp(torch.stack([a, one, two]), 0) + e[t]
        rows.append(a)
    return torch.stack(rows)


class Reference(object):
    """``costs (N,)``, the gradient of ``sum_b w_b costs[b]`` by ``log_probs`` (``w`` folded in), and the per-entry bounds"""

    def __init__(self, lp, targets, il, tl, blank=0, w=None, zero_infinity=False, feasible=True):
        x = lp.double().requires_grad_(True)
        self.w = torch.ones(lp.shape[1], dtype=torch.float64) if w is None else w.double()
        self.costs = torch.nn.functional.ctc_loss(x, targets.long(), il.long(), tl.long(), blank, 'none', zero_infinity)
        (self.grad,) = torch.autograd.grad(self.costs, x, self.w)
        self.costs = self.costs.detach()
        assert not feasible or bool(torch.isfinite(self.costs).all()), self.costs
        self.cost_bound = torch.zeros_like(self.costs)
        starts = torch.cumsum(tl, 0) - tl
        for b in range(lp.shape[1]):
            Tb, Lb = int(il[b]), int(tl[b])
            labels = (targets[b, :Lb] if targets.dim() == 2 else targets[int(starts[b]):int(starts[b]) + Lb]).long()
            mags = torch.cat([lattice(x.detach()[:Tb, b], labels, blank).abs().flatten(),
                              lattice(x.detach()[:Tb, b].flip(0), labels.flip(0), blank).abs().flatten()])
            a_b = max(3.0, float(mags[torch.isfinite(mags)].max()))
            self.cost_bound[b] = (Tb + 1) * K_STEP * EPS * a_b
        self.grad_bound = 4.0 * self.cost_bound + 2.0 ** -21


_references = {}


def reference(key, *args, **kw):
    """the ``Reference`` of a case, computed once per ``key`` and left unchanged"""
    if key not in _references:
        _references[key] = Reference(*args, **kw)
    return _references[key]


def assert_costs(got, ref, what):
    """``got (N,)`` within ``E_b`` of the reference where that is finite, equal to it where not; prints the worst fraction"""
    got = got.detach().cpu().double()
    fin = torch.isfinite(ref.costs)
    assert torch.equal(got[~fin], ref.costs[~fin]), (what, got, ref.costs)
    frac = ((got - ref.costs).abs() / ref.cost_bound)[fin].max().item() if fin.any() else 0.0
    print('%s: worst cost error %.3f of its bound' % (what, frac))
    assert frac <= 1.0, (what, frac, got, ref.costs)


def assert_grad(got, ref, what):
    """``got (T, N, C)`` within ``(4 E_b + 2^-21) |w_b|`` of the reference per element; NaN exactly where the reference has NaN"""
    got = got.detach().cpu().double()
    assert torch.equal(got.isnan(), ref.grad.isnan()), what
    err = torch.nan_to_num((got - ref.grad).abs(), nan=0.0)
    frac = (err / (ref.grad_bound * ref.w.abs())[None, :, None]).max().item()
    print('%s: worst gradient error %.3f of its bound' % (what, frac))
    assert frac <= 1.0, (what, frac)
