"""Per-channel energy normalisation restated in float64 — numpy for values, torch for autograd — and the comparison the pcen tests
share.  The only yardstick of tests/test_pcen_cpu.py and tests/test_pcen_gpu.py.

Definition (``functional.pcen``): per band, ``M[0] = E[0]``, ``M[t] = (1 - b) M[t-1] + b E[t]``,
``out = (E / (eps + M)**gain + bias)**power - bias**power``.

Bound of a float32 evaluation, per element: twice the error of the package's own float32 CPU route on the same inputs (the kernels
keep ``M`` beyond float32; the factor covers another ``exp`` / ``log`` / ``log1p`` / ``expm1``), floored at ``ULPS`` float32 ulps of the
element's scale.  Why 16: ``u**-gain = exp(-gain log u)`` turns the absolute error of its exponent into a relative one — ``|gain log u|
<= 14`` down to ``u = eps = 1e-6``, half an ulp of which is 4 ulps of 1 — and the chain adds a 1 – 2 ulp function five (forward) to
seven (backward) times with condition <= 1.  Scales: ``|out| + bias**power`` forward (``d out / d log w <= power (|out| + bias**power)``);
for a gradient the sum of the absolute values of the terms it adds up."""
import numpy as np
import torch

ULPS = 16 * 2.0 ** -23
DEFAULTS = dict(gain=0.98, bias=2.0, power=0.5, b=0.06, eps=1e-6)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


def _columns(E, params):
    return np.asarray(E, np.float64), [np.asarray(v, np.float64).reshape(-1, 1) for v in params]


def smoother(E, b):
    M = np.empty_like(E)
    M[..., 0] = E[..., 0]
    for t in range(1, E.shape[-1]):
        M[..., t] = (1 - b[:, 0]) * M[..., t - 1] + b[:, 0] * E[..., t]
    return M


def pcen(E, gain, bias, power, b, eps):
    """float64 values for ``E`` ``(…, F, T)``; parameters numbers or ``(F,)`` arrays"""
    E, (gain, bias, power, b) = _columns(E, (gain, bias, power, b))
    return (E / (eps + smoother(E, b)) ** gain + bias) ** power - bias ** power


def pcen_torch(E, gain, bias, power, b, eps):
    """the same in float64 torch operators, for autograd: ``E`` ``(…, F, T)``, parameters ``(F,)`` tensors"""
    s = b.unsqueeze(-1)
    m = [E[..., :1]]
    for t in range(1, E.shape[-1]):
        m.append((1 - s) * m[-1] + s * E[..., t:t + 1])
    M = torch.cat(m, dim=-1)
    return (E / (eps + M) ** gain.unsqueeze(-1) + bias.unsqueeze(-1)) ** power.unsqueeze(-1) - bias.unsqueeze(-1) ** power.unsqueeze(-1)


def gradients(E, g, params, eps):
    """float64 gradients for ``(E, gain, bias, power, b)``: autograd of ``pcen_torch`` under ``grad_out = g``"""
    ins = [torch.as_tensor(v, dtype=torch.float64).clone().requires_grad_(True) for v in (E,) + tuple(params)]
    got = torch.autograd.grad(pcen_torch(*ins, eps), ins, torch.as_tensor(g, dtype=torch.float64), allow_unused=True)
    return [np.zeros(tuple(i.shape)) if v is None else v.numpy() for i, v in zip(ins, got)]            # (one frame: b is unused)


def scales(E, g, params, eps):
    """per element of the five gradients, the sum of the absolute values of the terms it adds up (the chain rule written out: ``u =
    eps + M``, ``w = E u**-gain``, ``z = w + bias``, ``D = power z**(power-1)``, ``lam`` the reversed scan of ``|g| D gain w / u``)"""
    E, (gain, bias, power, b) = _columns(E, params)
    M, ag = smoother(E, b), np.abs(np.asarray(g, np.float64))
    u = eps + M
    w = E * u ** -gain
    z = w + bias
    D = power * z ** (power - 1)
    lam = ag * D * gain * w / u
    for t in range(E.shape[-1] - 2, -1, -1):
        lam[..., t] += (1 - b[:, 0]) * lam[..., t + 1]
    coef = np.where(np.arange(E.shape[-1]) == 0, 1.0, b)
    step = np.abs(E[..., 1:] - M[..., :-1])
    over = tuple(range(E.ndim - 2)) + (E.ndim - 1,)
    return [ag * D * u ** -gain + coef * lam, (ag * D * w * np.abs(np.log(u))).sum(over),
            (ag * power * np.abs(z ** (power - 1) - bias ** (power - 1))).sum(over),
            (ag * np.abs(z ** power * np.log(z) - bias ** power * np.log(bias))).sum(over), (lam[..., 1:] * step).sum(over)]


def signal(shape, seed):
    """positive float32 magnitudes over six decades with slow and fast variation along time; of several bands the last is all zero"""
    r = np.random.default_rng(seed)
    E = 10.0 ** r.uniform(-3, 3, shape) * (1.0 + 0.9 * np.sin(np.arange(shape[-1]) / 7.0))
    if shape[-2] > 1:
        E[..., -1, :] = 0.0
    return E.astype(np.float32)


def band_params(F, seed):
    """per-band float32 ``gain, bias, power, b`` inside the ranges a trained layer visits"""
    r = np.random.default_rng(seed)
    return tuple(r.uniform(lo, hi, F).astype(np.float32) for lo, hi in ((0.5, 1.0), (1.0, 3.0), (0.25, 0.75), (0.02, 0.5)))


def assert_close(got, value, yard, scale, what):
    """every element of ``got`` within ``max(2 |yard - value|, ULPS scale)`` of ``value``; prints the worst ratio, and the worst error in units of the floor"""
    got = got.detach().cpu().double().numpy()
    assert got.shape == value.shape, '%s: shape %r, expected %r' % (what, got.shape, value.shape)
    bound = np.maximum(2 * np.abs(np.asarray(yard, np.float64) - value), ULPS * scale) + 2.0 ** -126
    ratio = np.abs(got - value) / bound
    print('%s: worst |err| / bound %.3f, worst |err| / floor %.3f' % (what, ratio.max(), (np.abs(got - value) / (ULPS * scale + 2.0 ** -126)).max()))
    assert np.all(ratio <= 1.0), '%s: |err| / bound up to %g at %r' % (what, np.nanmax(ratio), np.unravel_index(np.nanargmax(ratio), ratio.shape))
