"""Shared by tests/test_augment_cpu.py and tests/test_augment_gpu.py (a plain module: no tests in here): what ``add_noise`` is, written
from the definition and without the package.

``definition``  torchaudio's ``functional.add_noise`` in torch operators, in the dtype of its inputs (float32 or float64): the mask
                multiplied in, the squares summed along time, ``scale = 10 ** ((10 (log10 E_s - log10 E_n) - snr) / 20)``, and ``waveform
                + scale * noise`` at every sample.
``terms``       the same in float64 from inputs of any dtype, with the parts the bounds need: ``E_s``, ``E_n``, ``scale``, the mask.
``gradients``   the three gradient formulas in float64, over the broadcast shape, with the sums of the absolute products that form
                each element (the bounds are stated in them).
``forward_bound``, ``gradient_bounds``, ``worst_ratio``   the bounds of the kernel route.  They are derived, not measured: ``scale`` is rounded to
                float32 once (relative ``u = 2^-24``) and each output is rounded once (relative ``u``); the factor 2 on the product
                term lets a multiply-then-add form pass as well as the fused one.  The float64 sums add terms of order ``L 2^-53``
                relative to ``scale``: below 2e-11 at every length here, far inside the slack between ``u |want|`` and the budget.
``QUOTED``, ``launch``, ``wrap_rows``, ``assert_wraps``   the grid of ``tac_add_noise_f32`` restated from its launcher
                (tests/test_augment_cpu.py looks the quoted expressions up in csrc/add_noise.hip) and the row counts at which every
                workgroup walks its loop more than twice."""
import math

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -149
TILE = 4096                                     # samples of a row per unit (csrc/add_noise.hip: AN_TILE)
SNRS = (-5.0, 0.0, 10.0, 40.0)


# ----------------------------------------------------------------------------- the definition
def definition(waveform, noise, snr, lengths=None):
    """torchaudio's ``add_noise``, literally, in the dtype of ``waveform``"""
    assert waveform.dim() - 1 == noise.dim() - 1 == snr.dim() and (lengths is None or lengths.dim() == snr.dim())
    assert waveform.shape[-1] == noise.shape[-1]
    if lengths is not None:
        mask = torch.arange(waveform.shape[-1]) < lengths.unsqueeze(-1)
        masked_waveform, masked_noise = waveform * mask, noise * mask
    else:
        masked_waveform, masked_noise = waveform, noise
    energy_signal = (masked_waveform * masked_waveform).sum(-1)
    energy_noise = (masked_noise * masked_noise).sum(-1)
    scale = 10 ** ((10 * (torch.log10(energy_signal) - torch.log10(energy_noise)) - snr) / 20)
    return waveform + scale.unsqueeze(-1) * noise


def broadcast(waveform, noise, snr, lengths):
    """the operands on the host, in float64, expanded to the broadcast shape: ``(w, n, snr, mask)`` with ``mask`` boolean"""
    waveform, noise, snr = (t.detach().cpu().double() for t in (waveform, noise, snr))
    lead = torch.broadcast_shapes(waveform.shape[:-1], noise.shape[:-1], snr.shape, *(() if lengths is None else (lengths.shape,)))
    length = waveform.shape[-1]
    w, n, s = waveform.expand(lead + (length,)), noise.expand(lead + (length,)), snr.expand(lead)
    if lengths is None:
        mask = torch.ones(lead + (length,), dtype=torch.bool)
    else:
        mask = (torch.arange(length) < lengths.detach().cpu().unsqueeze(-1)).expand(lead + (length,))
    return w, n, s, mask


def terms(waveform, noise, snr, lengths=None):
    """float64: ``dict(w, n, mask, e_s, e_n, scale, out)`` over the broadcast shape.  The masked samples are selected out, as the
    kernel leaves them unread (the deviation of DESIGN 7: it differs from ``definition`` only for a NaN or inf behind a length)."""
    w, n, s, mask = broadcast(waveform, noise, snr, lengths)
    zero = torch.zeros((), dtype=torch.float64)
    wm, nm = torch.where(mask, w, zero), torch.where(mask, n, zero)
    e_s, e_n = (wm * wm).sum(-1), (nm * nm).sum(-1)
    scale = 10 ** ((10 * (torch.log10(e_s) - torch.log10(e_n)) - s) / 20)
    return dict(w=w, n=n, mask=mask, wm=wm, nm=nm, e_s=e_s, e_n=e_n, snr=s, scale=scale, out=w + scale.unsqueeze(-1) * n)


def gradients(grad_out, waveform, noise, snr, lengths=None):
    """The gradient formulas in float64 over the broadcast shape: ``dict(g_wave, g_noise, g_snr)`` and, for the bounds,
    ``abs_wave`` / ``abs_noise`` (the sums of the absolute products that form each element) and ``abs_d`` (``sum |g n|`` per row)"""
    t = terms(waveform, noise, snr, lengths)
    g = grad_out.detach().cpu().double().expand(t['w'].shape)
    d = (g * t['n']).sum(-1)
    scale, e_s, e_n = t['scale'], t['e_s'], t['e_n']
    c_w, c_n = (scale / e_s * d).unsqueeze(-1), (scale / e_n * d).unsqueeze(-1)
    s = scale.unsqueeze(-1)
    return dict(g_wave=g + c_w * t['wm'], g_noise=s * g - c_n * t['nm'], g_snr=-(math.log(10.0) / 20.0) * scale * d,
                abs_wave=(c_w * t['wm']).abs(), abs_noise=(s * g).abs() + (c_n * t['nm']).abs(), abs_d=(g * t['n']).abs().sum(-1),
                scale=scale)


def sum_to(t, shape):
    return t.sum_to_size(tuple(shape))


# ----------------------------------------------------------------------------- values
def normal(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


def lengths_for(rows, length, seed, dtype=torch.int64):
    """``rows`` lengths drawn in turn from 0, 1, TILE, TILE + 1 (the mask edge inside the second tile), L, L + 7 and -1, starting at
    ``seed``: every batch mixes several of them"""
    pool = (length, 1, TILE, TILE + 1, 0, length + 7, -1)
    return torch.tensor([pool[(seed + i) % len(pool)] for i in range(rows)], dtype=dtype)


# ----------------------------------------------------------------------------- bounds
def worst_ratio(got, want, bound):
    """max |got - want| / bound over the finite elements of ``want``; the other elements have to agree in kind (NaN with NaN, an
    infinity with the same infinity)"""
    got, want, bound = (torch.as_tensor(t).detach().cpu().double() for t in (got, want, bound))
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    finite = torch.isfinite(want)
    odd = ~finite
    assert bool((torch.isnan(got[odd]) == torch.isnan(want[odd])).all()), 'NaN positions differ'
    both = odd & ~torch.isnan(want)
    assert bool((got[both] == want[both]).all()), 'infinities differ'
    assert bool(torch.isfinite(got[finite]).all()), 'a non-finite value where the definition is finite'
    if not bool(finite.any()):
        return 0.0
    return float(((got[finite] - want[finite]).abs() / bound.expand(want.shape)[finite]).max())


def forward_bound(t):
    """``u |want| + 2 u |scale n_t| + 2^-149`` of ``terms``' result"""
    prod = (t['scale'].unsqueeze(-1) * t['n']).abs()
    prod = torch.where(torch.isfinite(prod), prod, torch.zeros((), dtype=torch.float64))
    want = torch.where(torch.isfinite(t['out']), t['out'], torch.zeros((), dtype=torch.float64))
    return U * want.abs() + 2 * U * prod + TINY


def gradient_bounds(r, shapes=None):
    """the bounds of ``gradients``' three results, of the same form: ``u |want| + 2 u (sum of the absolute products)`` and, for
    ``g_snr``, ``u |want| + 2^-50 scale sum |g n|``.  ``shapes`` = the shapes of (waveform, noise, snr): a gradient that torch's
    ``sum`` folds over ``k`` broadcast rows gets the folded rows' bounds and, for the float32 sum of ``k`` terms, ``(k - 1) u sum
    |terms|``."""
    b = dict(g_wave=U * r['g_wave'].abs() + 2 * U * r['abs_wave'] + TINY,
             g_noise=U * r['g_noise'].abs() + 2 * U * r['abs_noise'] + TINY,
             g_snr=U * r['g_snr'].abs() + 2.0 ** -50 * r['scale'] * r['abs_d'] + TINY)
    want = dict((k, r[k]) for k in b)
    if shapes is not None:
        for key, shape in zip(('g_wave', 'g_noise', 'g_snr'), shapes):
            k = r[key].numel() // max(int(np.prod(shape)), 1)
            if k > 1:
                b[key] = sum_to(b[key], shape) + (k - 1) * U * sum_to(r[key].abs(), shape)
                want[key] = sum_to(r[key], shape)
    return want, b


# ----------------------------------------------------------------------------- the grid of tac_add_noise_f32
QUOTED = ('add_noise.hip', (
    '#define TAC_AN_PER_CU 32',
    'constexpr int AN_THREADS = 256;',
    'constexpr int AN_PASSES = 4;',
    'constexpr int AN_TILE = AN_THREADS * 4 * AN_PASSES;',
    'const long long tiles = (L + AN_TILE - 1) / AN_TILE;',
    'const long long units = rows * tiles;',
    'const long long blocks = persistent_blocks(units, 1, (long long)device_cu_count() * TAC_AN_PER_CU);',
    'const long long row_blocks = persistent_blocks(rows, 1, (long long)device_cu_count() * TAC_AN_PER_CU);',
    'for (unsigned u = blockIdx.x; u < g.units; u += gridDim.x, par ^= 1) {',
    'for (long long row = blockIdx.x; row < g.rows; row += gridDim.x) {',
    'for (unsigned v = blockIdx.x; v < g.units; v += gridDim.x) {',
))
CU_COUNTS = (256, 304)
BASE_ROWS = 5
PER_CU = 32
MAX_TENSOR_BYTES = 512 * 1000 * 1000            # per tensor, as tests/grid_rules.py


def ceil_div(a, b):
    return -(-a // b)


def launch(cus, rows, length):
    """(units, grid cap) of the reduce and the mix launch: the units (row, tile) and the most workgroups that walk them"""
    return rows * ceil_div(length, TILE), cus * PER_CU


#: (name, L, tiles per row): the issue's form — two tiles per row, L = TILE + 1, the dword accesses — and rows of one 16-byte chunk
WRAP_FORMS = (('two tiles per row, dwords', TILE + 1, 2), ('one tile per row, 16-byte chunks', 4, 1))


def wrap_rows(cus, tiles=2):
    """rows with which every workgroup walks its unit loop twice and some of them a third time on ``cus`` compute units.  At two tiles
    per row the units are even like twice the grid, so the remainder is an odd number of ROWS (``BASE_ROWS`` of them: ten units);
    at one tile per row it is an odd number of units.  Either count is past the grid of the row kernel too."""
    return (2 // tiles) * PER_CU * cus + BASE_ROWS


def assert_wraps(cus):
    for name, length, tiles in WRAP_FORMS:
        rows = wrap_rows(cus, tiles)
        units, grid = launch(cus, rows, length)
        r = units - 2 * grid
        assert units == rows * tiles and 0 < r < grid and r % tiles == 0 and (r // tiles) % 2 == 1, \
            '%s on %d CUs: %d units on a grid of %d' % (name, cus, units, grid)
        assert rows > grid                                                    # the row loop of the scale kernel wraps as well
        assert 4 * rows * length < MAX_TENSOR_BYTES
    return wrap_rows(cus)
