"""Shared by tests/test_mfcc_cpu.py and tests/test_mfcc_gpu.py: the DCT-II matrix in closed form (float64 numpy), the float64
reference of "rows times a matrix" and the bound every float32 result is held to.

The bound, per element:

    |got - ref| <= (n_in + 2) * 2^-24 * (|x| @ |D64|)

the standard bound of a float32 dot product of ``n_in`` terms in ANY summation order (n_in roundings of relative size 2^-24 on the
running sum of absolute products), plus one rounding of the matrix to float32 and one of the result.  Derived, not tuned: float32
``torch.matmul`` and a strictly sequential float32 accumulation on the CPU both stay below a third of it on dB-like inputs."""
import os

import numpy as np
import torch

EPS = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g13_dct.npz')
#: (num_mels, num_coeffs) of the golden file, each with norm None and 'ortho'
GOLDEN_SIZES = ((8, 8), (23, 13), (80, 40), (128, 40))


def norm_tag(norm):
    return 'none' if norm is None else norm


def dct_matrix64(num_coeffs, num_mels, norm='ortho'):
    """(num_mels, num_coeffs) float64: d[m][k] = cos(pi / num_mels * (m + 0.5) * k), times 2 (norm None) or orthonormalised."""
    m = np.arange(num_mels, dtype=np.float64)[:, None]
    k = np.arange(num_coeffs, dtype=np.float64)[None, :]
    d = np.cos(np.pi / num_mels * (m + 0.5) * k)
    if norm is None:
        return 2.0 * d
    assert norm == 'ortho'
    d[:, 0] *= 1.0 / np.sqrt(2.0)
    return d * np.sqrt(2.0 / num_mels)


def random_matrix64(n_in, n_out, seed):
    """a dense matrix with no structure (sizes a DCT cannot have: n_out > n_in), as float32 values held in float64"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n_in, n_out)).astype(np.float32).astype(np.float64)


def db_like(shape, seed, dtype=np.float32):
    """``30 * randn - 40`` over (…, n_in, T): the range of mel dB rows"""
    rng = np.random.default_rng(seed)
    return (30.0 * rng.standard_normal(shape) - 40.0).astype(dtype)


def _np64(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(np.float64)


def reference(x, d64):
    """float64 ``x64 @ D64`` along dim -2: (…, n_in, T) -> (…, n_out, T), and the per-element bound"""
    x64 = np.swapaxes(_np64(x), -1, -2)
    d64 = _np64(d64)
    ref = np.swapaxes(x64 @ d64, -1, -2)
    bound = (d64.shape[0] + 2) * EPS * np.swapaxes(np.abs(x64) @ np.abs(d64), -1, -2)
    return ref, bound


def assert_within(got, x, d64, what, skip_frames=()):
    """every element of ``got`` (…, n_out, T) within the bound of the float64 reference; NaN fails.  ``skip_frames``: time indices
    checked by the caller instead (a frame that holds a NaN on purpose).  Returns the worst |err| / bound."""
    ref, bound = reference(x, d64)
    g = _np64(got)
    assert g.shape == ref.shape, '%s: shape %s, expected %s' % (what, g.shape, ref.shape)
    keep = np.ones(g.shape[-1], dtype=bool)
    keep[list(skip_frames)] = False
    g, ref, bound = g[..., keep], ref[..., keep], bound[..., keep]
    assert not np.isnan(g).any(), '%s: %d NaN elements' % (what, int(np.isnan(g).sum()))
    err = np.abs(g - ref)
    bad = err > bound
    ratio = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max()) if err.size else 0.0
    assert not bad.any(), '%s: %d of %d elements beyond the bound, worst |err| / bound = %.3g (|err| %.3g)' % (
        what, int(bad.sum()), bad.size, ratio, float(err.max()))
    return ratio
