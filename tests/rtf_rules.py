"""Rules of the RTF beamforming tests: the complex128 restatement of torchaudio's ``rtf_evd`` / ``rtf_power`` / ``mvdr_weights_rtf`` /
``RTFMVDR`` (restated literally, as in tests/beamform_rules.py, whose generator, ``load``, ``kappa``, ``apply_beamforming`` and
constants are used here) and the error bounds the float32-in, float64-on-chip kernels of csrc/beamform.hip are held to.  Kernel and
restatement are always fed the SAME float32 tensors.

Notation: ``u = 2^-24``; ``κ`` the float64 2-norm condition number of the loaded ``Φn`` (``R.kappa``); ``C`` channels.  Every bound
gets ``+ R.TINY``.

rtf_evd bound.  An eigenvector is defined up to a unit phase, so the reference is first rotated by ``s = wantᴴ got / |wantᴴ got|``.
Then per complex component ``|got_c - s want_c| <= 3 u |want_c| + 64 C^3 2^-53 ‖Φs‖₂ / gap``, ``gap = λ1 - λ2`` in float64.  The
``3 u``: ``√2 u`` for the one rounding of the two real parts of a component, ``u`` for the first-order error of the alignment
itself (``s`` is estimated from the rounded vector), the sum rounded up.  The tail: float64 Jacobi leaves a backward error of a
modest multiple of ``C 2^-53 ‖Φs‖₂``, which moves the eigenvector by that over the gap (Davis–Kahan); the constant is the one of
the Souden weights bound.  The main inputs keep ``‖Φs‖₂ / gap <= GAP_CAP``.

rtf_evd checks without a gap, on every case, the degenerate ones included, with ``v`` the returned float32 vector:
``| ‖v‖₂ - 1 | <= 4 u`` (``C`` roundings of at most ``u`` relative each move the norm by at most ``u``; the rest is slack);
``‖Φs v - (vᴴ Φs v) v‖₂ <= 4 C u ‖Φs‖₂`` and ``vᴴ Φs v >= λ1 - 8 C u ‖Φs‖₂``: a unit vector within ``δ <= √C u`` of an exact
eigenvector has a residual of at most ``2 δ ‖Φs‖₂`` and a Rayleigh quotient within ``2 δ ‖Φs‖₂`` of ``λ1``.  The convention: some
component has an imaginary part of exactly 0 and a positive real part, and its modulus is at least ``(1 - 4 u)`` of the largest.

rtf_power bound.  Per real component ``|Δr| <= u |r| + 64 C^3 n_iter 2^-53 κ ‖L‖₂ ‖φ‖₂^(n_iter - 1) ‖u_ref‖₂``: one rounding to
float32, plus the float64 solve (the Souden constant and ``κ``) carried through ``n_iter`` products whose norms bound the growth;
``L = Φs`` for ``n_iter >= 2`` and the loaded ``Φn`` for ``n_iter == 1``, ``φ`` and the norms from the float64 restatement,
``‖u_ref‖₂ = 1`` for an int reference.

mvdr_weights_rtf bound.  Per real component ``|Δw| <= u |w| + 128 C^3 2^-53 κ max_c |w_c|``: the Souden bound with one more
solve-sized term for the quadratic form ``dᴴ Φn⁻¹ d`` in the denominator."""
import torch

import beamform_rules as R

U = R.U
GAP_CAP = 10.0

#: mirror of csrc/beamform.hip (tac_rtf_power_max_iter)
MAX_ITER = 64

N_ITERS = (1, 2, 3, 5)


# ----------------------------------------------------------------------------- the restatement (complex128)
def lead_phase(v):
    """the package's convention: the component of largest modulus (lowest index on a tie) real and positive"""
    v = v.to(torch.complex128)
    mag = v.abs()
    lead = mag.argmax(dim=-1, keepdim=True)
    h = torch.gather(v, -1, lead)
    out = torch.view_as_real(v * (h.conj() / torch.gather(mag, -1, lead))).clone()
    out[..., 1].scatter_(-1, lead, 0.0)
    return torch.view_as_complex(out)


def rtf_evd(psd_s):
    """``(…, F, C, C)`` → ``(…, F, C)``: the eigenvector of the largest eigenvalue (``eigh``: ascending, unit norm)"""
    _, v = torch.linalg.eigh(psd_s.to(torch.complex128))
    return lead_phase(v[..., -1])


def rtf_power(psd_s, psd_n, reference_channel, n_iter=3, diagonal_loading=True, diag_eps=1e-7):
    assert n_iter > 0
    s, n = psd_s.to(torch.complex128), psd_n.to(torch.complex128)
    if diagonal_loading:
        n = R.load(n, diag_eps)
    phi = torch.linalg.solve(n, s)
    if torch.is_tensor(reference_channel):
        rtf = torch.einsum('...c,...c->...', phi, reference_channel.to(torch.complex128)[..., None, None, :])
    else:
        rtf = phi[..., reference_channel]
    rtf = rtf.unsqueeze(-1)
    if n_iter >= 2:
        for _ in range(n_iter - 2):
            rtf = torch.matmul(phi, rtf)
        rtf = torch.matmul(s, rtf)
    else:
        rtf = torch.matmul(n, rtf)
    return rtf.squeeze(-1)


def mvdr_weights_rtf(rtf, psd_n, reference_channel=None, diagonal_loading=True, diag_eps=1e-7, eps=1e-8):
    d, n = rtf.to(torch.complex128), psd_n.to(torch.complex128)
    if diagonal_loading:
        n = R.load(n, diag_eps)
    numerator = torch.linalg.solve(n, d.unsqueeze(-1)).squeeze(-1)
    denominator = torch.einsum('...d,...d->...', d.conj(), numerator)
    w = numerator / (denominator.real.unsqueeze(-1) + eps)
    if reference_channel is None:
        return w
    if torch.is_tensor(reference_channel):
        scale = torch.einsum('...c,...c->...', d.conj(), reference_channel.to(torch.complex128)[..., None, :])
    else:
        scale = d[..., reference_channel].conj()
    return w * scale.unsqueeze(-1)


def rtf_mvdr(specgram, rtf, psd_n, reference_channel, diagonal_loading=True, diag_eps=1e-7, eps=1e-8):
    return R.apply_beamforming(mvdr_weights_rtf(rtf, psd_n, reference_channel, diagonal_loading, diag_eps, eps), specgram)


# ----------------------------------------------------------------------------- inputs
def psds(C, F, T, seed=11, lead=(2,)):
    """``(X, Φs, Φn)``: a scene and its two normalised float32 (complex64) PSDs, as tests/test_beamform_gpu.py builds them"""
    x, ms, mn = R.scene(lead, C, F, T, seed=seed)
    return x, R.psd(x, ms, True, 1e-15).to(torch.complex64), R.psd(x, mn, True, 1e-15).to(torch.complex64)


def references(C, lead=2):
    """the reference sweep: ``0``, ``C - 1``, a one-hot tensor per batch entry (``C - 1`` for entry 0, ``0`` for the others) and a
    mixed real vector"""
    one_hot = torch.zeros(lead, C)
    one_hot[0, C - 1] = 1
    one_hot[1:, 0] = 1
    return (0, C - 1, one_hot, torch.linspace(0.1, 1.0, C))


def ref_name(ref):
    return 'None' if ref is None else (str(ref) if isinstance(ref, int) else 'tensor%s' % (tuple(ref.shape),))


def norm2(m):
    return torch.linalg.matrix_norm(m.to(torch.complex128), ord=2)


def gap_ratio(psd_s):
    """``‖Φs‖₂ / (λ1 - λ2)`` per system, in float64"""
    lam = torch.linalg.eigvalsh(psd_s.to(torch.complex128))
    return lam.abs().amax(dim=-1) / (lam[..., -1] - lam[..., -2])


# ----------------------------------------------------------------------------- checks
def finite(z):
    return bool(torch.isfinite(torch.view_as_real(z)).all())


def assert_unit_vector(got, psd_s, what=''):
    """the gap-free checks of ``rtf_evd``: norm, convention, residual and Rayleigh quotient; ``got`` complex ``(…, F, C)``"""
    C = got.shape[-1]
    v, a = got.to(torch.complex128), psd_s.to(torch.complex128)
    assert finite(got), what
    assert float((torch.linalg.vector_norm(v, dim=-1) - 1).abs().max()) <= 4 * U, '%s: not a unit vector' % what
    mod = v.abs()
    marked = (got.imag == 0) & (got.real > 0) & (mod >= (1 - 4 * U) * mod.amax(dim=-1, keepdim=True))
    assert bool(marked.any(dim=-1).all()), '%s: no real positive component of largest modulus' % what
    av = torch.einsum('...ce,...e->...c', a, v)
    rho = torch.einsum('...c,...c->...', v.conj(), av).real
    scale = norm2(a)
    lam1 = torch.linalg.eigvalsh(a)[..., -1]
    res = torch.linalg.vector_norm(av - rho[..., None] * v, dim=-1)
    assert bool((res <= 4 * C * U * scale + R.TINY).all()), '%s: residual %.3g of its bound' % (
        what, float((res / (4 * C * U * scale + R.TINY)).max()))
    assert bool((rho >= lam1 - 8 * C * U * scale - R.TINY).all()), '%s: not the largest eigenvalue' % what


def assert_evd(got, psd_s, what='', cap=GAP_CAP):
    """``got`` against the restatement under the gap cap, after the gap-free checks; returns (worst error / bound, largest ratio)"""
    assert_unit_vector(got, psd_s, what)
    C = got.shape[-1]
    want = rtf_evd(psd_s)
    ratio = gap_ratio(psd_s)
    assert float(ratio.max()) <= cap, '%s: ‖Φs‖ / gap %.3g above the cap %g' % (what, float(ratio.max()), cap)
    g = got.to(torch.complex128)
    inner = torch.einsum('...c,...c->...', want.conj(), g)
    s = inner / inner.abs()
    bound = 3 * U * want.abs() + (64.0 * C ** 3 * 2.0 ** -53 * ratio)[..., None] + R.TINY
    worst = float(((g - s[..., None] * want).abs() / bound).max())
    assert worst <= 1.0, '%s: rtf_evd error is %.3g of its bound' % (what, worst)
    return worst, float(ratio.max())


def _componentwise(got, want, tail, what, name, k, cap):
    if cap is not None:
        assert float(k.max()) <= cap, '%s: condition number %.3g above the cap %g' % (what, float(k.max()), cap)
    assert finite(got), what
    diff = got.to(torch.complex128) - want
    bre, bim = U * want.real.abs() + tail[..., None] + R.TINY, U * want.imag.abs() + tail[..., None] + R.TINY
    worst = float(torch.maximum(diff.real.abs() / bre, diff.imag.abs() / bim).max())
    assert worst <= 1.0, '%s: %s error is %.3g of its bound (κ up to %.3g)' % (what, name, worst, float(k.max()))
    return worst, float(k.max())


def assert_power(got, psd_s, psd_n, reference_channel, n_iter, diagonal_loading=True, diag_eps=1e-7, what='', cap=R.KAPPA_CAP):
    C = got.shape[-1]
    want = rtf_power(psd_s, psd_n, reference_channel, n_iter, diagonal_loading, diag_eps)
    n = R.load(psd_n, diag_eps) if diagonal_loading else psd_n.to(torch.complex128)
    s = psd_s.to(torch.complex128)
    k = torch.linalg.cond(n)
    phi = torch.linalg.solve(n, s)
    ref_norm = 1.0
    if torch.is_tensor(reference_channel):
        ref_norm = torch.linalg.vector_norm(reference_channel.to(torch.float64), dim=-1)
        ref_norm = ref_norm[..., None] if ref_norm.dim() else float(ref_norm)
    tail = 64.0 * C ** 3 * n_iter * 2.0 ** -53 * k * norm2(s if n_iter >= 2 else n) * norm2(phi) ** (n_iter - 1) * ref_norm
    return _componentwise(got, want, tail, what, 'rtf_power', k, cap)


def assert_weights_rtf(got, rtf, psd_n, reference_channel, diagonal_loading=True, diag_eps=1e-7, eps=1e-8, what='', cap=R.KAPPA_CAP):
    C = got.shape[-1]
    want = mvdr_weights_rtf(rtf, psd_n, reference_channel, diagonal_loading, diag_eps, eps)
    k = R.kappa(psd_n, diagonal_loading, diag_eps)
    tail = 128.0 * C ** 3 * 2.0 ** -53 * k * want.abs().amax(dim=-1)
    return _componentwise(got, want, tail, what, 'mvdr_weights_rtf', k, cap)
