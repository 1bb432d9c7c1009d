"""Rules of the beamforming tests: the complex128 restatement of torchaudio's ``psd`` / ``mvdr_weights_souden`` /
``apply_beamforming`` / ``MVDR`` (torchaudio is not a dependency: the definitions are restated literally), the signal generator and
the error bounds the float32 kernels of csrc/beamform.hip are held to.

Notation: a spectrogram ``X[…, c, f, t]`` complex with ``C`` channels; ``u = 2^-24`` the float32 unit roundoff; ``γ_n = n u / (1 -
n u)``.

psd bound.  ``|ΔΦ[f, c, e]| <= γ_(T+8) Σ_t m'_t |X_c,t| |X_e,t|`` per real component: Higham's bound for a float32 sum of ``T`` terms
in any order, plus the roundings of the complex product, the mask product and the normalisation; evaluated in float64.

weights bound.  Against the restatement fed the SAME float32 PSDs: ``|Δw| <= u |w| + 64 C^3 2^-53 κ max_c |w_c|`` per real
component, ``κ`` the float64 2-norm condition number of the loaded ``Φn``: one rounding to float32, plus the bound of a float64
elimination with partial pivoting.  The main inputs keep ``κ <= KAPPA_CAP``.

apply bound.  ``|ΔY| <= γ_(2C+2) Σ_c |w_c| |X_c|`` per real component: a chain of ``2 C`` fused multiply-adds.

Every bound gets a floor of a few float32 subnormals (``TINY``) so that exact zeros compare."""
import torch

U = 2.0 ** -24
KAPPA_CAP = 1e3
TINY = 1e-44

#: the shapes the GPU sweep runs: channels, bins, frames
CHANNELS = (2, 3, 5, 8)
BINS = (1, 63, 65, 129)
FRAMES = (1, 2, 31, 257)

#: (C, F, T) of the cases held to the weights bound under the condition-number cap, and the rank-deficient case (T < C)
WEIGHT_CASES = ((2, 63, 33), (3, 65, 33), (5, 129, 64), (8, 65, 257))
RANK_DEFICIENT = (6, 65, 2)
#: (C, F, T) of the end-to-end cases: their PSDs come from the kernels, with mask_n given and as the complement of mask_s
FUSED_CASES = ((4, 129, 257), (8, 65, 300), (2, 63, 33))

#: mirrors of csrc/beamform.hip (tac_psd_plan, tac_beamform_grid)
CHUNK = 64
AP_FRAMES = 32
WAVES = 4


def gamma(n):
    return n * U / (1.0 - n * U)


def ceil_div(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------- the restatement (float64 / complex128)
def psd(specgram, mask=None, normalize=True, eps=1e-10):
    """``(…, C, F, T)`` complex128 → ``(…, F, C, C)``: ``Φ[f, c, e] = Σ_t m'[f, t] X[c, f, t] conj(X[e, f, t])``"""
    x = specgram.to(torch.complex128).transpose(-3, -2)                      # (…, F, C, T)
    outer = torch.einsum('...ct,...et->...tce', x, x.conj())                # (…, F, T, C, C)
    if mask is not None:
        m = mask.to(torch.float64)
        if normalize:
            m = m / (m.sum(dim=-1, keepdim=True) + eps)
        outer = outer * m[..., None, None]
    return outer.sum(dim=-3)


def load(psd_n, diag_eps=1e-7):
    """``Φn + (diag_eps Re tr Φn + 1e-8) I`` — the inner 1e-8 is fixed"""
    n = psd_n.to(torch.complex128)
    trace = n.diagonal(dim1=-1, dim2=-2).sum(-1).real[..., None, None]
    return n + (diag_eps * trace + 1e-8) * torch.eye(n.shape[-1], dtype=n.dtype)


def mvdr_weights_souden(psd_s, psd_n, reference_channel, diagonal_loading=True, diag_eps=1e-7, eps=1e-8):
    """two ``(…, F, C, C)`` → ``(…, F, C)``: ``N = Φn^-1 Φs`` by a solve, ``W = N / (tr N + eps)`` with the complex trace, column
    ``r`` for an int, ``Σ_c W[:, c] u[c]`` for a tensor"""
    s, n = psd_s.to(torch.complex128), psd_n.to(torch.complex128)
    if diagonal_loading:
        n = load(n, diag_eps)
    numerator = torch.linalg.solve(n, s)
    ws = numerator / (numerator.diagonal(dim1=-1, dim2=-2).sum(-1)[..., None, None] + eps)
    if torch.is_tensor(reference_channel):
        return torch.einsum('...fec,...c->...fe', ws, reference_channel.to(torch.complex128))
    return ws[..., :, reference_channel]


def apply_beamforming(weights, specgram):
    """``Y[f, t] = Σ_c conj(w[f, c]) X[c, f, t]``"""
    return torch.einsum('...fc,...cft->...ft', weights.to(torch.complex128).conj(), specgram.to(torch.complex128))


def mvdr(specgram, mask_s, mask_n=None, ref_channel=0, diag_loading=True, diag_eps=1e-7, multi_mask=False):
    """the ``MVDR`` layer at ``solution='ref_channel'``; PSDs with ``normalize=True, eps=1e-15``"""
    if mask_n is None:
        mask_n = 1 - mask_s
    if multi_mask:
        mask_s, mask_n = mask_s.mean(dim=-3), mask_n.mean(dim=-3)
    w = mvdr_weights_souden(psd(specgram, mask_s, True, 1e-15), psd(specgram, mask_n, True, 1e-15), ref_channel, diag_loading, diag_eps)
    return apply_beamforming(w, specgram)


def kappa(psd_n, diagonal_loading=True, diag_eps=1e-7):
    """the float64 2-norm condition number of the (loaded) ``Φn``, per system"""
    n = load(psd_n, diag_eps) if diagonal_loading else psd_n.to(torch.complex128)
    return torch.linalg.cond(n)


# ----------------------------------------------------------------------------- signals
def scene(lead, C, F, T, seed=0):
    """``(X complex64 (lead, C, F, T), mask_s, mask_n float32 (lead, F, T))``: one source through a random steering vector per
    (entry, bin) plus white noise at 0.3 of its level, and random masks in (0, 1)"""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * C + 31 * F + T)
    lead = tuple(lead)

    def cplx(*shape):
        return torch.complex(torch.randn(*shape, generator=g, dtype=torch.float64), torch.randn(*shape, generator=g, dtype=torch.float64))

    steer = cplx(*lead, C, F, 1)
    source = cplx(*lead, 1, F, T)
    noise = cplx(*lead, C, F, T)
    x = (steer * source + 0.3 * noise).to(torch.complex64)
    mask_s = (0.02 + 0.96 * torch.rand(*lead, F, T, generator=g, dtype=torch.float64)).to(torch.float32)
    mask_n = (0.02 + 0.96 * torch.rand(*lead, F, T, generator=g, dtype=torch.float64)).to(torch.float32)
    return x, mask_s, mask_n


def frame_major(x_pairs):
    """a ``(…, F, T, 2)`` tensor re-laid frame-major: the same values as the view ``stft`` returns"""
    return x_pairs.transpose(-3, -2).contiguous().transpose(-3, -2)


# ----------------------------------------------------------------------------- bounds
def psd_bound(specgram, mask=None, normalize=True, eps=1e-10):
    """``γ_(T+8) Σ_t m'_t |X_c,t| |X_e,t|``, real ``(…, F, C, C)``"""
    a = specgram.to(torch.complex128).abs().transpose(-3, -2)                # (…, F, C, T)
    T = a.shape[-1]
    if mask is not None:
        m = mask.to(torch.float64).abs()
        if normalize:
            m = m / (mask.to(torch.float64).sum(dim=-1, keepdim=True) + eps).abs()
        total = torch.einsum('...ct,...et,...t->...ce', a, a, m)
    else:
        total = torch.einsum('...ct,...et->...ce', a, a)
    return gamma(T + 8) * total + TINY


def assert_psd(got, specgram, mask=None, normalize=True, eps=1e-10, what=''):
    """``got``: complex ``(…, F, C, C)`` from the kernels; returns the worst error / bound"""
    want = psd(specgram, mask, normalize, eps)
    bound = psd_bound(specgram, mask, normalize, eps)
    diff = got.to(torch.complex128) - want
    worst = float(torch.maximum(diff.real.abs() / bound, diff.imag.abs() / bound).max())
    assert bool(torch.isfinite(got.real).all() and torch.isfinite(got.imag).all()), what
    assert worst <= 1.0, '%s: psd error is %.3g of its bound' % (what, worst)
    return worst


def weights_bound(want, psd_n32, diagonal_loading=True, diag_eps=1e-7):
    """``u |w| + 64 C^3 2^-53 κ max_c |w_c|`` per real component: ``(bound re, bound im, κ)``"""
    C = want.shape[-1]
    k = kappa(psd_n32, diagonal_loading, diag_eps)
    tail = 64.0 * C ** 3 * 2.0 ** -53 * k * want.abs().amax(dim=-1)
    return U * want.real.abs() + tail[..., None] + TINY, U * want.imag.abs() + tail[..., None] + TINY, k


def assert_weights(got, psd_s32, psd_n32, reference_channel, diagonal_loading=True, diag_eps=1e-7, eps=1e-8, what='', cap=KAPPA_CAP):
    """``got`` complex ``(…, F, C)`` against the restatement fed the same float32 PSDs; returns (worst error / bound, largest κ)"""
    want = mvdr_weights_souden(psd_s32, psd_n32, reference_channel, diagonal_loading, diag_eps, eps)
    bre, bim, k = weights_bound(want, psd_n32, diagonal_loading, diag_eps)
    if cap is not None:
        assert float(k.max()) <= cap, '%s: condition number %.3g above the cap %g' % (what, float(k.max()), cap)
    diff = got.to(torch.complex128) - want
    worst = float(torch.maximum(diff.real.abs() / bre, diff.imag.abs() / bim).max())
    assert bool(torch.isfinite(got.real).all() and torch.isfinite(got.imag).all()), what
    assert worst <= 1.0, '%s: weights error is %.3g of its bound (κ up to %.3g)' % (what, worst, float(k.max()))
    return worst, float(k.max())


def apply_bound(weights, specgram):
    """``γ_(2C+2) Σ_c |w_c| |X_c|``, real ``(…, F, T)``"""
    C = weights.shape[-1]
    return gamma(2 * C + 2) * torch.einsum('...fc,...cft->...ft', weights.to(torch.complex128).abs(),
                                           specgram.to(torch.complex128).abs()) + TINY


def assert_apply(got, weights, specgram, what=''):
    want = apply_beamforming(weights, specgram)
    bound = apply_bound(weights, specgram)
    diff = got.to(torch.complex128) - want
    worst = float(torch.maximum(diff.real.abs() / bound, diff.imag.abs() / bound).max())
    assert worst <= 1.0, '%s: apply error is %.3g of its bound' % (what, worst)
    return worst


# ----------------------------------------------------------------------------- launch geometry (csrc/beamform.hip)
def psd_plan(frames):
    """``(frames of a piece, pieces)``: time is cut into pieces of ``CHUNK`` frames whatever the batch, so that a system's sums do
    not depend on what else is in the call"""
    return CHUNK, ceil_div(frames, CHUNK)


def psd_units(systems, frames, cus):
    """``(workgroup units, grid)`` of the PSD launch: a wave takes 64 systems over one piece, a workgroup ``WAVES`` of them; the
    persistent grid holds two workgroups a CU"""
    _, pieces = psd_plan(frames)
    return ceil_div(ceil_div(systems, 64) * pieces, WAVES), 2 * cus


def apply_units(systems, frames, cus):
    """``(workgroup units, grid)`` of the apply launch: a wave takes 64 systems over ``AP_FRAMES`` frames; eight workgroups a CU"""
    return ceil_div(ceil_div(systems, 64) * ceil_div(frames, AP_FRAMES), WAVES), 8 * cus
