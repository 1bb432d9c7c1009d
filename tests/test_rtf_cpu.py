"""``rtf_evd`` / ``rtf_power`` / ``mvdr_weights_rtf`` / ``RTFMVDR`` on the CPU route (torch operators, ``_composite``) against the
complex128 restatement of tests/rtf_rules.py; known answers; argument errors; dtypes in and out; exports; gradients; and the
condition numbers and spectral gaps of every case tests/test_rtf_gpu.py holds to a bound."""
import os

import pytest
import torch

import beamform_rules as R
import rtf_rules as RT


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


def rel(got, want):
    return float((got.to(torch.complex128) - want).abs().max()) / (float(want.abs().max()) + 1e-300)


def aligned(got, want):
    """``want`` rotated onto ``got`` by the unit phase of ``wantᴴ got``"""
    inner = torch.einsum('...c,...c->...', want.conj(), got.to(torch.complex128))
    return want * (inner / inner.abs())[..., None]


def randc(g, *shape):
    return torch.complex(torch.randn(*shape, generator=g, dtype=torch.float64), torch.randn(*shape, generator=g, dtype=torch.float64))


def test_names(tac):
    for name in ('rtf_evd', 'rtf_power', 'mvdr_weights_rtf'):
        assert name in tac.functional.__all__ and getattr(tac, name) is getattr(tac.functional, name)
    assert tac.RTFMVDR is tac.layers.RTFMVDR and not tac.RTFMVDR().state_dict()
    for op in ('rtf_evd', 'rtf_power', 'mvdr_weights_rtf', 'rtf_mvdr'):
        assert op in tac._ops.cuda_kernels and hasattr(torch.ops.tac_amd, op)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tac_amd.h')) as f:
        header = f.read()
    for name in ('tac_rtf_evd_f32', 'tac_rtf_power_f32', 'tac_mvdr_weights_rtf_f32', 'tac_rtf_mvdr_f32', 'tac_rtf_power_max_iter'):
        assert name in tac._native.EXPORTS and ' %s(' % name in header


def test_plan_mirror(tac):
    assert tac._hip.rtf_power_max_iter() == RT.MAX_ITER == 64


def test_composite_against_the_restatement(tac):
    x, ps, pn = RT.psds(4, 9, 33, seed=1)
    ps, pn = ps.to(torch.complex128), pn.to(torch.complex128)
    got = tac.rtf_evd(ps)
    assert got.dtype == torch.complex128 and tuple(got.shape) == (2, 9, 4)
    assert rel(got, RT.rtf_evd(ps)) <= 1e-12
    RT.assert_unit_vector(got.to(torch.complex64), ps.to(torch.complex64).to(torch.complex128))
    u = torch.zeros(2, 4, dtype=torch.float64)
    u[:, 2] = 1
    mix = torch.tensor([0.25, 0.5, 0.0, 0.25], dtype=torch.float64)
    for ref in (0, 3, -1, u, mix):
        for loading in (True, False):
            for n_iter in RT.N_ITERS:
                got = tac.rtf_power(ps, pn, ref, n_iter=n_iter, diagonal_loading=loading)
                assert got.dtype == torch.complex128 and tuple(got.shape) == (2, 9, 4)
                assert rel(got, RT.rtf_power(ps, pn, ref, n_iter, loading)) <= 1e-12, (ref, loading, n_iter)
    assert torch.equal(tac.rtf_power(ps, pn, 2), tac.rtf_power(ps, pn, u))
    d = RT.rtf_evd(ps)
    for ref in (None, 0, 3, -1, u, mix):
        for loading in (True, False):
            got = tac.mvdr_weights_rtf(d, pn, ref, diagonal_loading=loading)
            assert got.dtype == torch.complex128 and tuple(got.shape) == (2, 9, 4)
            assert rel(got, RT.mvdr_weights_rtf(d, pn, ref, loading)) <= 1e-12, (ref, loading)
    y = tac.RTFMVDR()(x.to(torch.complex128), d, pn, 1)
    assert y.dtype == torch.complex128 and tuple(y.shape) == (2, 9, 33)
    assert rel(y, RT.rtf_mvdr(x, d, pn, 1)) <= 1e-12
    # complex64 in, complex64 out
    got = tac.mvdr_weights_rtf(d.to(torch.complex64), pn.to(torch.complex64), 0)
    assert got.dtype == torch.complex64 and rel(got, RT.mvdr_weights_rtf(d.to(torch.complex64), pn.to(torch.complex64), 0)) <= 1e-3


def test_known_answers(tac):
    g = torch.Generator().manual_seed(5)
    C, F = 5, 7
    a = randc(g, F, C)
    unit = a / torch.linalg.vector_norm(a, dim=-1, keepdim=True)
    eye = torch.eye(C, dtype=torch.complex128).expand(F, C, C).contiguous()
    rank_one = a[:, :, None] * a.conj()[:, None, :]
    # Φs = a aᴴ + σ I: the principal eigenvector is a / |a|
    for fn in (RT.rtf_evd, tac.rtf_evd):
        got = fn(rank_one + 0.3 * eye)
        assert float((got - aligned(got, unit)).abs().max()) <= 1e-13
        assert float((got - RT.lead_phase(unit)).abs().max()) <= 1e-13, 'the phase convention'
    # Φn = I, Φs = a aᴴ: every power iterate is a multiple of a
    for n_iter in RT.N_ITERS:
        for fn in (RT.rtf_power, tac.rtf_power):
            got = fn(rank_one, eye, 1, n_iter=n_iter, diagonal_loading=False)
            got = got / torch.linalg.vector_norm(got, dim=-1, keepdim=True)
            assert float((got - aligned(got, unit)).abs().max()) <= 1e-13, n_iter
    # Φn = I, no loading, eps = 0: w = d conj(d_r) / |d|², and wᴴ d = d_r
    for r in (0, 3):
        want = a * a[:, r:r + 1].conj() / (a.abs() ** 2).sum(-1, keepdim=True)
        for fn in (RT.mvdr_weights_rtf, tac.mvdr_weights_rtf):
            w = fn(a, eye, r, diagonal_loading=False, eps=0.0)
            assert float((w - want).abs().max()) <= 1e-13
            assert float(((w.conj() * a).sum(-1) - a[:, r]).abs().max()) <= 1e-13


def test_the_weights_do_not_depend_on_the_phase_of_the_rtf(tac):
    g = torch.Generator().manual_seed(6)
    x, ps, pn = RT.psds(3, 5, 20, seed=2)
    pn = pn.to(torch.complex128)
    d = randc(g, 2, 5, 3)
    theta = torch.rand(2, 5, 1, generator=g, dtype=torch.float64) * 6.28
    turned = d * torch.polar(torch.ones_like(theta), theta)
    for ref in (0, 2, torch.tensor([0.5, 0.2, 0.3], dtype=torch.float64)):
        assert rel(tac.mvdr_weights_rtf(turned, pn, ref), tac.mvdr_weights_rtf(d, pn, ref)) <= 1e-13


def test_errors(tac):
    x, ps, pn = RT.psds(3, 5, 12, seed=4)
    d = tac.rtf_evd(ps)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            tac.rtf_power(ps, pn, 0, n_iter=bad)
    with pytest.raises(ValueError):
        tac.rtf_power(ps, pn[:, :-1], 0)
    with pytest.raises(ValueError):
        tac.rtf_power(ps, pn, 3)
    with pytest.raises(TypeError):
        tac.rtf_power(ps, pn, 0.5)
    with pytest.raises(ValueError):
        tac.rtf_power(ps, pn, torch.ones(4))
    with pytest.raises(ValueError):
        tac.rtf_power(ps, pn, torch.ones(3, dtype=torch.complex64))
    with pytest.raises(ValueError):
        tac.rtf_evd(ps[..., :-1])                                            # not square
    with pytest.raises(ValueError):
        tac.rtf_evd(ps.real)                                                 # real, and not pairs
    with pytest.raises(ValueError):
        tac.mvdr_weights_rtf(d[:, :-1], pn, 0)
    with pytest.raises(ValueError):
        tac.mvdr_weights_rtf(d, pn, 3)
    with pytest.raises(TypeError):
        tac.mvdr_weights_rtf(d, pn, 0.5)
    with pytest.raises(ValueError):
        tac.mvdr_weights_rtf(d, pn, torch.ones(3, dtype=torch.complex64))
    with pytest.raises(ValueError):
        tac.RTFMVDR()(x, d[:, :-1], pn, 0)
    with pytest.raises(ValueError):
        tac.RTFMVDR()(x, d, pn, 3)
    with pytest.raises(ValueError):
        tac.RTFMVDR()(x[:, :2], d, pn, 0)


def test_pairs_in_pairs_out(tac):
    x, ps, pn = RT.psds(3, 5, 12, seed=2, lead=())
    psp, pnp = torch.view_as_real(ps), torch.view_as_real(pn)
    d = tac.rtf_evd(psp)
    assert d.dtype == torch.float32 and tuple(d.shape) == (5, 3, 2)
    assert torch.equal(torch.view_as_complex(d.contiguous()), tac.rtf_evd(ps))
    r = tac.rtf_power(psp, pnp, 1)
    assert r.dtype == torch.float32 and tuple(r.shape) == (5, 3, 2)
    assert torch.equal(torch.view_as_complex(r.contiguous()), tac.rtf_power(ps, pn, 1))
    w = tac.mvdr_weights_rtf(d, pnp, 1)
    assert w.dtype == torch.float32 and tuple(w.shape) == (5, 3, 2)
    assert torch.equal(torch.view_as_complex(w.contiguous()), tac.mvdr_weights_rtf(torch.view_as_complex(d.contiguous()), pn, 1))
    y = tac.RTFMVDR()(torch.view_as_real(x), d, pnp, 1)
    assert y.dtype == torch.float32 and tuple(y.shape) == (5, 12, 2) and y.transpose(-3, -2).is_contiguous()
    assert torch.equal(torch.view_as_complex(y.contiguous()), tac.RTFMVDR()(x, torch.view_as_complex(d.contiguous()), pn, 1))


def test_gradients_flow_through_rtfmvdr(tac):
    x, ps, pn = RT.psds(2, 3, 8, seed=6, lead=())
    xp = torch.view_as_real(x).clone().requires_grad_(True)
    d = torch.view_as_real(tac.rtf_power(ps, pn, 0)).clone().requires_grad_(True)
    n = torch.view_as_real(pn).clone().requires_grad_(True)
    tac.RTFMVDR()(xp, d, n, 0).square().sum().backward()
    for t in (xp, d, n):
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0
    s = torch.view_as_real(ps).clone().requires_grad_(True)
    tac.rtf_evd(s).square()[..., 0, :].sum().backward()
    tac.rtf_power(s, n, 0).square().sum().backward()
    assert s.grad is not None and bool(torch.isfinite(s.grad).all())


def test_conditions_of_the_gpu_cases():
    """every case tests/test_rtf_gpu.py holds to a bound keeps the loaded ``Φn`` under the condition cap and ``Φs`` under the gap
    cap; the rank-deficient case does neither and is held to finiteness only"""
    for C, F, T in R.WEIGHT_CASES:
        x, ps, pn = RT.psds(C, F, T, seed=11)
        for loading in (True, False):
            assert float(R.kappa(pn, loading).max()) <= R.KAPPA_CAP, (C, F, T)
        assert float(RT.gap_ratio(ps).max()) <= RT.GAP_CAP, (C, F, T)
    for C, F, T in R.FUSED_CASES:
        x, ps, pn = RT.psds(C, F, T, seed=8)
        assert float(R.kappa(pn).max()) <= R.KAPPA_CAP, (C, F, T)
    C, F, T = 4, 129, 257                                                     # the end-to-end case: its PSDs come from the kernels
    x, ps, pn = RT.psds(C, F, T, seed=12)
    assert float(R.kappa(pn).max()) <= R.KAPPA_CAP and float(RT.gap_ratio(ps).max()) <= RT.GAP_CAP
    C, F, T = R.RANK_DEFICIENT
    x, ps, pn = RT.psds(C, F, T, seed=11)
    assert float(R.kappa(pn).max()) > 1e5
    assert RT.finite(RT.rtf_power(ps, pn, 0)) and RT.finite(RT.mvdr_weights_rtf(RT.rtf_evd(ps), pn, 0))
