"""-m gpu: ``rtf_evd`` / ``rtf_power`` / ``mvdr_weights_rtf`` / ``RTFMVDR`` on the gfx950 kernels (csrc/beamform.hip) — strict mode and
poisoned outputs on, as in tests/test_beamform_gpu.py.

Reference and bounds: tests/rtf_rules.py — the complex128 restatement fed the SAME float32 PSDs and RTFs, and the derived bounds.
The fused entry is held to the bits of the two entries called by themselves, which are held to the bounds."""
import warnings

import pytest
import torch

import beamform_rules as R
import rtf_rules as RT

pytestmark = pytest.mark.gpu

EVD, POWER, WEIGHTS, FUSED = 'tac_rtf_evd_f32', 'tac_rtf_power_f32', 'tac_mvdr_weights_rtf_f32', 'tac_rtf_mvdr_f32'
PSD, APPLY = 'tac_psd_f32', 'tac_apply_beamforming_f32'
SWEEP_BINS = (1, 63, 65, 129)          # 2 F systems: a lone pair, a tile of 16 cut short, a tile that straddles the batch entries


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    t._native.lib()
    t.set_strict(True)
    t._hip.set_poison_outputs(True)
    yield t
    t._hip.set_poison_outputs(False)
    t.set_strict(False)
    t.set_lazy_fusion(True)


@pytest.fixture(autouse=True)
def every_output_written(tac):
    tac._hip.poison_report()
    yield
    left = tac._hip.poison_report()
    assert not left, 'kernel outputs left unwritten (poisoned elements per entry point): %r' % left


def launched_since(tac_, before):
    now = tac_._hip.launches
    return {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)}


def one(tac_, entry, fn, *args, **kw):
    before = dict(tac_._hip.launches)
    out = fn(*args, **kw)
    assert launched_since(tac_, before) == {entry: 1}, (entry, launched_since(tac_, before))
    return out


def fm(z):
    """a complex ``(…, F, T)`` tensor re-laid frame-major (bins of a frame contiguous): the layout ``stft`` returns"""
    return z.transpose(-2, -1).contiguous().transpose(-2, -1)


def dev(ref):
    return ref.cuda() if torch.is_tensor(ref) else ref


_cases = {}


def case(C, F, T):
    """``(X, Φs, Φn, rtf)`` of a case, float32 on the host, made once and left unchanged"""
    if (C, F, T) not in _cases:
        x, ps, pn = RT.psds(C, F, T, seed=11)
        _cases[(C, F, T)] = (x, ps, pn, RT.rtf_evd(ps).to(torch.complex64))
    return _cases[(C, F, T)]


# ----------------------------------------------------------------------------- 1. rtf_evd
@pytest.mark.parametrize('C,F,T', R.WEIGHT_CASES)
def test_evd_bound(tac, C, F, T):
    x, ps, pn, _ = case(C, F, T)
    psd_ = ps.cuda()
    got = one(tac, EVD, tac.rtf_evd, psd_)
    assert got.dtype == torch.complex64 and tuple(got.shape) == (2, F, C)
    worst, ratio = RT.assert_evd(got.cpu(), ps, 'C %d, F %d' % (C, F))
    print('C %d, F %d: worst rtf_evd error %.3f of its bound, ‖Φs‖ / gap up to %.2f' % (C, F, worst, ratio))
    pairs = one(tac, EVD, tac.rtf_evd, torch.view_as_real(psd_))
    assert pairs.dtype == torch.float32 and torch.equal(torch.view_as_complex(pairs), got)


@pytest.mark.parametrize('C', R.CHANNELS)
def test_evd_sweep(tac, C):
    for F in SWEEP_BINS:
        x, ps, pn = RT.psds(C, F, 40, seed=13)
        got = one(tac, EVD, tac.rtf_evd, ps.cuda())
        assert tuple(got.shape) == (2, F, C)
        RT.assert_evd(got.cpu(), ps, 'C %d, F %d' % (C, F), cap=float('inf'))     # (the bound carries each system's own gap)


@pytest.mark.parametrize('C', R.CHANNELS)
def test_evd_degenerate(tac, C):
    """no spectral gap: zero, identity, exactly rank one; and one system of NaNs among clean ones"""
    F = 21
    g = torch.Generator().manual_seed(C)
    a = torch.complex(torch.randint(-3, 4, (F, C), generator=g).float(), torch.randint(-3, 4, (F, C), generator=g).float())
    a[:, 0] += 1 + 4j                                                          # (never the zero vector)
    eye = torch.eye(C, dtype=torch.complex64).expand(F, C, C).contiguous()
    rank_one = a[:, :, None] * a.conj()[:, None, :]                            # small integers: exact in float32, Hermitian to the bit
    assert torch.equal(rank_one, rank_one.conj().transpose(-2, -1).resolve_conj())
    for name, p in (('zero', torch.zeros(F, C, C, dtype=torch.complex64)), ('identity', eye), ('rank one', rank_one),
                    ('identity scaled', 3e-20 * eye), ('two equal largest', eye * (torch.arange(C) < 2).to(torch.complex64))):
        got = one(tac, EVD, tac.rtf_evd, p.cuda()).cpu()
        RT.assert_unit_vector(got, p, '%s, C %d' % (name, C))
    x, ps, pn = RT.psds(C, F, 40, seed=14)
    clean = tac.rtf_evd(ps.cuda())
    bad = ps.clone()
    bad[1, 17, C - 1, 0] = float('nan')
    got = tac.rtf_evd(bad.cuda())
    keep = torch.ones(2, F, dtype=torch.bool, device='cuda')
    keep[1, 17] = False
    assert torch.equal(torch.view_as_real(got)[keep], torch.view_as_real(clean)[keep]), 'a system without the NaN changed'
    assert bool(torch.isnan(torch.view_as_real(got)[1, 17]).all())


# ----------------------------------------------------------------------------- 2. rtf_power
@pytest.mark.parametrize('C,F,T', R.WEIGHT_CASES)
def test_power_bound(tac, C, F, T):
    x, ps, pn, _ = case(C, F, T)
    psd_, pnd = ps.cuda(), pn.cuda()
    worst = 0.0
    for ref in RT.references(C):
        for loading in (True, False):
            for n_iter in RT.N_ITERS:
                what = 'C %d, F %d, ref %s, loading %s, n_iter %d' % (C, F, RT.ref_name(ref), loading, n_iter)
                got = one(tac, POWER, tac.rtf_power, psd_, pnd, dev(ref), n_iter=n_iter, diagonal_loading=loading)
                assert got.dtype == torch.complex64 and tuple(got.shape) == (2, F, C)
                w, k = RT.assert_power(got.cpu(), ps, pn, ref, n_iter, loading, what=what)
                worst = max(worst, w)
    print('C %d, F %d: worst rtf_power error %.3g of its bound, κ up to %.0f' % (C, F, worst, k))
    one_hot = RT.references(C)[2].cuda()
    for n_iter in RT.N_ITERS:
        by_vector = tac.rtf_power(psd_, pnd, one_hot, n_iter=n_iter)
        assert torch.equal(by_vector[0], tac.rtf_power(psd_, pnd, C - 1, n_iter=n_iter)[0])
        assert torch.equal(by_vector[1], tac.rtf_power(psd_, pnd, 0, n_iter=n_iter)[1])
    pairs = one(tac, POWER, tac.rtf_power, torch.view_as_real(psd_), torch.view_as_real(pnd), 0)
    assert pairs.dtype == torch.float32 and torch.equal(torch.view_as_complex(pairs), tac.rtf_power(psd_, pnd, 0))


@pytest.mark.parametrize('C', R.CHANNELS)
def test_power_sweep(tac, C):
    worst = 0.0
    for F in SWEEP_BINS:
        x, ps, pn = RT.psds(C, F, 40, seed=13)
        for ref in (C - 1, RT.references(C)[3]):
            for n_iter in (1, 3):
                got = one(tac, POWER, tac.rtf_power, ps.cuda(), pn.cuda(), dev(ref), n_iter=n_iter)
                worst = max(worst, RT.assert_power(got.cpu(), ps, pn, ref, n_iter, what='C %d, F %d' % (C, F), cap=None)[0])
    print('C %d: worst rtf_power error %.3g of its bound over the bin sweep' % (C, worst))


# ----------------------------------------------------------------------------- 3. mvdr_weights_rtf
@pytest.mark.parametrize('C,F,T', R.WEIGHT_CASES)
def test_weights_bound(tac, C, F, T):
    x, ps, pn, d = case(C, F, T)
    dd, pnd = d.cuda(), pn.cuda()
    worst = 0.0
    for ref in RT.references(C) + (None,):
        for loading in (True, False):
            what = 'C %d, F %d, ref %s, loading %s' % (C, F, RT.ref_name(ref), loading)
            got = one(tac, WEIGHTS, tac.mvdr_weights_rtf, dd, pnd, dev(ref), diagonal_loading=loading)
            assert got.dtype == torch.complex64 and tuple(got.shape) == (2, F, C)
            w, k = RT.assert_weights_rtf(got.cpu(), d, pn, ref, loading, what=what)
            worst = max(worst, w)
    print('C %d, F %d: worst mvdr_weights_rtf error %.3g of its bound, κ up to %.0f' % (C, F, worst, k))
    by_vector = tac.mvdr_weights_rtf(dd, pnd, RT.references(C)[2].cuda())
    assert torch.equal(by_vector[0], tac.mvdr_weights_rtf(dd, pnd, C - 1)[0])
    assert torch.equal(by_vector[1], tac.mvdr_weights_rtf(dd, pnd, 0)[1])
    pairs = one(tac, WEIGHTS, tac.mvdr_weights_rtf, torch.view_as_real(dd), torch.view_as_real(pnd), 0)
    assert pairs.dtype == torch.float32 and torch.equal(torch.view_as_complex(pairs), tac.mvdr_weights_rtf(dd, pnd, 0))


@pytest.mark.parametrize('C', R.CHANNELS)
def test_weights_sweep(tac, C):
    worst = 0.0
    for F in SWEEP_BINS:
        x, ps, pn = RT.psds(C, F, 40, seed=13)
        d = RT.rtf_power(ps, pn, 0).to(torch.complex64)
        for ref in (None, C - 1, RT.references(C)[3]):
            got = one(tac, WEIGHTS, tac.mvdr_weights_rtf, d.cuda(), pn.cuda(), dev(ref))
            worst = max(worst, RT.assert_weights_rtf(got.cpu(), d, pn, ref, what='C %d, F %d' % (C, F), cap=None)[0])
    print('C %d: worst mvdr_weights_rtf error %.3g of its bound over the bin sweep' % (C, worst))


def test_rank_deficient(tac):
    """``T < C``: ``κ`` near 1e7 — held to finiteness only"""
    C, F, T = R.RANK_DEFICIENT
    x, ps, pn = RT.psds(C, F, T, seed=11)
    d = one(tac, EVD, tac.rtf_evd, ps.cuda())
    RT.assert_unit_vector(d.cpu(), ps, 'rank-deficient')
    for got in (one(tac, POWER, tac.rtf_power, ps.cuda(), pn.cuda(), 0), one(tac, WEIGHTS, tac.mvdr_weights_rtf, d, pn.cuda(), 0)):
        assert RT.finite(got)


# ----------------------------------------------------------------------------- 4. batch independence
@pytest.mark.parametrize('C', (3, 8))
def test_a_system_does_not_depend_on_the_batch(tac, C):
    F = 37
    x, ps, pn = RT.psds(C, F, 40, seed=15)
    psd_, pnd = ps.cuda(), pn.cuda()
    u = RT.references(C)[3].cuda()
    calls = {
        'rtf_evd': lambda s, n, d: tac.rtf_evd(s),
        'rtf_power': lambda s, n, d: tac.rtf_power(s, n, u, n_iter=3),
        'mvdr_weights_rtf': lambda s, n, d: tac.mvdr_weights_rtf(d, n, 1),
    }
    dd = tac.rtf_evd(psd_)
    for name, call in calls.items():
        whole = call(psd_, pnd, dd)
        assert torch.equal(whole, call(psd_, pnd, dd)), name + ': two calls differ'
        for b, f in ((0, 0), (0, 17), (1, 20), (1, F - 1)):
            alone = call(psd_[b:b + 1, f:f + 1].contiguous(), pnd[b:b + 1, f:f + 1].contiguous(), dd[b:b + 1, f:f + 1].contiguous())
            assert torch.equal(alone[0, 0], whole[b, f]), '%s: system (%d, %d) alone differs from its bits in the batch' % (name, b, f)


def test_a_nan_reaches_only_its_system(tac):
    C, F = 5, 37
    x, ps, pn = RT.psds(C, F, 40, seed=16)
    d = tac.rtf_evd(ps.cuda())
    bad = pn.clone()
    bad[0, 30, 2, 1] = float('nan')
    keep = torch.ones(2, F, dtype=torch.bool, device='cuda')
    keep[0, 30] = False
    for clean, got in ((tac.rtf_power(ps.cuda(), pn.cuda(), 0), tac.rtf_power(ps.cuda(), bad.cuda(), 0)),
                       (tac.mvdr_weights_rtf(d, pn.cuda(), 0), tac.mvdr_weights_rtf(d, bad.cuda(), 0))):
        assert torch.equal(torch.view_as_real(got)[keep], torch.view_as_real(clean)[keep])
        assert bool(torch.isnan(torch.view_as_real(got)[0, 30]).any())


# ----------------------------------------------------------------------------- 5. RTFMVDR
@pytest.mark.parametrize('C,F,T', R.FUSED_CASES)
def test_fused_entry(tac, C, F, T):
    x, ps, pn = RT.psds(C, F, T, seed=8)
    d = RT.rtf_evd(ps).to(torch.complex64)
    xd, dd, pnd = fm(x.cuda()), d.cuda(), pn.cuda()
    xp = torch.view_as_real(xd)
    layout = dict(tac._hip.beamform_layout)
    for ref in (1, RT.references(C)[3], None):
        what = 'C %d, ref %s' % (C, RT.ref_name(ref))
        got = one(tac, FUSED, tac.RTFMVDR(), xd, dd, pnd, dev(ref))
        assert got.dtype == torch.complex64 and tuple(got.shape) == (2, F, T) and got.transpose(-2, -1).is_contiguous()
        w = one(tac, WEIGHTS, tac.mvdr_weights_rtf, dd, pnd, dev(ref))
        y = one(tac, APPLY, tac.apply_beamforming, w, xd)
        assert torch.equal(y, got), what
        vector, channel = (dev(ref), 0) if torch.is_tensor(ref) else (None, -1 if ref is None else ref)
        fused_y, fused_w = tac._hip.rtf_mvdr(xp, torch.view_as_real(dd), torch.view_as_real(pnd), vector, channel, True, 1e-7, 1e-8)
        assert torch.equal(torch.view_as_complex(fused_w), w) and torch.equal(torch.view_as_complex(fused_y), got), what
        RT.assert_weights_rtf(w.cpu(), d, pn, ref, what=what)
        R.assert_apply(got.cpu(), w.cpu(), x, what)
    assert tac._hip.beamform_layout['copied'] == layout['copied'], 'the frame-major spectrogram was copied'
    pairs = one(tac, FUSED, tac.RTFMVDR(), xp, torch.view_as_real(dd), torch.view_as_real(pnd), 1)
    assert pairs.dtype == torch.float32 and pairs.transpose(-3, -2).is_contiguous()


def test_stft_rtfmvdr_istft(tac):
    """the chain stays on the kernels under strict mode, and ``istft`` reads the beamformer's rows in place"""
    g = torch.Generator().manual_seed(9)
    wave = torch.randn(2, 4, 8000, generator=g)
    n_fft, hop = 512, 128
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac.CompositeRouteWarning)
        spec = tac.stft(wave.cuda(), n_fft, hop)
        T = spec.shape[-2]
        ms = torch.rand(2, n_fft // 2 + 1, T, generator=g).cuda()
        before, rows, layout = dict(tac._hip.launches), dict(tac._hip.istft_layout), dict(tac._hip.beamform_layout)
        ps, pn = tac.psd(spec, ms), tac.psd(spec, 1 - ms)
        enhanced = tac.RTFMVDR()(spec, tac.rtf_evd(ps), pn, 0)
        back = tac.istft(enhanced, n_fft, hop, length=8000)
    since = launched_since(tac, before)
    assert since.get(FUSED) == 1 and since.get(EVD) == 1 and since.get(PSD) == 2 and APPLY not in since
    assert tac._hip.beamform_layout['copied'] == layout['copied']
    assert tac._hip.istft_layout['in_place'] == rows['in_place'] + 1 and tac._hip.istft_layout['copied'] == rows['copied']
    assert tuple(back.shape) == (2, 8000) and bool(torch.isfinite(back).all())


@pytest.mark.parametrize('route', ('evd', 'power'))
def test_end_to_end(tac, route):
    """``psd → rtf_evd | rtf_power → RTFMVDR`` on the kernels against the complex128 chain; the apply bound is evaluated with the
    kernel's own weights, as in the Souden fused test"""
    C, F, T = 4, 129, 257
    x, ms, mn = R.scene((2,), C, F, T, seed=12)
    xd = fm(x.cuda())
    ps = one(tac, PSD, tac.psd, xd, ms.cuda(), eps=1e-15)
    pn = one(tac, PSD, tac.psd, xd, mn.cuda(), eps=1e-15)
    R.assert_psd(ps.cpu(), x, ms, True, 1e-15, 'psd_s')
    R.assert_psd(pn.cpu(), x, mn, True, 1e-15, 'psd_n')
    if route == 'evd':
        d = one(tac, EVD, tac.rtf_evd, ps)
        worst = RT.assert_evd(d.cpu(), ps.cpu(), 'end to end')[0]
    else:
        d = one(tac, POWER, tac.rtf_power, ps, pn, 1)
        worst = RT.assert_power(d.cpu(), ps.cpu(), pn.cpu(), 1, 3, what='end to end')[0]
    fused_y, w = tac._hip.rtf_mvdr(torch.view_as_real(xd), torch.view_as_real(d), torch.view_as_real(pn), None, 1, True, 1e-7, 1e-8)
    got = one(tac, FUSED, tac.RTFMVDR(), xd, d, pn, 1)
    assert torch.equal(torch.view_as_complex(fused_y), got)
    w = torch.view_as_complex(w)
    worst_w = RT.assert_weights_rtf(w.cpu(), d.cpu(), pn.cpu(), 1, what='end to end')[0]
    worst_y = R.assert_apply(got.cpu(), w.cpu(), x, 'end to end')
    # and the whole chain in complex128 from the same spectrogram: the float32 PSDs set the distance
    ps64, pn64 = R.psd(x, ms, True, 1e-15), R.psd(x, mn, True, 1e-15)
    d64 = RT.rtf_evd(ps64) if route == 'evd' else RT.rtf_power(ps64, pn64, 1)
    want = RT.rtf_mvdr(x, d64, pn64, 1)
    assert float((got.cpu().to(torch.complex128) - want).abs().max()) <= 2e-3 * float(want.abs().max())
    print('%s: rtf %.3g, weights %.3g, apply %.3g of their bounds' % (route, worst, worst_w, worst_y))


# ----------------------------------------------------------------------------- 6. routes
def test_routes(tac):
    C, F, T = 3, 9, 40
    x, ps, pn = RT.psds(C, F, T, seed=10)
    x9, ps9, pn9 = RT.psds(9, 5, 80, seed=10, lead=(1,))
    xd, psd_, pnd = fm(x.cuda()), ps.cuda(), pn.cuda()
    d = RT.rtf_evd(ps).to(torch.complex64)
    dd = d.cuda()
    d9 = RT.rtf_evd(ps9).to(torch.complex64)
    grad_in = torch.view_as_real(dd).clone().requires_grad_(True)

    def backward():
        tac.RTFMVDR()(torch.view_as_real(xd), grad_in, torch.view_as_real(pnd), 0).square().sum().backward()

    far = tac._hip.rtf_power_max_iter() + 1
    cases = (
        ('dtype float64', lambda: tac.rtf_evd(psd_.to(torch.complex128)), RT.rtf_evd(ps), 1e-12),
        ('dtype float64', lambda: tac.rtf_power(psd_.to(torch.complex128), pnd.to(torch.complex128), 0), RT.rtf_power(ps, pn, 0), 1e-10),
        ('dtype float64', lambda: tac.mvdr_weights_rtf(dd.to(torch.complex128), pnd.to(torch.complex128), 0),
         RT.mvdr_weights_rtf(d, pn, 0), 1e-10),
        ('dtype float64', lambda: tac.RTFMVDR()(xd.to(torch.complex128), dd.to(torch.complex128), pnd.to(torch.complex128), 0),
         RT.rtf_mvdr(x, d, pn, 0), 1e-10),
        ('9 channels', lambda: tac.rtf_evd(ps9.cuda()), RT.rtf_evd(ps9), 1e-4),
        ('9 channels', lambda: tac.rtf_power(ps9.cuda(), pn9.cuda(), 0), RT.rtf_power(ps9, pn9, 0), 5e-3),
        ('9 channels', lambda: tac.mvdr_weights_rtf(d9.cuda(), pn9.cuda(), 0), RT.mvdr_weights_rtf(d9, pn9, 0), 5e-3),
        ('9 channels', lambda: tac.RTFMVDR()(fm(x9.cuda()), d9.cuda(), pn9.cuda(), 0), RT.rtf_mvdr(x9, d9, pn9, 0), 5e-3),
        ('expanded or non-positive strides', lambda: tac.rtf_evd(psd_[:1].expand(2, F, C, C)), RT.rtf_evd(ps[:1].expand(2, F, C, C)), 1e-4),
        ('n_iter %d' % far, lambda: tac.rtf_power(psd_, pnd, 0, n_iter=far), RT.rtf_power(ps, pn, 0, far), 1e-2),
    )
    before = dict(tac._hip.launches)
    for reason, call, want, tol in cases:
        with pytest.raises(RuntimeError, match=reason):
            call()
    with pytest.raises(RuntimeError, match='backward'):
        backward()
    assert set(launched_since(tac, before)) <= {FUSED}                         # (the forward of the backward case ran on the kernels)
    tac.set_strict(False)
    try:
        for key in [k for k in tac._ops._warned if k[0] in ('rtf_evd', 'rtf_power', 'mvdr_weights_rtf', 'rtf_mvdr')]:
            tac._ops._warned.discard(key)
        for reason, call, want, tol in cases:
            before = dict(tac._hip.launches)
            with pytest.warns(tac.CompositeRouteWarning):
                got = call()
            assert launched_since(tac, before) == {}, reason
            err = float((got.cpu().to(torch.complex128) - want).abs().max())
            assert err <= tol * float(want.abs().max()) + 1e-30, (reason, err)
        grad_in.grad = None
        with pytest.warns(tac.CompositeRouteWarning):
            backward()
        host = torch.view_as_real(d).clone().requires_grad_(True)
        tac.RTFMVDR()(torch.view_as_real(x), host, torch.view_as_real(pn), 0).square().sum().backward()
        assert float((grad_in.grad.cpu() - host.grad).abs().max()) <= 5e-3 * float(host.grad.abs().max())
    finally:
        tac.set_strict(True)
