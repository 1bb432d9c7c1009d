"""-m gpu: ``psd`` / ``mvdr_weights_souden`` / ``apply_beamforming`` / ``MVDR`` on the gfx950 kernels (csrc/beamform.hip) — strict mode and
poisoned outputs on, as in tests/test_pitch_gpu.py.

Reference and bounds: tests/beamform_rules.py — the complex128 restatement, the generator (one source through a random steering
vector plus white noise, random masks) and the three derived bounds.  The weights are compared with the restatement fed the SAME
float32 PSDs.  The fused entry is held to the bits of the three entries called by themselves, which are held to the bounds."""
import warnings

import pytest
import torch

import beamform_rules as R

pytestmark = pytest.mark.gpu

PSD, WEIGHTS, APPLY, FUSED = 'tac_psd_f32', 'tac_mvdr_weights_souden_f32', 'tac_apply_beamforming_f32', 'tac_mvdr_souden_f32'


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


def fm(z):
    """a complex ``(…, F, T)`` tensor re-laid frame-major (bins of a frame contiguous): the layout ``stft`` returns"""
    return z.transpose(-2, -1).contiguous().transpose(-2, -1)


def cplx(pairs):
    return torch.view_as_complex(pairs)


def hermitian(p):
    """a complex ``(…, C, C)`` PSD equals its conjugate transpose bit for bit, with a zero imaginary diagonal"""
    return torch.equal(p, p.conj().transpose(-2, -1).resolve_conj()) and bool((p.diagonal(dim1=-2, dim2=-1).imag == 0).all())


def one(tac_, entry, fn, *args, **kw):
    before = dict(tac_._hip.launches)
    out = fn(*args, **kw)
    assert launched_since(tac_, before) == {entry: 1}, (entry, launched_since(tac_, before))
    return out


# ----------------------------------------------------------------------------- 1. psd
@pytest.mark.parametrize('C', R.CHANNELS)
def test_psd(tac, C):
    worst = 0.0
    for F in R.BINS:
        for T in R.FRAMES:
            what = 'C %d, F %d, T %d' % (C, F, T)
            x, ms, mn = R.scene((1,), C, F, T, seed=1)
            xd, msd, mnd = fm(x.cuda()), ms.cuda(), fm(mn.cuda())
            assert msd.stride(-1) == 1 and (T == 1 or F == 1 or mnd.stride(-1) == F)
            plain = one(tac, PSD, tac.psd, xd)
            worst = max(worst, R.assert_psd(plain.cpu(), x, what=what + ', no mask'))
            a = one(tac, PSD, tac.psd, xd, msd)                                  # a contiguous (F, T) mask: staged through the LDS
            worst = max(worst, R.assert_psd(a.cpu(), x, ms, what=what + ', contiguous mask'))
            b = one(tac, PSD, tac.psd, xd, mnd, normalize=False)                 # a frame-major mask: read directly
            worst = max(worst, R.assert_psd(b.cpu(), x, mn, False, what=what + ', frame-major mask, not normalised'))
            b_norm = one(tac, PSD, tac.psd, xd, mnd, eps=1e-15)
            worst = max(worst, R.assert_psd(b_norm.cpu(), x, mn, True, 1e-15, what=what + ', frame-major mask'))
            # two masks in one launch: the bits of the single calls
            xp = torch.view_as_real(xd)
            both = one(tac, PSD, tac._hip.psd, xp, msd, mnd, normalize=True, eps=1e-15)
            assert torch.equal(cplx(both[1]), b_norm) and torch.equal(cplx(both[0]), tac.psd(xd, msd, eps=1e-15)), what
            comp = one(tac, PSD, tac._hip.psd, xp, msd, None, complement=True, normalize=True, eps=1e-15)
            assert torch.equal(comp[0], both[0]) and torch.equal(cplx(comp[1]), tac.psd(xd, 1 - msd, eps=1e-15)), what
            for p in (plain, a, b, b_norm, cplx(comp[1])):
                assert p.dtype == torch.complex64 and tuple(p.shape) == (1, F, C, C) and hermitian(p), what
            again = tac._hip.psd(xp, msd, mnd, normalize=True, eps=1e-15)
            assert torch.equal(again[0], both[0]) and torch.equal(again[1], both[1]), what + ': two calls differ'
    print('C %d: worst psd error %.3f of its bound' % (C, worst))


# ----------------------------------------------------------------------------- 2. weights
@pytest.mark.parametrize('C,F,T', R.WEIGHT_CASES)
def test_weights(tac, C, F, T):
    x, ms, mn = R.scene((2,), C, F, T, seed=11)
    ps = R.psd(x, ms, True, 1e-15).to(torch.complex64)
    pn = R.psd(x, mn, True, 1e-15).to(torch.complex64)
    psd_, pnd = ps.cuda(), pn.cuda()
    one_hot = torch.zeros(2, C)
    one_hot[0, C - 1] = 1
    one_hot[1, 0] = 1
    mix = torch.linspace(0.1, 1.0, C)
    for ref in (0, C - 1, one_hot, mix):
        for loading in (True, False):
            what = 'C %d, F %d, T %d, ref %s, loading %s' % (C, F, T, ref if isinstance(ref, int) else tuple(ref.shape), loading)
            got = one(tac, WEIGHTS, tac.mvdr_weights_souden, psd_, pnd, ref.cuda() if torch.is_tensor(ref) else ref,
                      diagonal_loading=loading)
            assert got.dtype == torch.complex64 and tuple(got.shape) == (2, F, C)
            worst, k = R.assert_weights(got.cpu(), ps, pn, ref, loading, what=what)
    print('C %d, T %d: worst weights error %.3f of its bound, κ up to %.0f' % (C, T, worst, k))
    by_vector = tac.mvdr_weights_souden(psd_, pnd, one_hot.cuda())
    assert torch.equal(by_vector[0], tac.mvdr_weights_souden(psd_, pnd, C - 1)[0])
    assert torch.equal(by_vector[1], tac.mvdr_weights_souden(psd_, pnd, 0)[1])
    pairs = one(tac, WEIGHTS, tac.mvdr_weights_souden, torch.view_as_real(psd_), torch.view_as_real(pnd), 0)
    assert pairs.dtype == torch.float32 and torch.equal(torch.view_as_complex(pairs), tac.mvdr_weights_souden(psd_, pnd, 0))


def test_weights_rank_deficient(tac):
    """``T < C``: the loaded ``Φn`` has a condition number near 1e7 — float64 elimination keeps the same formula, with that ``κ``"""
    C, F, T = R.RANK_DEFICIENT
    x, ms, mn = R.scene((2,), C, F, T, seed=11)
    ps = R.psd(x, ms, True, 1e-15).to(torch.complex64)
    pn = R.psd(x, mn, True, 1e-15).to(torch.complex64)
    got = one(tac, WEIGHTS, tac.mvdr_weights_souden, ps.cuda(), pn.cuda(), 0)
    assert bool(torch.isfinite(torch.view_as_real(got)).all())
    worst, k = R.assert_weights(got.cpu(), ps, pn, 0, True, what='rank-deficient', cap=None)
    assert k > 1e5
    print('rank-deficient: κ %.3g, worst weights error %.3g of its bound' % (k, worst))


# ----------------------------------------------------------------------------- 3. apply
@pytest.mark.parametrize('C', R.CHANNELS)
def test_apply(tac, C):
    worst = 0.0
    g = torch.Generator().manual_seed(C)
    for F in R.BINS:
        for T in R.FRAMES:
            what = 'C %d, F %d, T %d' % (C, F, T)
            x, _, _ = R.scene((1,), C, F, T, seed=2)
            w = torch.complex(torch.randn(1, F, C, generator=g), torch.randn(1, F, C, generator=g))
            xd, wd = fm(x.cuda()), w.cuda()
            got = one(tac, APPLY, tac.apply_beamforming, wd, xd)
            assert got.dtype == torch.complex64 and tuple(got.shape) == (1, F, T) and got.transpose(-2, -1).is_contiguous(), what
            worst = max(worst, R.assert_apply(got.cpu(), w, x, what))
            assert torch.equal(got, tac.apply_beamforming(wd, xd)), what + ': two calls differ'
    print('C %d: worst apply error %.3f of its bound' % (C, worst))


# ----------------------------------------------------------------------------- 4. layouts
def all_three(tac_, x, ms):
    """(psd with a mask, apply with weights from it, MVDR) of a complex spectrogram on the device"""
    p = tac_.psd(x, ms)
    w = tac_.mvdr_weights_souden(p, tac_.psd(x, 1 - ms), 1)
    return p, tac_.apply_beamforming(w, x), tac_.MVDR(ref_channel=1)(x, ms)


def same(got, want):
    return all(torch.equal(g, w) for g, w in zip(got, want))


def test_layouts(tac):
    C, F, T = 3, 65, 31
    x, ms, _ = R.scene((2,), C, F, T, seed=3)
    xd, msd = fm(x.cuda()), ms.cuda()
    layout = tac._hip.beamform_layout
    before = dict(layout)
    plain = all_three(tac, xd, msd)
    assert layout['copied'] == before['copied'] and layout['in_place'] > before['in_place']
    R.assert_psd(plain[0].cpu(), x, ms, what='plain')
    # a time-contiguous spectrogram is copied into the frame-major layout, and gives the same bits
    before = dict(layout)
    assert same(all_three(tac, x.cuda(), msd), plain) and layout['copied'] > before['copied']
    # channel slices of a larger tensor, in place
    store = torch.full((2, C + 3, T, F), float('nan'), dtype=torch.complex64, device='cuda')
    store[:, 2:2 + C] = xd.transpose(-2, -1)
    view = store[:, 2:2 + C].transpose(-2, -1)
    before = dict(layout)
    assert not view.is_contiguous() and same(all_three(tac, view, msd), plain) and layout['copied'] == before['copied']
    # rows 8 bytes off a 16-byte boundary, in place; 4 bytes off an 8-byte boundary, copied
    n = 2 * C * T * F * 2
    for off, in_place in ((2, True), (1, False)):
        flat = torch.full((n + 4,), float('nan'), device='cuda')
        late = flat[off:off + n].view(2, C, T, F, 2)
        late.copy_(torch.view_as_real(xd.transpose(-2, -1)))
        late = late.transpose(2, 3)
        assert late.data_ptr() % 16 == 4 * off
        before = dict(layout)
        got = (tac.psd(late, msd), tac.MVDR(ref_channel=1)(late, msd))
        assert got[0].dtype == torch.float32 and torch.equal(torch.view_as_complex(got[0]), plain[0])
        assert torch.equal(cplx(got[1]), plain[2])
        assert (layout['copied'] == before['copied']) == in_place
    # three leading dimensions
    nested = torch.stack([xd, xd.flip(0)]).reshape(2, 1, 2, C, F, T)
    masks = torch.stack([msd, msd.flip(0)]).reshape(2, 1, 2, F, T)
    got = all_three(tac, nested, masks)
    for g, p in zip(got, plain):
        assert tuple(g.shape) == (2, 1, 2) + tuple(p.shape[1:])
        assert torch.equal(g[0, 0], p) and torch.equal(g[1, 0], p.flip(0))
    # a zero-size batch launches nothing
    before = dict(tac._hip.launches)
    empty = all_three(tac, xd[:0], msd[:0])
    assert [tuple(e.shape) for e in empty] == [(0, F, C, C), (0, F, T), (0, F, T)] and launched_since(tac, before) == {}


def test_the_view_stft_returns_is_used_in_place(tac):
    wave = torch.randn(2, 4, 4000, generator=torch.Generator().manual_seed(4)).cuda()
    spec = tac.stft(wave, 256, 64)
    assert tuple(spec.shape[:3]) == (2, 4, 129) and spec.shape[-1] == 2 and spec.transpose(-3, -2).is_contiguous()
    T = spec.shape[-2]
    ms = torch.rand(2, 129, T, generator=torch.Generator().manual_seed(5)).cuda()
    layout = tac._hip.beamform_layout
    before = dict(layout)
    p = one(tac, PSD, tac.psd, spec, ms)
    y = one(tac, FUSED, tac.MVDR(), spec, ms)
    assert layout['copied'] == before['copied'] and layout['in_place'] == before['in_place'] + 2
    R.assert_psd(torch.view_as_complex(p).cpu(), torch.view_as_complex(spec.cpu().contiguous()), ms.cpu(), what='stft view')
    assert tuple(y.shape) == (2, 129, T, 2) and y.transpose(-3, -2).is_contiguous()


# ----------------------------------------------------------------------------- 5. non-finite input
def test_a_nan_reaches_only_its_bin(tac):
    C, F, T = 5, 129, 257
    x, ms, mn = R.scene((2,), C, F, T, seed=6)
    xd, msd, mnd = fm(x.cuda()), ms.cuda(), fm(mn.cuda())
    clean = (tac.psd(xd, msd), tac.MVDR()(xd, msd, mnd), tac.MVDR()(xd, msd))
    bad = xd.clone()
    bad[1, 3, 70, 200] = float('nan')
    got = (tac.psd(bad, msd), tac.MVDR()(bad, msd, mnd), tac.MVDR()(bad, msd))
    keep = torch.ones(2, F, dtype=torch.bool, device='cuda')
    keep[1, 70] = False
    for g, c in zip(got, clean):
        assert torch.equal(torch.view_as_real(g)[keep], torch.view_as_real(c)[keep]), 'a bin without the NaN changed'
        assert bool(torch.isnan(torch.view_as_real(g)[1, 70]).any())


# ----------------------------------------------------------------------------- 6. more units than the persistent grids
def test_units_beyond_the_grids(tac):
    """more units than either persistent grid holds: workgroups of the PSD launch and of the apply launch take a second unit"""
    C, F, T = 2, 129, 31
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert tac._native.lib().tac_beamform_grid(0, cus) == R.psd_units(1, 1, cus)[1]
    assert tac._native.lib().tac_beamform_grid(1, cus) == R.apply_units(1, 1, cus)[1]
    B = 8
    while min(R.psd_units(B * F, T, cus)[0] - R.psd_units(B * F, T, cus)[1],
              R.apply_units(B * F, T, cus)[0] - R.apply_units(B * F, T, cus)[1]) <= 8:
        B += 8
    assert [tac._hip.psd_chunks(t) for t in (1, 31, 64, 65, 257)] == [R.psd_plan(t)[1] for t in (1, 31, 64, 65, 257)] == [1, 1, 1, 2, 5]
    x, ms, _ = R.scene((5,), C, F, T, seed=7)
    xd, msd = fm(x.cuda()), ms.cuda()
    small = all_three(tac, xd, msd)
    R.assert_psd(small[0].cpu(), x, ms, what='five entries')
    index = (torch.arange(B) % 5).cuda()
    big = all_three(tac, fm(xd[index]), msd[index].contiguous())
    for b, s in zip(big, small):
        assert torch.equal(b, s[index]), '%d entries: %d / %d units on grids of %d / %d' % (
            (B,) + R.psd_units(B * F, T, cus)[:1] + R.apply_units(B * F, T, cus)[:1] + (2 * cus, 8 * cus))


# ----------------------------------------------------------------------------- 7. end to end
@pytest.mark.parametrize('C,F,T', R.FUSED_CASES)
def test_fused_entry(tac, C, F, T):
    x, ms, mn = R.scene((2,), C, F, T, seed=8)
    xd, msd, mnd = fm(x.cuda()), ms.cuda(), mn.cuda()
    xp = torch.view_as_real(xd)
    for second in (mnd, None):
        what = 'C %d, mask_n %s' % (C, 'given' if second is not None else 'the complement')
        got = one(tac, FUSED, tac.MVDR(ref_channel=1), xd, msd, second)
        assert got.dtype == torch.complex64 and tuple(got.shape) == (2, F, T) and got.transpose(-2, -1).is_contiguous()
        # the three entries by themselves: the same bits
        ps, pn = one(tac, PSD, tac._hip.psd, xp, msd, second, complement=second is None, normalize=True, eps=1e-15)
        w = one(tac, WEIGHTS, tac._hip.mvdr_weights_souden, ps, pn, None, 1, True, 1e-7, 1e-8)
        y = one(tac, APPLY, tac._hip.apply_beamforming, w, xp)
        fused_y, fused_w = tac._hip.mvdr_souden(xp, msd, second, None, 1, True, 1e-7, 1e-8, 1e-15)
        assert torch.equal(fused_w, w) and torch.equal(fused_y, y) and torch.equal(cplx(y), got), what
        # and each of the three within its bound
        m2 = mn if second is not None else 1 - ms
        R.assert_psd(cplx(ps).cpu(), x, ms, True, 1e-15, what)
        R.assert_psd(cplx(pn).cpu(), x, m2, True, 1e-15, what)
        R.assert_weights(cplx(w).cpu(), cplx(ps).cpu(), cplx(pn).cpu(), 1, what=what)
        R.assert_apply(got.cpu(), cplx(w).cpu(), x, what)
    # SoudenMVDR with given PSDs: the weights entry and the apply entry
    before = dict(tac._hip.launches)
    souden = tac.SoudenMVDR()(xd, cplx(ps), cplx(pn), 1)
    assert launched_since(tac, before) == {WEIGHTS: 1, APPLY: 1} and torch.equal(souden, got)


def test_stft_mvdr_istft(tac):
    """the whole chain stays on the kernels under strict mode, and ``istft`` reads the beamformer's rows in place"""
    g = torch.Generator().manual_seed(9)
    wave = torch.randn(2, 4, 8000, generator=g)
    n_fft, hop = 512, 128
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac.CompositeRouteWarning)
        spec = tac.stft(wave.cuda(), n_fft, hop)
        T = spec.shape[-2]
        ms = torch.rand(2, n_fft // 2 + 1, T, generator=g)
        before, rows = dict(tac._hip.launches), dict(tac._hip.istft_layout)
        enhanced = tac.MVDR()(spec, ms.cuda())
        back = tac.istft(enhanced, n_fft, hop, length=8000)
    assert launched_since(tac, before).get(FUSED) == 1 and PSD not in launched_since(tac, before)
    assert tac._hip.istft_layout['in_place'] == rows['in_place'] + 1 and tac._hip.istft_layout['copied'] == rows['copied']
    assert tuple(back.shape) == (2, 8000) and bool(torch.isfinite(back).all())
    cpu_spec = tac.stft(wave, n_fft, hop)
    want = tac.istft(tac.MVDR()(cpu_spec, ms), n_fft, hop, length=8000)
    assert float((back.cpu() - want).abs().max()) <= 2e-3 * float(want.abs().max())


# ----------------------------------------------------------------------------- 8. routes
def test_routes(tac):
    C, F, T = 3, 9, 40
    x, ms, mn = R.scene((2,), C, F, T, seed=10)
    xd, msd, mnd = fm(x.cuda()), ms.cuda(), mn.cuda()
    x9, ms9, mn9 = R.scene((1,), 9, 5, 80, seed=10)
    grad_in = torch.view_as_real(xd).clone().requires_grad_(True)

    def backward():
        tac.MVDR()(grad_in, msd, mnd).square().sum().backward()

    cases = (
        ('dtype float64', lambda: tac.MVDR()(xd.to(torch.complex128), msd.double(), mnd.double()), R.mvdr(x, ms, mn), 1e-9),
        ('9 channels', lambda: tac.MVDR()(fm(x9.cuda()), ms9.cuda(), mn9.cuda()), R.mvdr(x9, ms9, mn9), 5e-3),
        ('expanded or non-positive strides', lambda: tac.psd(xd[:1].expand(2, C, F, T), msd), R.psd(x[:1].expand(2, C, F, T), ms), 2e-5),
        ('dtype float64', lambda: tac.psd(xd.to(torch.complex128), msd.double()), R.psd(x, ms), 1e-12),
        ('dtype float64', lambda: tac.apply_beamforming(xd[:, :, :, 0].transpose(1, 2).to(torch.complex128), xd.to(torch.complex128)),
         R.apply_beamforming(x[:, :, :, 0].transpose(1, 2), x), 1e-12),
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
        for key in [k for k in tac._ops._warned if k[0] in ('psd', 'mvdr_souden', 'apply_beamforming')]:
            tac._ops._warned.discard(key)
        for reason, call, want, tol in cases:
            before = dict(tac._hip.launches)
            with pytest.warns(tac.CompositeRouteWarning):
                got = call()
            assert launched_since(tac, before) == {}, reason
            err = float((got.cpu().to(torch.complex128) - want).abs().max())
            assert err <= tol * float(want.abs().max()), (reason, err)
        grad_in.grad = None
        with pytest.warns(tac.CompositeRouteWarning):
            backward()
        host = torch.view_as_real(x).clone().requires_grad_(True)
        tac.MVDR()(host, ms, mn).square().sum().backward()
        assert float((grad_in.grad.cpu() - host.grad).abs().max()) <= 5e-3 * float(host.grad.abs().max())
    finally:
        tac.set_strict(True)
