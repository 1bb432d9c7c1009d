"""-m gpu: ``fftconvolve`` / ``convolve`` on the gfx950 kernels (csrc/fftconvolve.hip) — strict mode and poisoned outputs on, as in
tests/test_istft_gpu.py.

``tac_spectral_mac_f32`` alone through the C ABI against the float64 complex sum (float64 torch operators on the device), every
part within the fused multiply-add chain's own bound ``(2 P + 2) 2^-24 sum_p (|Xr||Hr| + |Xi||Hi|)``; the partitioned route at
each transform length against ``numpy.convolve`` in float64 by the per-block measure (block N / 2, neighbourhood N) at the
project's ``TIGHT = 2e-6``; the direct route within ``(M + 2) 2^-24 (|x| * |h|)``.  Rules: tests/convolve_rules.py."""
import warnings

import numpy as np
import pytest
import torch

import convolve_rules as R
import frame_bounds as fbnd

pytestmark = pytest.mark.gpu

TIGHT = R.TIGHT
SPECTRAL, DIRECT, SPECTRA = 'tac_fftconvolve_f32', 'tac_fftconvolve_direct_f32', 'tac_fftconvolve_spectra_f32'


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


def dev(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.array(a))).to('cuda')


def run(tac_, xt, yt, n_fft=None, mode='full', entry=SPECTRAL, what=''):
    before = dict(tac_._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac_.CompositeRouteWarning)
        got = tac_.fftconvolve(xt, yt, mode, n_fft=n_fft)
    since = launched_since(tac_, before)
    since.pop(SPECTRA, None)                              # (the kernel's spectra: once per kernel tensor and transform length)
    assert since == {entry: 1}, (what, since)
    assert type(got) is torch.Tensor and got.dtype == torch.float32
    if entry == SPECTRAL:
        assert tac_._hip.last_route() == 'spectral-%d' % (n_fft or tac_._hip.fftconvolve_n_fft(yt.shape[-1])), what
    else:
        assert tac_._hip.last_route() == 'direct', what
    return got


def check_blocks(got, ref, n_fft, what):
    ratios = R.block_ratios(got, torch.from_numpy(np.ascontiguousarray(ref)), n_fft // 2, n_fft)
    worst = float(torch.nan_to_num(ratios, nan=float('inf')).max())
    print('%s: worst per-block ratio %.3g' % (what, worst))
    assert worst <= TIGHT, (what, worst)
    return worst


# ----------------------------------------------------------------------------- tac_spectral_mac_f32 through the C ABI
def mac_call(tac_, X, H, hrow, conj, P=None, out=None):
    rows, T, F = X.shape[0], X.shape[1], X.shape[2]
    P = H.shape[1] if P is None else P
    Y = tac_._hip.poison_fill(torch.empty_like(X)) if out is None else out
    hmap = None if hrow is None else torch.tensor(hrow, dtype=torch.int32, device='cuda')
    rc = tac_._native.lib().tac_spectral_mac_f32(
        tac_._native.ptr(X), tac_._native.ptr(H), None if hmap is None else tac_._native.ptr(hmap), rows, T, F, P, H.shape[0],
        int(conj), tac_._native.ptr(Y), tac_._native.stream_ptr(X.device))
    torch.cuda.synchronize()
    return rc, Y


def mac_inputs(rows, T, F, P, h_rows, seed):
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(rows, T, F, 2, generator=gen)
    X[1] = 0.0
    X[2] *= 2.0 ** -12
    H = torch.randn(h_rows, P, F, 2, generator=gen)
    return X.cuda(), H.cuda()


MAPS = {'shared': (1, None), 'per-row': (3, [0, 1, 2]), 'permuted': (3, [2, 0, 1])}


@pytest.mark.parametrize('P', [1, 4, 5, 8, 9, 16, 17, 64])
def test_spectral_mac_within_the_chain_bound(tac, P):
    tile = tac._native.lib().tac_spectral_mac_tile(P)
    assert tile >= 4 * P and tile % 16 == 0
    frames = sorted(set(t for t in (1, P - 1, P, tile - 1, tile + 1) if t > 0))
    combos = [(conj, name) for conj in (False, True) for name in MAPS]
    cases = [(T, 1025, combos[i % 6]) for i, T in enumerate(frames)]
    cases += [(tile + 1, 1025, c) for c in combos] + [(tile + 1, 2049, combos[P % 6]), (tile + 1, 4097, combos[(P + 3) % 6])]
    worst = 0.0
    for T, F, (conj, name) in cases:
        h_rows, hrow = MAPS[name]
        X, H = mac_inputs(3, T, F, P, h_rows, seed=1000 * P + T + F)
        rc, Y = mac_call(tac, X, H, hrow, conj)
        what = 'P %d, T %d, F %d, conj %s, %s map' % (P, T, F, conj, name)
        assert rc == 0, what
        assert int(tac._hip.poison_count(Y)) == 0, what + ': every output written'
        re, im, bre, bim = R.mac_reference(X.double(), H.double(), hrow, conj)
        for got, ref, bound in ((Y[..., 0], re, bre), (Y[..., 1], im, bim)):
            err = (got.double() - ref).abs()
            limit = (2 * P + 2) * R.U * bound
            assert bool((err <= limit).all()), what
            worst = max(worst, float((err / limit.clamp(min=1e-300)).max()))
        assert not bool(Y[1].any()), what + ': the silent row is exactly zero'
        rc2, Y2 = mac_call(tac, X, H, hrow, conj)
        assert rc2 == 0 and torch.equal(Y.view(torch.int32), Y2.view(torch.int32)), what + ': bit-identical on a second run'
    print('spectral mac P %d: worst |err| / bound %.3f' % (P, worst))


def test_spectral_mac_refuses_65_partitions(tac):
    X, H = mac_inputs(3, 4, 1025, 65, 1, seed=65)
    Y = tac._hip.poison_fill(torch.empty_like(X))
    rc, Y = mac_call(tac, X, H, None, False, out=Y)
    assert rc == tac._native.TAC_E_UNSUPPORTED
    assert int(tac._hip.poison_count(Y)) == Y.numel(), 'nothing was launched: the output is untouched'
    assert tac._native.lib().tac_spectral_mac_tile(65) == tac._native.TAC_E_UNSUPPORTED


# ----------------------------------------------------------------------------- the spectral route
@pytest.fixture(scope='module')
def case_5000(tac):
    x = R.waveform((3, 5000), seed=11)
    h = R.white_kernel((1, 3000), seed=12)
    return x, h, R.reference(x, h)


@pytest.mark.parametrize('n_fft', [2048, 4096, 8192])
def test_spectral_route_three_rows(tac, case_5000, n_fft):
    x, h, ref = case_5000
    got = run(tac, dev(x), dev(h), n_fft, what='5000 x 3000 at %d' % n_fft)
    assert tuple(got.shape) == (3, 7999) and got.is_contiguous()
    check_blocks(got, ref, n_fft, 'L 5000, M 3000, N %d' % n_fft)
    assert not bool(got[1].any()), 'the silent row is exactly zero'
    again = run(tac, dev(x), dev(h), n_fft)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), 'bit-identical on a second run'


def test_partition_edges_at_2048(tac):
    worst = 0.0
    for length, m in [(1, 1)] + [(l, m) for l in (1023, 1024, 1025) for m in (1024, 1025, 2049)]:
        x = R.waveform((3, length), seed=length)
        h = R.white_kernel((1, m), seed=m)
        got = run(tac, dev(x), dev(h), 2048, what='%d x %d' % (length, m))
        assert tuple(got.shape) == (3, length + m - 1)
        worst = max(worst, check_blocks(got, R.reference(x, h), 2048, 'L %d, M %d, N 2048' % (length, m)))
    print('partition edges: worst per-block ratio %.3g' % worst)


def test_sixty_four_partitions(tac):
    x = R.waveform((1, 4096), seed=64)
    h = R.white_kernel((1, 65536), seed=65)
    got = run(tac, dev(x), dev(h), 2048, what='64 partitions')
    check_blocks(got, R.reference(x, h), 2048, 'L 4096, M 65536, N 2048 (P 64)')


@pytest.mark.parametrize('n_fft', [4096, 8192])
@pytest.mark.parametrize('length,m', [(9000, 5000), (30000, 20000)])
def test_larger_transforms(tac, n_fft, length, m):
    x = R.waveform((1, length), seed=length + n_fft)
    h = R.white_kernel((1, m), seed=m)
    got = run(tac, dev(x), dev(h), n_fft, what='%d x %d at %d' % (length, m, n_fft))
    check_blocks(got, R.reference(x, h), n_fft, 'L %d, M %d, N %d' % (length, m, n_fft))


@pytest.mark.parametrize('n_fft', [2048, 4096, 8192])
def test_decaying_impulse_response_quiet_tail(tac, n_fft):
    x = R.waveform((1, 20000), seed=3)
    h = R.rir(16000, seed=0)[None]
    got = run(tac, dev(x), dev(h), n_fft, what='decaying kernel at %d' % n_fft)
    check_blocks(got, R.reference(x, h), n_fft, 'L 20000, decaying M 16000, N %d' % n_fft)


def test_silent_span_gives_exact_zeros(tac):
    n_fft, b, m = 2048, 1024, 2500                        # P = 3
    p = R.partitions(m, n_fft)
    x = R.waveform((2, 16 * b), seed=8)
    x[0, 3 * b + 17:3 * b + 17 + (p + 3) * b] = 0.0       # a silent span longer than (P + 2) B, off the block grid
    h = R.white_kernel((1, m), seed=9)
    got = run(tac, dev(x), dev(h), n_fft).cpu()
    check_blocks(got, R.reference(x, h), n_fft, 'silent span')
    blocks_in = np.pad(x[0], (0, (-x.shape[1]) % b)).reshape(-1, b)
    silent_in = ~blocks_in.any(axis=1)
    n_out = -(-got.shape[1] // b)
    found = 0
    for t in range(n_out):
        reads = [q for q in range(t - p, t + 1) if 0 <= q < len(silent_in)]
        if reads and all(silent_in[q] for q in reads) and len(reads) == p + 1:
            assert not bool(got[0, t * b:(t + 1) * b].any()), 'output block %d reads silent input blocks only' % t
            found += 1
    assert found >= 1


def test_nan_reaches_blocks_b_to_b_plus_p_only(tac):
    n_fft, b, m = 2048, 1024, 2500
    p = R.partitions(m, n_fft)
    x = R.waveform((3, 12 * b), seed=18)
    h = R.white_kernel((1, m), seed=19)
    at = 4 * b + 100                                      # block 4 of row 0
    clean = x.copy()
    clean[0, at] = 0.0
    bad = x.copy()
    bad[0, at] = np.nan
    want = run(tac, dev(clean), dev(h), n_fft).cpu()
    got = run(tac, dev(bad), dev(h), n_fft).cpu()
    mask = torch.zeros_like(got, dtype=torch.bool)
    mask[0, 4 * b:min((4 + p + 1) * b, got.shape[1])] = True
    assert torch.equal(~torch.isfinite(got), mask), 'exactly output blocks 4 .. 4 + P of row 0'
    assert torch.equal(got.view(torch.int32)[~mask], want.view(torch.int32)[~mask]), 'the rest: bit-identical to the zeroed run'


def test_non_contiguous_unaligned_rows(tac, case_5000):
    x, h, ref = case_5000
    store = torch.full((3, 5000 + 7), float('nan'), device='cuda')
    store[:, 1:5001] = dev(x)
    view = store[:, 1:5001]
    assert view.data_ptr() % 16 == 4 and not view.is_contiguous() and view.stride(0) > 5000
    got = run(tac, view, dev(h), 2048, what='strided rows')
    assert torch.equal(got.view(torch.int32), run(tac, dev(x), dev(h), 2048).view(torch.int32))
    check_blocks(got, ref, 2048, 'row stride 5007, offset one float')


def test_broadcast_kernels_against_the_row_loop(tac):
    x = R.waveform((2, 3, 3000), seed=21)
    xt = dev(x)
    for yshape in [(2, 1, 1500), (1, 3, 1500)]:
        h = R.white_kernel(yshape, seed=sum(yshape))
        ht = dev(h)
        got = run(tac, xt, ht, 2048, what='kernel %r' % (yshape,))
        assert tuple(got.shape) == (2, 3, 4499)
        he = np.broadcast_to(h, (2, 3, 1500))
        for i in range(2):
            for j in range(3):
                one = run(tac, dev(x[i, j][None]), dev(he[i, j][None]), 2048)
                assert torch.equal(got[i, j].view(torch.int32), one[0].view(torch.int32)), (yshape, i, j)
        check_blocks(got.reshape(6, -1), R.reference(x.reshape(6, -1), he.reshape(6, -1)), 2048, 'kernel %r' % (yshape,))


def test_three_modes_and_layers(tac, case_5000):
    x, h, ref = case_5000
    xt, ht = dev(x), dev(h)
    full = run(tac, xt, ht, 2048)
    for mode in ('valid', 'same'):
        got = run(tac, xt, ht, 2048, mode)
        want = R.crop(ref, 5000, 3000, mode)
        assert tuple(got.shape) == want.shape and got._base is not None, mode
        assert torch.equal(got, R.crop(full, 5000, 3000, mode)), mode
    for layer in (tac.FFTConvolve('same'), tac.Convolve('same')):
        out = layer(xt, ht)                                # (the default rule: 3000 taps -> 2048)
        assert torch.equal(out, R.crop(full, 5000, 3000, 'same')) and tac._hip.last_route() == 'spectral-2048'
    # L < M
    short = run(tac, xt[:, :700], ht, 2048, 'same')
    assert tuple(short.shape) == (3, 700)
    check_blocks(short, R.crop(R.reference(x[:, :700], h), 700, 3000, 'same'), 2048, "L 700 < M 3000, 'same'")


def test_kernel_spectra_are_cached_until_the_kernel_changes(tac):
    x = dev(R.waveform((1, 3000), seed=2))
    h = dev(R.white_kernel((1, 1500), seed=3))
    before = dict(tac._hip.launches)
    first = tac.fftconvolve(x, h, n_fft=2048)
    tac.fftconvolve(x, h, n_fft=2048)
    assert launched_since(tac, before) == {SPECTRA: 1, SPECTRAL: 2}
    h.mul_(2.0)
    assert torch.equal(tac.fftconvolve(x, h, n_fft=2048), 2.0 * first)       # (a power of two: every product scales exactly)
    assert launched_since(tac, before) == {SPECTRA: 2, SPECTRAL: 3}


def test_beyond_the_partition_cap(tac):
    x = dev(R.waveform((1, 2000), seed=4))
    h = dev(R.white_kernel((1, 64 * 1024 + 1), seed=5))
    before = dict(tac._hip.launches)
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.fftconvolve(x, h, n_fft=2048)
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.fftconvolve(x.double(), h.double())
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.fftconvolve(x.expand(3, 2000), h[:, :300])     # a stride of zero
    assert not launched_since(tac, before)
    tac.set_strict(False)
    try:
        tac._ops._warned.discard(('fftconvolve', 'a kernel of 65537 taps: more than 64 partitions of 1024 samples'))
        with pytest.warns(tac.CompositeRouteWarning, match='65537 taps'):
            got = tac.fftconvolve(x, h, n_fft=2048)
    finally:
        tac.set_strict(True)
    assert not launched_since(tac, before)
    ref = R.reference(x.cpu().numpy(), h.cpu().numpy())
    assert float((got.cpu().double() - torch.from_numpy(ref)).abs().max()) <= 1e-4 * np.abs(ref).max()
    # the same kernel under the default rule: 17 partitions of 4096
    check_blocks(run(tac, x, h), ref, 8192, 'M 65537 at the default transform length')


# ----------------------------------------------------------------------------- the direct route
def test_direct_route_within_the_chain_bound(tac):
    m_direct = tac._hip.M_DIRECT
    x = R.waveform((3, 3001), seed=31)
    xt = dev(x)
    for m in (1, 7, m_direct):
        h = R.white_kernel((1, m), seed=m)
        ref, bound = R.reference(x, h), R.direct_bound(x, h)
        for fn in (tac.fftconvolve, tac.convolve):
            before = dict(tac._hip.launches)
            got = fn(xt, dev(h))
            assert launched_since(tac, before) == {DIRECT: 1} and tac._hip.last_route() == 'direct', m
            err = np.abs(got.cpu().double().numpy() - ref)
            assert tuple(got.shape) == (3, 3000 + m) and bool((err <= bound).all()), m
            print('direct M %d: worst |err| / bound %.3f' % (m, float((err / bound).max())))
        for mode in ('valid', 'same'):
            assert torch.equal(tac.fftconvolve(xt, dev(h), mode), R.crop(got, 3001, m, mode))
    h = R.white_kernel((1, m_direct + 1), seed=77)
    got = run(tac, xt, dev(h), None, what='M_DIRECT + 1 taps')       # (asserts the spectral route at the default length)
    check_blocks(got, R.reference(x, h), 2048, 'M_DIRECT + 1')
    # per-row kernels have no direct form
    run(tac, xt, dev(R.white_kernel((3, 7), seed=1)), None, what='per-row short kernels')


# ----------------------------------------------------------------------------- gradients
def grad64(x, h, go):
    xt = torch.from_numpy(x).double().requires_grad_(True)
    rows, m = x.shape[0], h.shape[-1]
    he = torch.from_numpy(np.broadcast_to(h, (rows, m)).copy()).double()
    full = torch.nn.functional.conv1d(xt[None], he.flip(-1)[:, None], padding=m - 1, groups=rows)[0]
    return torch.autograd.grad(full, xt, torch.from_numpy(go).double())[0]


@pytest.mark.parametrize('case', [(2048, 5000, 3000, 1), (4096, 9000, 5000, 1), (8192, 9000, 5000, 1), (2048, 3000, 1500, 3),
                                  (None, 3001, 7, 1)])
def test_gradient_wrt_x(tac, case):
    n_fft, length, m, h_rows = case
    x = R.waveform((3, length), seed=length + m)
    h = R.white_kernel((h_rows, m), seed=m)
    go = np.random.default_rng(1).standard_normal((3, length + m - 1)).astype(np.float32)
    want = grad64(x, h, go)
    xt = dev(x).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac.CompositeRouteWarning)
        out = tac.fftconvolve(xt, dev(h), n_fft=n_fft)
        before = dict(tac._hip.launches)
        out.backward(dev(go))
    since = launched_since(tac, before)
    since.pop(SPECTRA, None)
    assert since == {(DIRECT if n_fft is None else SPECTRAL): 1}, since
    assert tuple(xt.grad.shape) == (3, length)
    worst = fbnd.assert_rows(xt.grad.cpu(), want, TIGHT, 'fftconvolve gradient %r' % (case,))
    print('gradient %r: worst row error %.3g' % (case, worst))
    # 'same': the crop's gradient is zero-padding by autograd, then the same route
    xs = dev(x).requires_grad_(True)
    tac.fftconvolve(xs, dev(h), 'same', n_fft=n_fft).backward(dev(go[:, :length]))
    pad = (m - 1) // 2
    gs = np.zeros_like(go)
    gs[:, pad:pad + length] = go[:, :length]
    fbnd.assert_rows(xs.grad.cpu(), grad64(x, h, gs), TIGHT, "fftconvolve gradient through 'same' %r" % (case,))


def test_kernel_gradient_is_announced(tac):
    x = dev(R.waveform((1, 3000), seed=4))
    h = dev(R.white_kernel((1, 1500), seed=5)).requires_grad_(True)
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.fftconvolve(x, h).sum().backward()
    tac.set_strict(False)
    try:
        tac._ops._warned.discard(('fftconvolve', 'backward: this gradient has no gfx950 kernel'))
        with pytest.warns(tac.CompositeRouteWarning, match='fftconvolve'):
            tac.fftconvolve(x, h).sum().backward()
    finally:
        tac.set_strict(True)
    want = torch.from_numpy(np.full(1500, 0.0))
    xs = x.cpu().double()[0]
    # d/dh[k] of sum(full) = sum(x) for every tap
    assert torch.allclose(h.grad.cpu().double()[0], want + float(xs.sum()), rtol=0, atol=1e-3 * float(xs.abs().sum()))


def test_trains_in_front_of_the_fused_mel_chain(tac):
    mel = dict(num_mels=40, sample_rate=16000, fft_length=400, hop_length=160)
    x = R.waveform((2, 1, 8000), seed=61)
    x[1] *= 2.0 ** 7
    h = R.rir(3000, seed=62)[None, None]
    ht = dev(h)
    conv = tac.FFTConvolve('same')

    class Reverb(torch.nn.Module):
        def forward(self, w):
            return conv(w, ht)

    def loss_of(model, w):
        return model(w).square().mean()

    chain = torch.nn.Sequential(Reverb(), *tac.Melspectrogram(**mel), tac.AmplitudeToDb()).cuda()
    xg = dev(x).requires_grad_(True)
    before = dict(tac._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac.CompositeRouteWarning)
        loss_of(chain, xg).backward()
    since = launched_since(tac, before)
    assert since.get(SPECTRAL) == 2, since                 # one forward, one backward
    assert bool(torch.isfinite(xg.grad).all()) and bool(xg.grad.any())

    def cpu_grad(dtype):
        cpu = torch.nn.Sequential(*tac.Melspectrogram(**mel), tac.AmplitudeToDb()).to(dtype)
        w = torch.from_numpy(x).to(dtype).requires_grad_(True)
        rev = tac.fftconvolve(w, torch.from_numpy(h).to(dtype), 'same')
        cpu(rev).square().mean().backward()
        return w.grad.reshape(2, -1)

    want, cpu32 = cpu_grad(torch.float64), cpu_grad(torch.float32)
    theirs = float(fbnd.row_errors(cpu32, want).max())
    mine = float(torch.nan_to_num(fbnd.row_errors(xg.grad.cpu().reshape(2, -1), want), nan=float('inf')).max())
    print('chain gradient: kernels %.3g, float32 CPU autograd %.3g' % (mine, theirs))
    fbnd.assert_rows(xg.grad.cpu().reshape(2, -1), want, 1e-3, 'waveform gradient through FFTConvolve -> mel dB')
    assert mine <= 4.0 * theirs, (mine, theirs)
