"""-m gpu: every persistent side kernel with more units than its grid has workgroups — strict mode and poisoned outputs on, as in
the files of the ops themselves.

``lfilter``, ``resample``, ``dct``, the delay line of ``fftconvolve`` and the ``hpss`` / ``istft`` gradients launch
``min(units, cap x CUs)`` workgroups that walk ``for (u = blockIdx.x; u < units; u += gridDim.x)``; their own test files stay below
the cap, where no workgroup takes that step.  Here the sizes come from ``grid_rules.shapes`` for the CU count of the device (two
rounds of the grid and an odd remainder: every workgroup takes two units, a few take three), and every test holds them to the
restated grid (``grid_rules.assert_wraps``) before it launches.

No tolerance is new: references and bounds are those of lfilter_rules, resample_rules, dct_rules, convolve_rules, grad_rules and
frame_bounds.  Where a kernel reads nothing outside a row or a frame, the big batch repeats a few base rows (5) or frames (67) —
numbers that share no factor with a grid, so that a workgroup's successive units hold different data — and is compared BIT FOR
BIT with a small launch of the base, which is compared with the float64 reference under the existing bound.  A unit skipped
leaves poison behind (the ``every_output_written`` fixture), a unit decoded wrongly or a state left over from the unit before
breaks the equality."""
import math
import warnings

import numpy as np
import pytest
import torch

import convolve_rules as CR
import dct_rules as DR
import frame_bounds as fbnd
import grad_rules as gr
import grid_rules as G
import istft_rules as IR
import lfilter_rules as LR
import polyphase_rules as PR
import resample_rules as RR

pytestmark = pytest.mark.gpu

TIGHT = CR.TIGHT
GRAD = 1e-3                          # tests/test_istft_gpu.py's
LFILTER, POLYPHASE, DCT = 'tac_lfilter_f32', 'tac_polyphase_f32', 'tac_dct_rows_f32'
SPECTRAL, SPECTRA = 'tac_fftconvolve_f32', 'tac_fftconvolve_spectra_f32'


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    t._native.lib()
    t.set_strict(True)
    t._hip.set_poison_outputs(True)
    assert t._hip.LFILTER_TILE == G.LFILTER_TILE and t._hip.RESAMPLE_TILE == G.POLYPHASE_TILE
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


@pytest.fixture(scope='module')
def cus(tac):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def wrapping(cus_, name):
    """the sizes of case ``name`` on this device, held to the restated grid before anything is launched"""
    c = G.shapes(cus_)[name]
    ratio = G.assert_wraps(cus_, name, c)
    print('%s on %d CUs: %.3f rounds of the grid' % (name, cus_, ratio))
    return c


def launched_since(tac_, before):
    now = tac_._hip.launches
    return {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)}


def dev(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to('cuda')


def cycle(n, period, shift=0):
    return (torch.arange(n, device='cuda') + shift) % period


def repeat_rows(base, rows):
    """row r = base[r % len(base)], dense"""
    return base.index_select(0, cycle(rows, base.shape[0])).contiguous()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def row_padded(x, pad):
    """the rows of ``x`` ``pad`` floats apart in a NaN-filled store"""
    store = torch.full(tuple(x.shape[:-1]) + (x.shape[-1] + pad,), float('nan'), device='cuda')
    store[..., :x.shape[-1]] = x
    return store[..., :x.shape[-1]]


def sixteen_byte_rows(x):
    return x.data_ptr() % 16 == 0 and (x.shape[0] == 1 or x.stride(0) % 4 == 0)


def t64(v):
    return torch.tensor(v, dtype=torch.float64)


# ----------------------------------------------------------------------------- 1. lfilter
def lfilter_once(tac_, xt, b, a, clamp, what):
    before = dict(tac_._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac_.CompositeRouteWarning)
        got = tac_.lfilter(xt, t64(a), t64(b), clamp=clamp)
    assert launched_since(tac_, before) == {LFILTER: 1}, what
    assert got.dtype == torch.float32 and got.is_contiguous() and got.shape == xt.shape, what
    return got


def lfilter_gradient(tac_, xt, gt, b, a, what):
    x = xt.clone().requires_grad_(True)
    before = dict(tac_._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac_.CompositeRouteWarning)
        y = tac_.lfilter(x, t64(a), t64(b), clamp=False)
        assert launched_since(tac_, before) == {LFILTER: 1}, what
        (gx,) = torch.autograd.grad(y, x, grad_outputs=gt)
    assert launched_since(tac_, before) == {LFILTER: 2}, what                     # one forward, one with reverse = 1
    assert gx.shape == x.shape and gx.is_contiguous(), what
    return gx


@pytest.mark.parametrize('loads', ['16-byte loads', 'float loads', 'full last tile'])
@pytest.mark.parametrize('which', ['high-pass 100 Hz at 16 kHz', 'preemphasis 0.97'])
def test_lfilter_rows_beyond_the_grid(tac, cus, which, loads):
    """two tiles per row: the first row's second tile leaves a carry behind in the LDS that the workgroup's next row must not
    take into its first tile.  Behind a SHORT second tile (TILE + 36, TILE + 37) that carry is zero to every digit — the last
    lane's chunk lies behind the row's end, so its two inputs are the zero padding and its state has decayed over 16 000 samples
    of silence — and a kernel that took it would still pass; rows of exactly two tiles leave the row's last two samples and its
    final state there (the kernel built with lane 0 taking the carry in tile 0 as well fails these cases and no other)."""
    c = wrapping(cus, 'lfilter, ' + loads)
    rows, length = c['rows'], c['length']
    (name, b, a), = [f for f in LR.filters(tac) if f[0] == which]
    recursive = any(v != 0.0 for v in a[1:])
    base = LR.waveform((G.BASE_ROWS, length), seed=length)
    ref, bound = LR.reference(base, b, a)
    small_in = dev(base)
    big_in = repeat_rows(small_in, rows)
    assert sixteen_byte_rows(big_in) == (loads != 'float loads') and G.LFILTER_TILE < length <= 2 * G.LFILTER_TILE
    assert (length == 2 * G.LFILTER_TILE) == (loads == 'full last tile') and bool(big_in[:, -2:].all())
    what = '%s, %d rows of %d' % (name, rows, length)
    small = lfilter_once(tac, small_in, b, a, False, what)
    worst = LR.assert_close(small, ref, bound, what + ': the base rows')
    big = lfilter_once(tac, big_in, b, a, False, what)
    assert same_bits(big, repeat_rows(small, rows)), what + ': a row depends on where in the batch it stands'
    if loads == 'full last tile':                                                   # ... and the float loads of the same rows
        apart = row_padded(big_in, 1)
        assert not sixteen_byte_rows(apart)
        assert same_bits(lfilter_once(tac, apart, b, a, False, what), big), what + ', rows one float apart'
    if loads == 'float loads' and recursive:
        assert (np.abs(ref) > 1.0).any()
        clamped = lfilter_once(tac, small_in, b, a, True, what)
        worst = max(worst, LR.assert_close(clamped, np.clip(ref, -1.0, 1.0), bound, what + ', clamp: the base rows'))
        assert same_bits(lfilter_once(tac, big_in, b, a, True, what), repeat_rows(clamped, rows)), what + ', clamp'
    if recursive:
        gy = LR.waveform((G.BASE_ROWS, length), seed=length + 1)
        aref, abound = LR.adjoint_reference(gy, b, a)
        g_small = lfilter_gradient(tac, small_in, dev(gy), b, a, what)
        worst = max(worst, LR.assert_close(g_small, aref, abound, what + ': the base rows\' gradient'))
        g_big = lfilter_gradient(tac, big_in, repeat_rows(dev(gy), rows), b, a, what)
        assert same_bits(g_big, repeat_rows(g_small, rows)), what + ': gradient'
    print('%s: worst |err| / bound %.3f' % (what, worst))


# ----------------------------------------------------------------------------- 2. resample
def resample_once(tac_, xt, orig, new, what):
    before = dict(tac_._hip.launches)
    got = tac_.resample(xt, orig, new)
    assert launched_since(tac_, before) == {POLYPHASE: 1}, what
    assert got.dtype == torch.float32 and got.is_contiguous(), what
    assert tuple(got.shape) == (xt.shape[0], RR.out_length(xt.shape[-1], orig, new)), what
    return got


@pytest.mark.parametrize('orig,new', [(2, 1), (3, 2), (160, 441), (12, 1), (16, 1)])
def test_resample_tiles_beyond_the_grid(tac, cus, orig, new):
    """(2, 1): one phase and a skewed span; (3, 2): phases, no skew; (160, 441): phases, skew and a large bank; (12, 1) and
    (16, 1): 512 and 256 outputs per tile on the grid of their own workgroups per CU"""
    c = wrapping(cus, 'resample %d:%d' % (orig, new))
    rows, length = c['rows'], c['length']
    key = tac._resample.constants(orig, new)
    assert c['tile'] == PR.pinned_tile(orig, new)
    assert tac._hip.resample_tile(tac._resample.bank(*key)) == c['tile'] and tac._hip.resample_covers(*key)
    assert 3 * c['tile'] < c['n_out'] < 4 * c['tile']
    base = RR.waveform((G.BASE_ROWS, length), seed=1000 * orig + new)
    ref, bound = RR.reference(base, orig, new)
    what = 'resample %d:%d, %d rows of %d' % (orig, new, rows, length)
    small = resample_once(tac, dev(base), orig, new, what)
    worst = RR.assert_close(small, ref, bound, what + ': the base rows')
    big_in = repeat_rows(dev(base), rows)
    layouts = [('dense', big_in), ('row stride a multiple of four', row_padded(big_in, (-length) % 4 or 4))]
    if (orig, new) == (3, 2):
        layouts.append(('padded by 3', row_padded(big_in, 3)))
    forms = set()
    for tag, xt in layouts:
        forms.add(sixteen_byte_rows(xt))
        got = resample_once(tac, xt, orig, new, what + ', ' + tag)
        assert same_bits(got, repeat_rows(small, rows)), '%s, %s: a row depends on where in the batch it stands' % (what, tag)
    assert forms == {False, True}, 'both load forms'
    print('%s, tile %d, %d per CU: worst |err| / bound %.3f' % (what, c['tile'], c['per_cu'], worst))


def resample_gradient_beyond_the_grid(tac, cus, orig, new):
    c = wrapping(cus, 'resample %d:%d gradient' % (orig, new))
    rows, length, n_out = c['rows'], c['length'], c['n_out']
    assert c['tile'] == PR.pinned_tile(orig, new, adjoint=True) and length > 3 * c['tile']
    assert tac._hip.resample_tile(tac._resample.adjoint_bank(*tac._resample.constants(orig, new))) == c['tile']
    g = RR.waveform((G.BASE_ROWS, n_out), seed=7)
    aref, abound = RR.adjoint_reference(g, length, orig, new)

    def gradient(n_rows):
        x = torch.zeros(n_rows, length, device='cuda', requires_grad=True)
        y = tac.resample(x, orig, new)
        before = dict(tac._hip.launches)
        with warnings.catch_warnings():
            warnings.simplefilter('error', tac.CompositeRouteWarning)
            (gx,) = torch.autograd.grad(y, x, grad_outputs=repeat_rows(dev(g), n_rows))
        assert launched_since(tac, before) == {POLYPHASE: 1} and tuple(gx.shape) == (n_rows, length) and gx.is_contiguous()
        return gx

    small = gradient(G.BASE_ROWS)
    worst = RR.assert_close(small, aref, abound, 'resample %d:%d gradient: the base rows' % (orig, new))
    assert same_bits(gradient(rows), repeat_rows(small, rows)), 'a row of the gradient depends on where in the batch it stands'
    print('resample %d:%d gradient, %d rows of %d, tile %d, %d per CU: worst |err| / bound %.3f' % (
        orig, new, rows, n_out, c['tile'], c['per_cu'], worst))


def test_resample_gradient_tiles_beyond_the_grid(tac, cus):
    resample_gradient_beyond_the_grid(tac, cus, 3, 2)


def test_resample_gradient_narrow_tiles_beyond_the_grid(tac, cus):
    """the gradient of 1:12 runs the bank of 12:1 at 512 outputs per tile"""
    resample_gradient_beyond_the_grid(tac, cus, 1, 12)


# ----------------------------------------------------------------------------- 3. dct
def dct_once(tac_, xt, d32, what):
    before = dict(tac_._hip.launches)
    got = tac_.dct(xt, d32)
    assert launched_since(tac_, before) == {DCT: 1}, what
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(xt.shape[:-2]) + (d32.shape[1], xt.shape[-1]), what
    return got


def frame_major(x, pad_frames=0, pad_floats=0):
    """device tensor with the values of ``x`` (rows, M, T), stored (rows, T + pad_frames, M + pad_floats) in a NaN-filled store"""
    rows, m, t = x.shape
    store = torch.full((rows, t + pad_frames, m + pad_floats), float('nan'), device='cuda')
    store[:, :t, :m] = x.transpose(-2, -1)
    return store[:, :t, :m].transpose(-2, -1)


def time_slice(x):
    """every second frame of a contiguous (rows, M, 2 T) tensor"""
    wide = torch.full(tuple(x.shape[:-1]) + (2 * x.shape[-1],), float('nan'), device='cuda')
    wide[..., ::2] = x
    return wide[..., ::2]


def dct_load_form(xt):
    """the kernel's three load forms, by the launcher's rule"""
    if xt.stride(1) != 1:
        return 'along time'
    quads = xt.shape[1] % 4 == 0 and xt.data_ptr() % 16 == 0 and xt.stride(2) % 4 == 0 and (xt.shape[0] == 1 or xt.stride(0) % 4 == 0)
    return '16 bytes along m' if quads else 'floats along m'


def dct_base(n_in, seed):
    x = DR.db_like((1, n_in, G.BASE_FRAMES), seed)
    x[..., 1] = 0.0
    x[..., G.BASE_FRAMES - 1] *= np.float32(1e-30)
    return x


@pytest.mark.parametrize('n_in,n_out', [(40, 13), (256, 128)])
def test_dct_tiles_beyond_the_grid(tac, cus, n_in, n_out):
    """(40, 13): tiles of 64 frames, eight workgroups per CU; (256, 128): tiles of 16 frames, one workgroup per CU"""
    d32, d64 = dev(tac.create_dct(n_out, n_in, 'ortho')), DR.dct_matrix64(n_out, n_in, 'ortho')
    base = dct_base(n_in, seed=n_in)
    small = dct_once(tac, frame_major(dev(base)), d32, 'the base frames')
    worst = DR.assert_within(small, base, d64, 'dct %d x %d: the base frames' % (n_in, n_out))
    assert not bool(small[..., 1].any())
    # one row of frames
    c = wrapping(cus, 'dct %d x %d, 1 row' % (n_in, n_out))
    frames = cycle(c['n_frames'], G.BASE_FRAMES)
    x = dev(base)[..., frames]
    forms = set()
    for tag, xt in (('frame-major', frame_major(x)), ('padded', frame_major(x, pad_floats=3)), ('contiguous', x.contiguous())):
        forms.add(dct_load_form(xt))
        got = dct_once(tac, xt, d32, tag)
        assert same_bits(got, small[..., frames]), 'dct %d x %d, %s: a frame depends on where in the row it stands' % (n_in, n_out, tag)
    assert forms == {'16 bytes along m', 'floats along m', 'along time'}
    # three rows the launcher cannot merge into one: row r holds the base frames from 7 r on
    c = wrapping(cus, 'dct %d x %d, 3 rows' % (n_in, n_out))
    frames = torch.stack([cycle(c['n_frames'], G.BASE_FRAMES, 7 * r) for r in range(3)])
    x = dev(base)[0][:, frames].transpose(0, 1)                                       # (3, n_in, T)
    want = small[0][:, frames].transpose(0, 1)
    forms = set()
    for tag, xt in (('frame-major, a frame between rows', frame_major(x, pad_frames=1)), ('time slice', time_slice(x))):
        assert xt.stride(0) != c['n_frames'] * xt.stride(2), 'rows whose frames continue each other would be merged'
        forms.add(dct_load_form(xt))
        got = dct_once(tac, xt, d32, tag)
        assert same_bits(got, want), 'dct %d x %d, 3 rows, %s: a frame depends on where it stands' % (n_in, n_out, tag)
    assert forms == {'16 bytes along m', 'along time'}
    print('dct %d x %d: worst |err| / bound %.3f' % (n_in, n_out, worst))


def test_dct_gradient_tiles_beyond_the_grid(tac, cus):
    n_in, n_out = 40, 13
    c = wrapping(cus, 'dct 40 x 13 gradient')
    d32, d64 = dev(tac.create_dct(n_out, n_in, 'ortho')), DR.dct_matrix64(n_out, n_in, 'ortho')
    g = dct_base(n_out, seed=3)

    def gradient(gt):
        x = frame_major(torch.zeros(1, n_in, gt.shape[-1], device='cuda')).requires_grad_(True)
        y = tac.dct(x, d32)
        before = dict(tac._hip.launches)
        with warnings.catch_warnings():
            warnings.simplefilter('error', tac.CompositeRouteWarning)
            (gx,) = torch.autograd.grad(y, x, grad_outputs=gt)
        assert launched_since(tac, before) == {DCT: 1} and tuple(gx.shape) == tuple(x.shape)
        return gx

    small = gradient(dev(g))
    worst = DR.assert_within(small, g, d64.T, 'dct gradient: the base frames')
    frames = cycle(c['n_frames'], G.BASE_FRAMES)
    big = dev(g)[..., frames]
    for tag, gt in (('contiguous', big.contiguous()), ('frame-major', frame_major(big))):
        assert same_bits(gradient(gt), small[..., frames]), 'dct gradient, grad_out %s: a frame depends on where it stands' % tag
    print('dct 40 x 13 gradient: worst |err| / bound %.3f' % worst)


# ----------------------------------------------------------------------------- 4. tac_spectral_mac_f32 through the C ABI
def mac_call(tac_, X, H, hrow, conj):
    rows, T, F = X.shape[0], X.shape[1], X.shape[2]
    Y = tac_._hip.poison_fill(torch.empty_like(X))
    hmap = None if hrow is None else torch.tensor(hrow, dtype=torch.int32, device='cuda')
    rc = tac_._native.lib().tac_spectral_mac_f32(
        tac_._native.ptr(X), tac_._native.ptr(H), None if hmap is None else tac_._native.ptr(hmap), rows, T, F, H.shape[1], H.shape[0],
        int(conj), tac_._native.ptr(Y), tac_._native.stream_ptr(X.device))
    torch.cuda.synchronize()
    return rc, Y


MAC_MAPS = {'shared': (1, None), 'per-row': (3, [0, 1, 2, 0, 1, 2, 0]), 'permuted': (3, [2, 0, 1, 1, 2, 0, 2])}


@pytest.mark.parametrize('P,conj,kernels', [(4, False, 'shared'), (8, True, 'per-row'), (16, False, 'permuted'), (17, True, 'shared')])
def test_spectral_mac_units_beyond_the_grid(tac, cus, P, conj, kernels):
    """F = 67: one full tile of bins and one of three live lanes, whose dead lanes ``continue`` inside the persistent loop"""
    c = wrapping(cus, 'mac P %d' % P)
    rows, T, F = c['rows'], c['n_frames'], c['n_bins']
    tile = tac._native.lib().tac_spectral_mac_tile(P)
    assert tile == G.mac_tile(P) and T % tile == 1 and F == 67
    h_rows, hrow = MAC_MAPS[kernels]
    gen = torch.Generator(device='cuda').manual_seed(1000 * P + T)
    X = torch.randn(rows, T, F, 2, device='cuda', generator=gen)
    X[1] = 0.0
    X[2] *= 2.0 ** -12
    H = torch.randn(h_rows, P, F, 2, device='cuda', generator=gen)
    what = 'P %d, %d rows of %d frames, conj %s, %s kernels' % (P, rows, T, conj, kernels)
    rc, Y = mac_call(tac, X, H, hrow, conj)
    assert rc == 0, what
    assert int(tac._hip.poison_count(Y)) == 0, what + ': every output written'
    worst = 0.0
    for r in range(rows):                                                             # (row by row: float64 copies of one row)
        re, im, bre, bim = CR.mac_reference(X[r:r + 1].double(), H.double(), None if hrow is None else hrow[r:r + 1], conj)
        for got, ref, bound in ((Y[r:r + 1, ..., 0], re, bre), (Y[r:r + 1, ..., 1], im, bim)):
            err = (got.double() - ref).abs()
            limit = (2 * P + 2) * CR.U * bound
            assert bool((err <= limit).all()), '%s, row %d' % (what, r)
            worst = max(worst, float((err / limit.clamp(min=1e-300)).max()))
    assert not bool(Y[1].any()), what + ': the silent row is exactly zero'
    rc2, Y2 = mac_call(tac, X, H, hrow, conj)
    assert rc2 == 0 and same_bits(Y, Y2), what + ': bit-identical on a second run'
    # the last row alone stays below the grid: the same bits
    rc1, Y1 = mac_call(tac, X[rows - 1:], H, None if hrow is None else hrow[rows - 1:], conj)
    assert rc1 == 0 and G.mac_launch(cus, 1, T, F, P)[0] < 8 * cus and same_bits(Y1[0], Y[rows - 1]), what + ': the last row alone'
    print('spectral mac %s: worst |err| / bound %.3f' % (what, worst))


# ----------------------------------------------------------------------------- 5. fftconvolve through the API
def check_blocks(got, ref, n_fft, what):
    ref = ref if torch.is_tensor(ref) else torch.from_numpy(np.ascontiguousarray(ref))
    ratios = CR.block_ratios(got, ref, n_fft // 2, n_fft)
    worst = float(torch.nan_to_num(ratios, nan=float('inf')).max())
    print('%s: worst per-block ratio %.3g of %.1g' % (what, worst, TIGHT))
    assert worst <= TIGHT, (what, worst)
    return worst


def fftconvolve_once(tac_, xt, ht, n_fft, spectra_launches, what):
    before = dict(tac_._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac_.CompositeRouteWarning)
        got = tac_.fftconvolve(xt, ht, 'full', n_fft=n_fft)
    assert launched_since(tac_, before) == {SPECTRAL: 1, SPECTRA: spectra_launches}, what
    assert got.dtype == torch.float32 and tac_._hip.last_route() == 'spectral-%d' % n_fft, what
    return got


def test_fftconvolve_padded_copy_and_kept_halves_beyond_the_grid(tac, cus):
    c = wrapping(cus, 'fftconvolve shared')
    rows, l_in, m, n_fft = c['rows'], c['l_in'], c['m'], c['n_fft']
    xb = CR.waveform((G.BASE_ROWS, l_in), seed=11)
    h = CR.white_kernel((1, m), seed=12)
    what = '%d rows of %d, one kernel of %d taps at %d' % (rows, l_in, m, n_fft)
    got = fftconvolve_once(tac, repeat_rows(dev(xb), rows), dev(h), n_fft, 1, what)
    assert tuple(got.shape) == (rows, l_in + m - 1) and got.is_contiguous()
    check_blocks(got[:G.BASE_ROWS], CR.reference(xb, h), n_fft, what)
    assert not bool(got[1].any()), 'the silent row is exactly zero'
    assert same_bits(got, repeat_rows(got[:G.BASE_ROWS], rows)), what + ': rows of the same data differ within one launch'


def test_fftconvolve_kernel_partitions_beyond_the_grid(tac, cus):
    c = wrapping(cus, 'fftconvolve per-row')
    rows, l_in, m, n_fft = c['rows'], c['l_in'], c['m'], c['n_fft']
    xb = CR.waveform((G.BASE_ROWS, l_in), seed=21)
    hb = CR.white_kernel((G.BASE_ROWS, m), seed=22)
    what = '%d rows of %d, each with its own kernel of %d taps at %d' % (rows, l_in, m, n_fft)
    got = fftconvolve_once(tac, repeat_rows(dev(xb), rows), repeat_rows(dev(hb), rows), n_fft, 1, what)
    assert tuple(got.shape) == (rows, l_in + m - 1)
    check_blocks(got[:G.BASE_ROWS], CR.reference(xb, hb), n_fft, what)
    assert same_bits(got, repeat_rows(got[:G.BASE_ROWS], rows)), what + ': rows of the same data differ within one launch'


# ----------------------------------------------------------------------------- 6. the row-chunk loop of tac_fftconvolve_f32
def test_fftconvolve_row_chunks_through_the_c_abi(tac):
    """a workspace of two rows for a call of five: the loop runs 2 + 2 + 1, each round with its own x, map and output offsets"""
    lib, ptr = tac._native.lib(), tac._native.ptr
    rows, l_in, stride_r, m, n_fft, h_rows = 5, 5000, 5003, 3000, 2048, 3
    hrow = [2, 0, 1, 2, 0]
    offset, l_out, out_stride = (m - 1) // 2, l_in, l_in + 5                          # what mode 'same' keeps
    x = CR.waveform((rows, l_in), seed=31)
    h = CR.white_kernel((h_rows, m), seed=32)
    ref = CR.crop(CR.reference(x, h[hrow]), l_in, m, 'same')
    assert ref.shape == (rows, l_out)
    store = torch.full((rows, stride_r), float('nan'), device='cuda')
    store[:, :l_in] = dev(x)
    H = tac._hip._conv_spectra(dev(h), n_fft, False)
    assert tuple(H.shape) == (h_rows, 3, n_fft // 2 + 1, 2)
    hmap = torch.tensor(hrow, dtype=torch.int32, device='cuda')

    def need(n_rows):
        return int(lib.tac_fftconvolve_workspace(n_rows, l_in, m, n_fft, offset, l_out))

    one, two, full = need(1), need(2), need(rows)
    per_row = two - one
    assert per_row > 0 and full == one + (rows - 1) * per_row
    work = torch.empty(full // 4, dtype=torch.float32, device='cuda')

    def call(workspace_bytes):
        out = torch.full((rows, out_stride), float('nan'), device='cuda')
        rc = lib.tac_fftconvolve_f32(ptr(store), rows, l_in, stride_r, ptr(H), ptr(hmap), h_rows, m, n_fft, 0, offset, l_out,
                                     ptr(work), workspace_bytes, ptr(out), out_stride, tac._native.stream_ptr(out.device))
        torch.cuda.synchronize()
        return rc, out

    rc, chunked = call(one + per_row)                                                 # room for two rows: 2 + 2 + 1
    assert rc == 0
    assert bool(torch.isnan(chunked[:, l_out:]).all()), 'the floats behind each output row are untouched'
    worst = check_blocks(chunked[:, :l_out], ref, n_fft, 'five rows through a workspace of two, each against its own kernel')
    rc, whole = call(full)
    assert rc == 0 and bool(torch.isnan(whole[:, l_out:]).all())
    check_blocks(whole[:, :l_out], ref, n_fft, 'five rows in one pass')
    check_blocks(chunked[:, :l_out], whole[:, :l_out].cpu().double(), n_fft, 'chunked against the one pass')
    print('row chunks: worst per-block ratio %.3g, bit-identical to the one pass: %s' % (worst, same_bits(chunked[:, :l_out], whole[:, :l_out])))
    rc, untouched = call(one - 1)                                                     # one byte short of a single row
    assert rc == tac._native.TAC_E_INVALID and bool(torch.isnan(untouched).all())


# ----------------------------------------------------------------------------- 7. hpss gradient
def test_hpss_gradient_elements_beyond_the_grid(tac, cus):
    c = wrapping(cus, 'hpss gradient')
    case = dict(case=0, rows=c['rows'], n_freqs=c['n_freqs'], n_frames=c['n_frames'], kf=5, kt=9, hard=False, mask_only=False,
                outputs=(0, 1, 2, 3), frame_major=False, power=2.0, first_gain=0, seed=77, silent_grad=False)
    worst = gr.hpss_case_body(tac, 'cuda', case, test='hpss_grad_wrap')              # (asserts one tac_hpss_backward_f32 launch)
    print('hpss gradient %d x %d x %d, widths (5, 9): worst row error %.3g of 1e-4' % (c['rows'], c['n_freqs'], c['n_frames'], worst))


# ----------------------------------------------------------------------------- 8. istft gradient
def test_istft_gradient_elements_beyond_the_grid(tac, cus):
    c = wrapping(cus, 'istft gradient')
    rows, n_fft, hop, frames = c['rows'], c['n_fft'], c['hop'], c['n_frames']
    w = torch.hann_window(n_fft, dtype=torch.float32) + 0.0625
    z = IR.random_spec(rows, n_fft, frames, seed=n_fft + hop)
    go = torch.randn(rows, hop * (frames - 1), generator=torch.Generator().manual_seed(9))
    want = IR.autograd_grad(z, go, n_fft, hop, w, True, False, None)
    cpu32 = IR.autograd_grad(z, go, n_fft, hop, w, True, False, None, dtype=torch.float32)
    zd = z.cuda().transpose(-3, -2).contiguous().transpose(-3, -2).requires_grad_(True)
    out = tac.istft(zd, n_fft, hop, n_fft, w.cuda())
    before = dict(tac._hip.launches)
    out.backward(go.cuda())
    since = launched_since(tac, before)
    assert since == {'tac_istft_grad_input_f32': 1, 'tac_stft_f32': 1, 'tac_istft_grad_bins_f32': 1}, since
    ref = fbnd.frames_of(want, 'complex')
    theirs = float(fbnd.linear_frame_errors(fbnd.frames_of(cpu32, 'complex'), ref).max())
    mine = float(torch.nan_to_num(fbnd.linear_frame_errors(fbnd.frames_of(zd.grad.cpu(), 'complex'), ref), nan=math.inf).max())
    bound = min(GRAD, 4.0 * theirs)
    print('istft gradient %d rows x %d frames: kernel %.3g, float32 CPU autograd %.3g, |err| / bound %.3f' % (rows, frames, mine, theirs, mine / bound))
    assert mine <= bound, (mine, theirs)
    g = zd.grad.cpu()
    assert not bool(g[:, 0, :, 1].any()) and not bool(g[:, -1, :, 1].any())
