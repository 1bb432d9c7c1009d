"""-m gpu: ``dct`` / ``DCT`` / ``MFCC`` on the gfx950 kernel (csrc/mfcc.hip) — strict mode and poisoned outputs on, as in
tests/test_istft_gpu.py.

Reference and bound: tests/dct_rules.py — float64 ``x @ D64`` and, per element, ``(n_in + 2) * 2^-24 * (|x| @ |D64|)``; every
element is checked.  The shapes are the smallest that reach each path of the kernel: 1 / 63 / 64 / 65 / 257 frames (a lone frame,
the edges of the 64-frame tile, more than one tile per row), 1 and 3 rows, matrices from 8 x 1 up to the cap (256 x 128: tiles of
16 frames; 129 x 254: odd sizes at the cap, more columns than rows), and every load form: frame-major (16-byte loads), frame-major
with a padded or misaligned row (float loads), time-contiguous, and a strided time slice.

The training step's tolerance, 1e-3 of a row's largest gradient, is the one tests/test_gpu_parity.py
(test_fft_length_400_trains_on_the_mixed_radix_kernels, ``rel_err(...) < 1e-3`` for the fused mel chain with its dB epilogue at
fft_length 400) holds the mel chain's waveform gradient to."""
import warnings

import numpy as np
import pytest
import torch

import dct_rules as R
from oracle import signals, torch_ref

pytestmark = pytest.mark.gpu

MEL400_GRAD = 1e-3
SIZES = [(8, 8), (8, 1), (23, 13), (40, 13), (80, 40), (128, 40), (128, 128), (256, 128), (129, 254)]
FRAMES = (1, 63, 64, 65, 257)
ENTRY = 'tac_dct_rows_f32'


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
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to('cuda')


def matrices(tac_, n_in, n_out, norm):
    """(float32 matrix for the kernel, float64 reference matrix): the DCT-II where one exists (n_out <= n_in), else a random
    matrix whose float32 values are the reference's"""
    if n_out <= n_in:
        return tac_.create_dct(n_out, n_in, norm), R.dct_matrix64(n_out, n_in, norm)
    d64 = R.random_matrix64(n_in, n_out, seed=7 if norm is None else 8)
    return torch.from_numpy(d64.astype(np.float32)), d64


def values(lead, n_in, frames, seed):
    """dB-like (…, n_in, frames) with one all-zero frame and one frame at 1e-30 scale (where there are frames to spare)"""
    x = R.db_like(tuple(lead) + (n_in, frames), seed)
    if frames >= 3:
        x[..., :, 1] = 0.0
        x[..., :, frames - 1] *= np.float32(1e-30)
    return x


def frame_major(x):
    """device tensor with the values of ``x`` (…, M, T), stored (…, T, M): what the mel kernels return"""
    return dev(np.swapaxes(x, -1, -2)).transpose(-2, -1)


def padded(x, pad=3):
    """frame-major with ``pad`` floats between frames: stride_t = M + pad, not a multiple of four for the sizes here"""
    lead, (m, t) = x.shape[:-2], x.shape[-2:]
    store = torch.full(tuple(lead) + (t, m + pad), float('nan'), device='cuda')
    store[..., :m] = dev(np.swapaxes(x, -1, -2))
    return store[..., :m].transpose(-2, -1)


def misaligned(x):
    """frame-major and dense, but starting one float into its allocation: 4-byte aligned only"""
    store = torch.full((x.size + 1,), float('nan'), device='cuda')
    store[1:] = dev(np.swapaxes(x, -1, -2)).reshape(-1)
    lead, (m, t) = x.shape[:-2], x.shape[-2:]
    return store[1:].view(tuple(lead) + (t, m)).transpose(-2, -1)


def time_slice(x):
    """every second frame of a contiguous (…, M, 2 T) tensor: stride_t = 2, stride_m = 2 T"""
    wide = torch.full(tuple(x.shape[:-1]) + (2 * x.shape[-1],), float('nan'), device='cuda')
    wide[..., ::2] = dev(x)
    return wide[..., ::2]


LAYOUTS = (('frame-major', frame_major), ('contiguous', dev), ('padded', padded), ('misaligned', misaligned),
           ('time slice', time_slice))


def run_one(tac_, xt, d32, what):
    before = dict(tac_._hip.launches)
    got = tac_.dct(xt, d32)
    assert launched_since(tac_, before) == {ENTRY: 1}, what
    assert type(got) is torch.Tensor and got.dtype == torch.float32
    assert tuple(got.shape) == tuple(xt.shape[:-2]) + (d32.shape[1], xt.shape[-1]), what
    assert got.transpose(-2, -1).is_contiguous(), '%s: strides %r are not frame-major' % (what, got.stride())
    return got


# ----------------------------------------------------------------------------- the kernel, element by element
@pytest.mark.parametrize('norm', [None, 'ortho'])
@pytest.mark.parametrize('n_in,n_out', SIZES)
def test_kernel_within_the_bound(tac, n_in, n_out, norm):
    d32, d64 = matrices(tac, n_in, n_out, norm)
    d32 = dev(d32)
    worst = 0.0
    for frames in FRAMES:
        for rows in (1, 3):
            x = values((rows,), n_in, frames, seed=1000 * n_in + 10 * frames + rows)
            for tag, build in LAYOUTS:
                what = '%d x %d %s, %d rows of %d frames, %s' % (n_in, n_out, norm, rows, frames, tag)
                xt = build(x)
                assert tuple(xt.shape) == x.shape and np.array_equal(xt.cpu().numpy(), x), what
                got = run_one(tac, xt, d32, what)
                worst = max(worst, R.assert_within(got, x, d64, what))
                if frames >= 3:
                    assert not bool(got[..., 1].any()), '%s: the all-zero frame is not exactly zero' % what
        x4 = values((2, 3), n_in, frames, seed=77 * n_in + frames)
        what = '%d x %d %s, (2, 3, M, %d)' % (n_in, n_out, norm, frames)
        worst = max(worst, R.assert_within(run_one(tac, frame_major(x4), d32, what), x4, d64, what))
        # leading dims no single row stride expresses (copied by the launcher), and a 2-D input
        swapped = dev(x4).transpose(0, 1)
        worst = max(worst, R.assert_within(run_one(tac, swapped, d32, what + ' swapped'), np.swapaxes(x4, 0, 1), d64, what))
        worst = max(worst, R.assert_within(run_one(tac, frame_major(x4[0, 0]), d32, what + ' 2-D'), x4[0, 0], d64, what))
    print('dct %d x %d %s: worst |err| / bound %.3f' % (n_in, n_out, norm, worst))


def test_two_calls_agree_bit_for_bit(tac):
    for n_in, n_out in ((128, 40), (129, 254)):
        d32, _ = matrices(tac, n_in, n_out, 'ortho')
        d32 = dev(d32)
        for build in (frame_major, dev, time_slice):
            xt = build(values((3,), n_in, 257, seed=n_in))
            assert torch.equal(tac.dct(xt, d32), tac.dct(xt, d32))


def test_nan_stays_in_its_frame(tac):
    for (n_in, n_out), build in (((128, 40), frame_major), ((80, 40), dev), ((23, 13), padded), ((256, 128), frame_major)):
        d32, d64 = matrices(tac, n_in, n_out, None)
        x = values((3,), n_in, 65, seed=5 + n_in)
        clean = x.copy()
        x[1, n_in // 2, 17] = np.nan
        got = tac.dct(build(x), dev(d32))
        hit = torch.isnan(got).cpu().numpy()
        want = np.zeros_like(hit)
        want[1, :, 17] = True
        assert np.array_equal(hit, want), 'NaN in %d elements, expected the %d of frame (1, 17)' % (int(hit.sum()), n_out)
        got = got.clone()
        got[1, :, 17] = 0.0
        clean[1, :, 17] = 0.0
        R.assert_within(got, clean, d64, 'the frames next to a NaN, %d x %d' % (n_in, n_out))


# ----------------------------------------------------------------------------- gradient
@pytest.mark.parametrize('n_in,n_out', [(23, 13), (128, 40), (256, 128)])
def test_gradient_is_the_kernel_with_the_transposed_matrix(tac, n_in, n_out):
    d32, d64 = matrices(tac, n_in, n_out, 'ortho')
    d32 = dev(d32)
    x = frame_major(values((3,), n_in, 65, seed=n_out)).requires_grad_(True)
    g = values((3,), n_out, 65, seed=n_out + 1)
    for tag, gt in (('contiguous', dev(g)), ('frame-major', frame_major(g))):
        y = tac.dct(x, d32)
        before = dict(tac._hip.launches)
        with warnings.catch_warnings():
            warnings.simplefilter('error', tac.CompositeRouteWarning)
            (gx,) = torch.autograd.grad(y, x, grad_outputs=gt)
        assert launched_since(tac, before) == {ENTRY: 1}, tag
        assert tuple(gx.shape) == tuple(x.shape) and gx.transpose(-2, -1).is_contiguous()
        R.assert_within(gx, g, d64.T, 'grad_x %d x %d, grad_out %s' % (n_in, n_out, tag))
    # the matrix's own gradient has no kernel: refused under strict
    dm = d32.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.dct(x.detach(), dm).sum().backward()


# ----------------------------------------------------------------------------- refusals
def test_sizes_beyond_the_cap(tac):
    n = 256
    x = R.db_like((2, n, 9), seed=3)
    xt = frame_major(x)
    d64 = R.random_matrix64(n, n, seed=4)
    d32 = dev(d64.astype(np.float32))
    rows = xt.transpose(-2, -1)                                      # (2, 9, 256) contiguous
    out = torch.full((2, 9, n), 123.0, device='cuda')
    rc = tac._native.lib().tac_dct_rows_f32(tac._native.ptr(rows), 2, n, 9, 9 * n, 1, n, tac._native.ptr(d32), n,
                                            tac._native.ptr(out), tac._native.stream_ptr(out.device))
    torch.cuda.synchronize()
    assert rc == tac._native.TAC_E_UNSUPPORTED and bool((out == 123.0).all())
    before = dict(tac._hip.launches)
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.dct(xt, d32)
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.dct(xt.double()[:, :8], dev(R.dct_matrix64(8, 8)))       # float64 on the device
    assert launched_since(tac, before) == {}
    tac.set_strict(False)
    try:
        for xin, mat, ref_d in ((xt, d32, d64), (xt.double()[:, :8], dev(R.dct_matrix64(8, 8)), R.dct_matrix64(8, 8))):
            for key in [k for k in tac._ops._warned if k[0] == 'dct']:
                tac._ops._warned.discard(key)
            with pytest.warns(tac.CompositeRouteWarning):
                got = tac.dct(xin, mat)
            assert got.dtype == xin.dtype and launched_since(tac, before) == {}
            R.assert_within(got, xin.cpu().numpy(), ref_d, 'stock-torch route, %s' % xin.dtype)
    finally:
        tac.set_strict(True)


# ----------------------------------------------------------------------------- the chain
@pytest.mark.parametrize('num_coeffs,num_mels,n_fft,hop', [(13, 40, 400, 160), (40, 128, 2048, 512)])
def test_mfcc_is_the_fused_mel_launch_plus_one(tac, num_coeffs, num_mels, n_fft, hop):
    kw = dict(num_mels=num_mels, sample_rate=16000, fft_length=n_fft, hop_length=hop)
    x = dev(signals.audio_like((2, 2, 24000), seed=13))
    parent = torch.nn.Sequential(*tac.Melspectrogram(**kw), tac.AmplitudeToDb()).cuda()
    before = dict(tac._hip.launches)
    db = parent(x)
    mel_launch = launched_since(tac, before)
    assert len(mel_launch) == 1 and list(mel_launch.values()) == [1], mel_launch
    mfcc = tac.MFCC(num_coeffs=num_coeffs, **kw).cuda()
    before = dict(tac._hip.launches)
    got = mfcc(x)
    assert launched_since(tac, before) == dict(mel_launch, **{ENTRY: 1})
    d32 = dev(tac.create_dct(num_coeffs, num_mels))
    assert type(got) is torch.Tensor and tuple(got.shape) == (2, 2, num_coeffs, 1 + 24000 // hop)
    assert torch.equal(got, tac.dct(db, d32)) and torch.equal(mfcc[4].dct_matrix, d32)
    R.assert_within(got, db.cpu().numpy(), R.dct_matrix64(num_coeffs, num_mels), 'MFCC %d/%d' % (n_fft, hop))
    # codes in front of the chain still reach the coded fused launch
    codes = tac.mu_law_encoding(x, 256)
    before = dict(tac._hip.launches)
    coded = torch.nn.Sequential(tac.MuLawDecoding(256), *parent)(codes)
    coded_launch = launched_since(tac, before)
    before = dict(tac._hip.launches)
    got_coded = torch.nn.Sequential(tac.MuLawDecoding(256), *mfcc)(codes)
    assert launched_since(tac, before) == dict(coded_launch, **{ENTRY: 1})
    assert torch.equal(got_coded, tac.dct(coded, d32))


def test_training_step(tac):
    kw = dict(num_mels=40, sample_rate=16000, fft_length=400, hop_length=160)
    x = signals.audio_like((2, 1, 8000), seed=21)
    mfcc = tac.MFCC(num_coeffs=13, **kw).cuda()
    xg = dev(x).requires_grad_(True)
    assert tac._ops.strict()
    before = dict(tac._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac.CompositeRouteWarning)
        mfcc(xg).square().mean().backward()
    assert launched_since(tac, before).get(ENTRY) == 2                  # forward, and the gradient with the transposed matrix
    got = xg.grad.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0
    xc = torch.from_numpy(x).double().requires_grad_(True)
    bank = torch_ref.create_mel_filter(201, 40, 0.0, 8000, False).double()
    db = torch_ref.amplitude_to_db(torch_ref.apply_filterbank(torch_ref.complex_norm(torch_ref.stft(xc, 400, 160), 2.0), bank))
    coeffs = torch_ref.apply_filterbank(db, torch.from_numpy(R.dct_matrix64(13, 40)))
    coeffs.square().mean().backward()
    want = xc.grad.numpy()
    for r in range(2):
        err = np.abs(got[r, 0] - want[r, 0]).max() / np.abs(want[r, 0]).max()
        print('MFCC 400/160 training step, row %d: gradient error %.3g of the row maximum' % (r, err))
        assert err < MEL400_GRAD, (r, err)
