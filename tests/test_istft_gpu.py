"""-m gpu: ``istft`` / ``ISTFT`` on the gfx950 kernels (csrc/istft.hip) — strict mode and poisoned outputs on, as in
tests/test_stretch_gpu.py.

Reference: ``torch.istft`` in float64 on the CPU on the same float32 spectrogram (tests/istft_rules.py).  Bounds:

  * every row within TIGHT = 2e-6 of its own maximum (the constant the forward rows are held to; ``torch.istft`` in float32
    stays within 2.3e-7 on these geometries);
  * every block of ``hop`` samples within 4 x the worst ratio ``torch.istft`` in float32 on the CPU reaches over the same
    inputs, its error divided by the largest reference magnitude over the blocks within ``fft_length`` of it
    (``istft_rules.block_ratios``); computed here, reported through ``frame_bounds.report``;
  * round trip: 4 x the worst per-row error of ``torch.stft`` / ``torch.istft`` in float32 on the CPU over the same inputs;
  * gradient: per frame within GRAD = 1e-3 and within 4 x the worst per-frame error of float32 CPU autograd.

fft_length 2048 at hop 256 / 512 / 1024 runs the fused one-launch route (``istft_fused_kernel``), everything else the general
(two-launch) route; the route tests assert which by name.
"""
import math

import numpy as np
import pytest
import torch

import frame_bounds as fbnd
import istft_rules as R
from oracle import signals, torch_ref
from stretch_rules import phase_advance

pytestmark = pytest.mark.gpu

TIGHT = 2e-6
GRAD = 1e-3
GOLDEN = 'g12_stft_backward_pin'


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


def hann(n):
    return torch.hann_window(n, dtype=torch.float32)


#: (tag, fft_length, hop, win_length, normalized, user window, rows, frames)
CASES = [
    ('2048/256', 2048, 256, 2048, False, False, 3, 40), ('2048/512', 2048, 512, 2048, False, False, 64, 120),
    ('2048/1024', 2048, 1024, 2048, False, False, 3, 33), ('2048/128', 2048, 128, 2048, False, False, 1, 300),
    ('2048/384', 2048, 384, 2048, False, False, 3, 21), ('2048/640', 2048, 640, 2048, True, False, 3, 17),
    ('2048/512 two frames', 2048, 512, 2048, False, False, 3, 2), ('2048/512 short window', 2048, 512, 1200, False, False, 3, 25),
    ('256/64', 256, 64, 256, False, False, 64, 301), ('256/32 user', 256, 32, 256, True, True, 3, 50),
    ('400/160', 400, 160, 400, False, False, 64, 200), ('400/100 short window', 400, 100, 256, False, False, 3, 31),
    ('400/160 two frames', 400, 160, 400, True, False, 1, 2),
    ('512/128', 512, 128, 512, False, False, 3, 150), ('512/100 user', 512, 100, 512, False, True, 3, 41),
    ('1024/256', 1024, 256, 1024, True, False, 64, 80), ('1024/255', 1024, 255, 1024, False, False, 3, 19),
    ('4096/1024', 4096, 1024, 4096, False, False, 3, 40), ('4096/512 short window', 4096, 512, 3000, True, False, 1, 12),
    ('960/240', 960, 240, 960, False, False, 3, 60), ('960/480 user', 960, 480, 960, True, True, 64, 35),
    ('8192/2048', 8192, 2048, 8192, False, False, 3, 9), ('8192/1024', 8192, 1024, 8192, True, False, 1, 5),
]


def case_window(case):
    _, n_fft, hop, wl, normalized, user, rows, frames = case
    if not user:
        return hann(wl)
    gen = torch.Generator().manual_seed(wl + hop)
    return (hann(wl) * 0.75 + 0.25 + 0.05 * torch.rand(wl, generator=gen)).float()


def case_specs(case, seed):
    """the two spectrograms of a case: the CPU stft of audio-like rows (row 1 silent, row 2 at gain 2^-12 when there are three
    or more), and normal pairs no waveform has as its stft — with the same silent row"""
    _, n_fft, hop, wl, normalized, user, rows, frames = case
    w = case_window(case)
    x, z = R.consistent_spec((rows, hop * (frames - 1)), n_fft, hop, w, seed, normalized=normalized)
    assert z.shape == (rows, n_fft // 2 + 1, frames, 2)
    zr = R.random_spec(rows, n_fft, frames, seed + 1)
    if rows >= 3:
        zr[1] = 0.0
        zr[2] *= 2.0 ** -12
    return w, x, (('stft', z), ('randn', zr))


def check_parity(tac, got, spec, n_fft, hop, w, normalized, length, test, tag):
    """rows against TIGHT, silent rows exactly zero.  Returns the worst block ratio of the kernel and of ``torch.istft`` in float32
    on the CPU (the sweep holds the former to 4 x the latter's worst over all of its inputs)."""
    want = R.torch_istft(spec, n_fft, hop, w, True, normalized, length)
    cpu32 = R.torch_istft(spec, n_fft, hop, w, True, normalized, length, dtype=torch.float32)
    g = got.detach().cpu()
    assert g.shape == want.shape, (g.shape, want.shape)
    worst = fbnd.assert_rows(g.reshape(-1, g.shape[-1]), want.reshape(-1, want.shape[-1]), TIGHT, '%s %s' % (test, tag))
    fbnd.report(test, tag, n_fft, 'rows', worst, TIGHT)
    for r in range(want.reshape(-1, want.shape[-1]).shape[0]):
        if not bool(spec.reshape((-1,) + tuple(spec.shape[-3:]))[r].any()):
            assert not bool(g.reshape(-1, g.shape[-1])[r].any()), '%s %s: silent row %d is not exactly zero' % (test, tag, r)
    mine = float(torch.nan_to_num(R.block_ratios(g, want, hop, n_fft), nan=math.inf).max())
    theirs = float(R.block_ratios(cpu32, want, hop, n_fft).max())
    return mine, theirs


# ----------------------------------------------------------------------------- G1
def test_parity_sweep(tac):
    results, ref_worst = [], 0.0
    for i, case in enumerate(CASES):
        tag, n_fft, hop, wl, normalized, user, rows, frames = case
        w, x, specs = case_specs(case, 300 + i)
        for name, z in specs:
            before = dict(tac._hip.launches)
            got = tac.istft(z.cuda().transpose(-3, -2).contiguous().transpose(-3, -2), n_fft, hop, wl, w.cuda(),
                            normalized=normalized)
            assert launched_since(tac, before).get('tac_istft_f32') == 1, (tag, launched_since(tac, before))
            route = tac._native.lib().tac_last_route().decode()
            assert route.startswith('istft_fused_kernel' if (n_fft == 2048 and hop in (256, 512, 1024)) else 'istft_general'), (tag, route)
            mine, theirs = check_parity(tac, got, z, n_fft, hop, w, normalized, None, 'istft_parity', '%s %s' % (tag, name))
            results.append((tag, name, n_fft, mine))
            ref_worst = max(ref_worst, theirs)
    bound = 4.0 * ref_worst
    assert bound > 0.0
    bad = []
    for tag, name, n_fft, mine in results:
        fbnd.report('istft_parity', '%s %s' % (tag, name), n_fft, 'blocks', mine, bound)
        if not mine <= bound:
            bad.append((tag, name, mine))
    print('istft block ratios: worst kernel %.3g, float32 CPU reference %.3g, bound %.3g'
          % (max(r[3] for r in results), ref_worst, bound))
    assert not bad, 'blocks beyond 4 x the float32 reference worst ratio %.3g: %r' % (ref_worst, bad)


# ----------------------------------------------------------------------------- G2
def test_routes_and_layouts(tac):
    h = tac._native.lib()
    x = torch.from_numpy(signals.audio_like((2, 3, 16000), seed=21)).cuda()
    for n_fft, hop in ((2048, 256), (2048, 512), (2048, 1024), (2048, 384), (400, 160), (960, 240), (8192, 2048)):
        fused = n_fft == 2048 and hop in (256, 512, 1024)
        z = tac.stft(x, n_fft, hop)
        want = R.torch_istft(z, n_fft, hop, hann(n_fft), True, False, 16000)
        before, lay = dict(tac._hip.launches), dict(tac._hip.istft_layout)
        got = tac.istft(z, n_fft, hop, length=16000)
        since = launched_since(tac, before)
        since.pop('tac_istft_envelope_f32', None)            # (once per window and geometry)
        assert since == {'tac_istft_f32': 1}, (n_fft, since)
        assert tac._hip.istft_layout['in_place'] == lay['in_place'] + 1 and tac._hip.istft_layout['copied'] == lay['copied']
        route = h.tac_last_route().decode()
        assert route == ('istft_fused_kernel<%d>' % hop) if fused else route.startswith('istft_general<%d>' % n_fft), route
        fbnd.assert_rows(got.reshape(6, -1), want.reshape(6, -1), TIGHT, 'istft route %d' % n_fft)
        # a dense (F, T, 2)-ordered tensor: copied to frame-major first, same values
        dense = z.contiguous()
        assert dense.stride(-3) == dense.shape[-2] * 2
        again = tac.istft(dense, n_fft, hop, length=16000)
        assert tac._hip.istft_layout['copied'] == lay['copied'] + 1
        assert torch.equal(again, got)
        desc = tac._hip._istft_desc(6, 16000, 16000, n_fft, hop, n_fft, True, False)
        assert h.tac_istft_workspace(desc, z.shape[-2]) == (0 if fused else 6 * z.shape[-2] * n_fft * 4)
        if fused:       # the general route on the same input (the measuring tool's switch): the same frames added in the same order
            general = tac._hip.istft(z, tac.functional.default_window(n_fft, z), n_fft, hop, n_fft, True, False, 16000, route='general')
            assert h.tac_last_route().decode().startswith('istft_general<2048>')
            fbnd.assert_rows(general.reshape(6, -1), want.reshape(6, -1), TIGHT, 'istft general route %d/%d' % (n_fft, hop))
            assert float((general - got).abs().max()) <= 2 * TIGHT * float(want.abs().max())
    # the rows the phase vocoder writes are read in place as well
    z = tac.stft(x, 512, 128)
    st = tac.phase_vocoder(z, 1.3, phase_advance(128, 257).cuda())
    lay = dict(tac._hip.istft_layout)
    out = tac.istft(st, 512, 128)
    assert tac._hip.istft_layout['in_place'] == lay['in_place'] + 1 and tac._hip.istft_layout['copied'] == lay['copied']
    assert out.shape == (2, 3, 128 * (st.shape[-2] - 1))
    # second call on the same window and geometry: no envelope launch, nothing but the inverse
    before = dict(tac._hip.launches)
    tac.istft(st, 512, 128)
    assert launched_since(tac, before) == {'tac_istft_f32': 1}


def test_off_the_kernels_is_announced(tac):
    z = torch.randn(2, 512, 9, 2, device='cuda')
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.istft(z, 512, 128, onesided=False)
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.istft(torch.randn(2, 257, 9, 2, device='cuda', dtype=torch.float64), 512, 128)
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.istft(torch.randn(2, 12, 9, 2, device='cuda'), 22, 5)              # 11 is not 7-smooth
    tac.set_strict(False)
    try:
        with pytest.warns(tac.CompositeRouteWarning):
            got = tac.istft(z, 512, 128, window=hann(512).cuda(), onesided=False)
        want = torch.istft(torch.view_as_complex(z), 512, 128, window=hann(512).cuda(), onesided=False)
        assert torch.equal(got, want)
    finally:
        tac.set_strict(True)
    # NOLA on the device: the same error kind and condition as torch.istft
    with pytest.raises(RuntimeError, match='window overlap add'):
        tac.istft(z[:, :257], 512, 512)
    with pytest.raises(RuntimeError, match='window overlap add'):
        tac.istft(z[:, :257], 512, 128, center=False)
    # center=False runs on the kernels where the window allows it
    ones = torch.ones(512)
    got = tac.istft(z[:, :257], 512, 128, window=ones.cuda(), center=False)
    want = torch.istft(torch.view_as_complex(z[:, :257].cpu().double().contiguous()), 512, 128, window=ones.double(), center=False)
    fbnd.assert_rows(got, want, TIGHT, 'istft center=False')


# ----------------------------------------------------------------------------- G3
def test_round_trip(tac):
    for seed, (n_fft, hop, rows, length) in enumerate(((2048, 512, 3, 40000), (400, 160, 64, 16000), (1024, 256, 3, 30000),
                                                       (960, 240, 3, 20000), (4096, 1024, 1, 50000))):
        x = torch.from_numpy(signals.audio_like((rows, length), seed=40 + seed))
        w = hann(n_fft)
        z32 = torch.stft(x, n_fft, hop, window=w, return_complex=True)
        back32 = torch.istft(z32, n_fft, hop, window=w, length=length)
        cpu_err = (back32.double() - x.double()).abs().amax(-1)                 # per row, float32 CPU round trip
        got = tac.istft(tac.stft(x.cuda(), n_fft, hop), n_fft, hop, length=length)
        err = (got.cpu().double() - x.double()).abs().amax(-1)
        bound = 4.0 * float(cpu_err.max())
        fbnd.report('istft_round_trip', '%d/%d' % (n_fft, hop), n_fft, 'abs', float(err.max()), bound)
        print('round trip %d/%d: kernel %.3g, float32 CPU %.3g' % (n_fft, hop, float(err.max()), float(cpu_err.max())))
        assert float(err.max()) <= bound, (n_fft, hop, float(err.max()), bound)


def test_stretch_chain(tac):
    """STFT -> TimeStretch(rate) -> ISTFT against the float64 oracle chain.  The phase vocoder is documented to 1e-5 of the
    tensor maximum per component (tests/test_gpu_parity.py); carried through the linear inverse: a frame's irfft of a spectrum
    error of at most e = sqrt(2) 1e-5 max|Z| per complex bin is at most e per sample ((1 / N) times N bins), and the windowed
    overlap-add over the envelope is at most kappa = max_j sum_t |w| / sum_t w^2 times that (4 / 3 for Hann at 75 % overlap,
    evaluated from the window below) — plus TIGHT of the row maximum for the inverse itself.  The oracle's stretched spectrogram
    is ``torch_ref.phase_vocoder`` itself: ``stretch_rules.oracle_chain`` ends in ``complex_norm`` and its magnitudes cannot feed an
    inverse."""
    n_fft, hop = 512, 128
    x = torch.from_numpy(signals.audio_like((2, 2, 12000), seed=77))
    w64 = hann(n_fft).double()
    for rate in (0.8, 1.3):
        model = torch.nn.Sequential(tac.STFT(n_fft, hop), tac.TimeStretch(hop, n_fft // 2 + 1, fixed_rate=rate),
                                    tac.ISTFT(n_fft, hop)).cuda()
        got = model(x.cuda())
        z = torch_ref.stft(x.double(), n_fft, hop, window=w64)
        n_out = int(math.ceil(z.shape[-2] / rate))
        assert got.shape == (2, 2, hop * (n_out - 1)), got.shape
        st = torch_ref.phase_vocoder(z, rate, phase_advance(hop, n_fft // 2 + 1, torch.float64))
        want = R.torch_istft(st, n_fft, hop, w64)
        num = torch.zeros(hop * (n_out - 1) + n_fft, dtype=torch.float64)
        den = torch.zeros_like(num)
        for t in range(n_out):
            num[t * hop:t * hop + n_fft] += w64.abs()
            den[t * hop:t * hop + n_fft] += w64 * w64
        kappa = float((num / den)[n_fft // 2:-(n_fft // 2)].max())
        bound = math.sqrt(2.0) * 1e-5 * float(st.abs().max()) * kappa + TIGHT * float(want.abs().max())
        err = float((got.cpu().double() - want).abs().max())
        fbnd.report('istft_stretch_chain', 'rate %g' % rate, n_fft, 'abs', err, bound)
        assert err <= bound, (rate, err, bound)


# ----------------------------------------------------------------------------- G4
@pytest.mark.parametrize('n_fft,hop', [(2048, 512), (400, 160), (512, 100)])
def test_length_trims_and_pads(tac, n_fft, hop):
    """``torch.istft`` keeps the padded positions [pad, pad + length): a length beyond hop (T - 1) reads on into the last half frame,
    where a Hann window's envelope falls to w[N - 1]^2 (5.5e-12 at 2048: the NOLA error; 4e-9 at 400: float32 rounding divided by
    it) — so the longer lengths run with a window that has no vanishing tap, the shorter ones with Hann."""
    frames = 23
    z = R.random_spec(3, n_fft, frames, seed=n_fft)
    full = hop * (frames - 1)
    for length in (full - 3 * hop - 5, full - 1, full + 7, full + n_fft // 2, full + n_fft // 2 + 1001):
        w = hann(n_fft) if length <= full else hann(n_fft) + 0.125
        got = tac.istft(z.cuda(), n_fft, hop, window=w.cuda(), length=length)
        assert got.shape == (3, length)
        want = R.torch_istft(z, n_fft, hop, w, True, False, length)
        fbnd.assert_rows(got, want, TIGHT, 'istft length %d of %d' % (length, full))
        tail = full + n_fft // 2                          # torch.istft keeps positions up to the end of the last frame
        if length > tail:
            assert not bool(want[:, tail:].any()) and not bool(got[:, tail:].any()), 'the tail is exactly zero'
    lay = tac.ISTFT(n_fft, hop).cuda()
    assert torch.equal(lay(z.cuda(), length=full - 1), tac.istft(z.cuda(), n_fft, hop, window=lay.window, length=full - 1))
    if n_fft == 2048:                                    # Hann read to the end of the last frame: NOLA, here as in torch.istft
        with pytest.raises(RuntimeError, match='window overlap add'):
            R.torch_istft(z, n_fft, hop, hann(n_fft), True, False, full + n_fft // 2, dtype=torch.float32)
        with pytest.raises(RuntimeError, match='window overlap add'):
            tac.istft(z.cuda(), n_fft, hop, window=hann(n_fft).cuda(), length=full + n_fft // 2)


# ----------------------------------------------------------------------------- G5
@pytest.mark.parametrize('n_fft,hop', [(2048, 512), (400, 160), (960, 240)])
def test_nan_bin_poisons_its_frame_only(tac, n_fft, hop):
    frames = 30
    z = R.random_spec(2, n_fft, frames, seed=3 * n_fft)
    z[0, 17, 11, 1] = float('nan')
    w = hann(n_fft) + 0.125                               # (no zero tap: NaN x 0 does not decide the edge of the frame)
    want32 = R.torch_istft(z, n_fft, hop, w, True, False, None, dtype=torch.float32)
    got = tac.istft(z.cuda(), n_fft, hop, window=w.cuda()).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want32))
    lo, hi = 11 * hop - n_fft // 2, 11 * hop + n_fft // 2
    mask = torch.zeros_like(got, dtype=torch.bool)
    mask[0, max(lo, 0):hi] = True
    assert torch.equal(torch.isnan(got), mask), 'exactly the samples of frame 11 inside the kept range'
    want = R.torch_istft(torch.nan_to_num(z), n_fft, hop, w)
    keep = ~mask
    assert float((got.double() - want).abs()[keep].max()) <= TIGHT * float(want.abs().max())


# ----------------------------------------------------------------------------- G6
@pytest.mark.parametrize('case', [(2048, 512, 2048, False, 3, 20, None), (2048, 384, 1200, True, 2, 9, 3000), (400, 160, 400, False, 3, 40, None),
                                  (960, 240, 960, True, 2, 15, 4000), (512, 128, 512, False, 3, 33, 4600), (8192, 2048, 8192, False, 1, 4, None)])
def test_gradient(tac, case):
    n_fft, hop, wl, normalized, rows, frames, length = case
    w = hann(wl) + 0.0625
    z = R.random_spec(rows, n_fft, frames, seed=n_fft + hop)
    out_len = length or hop * (frames - 1)
    go = torch.randn(rows, out_len, generator=torch.Generator().manual_seed(9))
    want = R.autograd_grad(z, go, n_fft, hop, w, True, normalized, length)
    cpu32 = R.autograd_grad(z, go, n_fft, hop, w, True, normalized, length, dtype=torch.float32)
    zd = z.cuda().transpose(-3, -2).contiguous().transpose(-3, -2).requires_grad_(True)
    out = tac.istft(zd, n_fft, hop, wl, w.cuda(), normalized=normalized, length=length)
    before = dict(tac._hip.launches)
    out.backward(go.cuda())
    since = launched_since(tac, before)
    assert since == {'tac_istft_grad_input_f32': 1, 'tac_stft_f32': 1, 'tac_istft_grad_bins_f32': 1}, since
    ref = fbnd.frames_of(want, 'complex')
    theirs = float(fbnd.linear_frame_errors(fbnd.frames_of(cpu32, 'complex'), ref).max())
    mine = float(torch.nan_to_num(fbnd.linear_frame_errors(fbnd.frames_of(zd.grad.cpu(), 'complex'), ref), nan=math.inf).max())
    bound = min(GRAD, 4.0 * theirs)
    fbnd.report('istft_gradient', str(case), n_fft, 'grad', mine, bound)
    print('istft gradient %r: kernel %.3g, float32 CPU autograd %.3g' % (case, mine, theirs))
    assert mine <= bound, (case, mine, theirs)
    g = zd.grad.cpu()
    assert not bool(g[:, 0, :, 1].any()) and not bool(g[:, -1, :, 1].any())
    # the window's gradient has no kernel: announced, an error in strict mode
    wd = w.cuda().requires_grad_(True)
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.istft(zd.detach(), n_fft, hop, wl, wd, normalized=normalized, length=length).sum().backward()


# ----------------------------------------------------------------------------- G7
def test_full_size(tac):
    """256 rows x 160 000 samples at 2048 / 512 through the fused route, compared row chunk by row chunk against ``torch.istft``
    in float64 on the device tensors' values (CPU float64 per chunk)."""
    n_fft, hop, rows, length = 2048, 512, 256, 160000
    x = torch.from_numpy(signals.audio_like((rows, length), seed=5)).cuda()
    z = tac.stft(x, n_fft, hop)
    before = dict(tac._hip.launches)
    got = tac.istft(z, n_fft, hop, length=length)
    since = launched_since(tac, before)
    since.pop('tac_istft_envelope_f32', None)
    assert since == {'tac_istft_f32': 1}, since
    assert got.shape == (rows, length)
    assert tac._native.lib().tac_last_route().decode() == 'istft_fused_kernel<512>'
    w = hann(n_fft)
    worst = 0.0
    for r0 in range(0, rows, 32):
        want = R.torch_istft(z[r0:r0 + 32], n_fft, hop, w, True, False, length)
        worst = max(worst, fbnd.assert_rows(got[r0:r0 + 32], want, TIGHT, 'istft full size', row0=r0))
        assert float((got[r0:r0 + 32].cpu().double() - x[r0:r0 + 32].cpu().double()).abs().max()) < 1e-5
    fbnd.report('istft_full_size', '256x160000', n_fft, 'rows', worst, TIGHT)


# ----------------------------------------------------------------------------- F
def test_stft_backward_bits_unchanged(tac, golden):
    """tac_stft_backward_f32 (the gradient mode of the frame kernels that gained the inverse mode) returns the bits it returned on
    the parent commit (tests/golden/make_golden_istft.py, run there before any kernel file changed)."""
    import importlib.util
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location('make_golden_istft', os.path.join(here, 'golden', 'make_golden_istft.py'))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    pin = golden(GOLDEN)
    assert len(str(pin['commit'])) >= 7
    tac._hip.set_poison_outputs(False)
    try:
        for case in mg.CASES:
            gs, w = mg.case_inputs(*case)
            got = mg.frame_gradients(gs, w, *case[:4]).numpy().view(np.uint32)
            want = pin[mg.key(*case)]
            assert got.shape == want.shape
            assert np.array_equal(got, want), '%r: %d of %d words differ' % (case, int((got != want).sum()), got.size)
    finally:
        tac._hip.set_poison_outputs(True)
