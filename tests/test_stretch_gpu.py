"""-m gpu: ``STFT -> TimeStretch -> ComplexNorm [-> ApplyFilterbank] [-> AmplitudeToDb]`` on magnitudes alone (csrc/stretch.hip).

Strict mode and poisoned outputs are on (as in tests/test_gpu_fullsize.py).  Each chain asserts its launch counters — one
spectrogram launch, one ``tac_stretch_*`` launch, no complex STFT / phase-vocoder / complex-norm launch — and its values against
the float64 oracle chain ``complex_norm(phase_vocoder(stft(x)))`` per output frame:

  * power 1 rows: within 2 x TIGHT of the output frame's own maximum.  The factor 2 is derived: each source frame is within
    TIGHT of its maximum, so the blend's error is at most TIGHT (a max1 + (1 - a) max0), and the output frame's maximum is at
    least max(a max1, (1 - a) max0) >= half of that sum;
  * other powers: ``frame_bounds.power_linear_bound`` of that per-frame bound, element by element;
  * mel: that bound carried through the bank (sum_f bound[f] |fb[f, m]|) plus ACC x the mel value for the float32 accumulation
    (at most 144 four-tap products of non-negative terms: 144 x 2^-24 = 8.6e-6, rounded up to 1e-5);
  * dB: ``frame_bounds.assert_db`` with those bounds as ``lin``, ``db_tol`` 1e-3, and the mask keeping 99 % of the elements above
    the clamp (``signals.audio_like`` inputs keep the oracle's own float32 evaluation inside that share).

Measured worst ratios go through ``frame_bounds.report`` (``TAC_FUZZ_REPORT``) and are printed.
"""
import math

import numpy as np
import pytest
import torch

import frame_bounds as fbnd
from oracle import signals, torch_ref
from grad_rules import grid, interpolated
from stretch_rules import lost_positions, oracle_chain, phase_advance

pytestmark = pytest.mark.gpu

TIGHT = 2e-6
GRAD = 1e-3
ACC = 1e-5
SPEC = 'tac_spectrogram_f32'
FORBIDDEN = ('tac_stft_f32', 'tac_phase_vocoder_f32', 'tac_complex_norm_f32')


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


QUIET = 2.0 ** -9    # gain of the dB cases' inputs.  Which elements assert_db's mask keeps is decided by the reference values and the
                     # linear bound alone (whatever the kernel returns): with 2 x TIGHT per frame an element below 7 % (3.5 % at power
                     # 1) of its frame's maximum cannot be held to 1e-3 dB.  At this level such elements of signals.audio_like are under
                     # the amin clamp and the mask keeps >= 99.1 % of the rest in every case below (evaluated on the CPU beforehand; at
                     # full scale fft_length 2048 / power 2 keeps 96.2 %)


def wave(shape, seed, dtype='f32', gain=1.0):
    """(device tensor handed to the chain, the float64 samples it stands for)"""
    x = signals.audio_like(shape, seed=seed) * np.float32(gain)
    if dtype == 'i16':
        q = np.round(x * 32768.0).astype(np.int16)
        return torch.from_numpy(q).cuda(), torch.from_numpy(q.astype(np.float64) / 32768.0)
    if dtype == 'f16':
        h = torch.from_numpy(x).half()
        return h.cuda(), h.double()
    return torch.from_numpy(x).cuda(), torch.from_numpy(x).double()


CENTER = True        # (the one- and two-frame cases frame without padding: reflect padding needs more samples than fft_length / 2)


def oracle_rows(x64, n_fft, hop, rate, power):
    z = torch_ref.stft(x64, n_fft, hop, center=CENTER)
    return oracle_chain(z, rate, phase_advance(hop, n_fft // 2 + 1, torch.float64), power)


def check_rows(got, x64, n_fft, hop, rate, power, test, case, db=None):
    """rows of the chain (*, F, n_out) [in dB] against the float64 oracle; returns the worst ratio to the bound"""
    mag = fbnd.frames_of(oracle_rows(x64, n_fft, hop, rate, 1.0), 'spec')
    ref = mag if power == 1.0 else mag ** power
    g = fbnd.as_frames(got, 'spec')
    assert g.shape == ref.shape, (g.shape, ref.shape)
    lin = fbnd.power_linear_bound(mag, power, 2 * TIGHT)
    if db is not None:
        worst, kept, _ = fbnd.assert_db(g, ref, None, db_tol=1e-3, amin=db[1], ref=db[0], what='%s %r' % (test, case), keep=0.99, lin=lin)
        fbnd.report(test, case, n_fft, 'rows_db', worst, 1e-3, kept=kept)
        return worst / 1e-3
    if power == 1.0:
        worst = fbnd.assert_linear(g, ref, 2 * TIGHT, '%s %r' % (test, case))
        fbnd.report(test, case, n_fft, 'rows', worst, 2 * TIGHT)
        return worst / (2 * TIGHT)
    assert bool(torch.isfinite(g).all()), (test, case)
    ratio = float(((g - ref).abs() / lin.clamp(min=1e-300)).max())
    fbnd.report(test, case, n_fft, 'rows_pow', ratio, 1.0)
    assert ratio <= 1.0, '%s %r: |X|^%g is %.3g of its per-element bound' % (test, case, power, ratio)
    return ratio


def mel_bound(x64, n_fft, hop, rate, power, fb64):
    mag = fbnd.frames_of(oracle_rows(x64, n_fft, hop, rate, 1.0), 'spec')
    ref = (mag if power == 1.0 else mag ** power) @ fb64
    lin = fbnd.power_linear_bound(mag, power, 2 * TIGHT) @ fb64.abs() + ACC * ((mag ** power) @ fb64.abs())
    return ref, lin


def check_mel(got, x64, n_fft, hop, rate, power, fb, test, case, db=None):
    ref, lin = mel_bound(x64, n_fft, hop, rate, power, fb.detach().cpu().double())
    g = fbnd.as_frames(got, 'spec')
    assert g.shape == ref.shape, (g.shape, ref.shape)
    if db is not None:
        worst, kept, _ = fbnd.assert_db(g, ref, None, db_tol=1e-3, amin=db[1], ref=db[0], what='%s %r' % (test, case), keep=0.99, lin=lin)
        fbnd.report(test, case, n_fft, 'mel_db', worst, 1e-3, kept=kept)
        return worst / 1e-3
    assert bool(torch.isfinite(g).all()), (test, case)
    ratio = float(((g - ref).abs() / lin.clamp(min=1e-300)).max())
    fbnd.report(test, case, n_fft, 'mel', ratio, 1.0)
    assert ratio <= 1.0, '%s %r: mel values at %.3g of their per-element bound' % (test, case, ratio)
    return ratio


def assert_counters(tac_, before, stretch_entry, extra=()):
    got = launched_since(tac_, before)
    assert got.get(SPEC) == 1 and got.get(stretch_entry) == 1, got
    for name in FORBIDDEN:
        assert name not in got, got
    assert set(got) <= {SPEC, stretch_entry} | set(extra), got


CASES = [  # fft_length, hop, rate, power, input dtype, shape
    (400, 160, 0.5, 1.0, 'f32', (2, 2, 5000)),
    (512, 128, 0.9, 2.0, 'i16', (3, 1, 6000)),
    (1024, 256, 1.3, 0.7, 'f16', (2, 1, 9000)),
    (2048, 512, 2.0, 2.0, 'f32', (1, 1, 24000)),          # one row
    (4096, 1024, 2.7, 1.0, 'f32', (2, 1, 40000)),
    (480, 120, 1.3, 2.0, 'f32', (2, 2, 5000)),             # 7-smooth
    (2048, 512, 0.5, 0.7, 'f32', (2, 3, 20000)),
    (512, 256, 1.3, 1.0, 'f32', (2, 1, 600), False),       # one frame (center=False)
    (512, 256, 0.9, 2.0, 'f32', (2, 1, 800), False),       # two frames
]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'n%d_r%g_p%g_%s' % (c[0], c[2], c[3], c[4]))
def test_stretched_chains(tac, case):
    global CENTER
    n_fft, hop, rate, power, dtype, shape = case[:6]
    CENTER = case[6] if len(case) > 6 else True
    n_freqs = n_fft // 2 + 1
    x, x64 = wave(shape, seed=n_fft + int(10 * rate), dtype=dtype, gain=QUIET)
    # (40 bands over 1025 / 2049 bins are wider than the one-frame-per-wave layout packs: those banks take the rows form, covered by
    # test_dense_bank_takes_rows_form_and_gemm; the fused mel form is exercised with the 128 bands cfg-2 uses there)
    fb = tac.MelFilterbank(num_freqs=n_freqs, num_mels=40 if n_fft <= 1024 else 128, sample_rate=16000).get_filterbank().cuda()
    layers = [tac.STFT(n_fft, hop, center=CENTER), tac.TimeStretch(hop, n_freqs, fixed_rate=rate), tac.ComplexNorm(power=power)]
    worst = {}
    pcm = ('tac_pcm16_to_f32',) if dtype == 'i16' else ()      # (int16 samples are converted by their own kernel in front of |X|)
    # rows
    chain = torch.nn.Sequential(*layers).cuda()
    before = dict(tac._hip.launches)
    y = chain(x)
    assert type(y) is torch.Tensor
    assert_counters(tac, before, 'tac_stretch_norm_f32', pcm)
    worst['rows'] = check_rows(y, x64, n_fft, hop, rate, power, 'stretched_chains', case[:5])
    # rows -> dB
    chain_db = torch.nn.Sequential(*layers, tac.AmplitudeToDb()).cuda()
    before = dict(tac._hip.launches)
    y_db = chain_db(x)
    assert type(y_db) is torch.Tensor
    assert_counters(tac, before, 'tac_stretch_norm_f32', pcm)
    worst['rows_db'] = check_rows(y_db, x64, n_fft, hop, rate, power, 'stretched_chains', case[:5], db=(1.0, 1e-7))
    # mel, mel -> dB
    mel_chain = torch.nn.Sequential(*layers, tac.ApplyFilterbank(fb)).cuda()
    before = dict(tac._hip.launches)
    m = mel_chain(x)
    assert type(m) is torch.Tensor
    assert_counters(tac, before, 'tac_stretch_mel_f32', pcm)
    worst['mel'] = check_mel(m, x64, n_fft, hop, rate, power, fb, 'stretched_chains', case[:5])
    mel_db = torch.nn.Sequential(*layers, tac.ApplyFilterbank(fb), tac.AmplitudeToDb(ref=2.0, amin=1e-6)).cuda()
    before = dict(tac._hip.launches)
    m_db = mel_db(x)
    assert type(m_db) is torch.Tensor
    assert_counters(tac, before, 'tac_stretch_mel_f32', pcm)
    worst['mel_db'] = check_mel(m_db, x64, n_fft, hop, rate, power, fb, 'stretched_chains', case[:5], db=(2.0, 1e-6))
    assert tac._hip.poison_report() == {}
    print('stretched_chains %r: worst ratio to bound %r' % (case[:5], worst))
    # the five-launch route of the same build: same shapes, values within the sum of both bounds
    tac.set_lazy_fusion(False)
    try:
        before = dict(tac._hip.launches)
        y5, m5 = chain(x), mel_chain(x)
        got5 = launched_since(tac, before)
        assert got5.get('tac_phase_vocoder_f32') == 2 and 'tac_stretch_norm_f32' not in got5 and 'tac_stretch_mel_f32' not in got5, got5
    finally:
        tac.set_lazy_fusion(True)
    assert y5.shape == y.shape and m5.shape == m.shape
    mag = fbnd.frames_of(oracle_rows(x64, n_fft, hop, rate, 1.0), 'spec')
    lin = fbnd.power_linear_bound(mag, power, 2 * TIGHT)
    assert bool(((fbnd.as_frames(y5, 'spec') - fbnd.as_frames(y, 'spec')).abs() <= 2 * lin).all())
    _, lin_m = mel_bound(x64, n_fft, hop, rate, power, fb.cpu().double())
    assert bool(((fbnd.as_frames(m5, 'spec') - fbnd.as_frames(m, 'spec')).abs() <= 2 * lin_m).all())
    CENTER = True


def test_overriding_rate_direct_calls_and_planned(tac):
    n_fft, hop, n_freqs = 512, 128, 257
    x, x64 = wave((2, 1, 6000), seed=5)
    stft, ts, cn = tac.STFT(n_fft, hop).cuda(), tac.TimeStretch(hop, n_freqs, fixed_rate=1.3).cuda(), tac.ComplexNorm(2.0)
    before = dict(tac._hip.launches)
    d = cn(ts(stft(x), overriding_rate=0.9))
    assert isinstance(d, tac._lazy.DeferredSpectral) and launched_since(tac, before) == {}
    y = tac.realize(d)
    assert_counters(tac, before, 'tac_stretch_norm_f32')
    check_rows(y, x64, n_fft, hop, 0.9, 2.0, 'overriding_rate', 0.9)
    # a stretched recipe that reaches anything but ComplexNorm: the STFT kernel, then the phase vocoder — the complex result
    before = dict(tac._hip.launches)
    z = tac.realize(ts(stft(x)))
    got = launched_since(tac, before)
    assert got == {'tac_stft_f32': 1, 'tac_phase_vocoder_f32': 1}, got
    tac.set_lazy_fusion(False)
    try:
        z5 = ts(stft(x))
    finally:
        tac.set_lazy_fusion(True)
    assert torch.equal(z, z5)
    end = torch.nn.Sequential(stft, ts)(x)                                   # TimeStretch as the chain's last layer
    assert type(end) is torch.Tensor and torch.equal(end, z5)
    # rate 1 stays the identity on the recipe; a non-finite phase_advance takes the ordinary route
    assert ts(stft(x), 1.0)._stretch is None
    bad = tac.TimeStretch(hop, n_freqs, fixed_rate=1.3).cuda()
    bad.phase_advance[3] = float('inf')
    before = dict(tac._hip.launches)
    tac.realize(cn(bad(stft(x))))
    got = launched_since(tac, before)
    assert got.get('tac_phase_vocoder_f32') == 1 and 'tac_stretch_norm_f32' not in got, got
    # tac.planned does not know the chain: it runs model(x)
    fb = tac.MelFilterbank(num_freqs=n_freqs, num_mels=40, sample_rate=16000).get_filterbank().cuda()
    model = torch.nn.Sequential(stft, ts, cn, tac.ApplyFilterbank(fb), tac.AmplitudeToDb()).cuda()
    p = tac.planned(model, x)
    assert not p.fused()
    before = dict(tac._hip.launches)
    out = p(x)
    assert_counters(tac, before, 'tac_stretch_mel_f32')
    assert torch.equal(out, model(x))


def test_dense_bank_takes_rows_form_and_gemm(tac):
    n_fft, hop, n_freqs, rate, power = 512, 128, 257, 1.3, 2.0
    x, x64 = wave((2, 2, 6000), seed=9)
    rng = np.random.default_rng(3)
    fb = torch.from_numpy(np.abs(rng.standard_normal((n_freqs, 24))).astype(np.float32)).cuda()
    chain = torch.nn.Sequential(tac.STFT(n_fft, hop), tac.TimeStretch(hop, n_freqs, fixed_rate=rate), tac.ComplexNorm(power),
                                tac.ApplyFilterbank(fb), tac.AmplitudeToDb()).cuda()
    before = dict(tac._hip.launches)
    y = chain(x)
    got = launched_since(tac, before)
    assert got == {SPEC: 1, 'tac_stretch_norm_f32': 1, 'tac_apply_filterbank_f32': 1, 'tac_amplitude_to_db_f32': 1}, got
    mag = fbnd.frames_of(oracle_rows(x64, n_fft, hop, rate, 1.0), 'spec')
    fb64 = fb.cpu().double()
    lin = fbnd.power_linear_bound(mag, power, 2 * TIGHT) @ fb64 + 257 * 2.0 ** -24 * ((mag ** power) @ fb64)   # (257-term float32 sums)
    fbnd.assert_db(fbnd.as_frames(y, 'spec'), (mag ** power) @ fb64, None, db_tol=1e-3, what='dense bank', keep=0.99, lin=lin)


def _nonfinite_expect(mag_np, rate):
    nan_mask = np.zeros(mag_np.shape[:-1] + (len(grid(mag_np.shape[-1], rate)[0]),), dtype=bool)
    bad_mask = np.zeros_like(nan_mask)
    for i in np.ndindex(mag_np.shape[:-2]):
        nan_mask[i], bad_mask[i] = lost_positions(mag_np[i], rate)
    return nan_mask, bad_mask


@pytest.mark.parametrize('rate', (0.8, 1.3, 2.7))
def test_non_finite_magnitudes_follow_the_position_rule(tac, rate):
    """NaN / Inf planted in the magnitude tensor handed to the op (data only): read frames, a frame rate 2.7 skips, frame 0."""
    rng = np.random.default_rng(17)
    clean = (np.abs(rng.standard_normal((2, 33, 21))) + 0.1).astype(np.float32)
    idx0, _ = grid(21, rate)
    read = set(idx0.tolist()) | set((idx0 + 1).tolist())
    skipped = [t for t in range(21) if t not in read]
    mag = clean.copy()
    mag[0, 5, 7 if 7 in read else sorted(read)[3]] = np.nan
    mag[0, 9, 0] = np.nan
    mag[1, 12, sorted(read)[5]] = np.inf
    if skipped:
        mag[1, 20, skipped[0]] = np.nan
    nan_mask, bad_mask = _nonfinite_expect(mag, rate)
    for power, db in ((1.0, False), (2.0, True), (0.7, False)):
        got = torch.ops.tac_amd.stretch_norm(torch.from_numpy(mag).cuda(), rate, power, db, 1.0, 1e-7).cpu().numpy()
        ref = torch.ops.tac_amd.stretch_norm(torch.from_numpy(clean).cuda(), rate, power, db, 1.0, 1e-7).cpu().numpy()
        assert np.array_equal(~np.isfinite(got), bad_mask), (rate, power)
        assert np.array_equal(np.isnan(got) | ~nan_mask, np.ones_like(nan_mask)), (rate, power)
        touched = np.zeros_like(bad_mask)
        for r, f in ((0, 5), (0, 9), (1, 12)):
            touched[r, f] = True
        assert np.array_equal(got[~touched].view(np.int32), ref[~touched].view(np.int32)), (rate, power)
    # mel form: a non-finite bin makes its frame non-finite throughout; every frame behind a NaN source too
    fb = torch_ref.create_mel_filter(33, 8, 0.0, 8000.0, False).cuda()
    before = dict(tac._hip.launches)
    got = torch.ops.tac_amd.stretch_mel(torch.from_numpy(mag).cuda(), fb, rate, 2.0, False, 1.0, 1e-7).cpu().numpy()
    assert launched_since(tac, before).get('tac_stretch_mel_f32') == 1
    ref = torch.ops.tac_amd.stretch_mel(torch.from_numpy(clean).cuda(), fb, rate, 2.0, False, 1.0, 1e-7).cpu().numpy()
    frame_bad = bad_mask.any(-2)
    want = torch_ref.apply_filterbank(torch.from_numpy(np.where(bad_mask, np.nan, 1.0)), fb.cpu().double()).numpy()
    assert np.array_equal(~np.isfinite(got), ~np.isfinite(want))
    assert np.array_equal(~np.isfinite(got), np.broadcast_to(frame_bad[:, None, :], got.shape))
    assert np.array_equal(got[np.isfinite(got)].view(np.int32), ref[np.isfinite(got)].view(np.int32))


@pytest.mark.parametrize('value', (float('nan'), float('inf')))
def test_non_finite_samples_in_the_waveform(tac, value):
    n_fft, hop, n_freqs, rate = 512, 128, 257, 1.3
    x, x64 = wave((2, 1, 8000), seed=23)
    x[1, 0, 3000] = value
    x64[1, 0, 3000] = value
    chain = torch.nn.Sequential(tac.STFT(n_fft, hop), tac.TimeStretch(hop, n_freqs, fixed_rate=rate), tac.ComplexNorm(2.0)).cuda()
    before = dict(tac._hip.launches)
    y = chain(x).cpu().numpy()
    assert_counters(tac, before, 'tac_stretch_norm_f32')
    want = oracle_rows(x64, n_fft, hop, rate, 2.0).numpy()
    assert np.array_equal(~np.isfinite(y), ~np.isfinite(want))
    x[1, 0, 3000] = 0.25
    clean = chain(x).cpu().numpy()
    assert np.array_equal(y[0].view(np.int32), clean[0].view(np.int32))
    ok = np.isfinite(y)
    untouched = ok & (np.arange(y.shape[-1]) < int((3000 - n_fft) / hop / rate) - 1)
    assert untouched[1].any() and np.array_equal(y[untouched].view(np.int32), clean[untouched].view(np.int32))


def test_gradients(tac):
    """The waveform gradient through the stretched mel-dB chain against float64 autograd through the oracle, per row within GRAD;
    the op's own gradient at power 0.7 with exact zeros in the magnitudes (torch's pow backward: inf / NaN there) by position."""
    n_fft, hop, n_freqs, rate = 512, 128, 257, 1.3
    x_np = signals.audio_like((3, 1, 6000), seed=61)
    fb = tac.MelFilterbank(num_freqs=n_freqs, num_mels=40, sample_rate=16000).get_filterbank()
    xr = torch.from_numpy(x_np).double().requires_grad_(True)
    yr = torch_ref.amplitude_to_db(torch_ref.apply_filterbank(
        oracle_chain(torch_ref.stft(xr, n_fft, hop), rate, phase_advance(hop, n_freqs, torch.float64), 2.0), fb.double()))
    c = torch.from_numpy(np.random.default_rng(4).standard_normal(tuple(yr.shape)).astype(np.float32))
    (want,) = torch.autograd.grad((yr * c.double()).sum(), xr)
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    chain = torch.nn.Sequential(tac.STFT(n_fft, hop), tac.TimeStretch(hop, n_freqs, fixed_rate=rate), tac.ComplexNorm(2.0),
                                tac.ApplyFilterbank(fb), tac.AmplitudeToDb()).cuda()
    before = dict(tac._hip.launches)
    y = chain(x)
    (got,) = torch.autograd.grad((y * c.cuda()).sum(), x)
    counts = launched_since(tac, before)
    assert counts.get('tac_stretch_mel_f32') == 1 and counts.get('tac_stretch_norm_backward_f32') == 1, counts
    for name in FORBIDDEN + ('tac_phase_vocoder_backward_f32',):
        assert name not in counts, counts
    worst = fbnd.check_rows(got, want, GRAD, 'stretch_gradient', 'mel_db', n_fft)
    print('stretch_gradient: worst per-row ratio %.3g (bound %.1e)' % (worst, GRAD))
    # the op alone: rates below / above one and beyond two, all three powers, the bank's gradient
    rng = np.random.default_rng(8)
    mag_np = (np.abs(rng.standard_normal((2, 2, 37, 29))) + 0.05).astype(np.float32)
    bank_np = np.abs(rng.standard_normal((37, 12))).astype(np.float32)
    for r in (0.6, 1.3, 2.5):
        for power in (1.0, 2.0, 0.7):
            mr = torch.from_numpy(mag_np).double().requires_grad_(True)
            br = torch.from_numpy(bank_np).double().requires_grad_(True)
            outr = torch_ref.apply_filterbank(interpolated(mr, r, power), br)
            g_np = rng.standard_normal(tuple(outr.shape)).astype(np.float32)
            want_m, want_b = torch.autograd.grad(outr, [mr, br], torch.from_numpy(g_np).double())
            m = torch.from_numpy(mag_np).cuda().requires_grad_(True)
            b = torch.from_numpy(bank_np).cuda().requires_grad_(True)
            got_m, got_b = torch.autograd.grad(torch.ops.tac_amd.stretch_mel(m, b, r, power, False, 1.0, 1e-7), [m, b],
                                               torch.from_numpy(g_np).cuda())
            assert fbnd.row_errors(got_m.cpu().reshape(4, -1), want_m.reshape(4, -1)).max() <= 2e-5, (r, power)
            assert fbnd.row_errors(got_b.cpu().reshape(1, -1), want_b.reshape(1, -1)).max() <= 2e-5, (r, power)
    zeros = mag_np.copy()
    zeros[0, 0, 3, 4:9] = 0.0                                               # frames 4 .. 8 of one bin: blends that are exactly zero
    zr = torch.from_numpy(zeros).double().requires_grad_(True)
    g_np = rng.standard_normal((2, 2, 37, len(grid(29, 1.3)[0]))).astype(np.float32)
    g_np[0, 0, 3, 5] = 0.0
    (want_z,) = torch.autograd.grad(interpolated(zr, 1.3, 0.7), zr, torch.from_numpy(g_np).double())
    z = torch.from_numpy(zeros).cuda().requires_grad_(True)
    (got_z,) = torch.autograd.grad(torch.ops.tac_amd.stretch_norm(z, 1.3, 0.7, False, 1.0, 1e-7), z, torch.from_numpy(g_np).cuda())
    got_z, want_z = got_z.cpu().numpy(), want_z.numpy()
    assert not np.isfinite(want_z).all()
    assert np.array_equal(np.isnan(got_z), np.isnan(want_z)) and np.array_equal(np.isinf(got_z), np.isinf(want_z))
    ok = np.isfinite(want_z)
    assert np.abs(got_z[ok] - want_z[ok]).max() <= 2e-5 * np.abs(want_z[ok]).max()


def test_full_size_cfg2_mel_db(tac):
    """cfg-2 shape (256 rows of 10 s at 16 kHz, fft_length 2048 / hop 512, 128 mels + dB) at rate 1.3: every element, in row
    chunks, against the float64 oracle STFT on the device and the interpolation it equals (tests/test_stretch_cpu.py holds that
    identity to 1e-14; the oracle's own vocoder would take its grid from device arithmetic, which is not the reference's)."""
    n_fft, hop, n_freqs, rate = 2048, 512, 1025, 1.3
    gen = torch.Generator(device='cuda').manual_seed(11)
    x = torch.rand((256, 1, 160000), device='cuda', generator=gen) * 2 - 1
    x.view(-1, 160000).mul_((2.0 ** -(torch.arange(256, device='cuda') % 13).float())[:, None])
    fb = tac.MelFilterbank(num_freqs=n_freqs, num_mels=128, sample_rate=16000).get_filterbank().cuda()
    chain = torch.nn.Sequential(tac.STFT(n_fft, hop), tac.TimeStretch(hop, n_freqs, fixed_rate=rate), tac.ComplexNorm(2.0),
                                tac.ApplyFilterbank(fb), tac.AmplitudeToDb()).cuda()
    before = dict(tac._hip.launches)
    y = chain(x)
    assert_counters(tac, before, 'tac_stretch_mel_f32')
    idx0, alpha = grid(313, rate)
    i0 = torch.from_numpy(idx0).cuda()
    a = torch.from_numpy(alpha).cuda().double()
    fb64 = fb.double()
    rows, got = x.view(-1, 160000), y.reshape(256, 128, -1)
    worst, kept_min = 0.0, 1.0
    for r0 in range(0, 256, 16):
        z = torch_ref.stft(rows[r0:r0 + 16].double(), n_fft, hop, window=torch.hann_window(n_fft, device='cuda'))
        mag = torch.nn.functional.pad(z.norm(dim=-1), [0, 2])
        blend = (a * mag[..., i0 + 1] + (1 - a) * mag[..., i0]).transpose(1, 2)          # (rows, n_out, F)
        lin = fbnd.power_linear_bound(blend, 2.0, 2 * TIGHT) @ fb64 + ACC * ((blend ** 2) @ fb64)
        w, kept, _ = fbnd.assert_db(got[r0:r0 + 16].transpose(1, 2), (blend ** 2) @ fb64, None, db_tol=1e-3, what='cfg-2 stretched',
                                    row0=r0, keep=0.99, lin=lin)
        worst, kept_min = max(worst, w), min(kept_min, kept)
    fbnd.report('full_size_cfg2_mel_db', 'rate1.3', n_fft, 'mel_db', worst, 1e-3, kept=kept_min)
    print('full_size_cfg2_mel_db: worst |d dB| %.3g over the mask, kept %.4f' % (worst, kept_min))
