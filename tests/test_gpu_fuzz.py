"""-m gpu: randomised differential check of the HIP path against the CPU oracle over the whole argument space of the
hot path (reference functional.py:48-184, 291-296; layers.py:307-381) — every kernel family, fused route and fallback.

The default run draws a few dozen cases per op (seconds); ``TAC_FUZZ_CASES=N`` draws N per op and ``TAC_FUZZ_SEED`` moves
the stream, for the deep runs recorded in DESIGN.md.  Tolerances are those of test_gpu_parity.py (north_star 1e-4
relative; what is asserted here is tighter): linear outputs to 5e-6 .. 2e-5 of the tensor maximum, dB to 1e-3 dB where
the value is not at cancellation level.

dB outputs are compared where the linear reference exceeds 1e-6 of its maximum (see tests/test_gpu_parity.py: below
that the float32 FFT's own rounding decides the digits); every bin is checked on the linear output first.

Per frame (tests/frame_bounds.py): inputs come from ``signals.gained_with_silence`` (row gains 2^0 ... 2^-12, silent spans,
a silent row), and every op is also compared frame by frame (gradients row by row) with its float64 reference — the oracle
evaluated in float64 on the module's own window and filterbank — where a silent frame (row) must come out exactly zero and
the dB masks follow from the linear bounds.  ``TAC_FUZZ_REPORT=path`` appends one JSON line per check.

The gradients beside the main chain — window, filterbank, ``hpss``, ``phase_vocoder``, ``stretch_norm`` / ``stretch_mel`` — are swept
in tests/test_gradient_sweeps_gpu.py (generators and bounds in tests/grad_rules.py, the same bodies on the CPU route in
tests/test_grad_rules_cpu.py) under the same three knobs: ``TAC_FUZZ_CASES``, ``TAC_FUZZ_SEED``, ``TAC_FUZZ_REPORT``.
"""
import os

import numpy as np
import pytest
import torch

import frame_bounds as fbnd
from conftest import rel_err
from oracle import signals, torch_ref

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get('TAC_FUZZ_CASES', '32'))
SEED = int(os.environ.get('TAC_FUZZ_SEED', '0'))
DB_ABS = 1e-3
FFT_SIZES = [32, 64, 128, 256, 400, 512, 1024, 2048, 4096]
ODD_SIZES = [100, 300, 1000, 1536, 3000, 882, 960, 6000,      # generic Stockham kernel (even, 7-smooth half: csrc/stft_smooth.hip)
             77, 501, 1018, 2602]                          # windowed-DFT matrix route (odd, or a half with a larger prime factor)
FRAME = 2e-6        # complex rows and |X|, per frame
FRAME_DFT = 5e-6    # complex rows and |X| of the windowed-DFT matrix route (one fp32 dot product of fft_length terms per
                    # bin): 4.1e-6 measured at fft_length 2602 (deep run, seed 0); the per-tensor bound beside it is 5e-6
FRAME_POW = 2e-5    # |X|^p (p != 1), power and mel, per frame
GRAD = 1e-4         # waveform gradients of linear / power / mel outputs, per row
GRAD_DB = 1e-3      # ... through dB or |X|, per row
FRAME_F64 = 2e-12   # the float64 chain: complex rows and |X|^p, per frame
DB_F64 = 1e-8       # ... its dB values


def frame_tol(n):
    """Per-frame bound on complex rows and |X| for the route fft_length ``n`` takes."""
    return FRAME_DFT if n in ODD_SIZES[8:] else FRAME


def silent_input(shape, seed, n, hop):
    """(waveform, whether it holds a silent frame for every pad mode and centring)."""
    return signals.gained_with_silence(shape, seed, n, hop), signals.has_silence(shape, n, hop)


def mel_db_mask(x, n, hop, window, fb, amin, **kw):
    """1 where the dB value of the float32 mel chain is determined to DB_ABS by fbnd.POW_TOL (check_mel_grad's rule), else 0:
    (*, M, T) float64, for the weights of a gradient through dB."""
    with torch.no_grad():
        pw = fbnd.ref64(x, n, hop, window, 2.0, **kw)
        mel = torch_ref.apply_filterbank(pw, fb.detach().cpu().double())
        lin = fbnd.mel_linear_bound(fbnd.frames_of(pw, 'spec'), fb.detach().cpu(), fbnd.POW_TOL).transpose(-1, -2)
        lin = lin.reshape(mel.shape)
    bound = fbnd.DB_PER_REL * lin / mel.abs().clamp(min=amin ** 0.5)
    return (((mel - lin).clamp(min=0) ** 2 > amin) & (bound <= DB_ABS)).double()


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    t._native.lib()
    t.set_strict(True)
    t._hip.set_poison_outputs(True)       # every kernel output starts as a NaN pattern: a sample no kernel writes cannot pass by luck
    yield t
    t._hip.set_poison_outputs(False)
    t.set_strict(False)


@pytest.fixture(autouse=True)
def every_output_written(tac):
    """After each test: no launch left a position of what it fills holding the poison pattern (named per entry point)."""
    tac._hip.poison_report()
    yield
    left = tac._hip.poison_report()
    assert not left, 'kernel outputs left unwritten (poisoned elements per entry point): %r' % left


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t_):
    return t_.detach().cpu().numpy()


def draw_stft_args(rng, sizes, max_rows=6, max_len_factor=12):
    n = int(rng.choice(sizes))
    hop = int(rng.integers(1, n + 1)) if rng.random() < 0.5 else int(rng.choice([n // 4, n // 2, max(1, n // 8)]))
    win_length = n if rng.random() < 0.6 else int(rng.integers(max(2, n // 4), n + 1))
    center = bool(rng.random() < 0.75)
    pad_mode = str(rng.choice(['reflect', 'constant', 'replicate', 'circular']))
    lead = tuple(int(v) for v in rng.integers(1, max_rows + 1, size=int(rng.integers(1, 3))))
    lo = n + 1 if center else n
    length = int(rng.integers(lo, max(lo + 2, int(n * rng.uniform(1.0, max_len_factor)))))
    return n, hop, win_length, center, pad_mode, lead, length


def test_fuzz_stft(tac):
    rng = np.random.default_rng(1000 + SEED)
    for case in range(CASES):
        n, hop, win_length, center, pad_mode, lead, length = draw_stft_args(
            rng, FFT_SIZES + (ODD_SIZES if case % 4 == 0 else []))
        normalized, onesided = bool(rng.random() < 0.3), bool(rng.random() < 0.7)
        x, silent = silent_input(lead + (length,), 5000 + case + 7919 * SEED, n, hop)
        window = None if rng.random() < 0.5 else \
            torch.from_numpy(signals.uniform((win_length,), seed=6000 + case) * 0.5 + 0.75)
        kw = dict(win_length=win_length, center=center, pad_mode=pad_mode, normalized=normalized, onesided=onesided)
        want = torch_ref.stft(torch.from_numpy(x), n, hop, window=window, **kw).numpy()
        got = host(tac.stft(dev(x), n, hop_length=hop, window=None if window is None else window.cuda(), **kw))
        tag = ('stft', case, n, hop, kw, lead, length, window is not None)
        assert got.shape == want.shape, tag
        assert rel_err(got, want) < 5e-6, tag
        want64 = fbnd.ref64(x, n, hop, torch.hann_window(win_length, device='cuda') if window is None else window, **kw)
        fbnd.check_frames(got, want64, 'complex', frame_tol(n), 'fuzz_stft', tag, n, silent)


def test_fuzz_stft_big(tac):
    """fft_length 8192 / 16384 / 32768 (csrc/stft_big.hip): random hops (aligned or not), window lengths, pad modes, sidedness,
    row counts; complex rows and |X|^p rows with the dB epilogue against torch's CPU operators."""
    rng = np.random.default_rng(1500 + SEED)
    for case in range(max(4, CASES // 4)):
        n = int(rng.choice([8192, 16384, 32768]))
        hop = int(rng.integers(n // 8, n + 1)) if rng.random() < 0.5 else int(rng.choice([n // 4, n // 2, n // 8]))
        win_length = n if rng.random() < 0.6 else int(rng.integers(n // 4, n + 1))
        center = bool(rng.random() < 0.75)
        pad_mode = str(rng.choice(['reflect', 'constant', 'replicate', 'circular']))
        lead = tuple(int(v) for v in rng.integers(1, 4, size=int(rng.integers(1, 3))))
        lo = n + 1 if center else n
        length = int(rng.integers(lo, lo + 6 * n))
        normalized, onesided = bool(rng.random() < 0.3), bool(rng.random() < 0.7)
        x, silent = silent_input(lead + (length,), 5500 + case + 7919 * SEED, n, hop)
        window = None if rng.random() < 0.5 else \
            torch.from_numpy(signals.uniform((win_length,), seed=6500 + case) * 0.5 + 0.75)
        kw = dict(win_length=win_length, center=center, pad_mode=pad_mode, normalized=normalized, onesided=onesided)
        want = torch_ref.stft(torch.from_numpy(x), n, hop, window=window, **kw)
        wdev = None if window is None else window.cuda()
        tag = ('stft_big', case, n, hop, kw, lead, length, window is not None)
        before = dict(tac._hip.launches)
        got = host(tac.stft(dev(x), n, hop_length=hop, window=wdev, **kw))
        assert tac._hip.launches['tac_stft_f32'] - before.get('tac_stft_f32', 0) == 1, tag
        assert got.shape == tuple(want.shape), tag
        assert rel_err(got, want.numpy()) < 5e-6, tag
        want64 = fbnd.ref64(x, n, hop, torch.hann_window(win_length, device='cuda') if window is None else window, **kw)
        fbnd.check_frames(got, want64, 'complex', FRAME, 'fuzz_stft_big', tag, n, silent)
        power = float(rng.choice([1.0, 2.0, 0.7]))
        mag = torch_ref.complex_norm(want.double(), power)
        gs = host(torch.ops.tac_amd.spectrogram(dev(x), torch.hann_window(win_length).cuda() if wdev is None else wdev, n, hop, win_length,
                                                 center, pad_mode, normalized, onesided, power, False, 1.0, 1e-7))
        assert rel_err(gs, mag.numpy()) < 2e-5, tag + (power,)
        if window is None:                  # (the op got the host-built window here)
            want64 = fbnd.ref64(x, n, hop, torch.hann_window(win_length), **kw)
        fbnd.check_frames(gs, torch_ref.complex_norm(want64, power), 'spec', FRAME if power == 1.0 else FRAME_POW,
                          'fuzz_stft_big', tag + (power,), n, silent)


def test_fuzz_spectrogram(tac):
    rng = np.random.default_rng(2000 + SEED)
    for case in range(CASES):
        n, hop, win_length, center, pad_mode, lead, length = draw_stft_args(
            rng, FFT_SIZES + (ODD_SIZES if case % 4 == 0 else []))
        power = float(rng.choice([1.0, 2.0, 2.0, 0.7, 3.0]))
        normalized = bool(rng.random() < 0.3)
        x, silent = silent_input(lead + (length,), 7000 + case + 7919 * SEED, n, hop)
        layer = tac.Spectrogram(n, hop, win_length, power=power, center=center, pad_mode=pad_mode,
                                normalized=normalized).cuda()
        z = torch_ref.stft(torch.from_numpy(x), n, hop, win_length=win_length, center=center, pad_mode=pad_mode,
                           normalized=normalized)
        want = torch_ref.complex_norm(z, power).numpy()
        got = host(layer(dev(x)))
        tag = ('spec', case, n, hop, win_length, center, pad_mode, normalized, power, lead, length)
        assert got.shape == want.shape, tag
        assert rel_err(got, want) < 2e-5, tag
        chain = torch.nn.Sequential(*layer, tac.AmplitudeToDb(ref=1.0, amin=1e-10)).cuda()
        got_db = host(chain(dev(x)))
        want_db = torch_ref.amplitude_to_db(torch.from_numpy(want), ref=1.0, amin=1e-10).numpy()
        # a single bin may sit at cancellation level, where fp32's absolute error (~3e-7 of the maximum AMPLITUDE, checked above)
        # is a large relative one: the dB epilogue is pinned on the bins that carry signal — amplitude above 3 % of the maximum,
        # whatever the power (round 6: the mask used to be taken on |X|^power, which for power 0.7 let bins at 0.14 % of the
        # maximum amplitude through, where 3.6e-7 of the maximum is 1.6e-3 dB: soak seed 8, case 108, fft_length 2602)
        big = want > (3e-2 ** power) * want.max()
        assert np.abs(got_db - want_db)[big].max() < DB_ABS, tag
        mag64 = fbnd.ref64(x, n, hop, layer[0].window, 1.0, win_length=win_length, center=center, pad_mode=pad_mode,
                      normalized=normalized)
        fbnd.check_frames(got, mag64 ** power, 'spec', frame_tol(n) if power == 1.0 else FRAME_POW, 'fuzz_spectrogram', tag, n,
                          silent)
        fbnd.check_power_db64(got_db, x, n, hop, power, 'fuzz_spectrogram', tag, frame_tol(n), layer[0].window, amin=1e-10,
                              win_length=win_length, center=center, pad_mode=pad_mode, normalized=normalized)


def test_fuzz_melspectrogram(tac):
    rng = np.random.default_rng(3000 + SEED)
    for case in range(CASES):
        n, hop, win_length, center, pad_mode, lead, length = draw_stft_args(
            rng, [64, 128, 256, 400, 512, 1024, 2048, 4096], max_rows=9, max_len_factor=24)
        sr = int(rng.choice([8000, 16000, 22050, 44100, 48000]))
        num_mels = int(rng.choice([1, 5, 13, 23, 40, 64, 80, 96, 128, 160, 229, 256, 300]))
        if num_mels > n // 2:
            num_mels = max(1, n // 4)
        htk = bool(rng.random() < 0.5)
        min_freq = float(rng.choice([0.0, 20.0, 125.0]))
        max_freq = None if rng.random() < 0.6 else float(sr // 2 - int(rng.integers(0, sr // 8)))
        x, silent = silent_input(lead + (length,), 8000 + case + 7919 * SEED, n, hop)
        mel = tac.Melspectrogram(num_mels=num_mels, sample_rate=sr, min_freq=min_freq, max_freq=max_freq, htk=htk,
                                 fft_length=n, hop_length=hop, win_length=win_length, center=center,
                                 pad_mode=pad_mode).cuda()
        want = torch_ref.melspectrogram(torch.from_numpy(x), num_mels=num_mels, sample_rate=sr, min_freq=min_freq,
                                        max_freq=max_freq, htk=htk, n_fft=n, hop=hop, win_length=win_length,
                                        center=center, pad_mode=pad_mode).numpy()
        got = host(mel(dev(x)))
        tag = ('mel', case, n, hop, win_length, center, pad_mode, num_mels, sr, htk, min_freq, max_freq, lead, length)
        assert got.shape == want.shape, tag
        assert rel_err(got, want) < 2e-5, tag
        chain = torch.nn.Sequential(*mel, tac.AmplitudeToDb(ref=1.0, amin=1e-7)).cuda()
        got_db = host(chain(dev(x)))
        want_db = torch_ref.amplitude_to_db(torch.from_numpy(want), ref=1.0, amin=1e-7).numpy()
        big = want > 1e-6 * want.max()
        if big.any():
            assert np.abs(got_db - want_db)[big].max() < DB_ABS, tag
        kw = dict(win_length=win_length, center=center, pad_mode=pad_mode)
        pw64 = fbnd.ref64(x, n, hop, mel[0].window, 2.0, **kw)
        mel64 = torch_ref.apply_filterbank(pw64, mel[2].filterbank.cpu().double())
        fbnd.check_frames(got, mel64, 'spec', FRAME_POW, 'fuzz_melspectrogram', tag, n, silent)
        fbnd.check_mel_db64(got_db, x, n, hop, mel[2].filterbank, 'fuzz_melspectrogram', tag, mel[0].window, **kw)


def test_fuzz_apply_filterbank(tac):
    """Standalone filterbank contraction on frame-major and bin-major spectrograms: triangular, random band-sparse
    (interior zeros, empty bands, overlapping wide bands) and dense banks."""
    rng = np.random.default_rng(4000 + SEED)
    for case in range(CASES):
        n_freqs = int(rng.choice([33, 65, 129, 201, 257, 513, 1025, 2049]))
        n_mels = int(rng.integers(1, 200))
        lead = tuple(int(v) for v in rng.integers(1, 5, size=int(rng.integers(0, 3))))
        n_frames = int(rng.integers(1, 400))
        kind = case % 3
        fb = np.zeros((n_freqs, n_mels), dtype=np.float32)
        if kind == 0:
            fb = signals.uniform((n_freqs, n_mels), seed=9000 + case)
        else:
            widest = max(2, int(n_freqs * (0.05 if kind == 1 else 0.4)))
            for m in range(n_mels):
                if rng.random() < 0.1:
                    continue
                ln = int(rng.integers(1, widest))
                lo = int(rng.integers(0, max(1, n_freqs - ln)))
                fb[lo:lo + ln, m] = rng.random(ln).astype(np.float32) + 0.05
                if ln > 4 and rng.random() < 0.3:
                    fb[lo + 1:lo + ln // 2, m] = 0.0
        # frames with gains 2^0 ... 2^-12, runs of zero bins, a silent frame (the generator's rows are this spectrogram's frames)
        spec = np.swapaxes(np.abs(signals.gained_with_silence(lead + (n_frames, n_freqs), 9500 + case, max(1, n_freqs // 8), 1)), -1, -2)
        silent = signals.has_silence(lead + (n_frames, n_freqs), n_freqs, 0)
        want = np.einsum('...ft,fm->...mt', spec.astype(np.float64), fb.astype(np.float64))
        frame_major = dev(np.swapaxes(spec, -1, -2)).transpose(-1, -2)          # the layout the kernels here write
        for name, s in (('bin-major', dev(spec)), ('frame-major', frame_major)):
            got = host(tac.apply_filterbank(s, dev(fb)))
            tag = ('fb', case, name, n_freqs, n_mels, lead, n_frames, kind)
            assert got.shape == want.shape, tag
            assert rel_err(got, want) < 1e-5, tag
            fbnd.check_frames(got, want, 'spec', 1e-5, 'fuzz_apply_filterbank', tag, n_freqs, silent)


def check_gradient_per_row(tac_, module, kind, x, w, n, hop, kw, test, tag, db=None):
    """Waveform gradient of (w * module(x)).sum(), row by row, against float64 autograd through the oracle on the module's
    window and filterbank.  Weights are zeroed where the float32 forward does not determine the output's derivative: mel
    bands whose dB value it does not fix to DB_ABS (``db`` = (ref, amin)), and |X| below 1e-3 of its row's maximum
    (``magnitude``; |X| is not differentiable at 0).  A silent row (row 1 of 3 or more) must get an exactly zero gradient:
    from its full weights for power, mel and mel + dB (the clamp of dB has a defined zero derivative there, so the silent row
    keeps its weights); for ``magnitude`` its weights are all zero, so there the condition only says that zero weights give
    an exactly zero gradient."""
    stft_mod = module if kind == 'stft' else module[0]
    window = stft_mod.window
    fb = None if kind in ('stft', 'power', 'magnitude') else module[2].filterbank
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    if kind == 'stft':
        y64 = fbnd.ref64(x64, n, hop, window, **kw)
    else:
        y64 = fbnd.ref64(x64, n, hop, window, 1.0 if kind == 'magnitude' else 2.0, fb=fb, **kw)
    w = torch.from_numpy(np.asarray(w, dtype=np.float64))
    if kind == 'magnitude':
        rows = y64.detach().reshape(-1, y64.shape[-2] * y64.shape[-1])
        w = w * (rows > 1e-3 * rows.amax(-1, keepdim=True)).reshape(y64.shape)
    n_rows = int(np.prod(x.shape[:-1]))
    if db is not None:
        ref, amin = db
        masked = w * mel_db_mask(x, n, hop, window, fb, amin, **kw)
        if n_rows >= 3:
            masked.reshape(n_rows, -1)[1] = w.reshape(n_rows, -1)[1]
        w = masked
        y64 = torch_ref.amplitude_to_db(y64, ref=ref, amin=amin)
    (want,) = torch.autograd.grad((y64 * w).sum(), x64)
    xg = dev(x).requires_grad_(True)
    (got,) = torch.autograd.grad((module(xg) * dev(w.float())).sum(), xg)
    silent_rows = (1,) if kind != 'stft' and n_rows >= 3 else ()
    fbnd.check_rows(host(got), want, GRAD_DB if (db is not None or kind == 'magnitude') else GRAD, test, tag, n,
                    silent_rows=silent_rows)


def test_fuzz_gradients(tac):
    """Gradients w.r.t. the waveform through the HIP backward kernels (csrc/backward.hip) against torch.autograd through
    the CPU restatement of the reference chain, over random STFT arguments: the complex STFT (linear), the power
    spectrogram, the mel chain and mel + dB."""
    rng = np.random.default_rng(5000 + SEED)
    for case in range(max(8, CASES // 2)):
        n, hop, win_length, center, pad_mode, lead, length = draw_stft_args(
            rng, [64, 256, 400, 512, 1024, 2048, 4096] + ([300] if case % 5 == 0 else []), max_rows=3, max_len_factor=6)
        normalized = bool(rng.random() < 0.3)
        kind = ['stft', 'power', 'mel', 'mel_db'][case % 4]
        num_mels = int(rng.choice([13, 40, 80, 128]))
        if num_mels > n // 4:
            num_mels = max(2, n // 8)
        x = signals.gained_with_silence(lead + (length,), seed=9900 + case + 7919 * SEED, n_fft=n, hop=hop)
        xc = torch.from_numpy(x).requires_grad_(True)
        xg = dev(x).requires_grad_(True)
        kw = dict(win_length=win_length, center=center, pad_mode=pad_mode, normalized=normalized)
        if kind == 'stft':
            want_y = torch_ref.stft(xc, n, hop, **kw)
            module = tac.STFT(n, hop, **kw).cuda()
            y = module(xg)
        elif kind == 'power':
            want_y = torch_ref.complex_norm(torch_ref.stft(xc, n, hop, **kw), 2.0)
            module = tac.Spectrogram(n, hop, power=2.0, **kw).cuda()
            y = module(xg)
        else:
            want_y = torch_ref.melspectrogram(xc, num_mels=num_mels, sample_rate=16000, n_fft=n, hop=hop, **kw)
            chain = tac.Melspectrogram(num_mels=num_mels, sample_rate=16000, fft_length=n, hop_length=hop, **kw)
            if kind == 'mel_db':
                floor = 1e-3 * float(want_y.detach().max())          # clamp well above cancellation level
                ref = max(1.0, 2.0 * floor * floor)                  # (the layer insists on ref > amin, layers.py:369)
                want_y = torch_ref.amplitude_to_db(want_y, ref=ref, amin=floor * floor)
                chain = torch.nn.Sequential(*chain, tac.AmplitudeToDb(ref=ref, amin=floor * floor))
            module = chain.cuda()
            y = module(xg)
        tag = ('grad', case, kind, n, hop, kw, num_mels, lead, length)
        assert tuple(y.shape) == tuple(want_y.shape), tag
        w = signals.uniform(tuple(want_y.shape), seed=9950 + case)
        (want,) = torch.autograd.grad((want_y * torch.from_numpy(w)).sum(), xc)
        (got,) = torch.autograd.grad((y * dev(w)).sum(), xg)
        assert rel_err(host(got), want.numpy()) < (1e-3 if kind == 'mel_db' else 1e-4), tag
        check_gradient_per_row(tac, module, kind, x, w, n, hop, kw, 'fuzz_gradients', tag,
                               None if kind != 'mel_db' else (ref, floor * floor))


def test_fuzz_gradients_overlap_add_in_lds(tac):
    """The hop = (fft_length / 16)·H backward form for fft_length 256 / 512 / 1024 / 2048 and the hop = 4·k form of fft_length 400
    (csrc/backward.hip, stft_n400.hip: overlap-add in
    an LDS ring over segments of consecutive frames, partial sums at segment borders folded afterwards) over every H, pad
    mode, centring, short windows and signal lengths from one frame to hundreds (one to many segments per row, ragged
    segment lengths inside a wave for the sizes that carry several frames per wave)."""
    rng = np.random.default_rng(6000 + SEED)
    for case in range(max(16, CASES // 2)):
        n = int(rng.choice([2048, 1024, 512, 256, 400]))
        if n == 400:                       # the mixed-radix kernel: any hop that is a multiple of four from 52 up
            hop = 4 * int(rng.integers(13, 101)) if case % 3 else 160
        else:
            hop = (n // 16) * int(rng.integers(1, 17)) if case % 3 else n // 4
        win_length = n if rng.random() < 0.6 else int(rng.integers(n // 4, n + 1))
        center = bool(rng.random() < 0.75)
        pad_mode = str(rng.choice(['reflect', 'constant', 'replicate', 'circular']))
        normalized = bool(rng.random() < 0.3)
        lead = tuple(int(v) for v in rng.integers(1, 4, size=int(rng.integers(1, 3))))
        lo = n + 1 if center else n
        length = int(rng.integers(lo, lo + int(rng.choice([3, 40, 400])) * hop + 7))
        kind = ['power', 'mel', 'mel_db', 'magnitude'][case % 4]
        x = signals.gained_with_silence(lead + (length,), seed=9700 + case + 7919 * SEED, n_fft=n, hop=hop)
        xc = torch.from_numpy(x).requires_grad_(True)
        xg = dev(x).requires_grad_(True)
        kw = dict(win_length=win_length, center=center, pad_mode=pad_mode, normalized=normalized)
        before = dict(tac._hip.launches)
        if kind in ('power', 'magnitude'):
            power = 2.0 if kind == 'power' else 1.0
            want_y = torch_ref.complex_norm(torch_ref.stft(xc, n, hop, **kw), power)
            module = tac.Spectrogram(n, hop, power=power, **kw).cuda()
            y = module(xg)
        else:
            mels = min(64, n // 8)
            want_y = torch_ref.melspectrogram(xc, num_mels=mels, sample_rate=16000, n_fft=n, hop=hop, **kw)
            chain = tac.Melspectrogram(num_mels=mels, sample_rate=16000, fft_length=n, hop_length=hop, **kw)
            if kind == 'mel_db':
                floor = 1e-3 * float(want_y.detach().max())
                ref = max(1.0, 2.0 * floor * floor)
                want_y = torch_ref.amplitude_to_db(want_y, ref=ref, amin=floor * floor)
                chain = torch.nn.Sequential(*chain, tac.AmplitudeToDb(ref=ref, amin=floor * floor))
            module = chain.cuda()
            y = module(xg)
        tag = ('grad-ola', case, kind, n, hop, kw, lead, length)
        w = signals.uniform(tuple(want_y.shape), seed=9750 + case)
        if kind == 'magnitude':            # |z| is not differentiable at 0: weight only bins that carry signal
            w = w * (want_y.detach().numpy() > 1e-3 * float(want_y.detach().max()))
        (want,) = torch.autograd.grad((want_y * torch.from_numpy(w)).sum(), xc)
        (got,) = torch.autograd.grad((y * dev(w.astype(np.float32))).sum(), xg)
        ran = {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}
        # the mel chain at fft_length 2048 folds the filterbank adjoint into the backward kernel as well
        fused = kind.startswith('mel') and (n in (2048, 400) or (n in (512, 1024) and hop in (n // 8, n // 4, n // 2)))
        entry = 'tac_melspectrogram_backward_ola_f32' if fused else 'tac_spectrogram_backward_ola_f32'
        assert ran.get(entry) == 1 and 'tac_overlap_add_f32' not in ran, (tag, ran)
        assert entry == 'tac_spectrogram_backward_ola_f32' or 'tac_apply_filterbank_adjoint_f32' not in ran, (tag, ran)
        assert rel_err(host(got), want.numpy()) < (1e-3 if kind in ('mel_db', 'magnitude') else 1e-4), tag
        check_gradient_per_row(tac, module, kind, x, signals.uniform(tuple(want_y.shape), seed=9750 + case), n, hop, kw,
                               'fuzz_gradients_ola', tag, None if kind != 'mel_db' else (ref, floor * floor))


def test_fuzz_float64_chain(tac):
    """csrc/chain_f64.hip over random STFT arguments and sizes of every kind its plan distinguishes (radix-4 only, with a
    radix-2 / 3 / 5 pass, 8192 = twiddles from global memory, direct transform for odd lengths and halves with a prime
    factor above 5) against the float64 oracle: complex STFT, |X|^p (+ dB) and the mel chain; launch counters assert the
    float64 kernels ran."""
    rng = np.random.default_rng(8000 + SEED)
    sizes = [8, 12, 64, 100, 128, 256, 400, 480, 512, 1000, 1024, 2048, 4096, 6000, 8192, 77, 134, 331, 502]    # (direct transform: <= 512, _hip64.DIRECT_MAX)
    for case in range(max(12, CASES // 2)):
        n, hop, win_length, center, pad_mode, lead, length = draw_stft_args(rng, sizes, max_rows=3, max_len_factor=5)
        hop = max(hop, n // 16)                                          # (keeps the direct-transform cases small)
        normalized, onesided = bool(rng.random() < 0.3), bool(rng.random() < 0.7)
        x = signals.gained_with_silence(lead + (length,), seed=5500 + case + 7919 * SEED, n_fft=n, hop=hop).astype(np.float64)
        x *= 1.0 + 1e-9 * np.random.default_rng(case).standard_normal(x.shape)   # bits below float32 (silence stays exact)
        window = torch.from_numpy(signals.uniform((win_length,), seed=6500 + case).astype(np.float64) * 0.5 + 0.75)
        kw = dict(win_length=win_length, center=center, pad_mode=pad_mode, normalized=normalized)
        tag = ('f64', case, n, hop, kw, onesided, lead, length)
        before = dict(tac._hip.launches)
        want = torch_ref.stft(torch.from_numpy(x), n, hop, window=window, onesided=onesided, **kw).numpy()
        got = host(tac.stft(dev(x), n, hop_length=hop, window=window.cuda(), onesided=onesided, **kw))
        assert got.dtype == np.float64 and got.shape == want.shape, tag
        assert np.abs(got - want).max() <= FRAME_F64 * max(np.abs(want).max(), 1e-300), tag
        fbnd.check_frames(got, want, 'complex', FRAME_F64, 'fuzz_float64_chain', tag, n, signals.has_silence(x.shape, n, hop))
        power = float(rng.choice([1.0, 2.0, 0.7]))
        mels = int(rng.choice([5, 40, 80]))
        bank = torch.from_numpy(signals.uniform((n // 2 + 1, mels), seed=6600 + case).astype(np.float64))
        z = torch_ref.stft(torch.from_numpy(x), n, hop, window=window, **kw)
        want_m = torch_ref.amplitude_to_db(torch_ref.apply_filterbank(torch_ref.complex_norm(z, power), bank)).numpy()
        got_m = host(torch.ops.tac_amd.melspectrogram(dev(x), window.cuda(), bank.cuda(), n, hop, win_length, center, pad_mode,
                                                      normalized, True, power, True, 1.0, 1e-7))
        assert got_m.dtype == np.float64 and np.abs(got_m - want_m).max() < DB_F64, tag
        ran = {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}
        assert ran == {'tac_stft_f64': 1, 'tac_spectrogram_f64': 1, 'tac_apply_filterbank_f64': 1}, (tag, ran)


def test_fuzz_hpss(tac):
    """csrc/hpss.hip over random shapes, widths (equal: the fused tile kernel; unequal / small: the two-launch route), layouts
    (contiguous (F, T), the frame-major strided view the STFT kernels return), powers and mask kinds against a numpy
    restatement of beta_hpss.py:86-127.  Medians select existing values, so hard masks and the enhanced spectrograms behind
    the soft masks are exact; a few NaNs are planted in some cases (torch.median: a window that holds one has a NaN median)."""
    rng = np.random.default_rng(9000 + SEED)
    odd = list(range(1, 64, 2))           # (33 ... 63 since round 5: the two-launch route with a 32-column halo)
    for case in range(CASES):
        rows = int(rng.integers(1, 4))
        F, T = int(rng.integers(16, 300)), int(rng.integers(16, 300))
        if rng.random() < 0.5:
            kf = kt = int(rng.choice(odd[4:]))
        else:
            kf, kt = int(rng.choice(odd)), int(rng.choice(odd))
        kf, kt = min(kf, 2 * ((F - 1) // 2) - 1 if F < 65 else kf), min(kt, 2 * ((T - 1) // 2) - 1 if T < 65 else kt)
        kf, kt = max(kf, 1), max(kt, 1)
        s = (rng.random((rows, F, T), dtype=np.float32) * rng.integers(1, 5, (rows, F, T))).astype(np.float32)
        with_nan = rng.random() < 0.25
        if with_nan:
            for _ in range(int(rng.integers(1, 4))):
                s[int(rng.integers(rows)), int(rng.integers(F)), int(rng.integers(T))] = np.nan
        padf = np.pad(s, ((0, 0), (kf // 2, kf // 2), (0, 0)), mode='reflect')
        padt = np.pad(s, ((0, 0), (0, 0), (kt // 2, kt // 2)), mode='reflect')
        stf = np.stack([padf[:, i:i + F] for i in range(kf)], -1)
        stt = np.stack([padt[..., i:i + T] for i in range(kt)], -1)
        perc = np.sort(stf, -1)[..., kf // 2]
        harm = np.sort(stt, -1)[..., kt // 2]
        perc = np.where(np.isnan(stf).any(-1), np.float32(np.nan), perc)     # np.sort puts NaN last: restore torch.median's rule
        harm = np.where(np.isnan(stt).any(-1), np.float32(np.nan), harm)
        frame_major = bool(rng.random() < 0.5)
        x = dev(np.ascontiguousarray(s.transpose(0, 2, 1))).transpose(1, 2) if frame_major else dev(s)
        power = float(rng.choice([1.0, 2.0]))
        tag = ('hpss', case, rows, F, T, kf, kt, frame_major, power, with_nan)
        before = dict(tac._hip.launches)
        h, p, mh, mp = tac.hpss(x, (kf, kt), power, False)
        assert tac._hip.launches['tac_hpss_f32'] - before.get('tac_hpss_f32', 0) == 1, tag
        hp, pp = harm.astype(np.float32) ** np.float32(power), perc.astype(np.float32) ** np.float32(power)
        want_mh = (hp + np.float32(1e-6)) / (hp + pp + np.float32(1e-6))
        want_mp = (pp + np.float32(1e-6)) / (hp + pp + np.float32(1e-6))
        for got, want in ((mh, want_mh), (mp, want_mp), (h, s * want_mh), (p, s * want_mp)):
            got = host(got)
            assert np.array_equal(np.isnan(got), np.isnan(want)), tag
            ok = ~np.isnan(want)
            assert np.abs(got[ok] - want[ok]).max() <= 5e-7 * max(1.0, float(np.nanmax(s))), tag
        hard = tac.hpss(x, (kf, kt), power, True)
        ok = ~(np.isnan(harm) | np.isnan(perc))
        assert np.array_equal(host(hard[2])[ok], (harm > perc)[ok]) and np.array_equal(host(hard[3])[ok], (harm < perc)[ok]), tag


def test_fuzz_phase_vocoder(tac):
    """csrc/phase_vocoder.hip (running phase as a 32-bit fraction of a turn) over random shapes, rates, phase advances and
    layouts against the float64 evaluation of the reference's formula (functional.py:204-274) on the same float32 inputs."""
    rng = np.random.default_rng(9500 + SEED)
    for case in range(CASES):
        lead = tuple(int(v) for v in rng.integers(1, 4, size=int(rng.integers(1, 3))))
        F, T = int(rng.integers(3, 200)), int(rng.integers(2, 120))
        rate = float(rng.choice([0.5, 0.7, 0.9, 1.1, 1.3, 1.5, 2.0, 2.7])) if rng.random() < 0.7 else float(rng.uniform(0.3, 3.0))
        z = signals.audio_like(lead + (F, T, 2), seed=9600 + case + 7919 * SEED)
        adv = torch.from_numpy((rng.uniform(0, 2000.0) * np.linspace(0, 1, F)).astype(np.float32))[..., None]
        frame_major = bool(rng.random() < 0.5)
        x = dev(np.ascontiguousarray(z.swapaxes(-3, -2))).transpose(-3, -2) if frame_major else dev(z)
        tag = ('pv', case, lead, F, T, rate, frame_major)
        want = torch_ref.phase_vocoder(torch.from_numpy(z).double(), rate, adv.double()).numpy()
        before = dict(tac._hip.launches)
        got = host(tac.phase_vocoder(x, rate, adv.cuda()))
        assert tac._hip.launches['tac_phase_vocoder_f32'] - before.get('tac_phase_vocoder_f32', 0) == 1, tag
        assert got.shape == want.shape and got.dtype == np.float32, tag
        assert rel_err(got, want) < 2e-5, tag
