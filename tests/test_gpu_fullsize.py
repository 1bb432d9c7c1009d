"""-m gpu: every element of the outputs bench.py times, at the sizes it times them, against a float64 reference.

The persistent kernels decide which workgroup writes which rows from the grid and the batch, so the schedule at 256 or 512
rows is not the one the small parity shapes exercise.  Here each benchmarked call runs at its benchmarked shape and
parameters (routes depend on those, not on values), and every element it writes is compared per frame
(``frame_bounds``) with the oracle's own functions evaluated in float64 on the device (torch's FFT, independent of this
project's kernels), in row chunks.  Outputs start as a NaN pattern (``set_poison_outputs``) and every launch is checked
for positions it left.

Inputs: uniform in [-1, 1) from a seeded device generator (bench.py's distribution), row r scaled by 2^-(r mod 13), three
silent spans of 3 fft_length samples (start, mid-row off the hop grid, end) in every 16th row, one row all zeros.

``TAC_FULLSIZE_REPORT=path`` appends one JSON line per test: worst per-frame (per-row) error and its bound, the share of
dB elements the derived mask kept, wall time and peak device memory.
"""
import json
import math
import os
import time

import numpy as np
import pytest
import torch

import frame_bounds as fbnd
from oracle import torch_ref

pytestmark = pytest.mark.gpu

TIGHT = 2e-6        # complex rows and |X|, per frame
MEL = 2e-5          # power and mel, per frame
GRAD = 1e-3         # waveform gradient through dB, per row
DB_ABS = 1e-3
AMIN = 1e-7
POW_TOL = 1e-6     # per-frame accuracy of the power spectrum the dB mask assumes under the mel bank (measured: < 8e-7)
REF_BYTES = 3 << 30     # float64 reference bytes per row chunk (the chunk's peak extra memory is a few times this)


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


@pytest.fixture(autouse=True)
def every_output_written(tac):
    tac._hip.poison_report()
    yield
    left = tac._hip.poison_report()
    assert not left, 'kernel outputs left unwritten (poisoned elements per entry point): %r' % left


class Record(object):
    """wall time, peak device memory and the worst errors of one test (printed, and appended to TAC_FULLSIZE_REPORT)."""

    def __init__(self, name):
        self.name = name
        self.items = {}
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        self.base = torch.cuda.memory_allocated()
        self.t0 = time.time()

    def worst(self, key, value, bound, **extra):
        old = self.items.get(key)
        if old is None or value > old['worst']:
            self.items[key] = dict(worst=value, bound=bound, **extra)
        elif extra:
            old.update({k: min(v, old.get(k, v)) for k, v in extra.items()})

    def done(self):
        torch.cuda.synchronize()
        line = {'test': self.name, 'wall_s': round(time.time() - self.t0, 2),
                'peak_extra_GB': round((torch.cuda.max_memory_allocated() - self.base) / 1e9, 2), 'checks': self.items}
        print(json.dumps(line))
        path = os.environ.get('TAC_FULLSIZE_REPORT')
        if path:
            with open(path, 'a') as f:
                f.write(json.dumps(line) + '\n')


def launched_since(tac_, before):
    now = tac_._hip.launches
    return {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)}


def bench_input(shape, n_fft, hop, seed):
    """bench.py's distribution with per-row gains and silence (module docstring)."""
    gen = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.rand(shape, device='cuda', generator=gen) * 2 - 1
    rows = x.view(-1, shape[-1])
    n, length = rows.shape
    rows.mul_((2.0 ** -(torch.arange(n, device='cuda') % 13).float())[:, None])
    span = 3 * n_fft
    mid = length // 2 + hop // 3
    for r in range(0, n, 16):
        rows[r, :span] = 0
        rows[r, mid:mid + span] = 0
        rows[r, length - span:] = 0
    rows[n - 3] = 0
    return x


def row_chunks(n_rows, bytes_per_row):
    step = max(1, min(n_rows, REF_BYTES // max(1, bytes_per_row)))
    return [(r, min(n_rows, r + step)) for r in range(0, n_rows, step)]


def ref_stft(x_rows, n_fft, hop, window):
    """(rows, F, T, 2) float64 on the device: the oracle's stft with the module's window."""
    return torch_ref.stft(x_rows.double(), n_fft, hop, window=window.double())


def pin_reference(x_rows, pick, n_fft, hop, window, fb=None, power=2.0):
    """The device float64 reference equals the CPU oracle in float64 on the rows ``pick`` (one loud, one quiet with silence)."""
    for r in pick:
        xr = x_rows[r:r + 1]
        d = torch_ref.complex_norm(ref_stft(xr, n_fft, hop, window), power)
        c = torch_ref.complex_norm(torch_ref.stft(xr.double().cpu(), n_fft, hop, window=window.double().cpu()), power)
        if fb is not None:
            d, c = torch_ref.apply_filterbank(d, fb.double()), torch_ref.apply_filterbank(c, fb.double().cpu())
        err = float((d.cpu() - c).abs().max() / c.abs().max())
        assert err < 1e-12, 'device float64 reference differs from the CPU oracle on row %d: %.3e' % (r, err)


def ref_mel(x_rows, n_fft, hop, window, fb64):
    """(mel, lin) in frames layout (rows, T, M), float64: the oracle's mel values and their per-element linear bound."""
    power = torch_ref.complex_norm(ref_stft(x_rows, n_fft, hop, window), 2.0)
    mel = fbnd.frames_of(torch_ref.apply_filterbank(power, fb64), 'spec')
    return mel, fbnd.mel_linear_bound(fbnd.frames_of(power, 'spec'), fb64, POW_TOL)


def check_mel_db(rec, key, got, x, n_fft, hop, window, fb, pick):
    """``got`` (*, M, T) dB of the mel chain of ``x`` (*, L), every element."""
    xr = x.reshape(-1, x.shape[-1])
    g = got.reshape(-1, got.shape[-2], got.shape[-1])
    pin_reference(xr, pick, n_fft, hop, window, fb)
    fb64 = fb.double()
    per_row = (n_fft // 2 + 1) * g.shape[-1] * 16 * 3
    for r0, r1 in row_chunks(xr.shape[0], per_row):
        mel, lin = ref_mel(xr[r0:r1], n_fft, hop, window, fb64)
        worst, kept, cdev = fbnd.assert_db(fbnd.frames_of(g[r0:r1], 'spec'), mel, MEL, DB_ABS, AMIN, what=key, row0=r0, lin=lin)
        rec.worst(key, worst, DB_ABS, kept=kept, clamp_dev=cdev)
        del mel, lin


def check_linear(rec, key, got, x, n_fft, hop, window, kind, power, tol, pick):
    """``got``: complex rows (*, F, T, 2) (``kind`` 'complex') or |X|^power (*, F, T) of ``x``, every element."""
    xr = x.reshape(-1, x.shape[-1])
    pin_reference(xr, pick, n_fft, hop, window, None, 1.0 if kind == 'complex' else power)
    n_bins = n_fft // 2 + 1
    g = got.reshape((-1,) + tuple(got.shape[-3 if kind == 'complex' else -2:]))
    per_row = n_bins * g.shape[2 if kind == 'complex' else -1] * 16 * 3
    for r0, r1 in row_chunks(xr.shape[0], per_row):
        z = ref_stft(xr[r0:r1], n_fft, hop, window)
        ref = z if kind == 'complex' else torch_ref.complex_norm(z, power)
        del z
        rec.worst(key, fbnd.assert_linear(fbnd.frames_of(g[r0:r1], kind), fbnd.frames_of(ref, kind), tol, key, r0), tol)
        del ref


def mel_model(tac_, num_mels, sr, n_fft, hop):
    return torch.nn.Sequential(*tac_.Melspectrogram(num_mels=num_mels, sample_rate=sr, fft_length=n_fft, hop_length=hop),
                               tac_.AmplitudeToDb()).cuda()


def check_mel_grad(rec, key, tac_, model, x, n_fft, hop, backward_entry, seed):
    """Waveform gradient of (w * model(x)).sum() against float64 device autograd through the oracle chain, every sample.
    ``w`` is zeroed on the bands whose dB value the float32 forward does not determine to DB_ABS (reference mel within its
    linear bound of the clamp, or a derived dB bound above DB_ABS): the gradient through them is not comparable."""
    window, fb = model[0].window, model[2].filterbank
    xr = x.reshape(-1, x.shape[-1])
    fb64 = fb.double()
    gen = torch.Generator(device='cuda').manual_seed(seed)
    n_frames = 1 + x.shape[-1] // hop
    w = torch.rand((xr.shape[0], fb.shape[1], n_frames), device='cuda', generator=gen)
    chunks = row_chunks(xr.shape[0], (n_fft // 2 + 1) * n_frames * 16 * 8)
    kept = 0
    for r0, r1 in chunks:
        with torch.no_grad():
            mel, lin = ref_mel(xr[r0:r1], n_fft, hop, window, fb64)
        bound = fbnd.DB_PER_REL * lin / mel.abs().clamp(min=math.sqrt(AMIN))
        ok = ((mel - lin).clamp(min=0) ** 2 > AMIN) & (bound <= DB_ABS)
        w[r0:r1] *= ok.transpose(1, 2)
        kept += int(ok.sum())
        del mel, lin, bound, ok
    rec.worst(key + ' (w kept)', 0.0, 0.0, kept=kept / w.numel())
    xg = x.clone().requires_grad_(True)
    before = dict(tac_._hip.launches)
    y = model(xg)
    (w.view(y.shape) * y).sum().backward()
    ran = launched_since(tac_, before)
    assert ran.get(backward_entry) == 1, ran
    got = xg.grad.reshape(xr.shape)
    del y, xg
    for r0, r1 in chunks:
        xc = xr[r0:r1].double().requires_grad_(True)
        mel = torch_ref.apply_filterbank(torch_ref.complex_norm(ref_stft(xc, n_fft, hop, window), 2.0), fb64)
        (w[r0:r1].double() * torch_ref.amplitude_to_db(mel, 1.0, AMIN)).sum().backward()
        rec.worst(key, fbnd.assert_rows(got[r0:r1], xc.grad, GRAD, key, r0), GRAD)
        del xc, mel
    del got, w


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ self-test of the write check
def test_write_check_reports_an_unwritten_row(tac):
    """A launch through the C ABI whose descriptor names one row fewer than the buffers hold: the kernel reads and writes
    strictly inside them, and the check names the entry point and counts exactly the untouched last row."""
    H, N = tac._hip, tac._native
    rows, length, n_fft, hop = 4, 8000, 512, 128
    x = bench_input((rows, length), n_fft, hop, seed=11)
    win = torch.hann_window(n_fft, device='cuda')
    g = H.geometry(x, n_fft, hop, n_fft, True, 'reflect', False, True)
    desc = N.StftDesc(rows=rows - 1, length=length, row_stride=length, n_fft=n_fft, hop=hop, win_length=n_fft, center=1,
                      pad_mode=N.PAD_MODES['reflect'], normalized=0, onesided=1, reserved=0)
    out = H._empty(g.spec_shape, device='cuda')
    H.poison_report()
    with N.on_device(x.device):
        rc = N.lib().tac_spectrogram_f32(N.ptr(x), N.ptr(win), desc, 2.0, 0, 1.0, AMIN, N.ptr(out), N.stream_ptr(x.device))
    N.check(rc, 'tac_spectrogram_f32')
    H.check_written('selftest_short_descriptor', out)
    assert H.poison_report() == {'selftest_short_descriptor': g.n_frames * g.n_bins}
    assert int(H.poison_count(out[:rows - 1])) == 0 and int(H.poison_count(out[rows - 1])) == out[rows - 1].numel()


# ------------------------------------------------------------------ 1. cfg-2 headline
def test_cfg2_headline_every_element(tac):
    rec = Record('cfg2_headline')
    model = mel_model(tac, 128, 16000, 2048, 512)
    window, fb = model[0].window, model[2].filterbank
    xs = [bench_input((256, 1, 160000), 2048, 512, seed=s) for s in range(4)]
    before = dict(tac._hip.launches)
    out = model(xs[0])
    assert type(out) is torch.Tensor and tuple(out.shape) == (256, 1, 128, 313)
    assert launched_since(tac, before) == {'tac_melspec_sparse_f32': 1}
    check_mel_db(rec, 'module', out, xs[0], 2048, 512, window, fb, pick=(1, 16))
    del out
    call = tac.planned(model, xs[0])
    assert call.fused()
    before = dict(tac._hip.launches)
    out = call(xs[0])
    assert launched_since(tac, before) == {'tac_melspec_sparse_f32': 1}
    check_mel_db(rec, 'planned', out, xs[0], 2048, 512, window, fb, pick=())
    del out
    before = dict(tac._hip.launches)
    outs = [model(x) for x in xs]                                   # bench's rotation: back to back, no synchronisation
    assert launched_since(tac, before) == {'tac_melspec_sparse_f32': 4}
    for i, (x, out) in enumerate(zip(xs, outs)):
        check_mel_db(rec, 'rotation[%d]' % i, out, x, 2048, 512, window, fb, pick=(1, 16) if i else ())
    del outs, xs, model
    rec.done()
    _free()


# ------------------------------------------------------------------ 2. cfg-2 stages
def test_cfg2_stages_every_element(tac):
    rec = Record('cfg2_stages')
    x = bench_input((256, 1, 160000), 2048, 512, seed=5)
    win = torch.hann_window(2048, device='cuda')
    before = dict(tac._hip.launches)
    z = tac.realize(tac.stft(x, 2048, hop_length=512, window=win))
    assert launched_since(tac, before) == {'tac_stft_f32': 1}
    check_linear(rec, 'stft_complex', z, x, 2048, 512, win, 'complex', 1.0, TIGHT, pick=(2, 32))
    del z
    spec = tac.Spectrogram(2048, 512, power=2.).cuda()
    p = tac.realize(spec(x))
    check_linear(rec, 'spectrogram_power', p, x, 2048, 512, spec[0].window, 'spec', 2.0, MEL, pick=())
    fb_dense = torch.rand(1025, 128, device='cuda', generator=torch.Generator(device='cuda').manual_seed(7))
    before = dict(tac._hip.launches)
    m = tac.realize(tac.apply_filterbank(p, fb_dense))
    assert launched_since(tac, before) == {'tac_apply_filterbank_f32': 1}          # the fp32 MFMA GEMM (dense bank)
    pr, mr = p.reshape(256, 1025, 313), m.reshape(256, 128, 313)
    for r0, r1 in row_chunks(256, 1025 * 313 * 8 * 2):
        ref = torch_ref.apply_filterbank(pr[r0:r1].double(), fb_dense.double())      # the kernel's own input, in float64
        rec.worst('filterbank_mfma_dense', fbnd.assert_linear(fbnd.frames_of(mr[r0:r1], 'spec'), fbnd.frames_of(ref, 'spec'),
                                                              MEL, 'filterbank_mfma_dense', r0), MEL)
    del x, p, m, pr, mr, spec
    rec.done()
    _free()


# ------------------------------------------------------------------ 3. cfg-2 training step
def test_cfg2_training_step_gradient(tac):
    rec = Record('cfg2_train_step')
    model = mel_model(tac, 128, 16000, 2048, 512)
    x = bench_input((256, 1, 160000), 2048, 512, seed=6)
    check_mel_grad(rec, 'grad_wave', tac, model, x, 2048, 512, 'tac_melspectrogram_backward_ola_f32', seed=8)
    del x, model
    rec.done()
    _free()


# ------------------------------------------------------------------ 4. cfg-3 shard
def test_cfg3_shard_every_element(tac):
    rec = Record('cfg3_shard')
    model = mel_model(tac, 128, 44100, 2048, 512)
    x = bench_input((256, 1, 44100 * 30), 2048, 512, seed=9)
    before = dict(tac._hip.launches)
    out = model(x)
    assert launched_since(tac, before) == {'tac_melspec_sparse_f32': 1}
    check_mel_db(rec, 'mel_db', out, x, 2048, 512, model[0].window, model[2].filterbank, pick=(1, 48))
    del out, x, model
    rec.done()
    _free()


# ------------------------------------------------------------------ 5. cfg-4
def test_cfg4_every_element(tac):
    rec = Record('cfg4_spectrogram_4096')
    spec = tac.Spectrogram(4096, 1024, power=1.).cuda()
    x = bench_input((64, 8, 48000 * 60), 4096, 1024, seed=10)
    before = dict(tac._hip.launches)
    out = tac.realize(spec(x))
    assert launched_since(tac, before) == {'tac_spectrogram_f32': 1}
    assert tuple(out.shape) == (64, 8, 2049, 2813)
    check_linear(rec, 'magnitude', out, x, 4096, 1024, spec[0].window, 'spec', 1.0, TIGHT, pick=(3, 256))
    del out, x, spec
    rec.done()
    _free()


# ------------------------------------------------------------------ 6. mel4096 in one launch
def test_mel4096_one_launch_every_element(tac):
    rec = Record('mel4096_one_launch')
    model = mel_model(tac, 128, 48000, 4096, 1024)
    x = bench_input((8, 8, 480000), 4096, 1024, seed=12)
    before = dict(tac._hip.launches)
    out = model(x)
    assert launched_since(tac, before) == {'tac_melspec_sparse_f32': 1}
    check_mel_db(rec, 'mel_db', out, x, 4096, 1024, model[0].window, model[2].filterbank, pick=(1, 32))
    del out, x, model
    rec.done()
    _free()


# ------------------------------------------------------------------ 7. fft_length 400 front end
def test_n400_front_end_every_element(tac):
    rec = Record('n400_front_end')
    x = bench_input((256, 160000), 400, 160, seed=13)
    st = tac.STFT(400, 160).cuda()
    z = tac.realize(st(x))
    check_linear(rec, 'stft_complex', z, x, 400, 160, st.window, 'complex', 1.0, TIGHT, pick=(1, 16))
    del z
    model = mel_model(tac, 80, 16000, 400, 160)
    before = dict(tac._hip.launches)
    out = model(x)
    assert launched_since(tac, before) == {'tac_melspec_sparse_f32': 1}
    check_mel_db(rec, 'mel80_db', out, x, 400, 160, model[0].window, model[2].filterbank, pick=())
    del out
    check_mel_grad(rec, 'grad_wave', tac, model, x, 400, 160, 'tac_melspectrogram_backward_ola_f32', seed=14)
    del x, model
    rec.done()
    _free()


# ------------------------------------------------------------------ 8. cfg-5 mu-law
def _mulaw_encode_pinned(golden):
    """The host oracle's mu-law codes depend on its vectorised log1p: it is trusted for the encoder only where it reproduces
    the golden codes captured from the reference (the encoder half of test_gpu_parity.mulaw_oracle_pinned; the decoder is
    compared with the golden table itself)."""
    from oracle import signals
    g = golden('g5_mulaw')
    x2 = torch.from_numpy(signals.uniform((1000000,), seed=8, scale=1.0))
    return np.array_equal(torch_ref.mu_law_encoding(x2, 256).numpy(), g['enc256_unit'].astype(np.int64))


def test_cfg5_mulaw_every_sample(tac, golden):
    rec = Record('cfg5_mulaw')
    x = bench_input((1024, 1, 120000), 1, 1, seed=15)
    before = dict(tac._hip.launches)
    codes = tac.mu_law_encoding(x, 256)
    assert launched_since(tac, before) == {'tac_mulaw_encode_f32_i64': 1}
    assert codes.dtype == torch.int64 and bool((codes >= 0).all()) and bool((codes <= 255).all())
    if _mulaw_encode_pinned(golden):
        want = torch_ref.mu_law_encoding(x.cpu(), 256)
        nbad = int((codes.cpu() != want).sum())
        assert nbad == 0, 'mu-law codes differ from the pinned host oracle on %d samples' % nbad
        rec.worst('encode mismatches', float(nbad), 0.0)
    lut = torch.from_numpy(np.ascontiguousarray(golden('g5_mulaw')['lut256'].view(np.int32))).cuda()
    back = tac.realize(tac.mu_law_decoding(codes, 256))
    assert back.dtype == torch.float32
    assert int(torch.unique(codes).numel()) == 256                                  # every code is decoded
    nbad = int((back.view(torch.int32) != lut[codes]).sum())
    assert nbad == 0, 'mu-law decode differs from the reference table on %d codes' % nbad
    rec.worst('decode mismatches', float(nbad), 0.0)
    del x, codes, back
    rec.done()
    _free()
