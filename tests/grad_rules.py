"""Shared by tests/test_grad_rules_cpu.py and tests/test_gradient_sweeps_gpu.py (a plain module: no tests in here): case
generators, float64 references and bounds for the gradients beside the main chain — the window gradient
(``tac_window_grad_f32`` + ``tac_sum_slabs_f32``), the filterbank gradient (``_hip.filterbank_grad``: the MFMA GEMM contracting
over every frame of the batch), and the ``hpss`` / ``phase_vocoder`` / ``stretch_norm`` / ``stretch_mel`` gradient kernels.

Every sweep body is written once and takes a device: the GPU file runs it on the kernels (strict mode, poisoned outputs, launch
counters), the CPU file on the package's CPU route at the same shapes and bounds — so inputs, references and bounds are known to
be sound before a GPU sees them, and the float32 CPU evaluation is shown to stay inside every bound asserted.

References are float64 autograd through ``oracle/torch_ref.py`` on the CPU, on the float32 window / bank cast to float64.

How accumulated gradients are bounded.  The error of element e is |got - ref64| / A_e with A_e the float64 sum of the absolute
values of the K terms that make the element up (``acc_measure``).  Two bounds are asserted (``check_acc``):

  * ``acc_hard(K) = K 2^-24``: what no summation order of fused multiply-adds can break;
  * ``acc_tight(K) = 4 sqrt(K) 2^-24`` (never above the hard bound).  The accuracy class the choice was made against is torch's
    float32 CPU evaluation of the same sum on the same operands (blocked summation), NOT the kernels.  Worst measure over every
    n_mels / layout / row mode, in units of 2^-24 (seed 0; the kernel column on the MI355X, the tables ACC_* below):

        filterbank gradient     K = 1    31     32     33     4097    70001
            CPU float32         1.00    6.37   7.91   7.00   4.22    3.91     (0.4 .. 1.0 at n_mels 1 / 23 / 128 from K = 4097 on)
            kernel              1.00    6.37   7.91   7.00   8.78    7.57
        window gradient, K = rows x frames from P - 1 = 1023 to 3591 (P = 1024 partial rows on this part)
            CPU float32         0.27 .. 0.83
            kernel              0.69 .. 4.16

    Up to K = 33 kernel and CPU agree to the last bit (the same fused multiply-adds in the same order).  From K = 4097 on torch's
    CPU sums are blocked and the kernels are up to 13 x (filterbank, n_mels 128 at K = 70 001) and 7 x (window) the CPU value:
    outside 4 x.  The cause is the summation order, not an indexing fault: every one-hot probe is exact at every K, and the
    kernels add in ONE sequential order (one workgroup walks the whole K range in 32-deep chunks of the MFMA; the window
    kernel's P partial rows are added up in order by ``tac_sum_slabs_f32``), where a rounding of size 2^-24 |partial sum| enters
    at every step.  On these inputs — incoming gradients of either sign, frame gains 2^0 .. 2^-12 — the partial sums stay near
    sqrt(K) terms in size while A_e grows like K, so the measure is flat in K (8.8 at 4097, 7.6 at 70 001) and far inside the
    envelope 4 sqrt(K) 2^-24 that a sequential float32 sum keeps with terms of one sign; that envelope is the bound asserted,
    and the kernels stay as they are ("Gradient sweeps", says why no split-K form was written).
"""
import math
import os

import numpy as np
import torch

import frame_bounds as fbnd
from conftest import rel_err
from oracle import signals, torch_ref
from stretch_rules import grid, interpolated                      # (re-exported: the stretch sweeps and tests/test_stretch_gpu.py)

CASES = int(os.environ.get('TAC_FUZZ_CASES', '32'))
SEED = int(os.environ.get('TAC_FUZZ_SEED', '0'))
U = 2.0 ** -24                                                     # unit roundoff of float32

# measured worst acc_measure / 2^-24 (seed 0; the kernel values on the MI355X, the CPU values torch's float32 on the host)
ACC_FB_CPU = {1: 1.00, 31: 6.37, 32: 7.91, 33: 7.00, 4097: 4.22, 70001: 3.91}
ACC_FB_GPU = {1: 1.00, 31: 6.37, 32: 7.91, 33: 7.00, 4097: 8.78, 70001: 7.57}
ACC_WIN_CPU = (0.27, 0.83)         # (least, largest) over the ten window cases
ACC_WIN_GPU = (0.69, 4.16)

def to(device, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def host(t):
    return t.detach().cpu().numpy()


def launched_since(tac, before):
    now = tac._hip.launches
    return {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)}


def on_gpu(device):
    return torch.device(device).type == 'cuda'


# ----------------------------------------------------------------------------- accumulated sums
def acc_measure(got, ref64, abs64):
    """max over the elements of |got - ref64| / A_e; an element whose terms are all zero (A_e == 0) must be exactly zero (inf
    otherwise); NaN anywhere gives NaN."""
    g = torch.as_tensor(got).detach().cpu().to(torch.float64).reshape(ref64.shape)
    d = (g - ref64).abs()
    if bool(torch.isnan(d).any()):
        return float('nan')
    zero = abs64 == 0
    ratio = d / torch.where(zero, torch.ones_like(abs64), abs64)
    ratio = torch.where(zero & (d > 0), torch.full_like(ratio, math.inf), ratio)
    return float(ratio.max())


def acc_hard(k):
    return k * U


def acc_tight(k):
    return min(acc_hard(k), 4.0 * math.sqrt(k) * U)


def check_acc(got, ref64, abs64, k, test, case, cpu32=None):
    """Both bounds on an accumulated gradient of ``k`` terms per element, reported (``cpu32``: torch's float32 CPU evaluation of the
    same sum, reported beside it as kind 'acc_cpu32').  Returns the measure."""
    m = acc_measure(got, ref64, abs64)
    fbnd.report(test, case, k, 'acc', m, acc_tight(k))
    if cpu32 is not None:
        fbnd.report(test, case, k, 'acc_cpu32', acc_measure(cpu32, ref64, abs64), acc_tight(k))
    assert m <= acc_hard(k), '%s %r: accumulation error %.3e of sum |terms| beyond K 2^-24 = %.3e' % (test, case, m, acc_hard(k))
    assert m <= acc_tight(k), '%s %r: accumulation error %.3e of sum |terms| beyond 4 sqrt(K) 2^-24 = %.3e' % (
        test, case, m, acc_tight(k))
    return m


# ----------------------------------------------------------------------------- 1. window gradient
P_DEFAULT = 1024                                                   # 4 x 256 CUs: what the CPU file generates for (the GPU file reads its own)
_ROW_PREFERENCE = (3, 7, 5, 9, 11, 13, 4, 8, 6, 15, 10, 12, 14, 16, 2, 1)


def window_partials(tac):
    """P of the device: what ``tac_window_grad_partials`` answers for more frames than any part has partial rows."""
    desc = tac._native.StftDesc(rows=1 << 16, length=1 << 16, row_stride=1 << 16, n_fft=64, hop=16, win_length=64, center=1,
                                pad_mode=tac._native.PAD_MODES['reflect'], normalized=0, onesided=1, reserved=0)
    p = int(tac._native.lib().tac_window_grad_partials(desc))
    assert p > 0, p
    return p


def rows_for(total, prefer=_ROW_PREFERENCE):
    for r in prefer:
        if total % r == 0 and total // r >= 2:
            return r
    return 1


def length_for(n_frames, n_fft, hop, center, extra):
    """A row length that frames into exactly ``n_frames`` frames, ``extra`` (< hop) samples past the hop grid."""
    pad = n_fft // 2 if center else 0
    return (n_frames - 1) * hop + n_fft - 2 * pad + min(extra, hop - 1)


def window_cases(p):
    """The cases of section 1 for ``p`` partial rows: total frame counts p - 1, p, p + 1, 2 p + 3 and about 3.5 p, in 3 and 7 rows
    where the total divides (else the nearest row count that does), every pad mode, center=False, a short window, normalized,
    two-sided, strided rows, and one case per other route into ``_frame_gradients``."""
    seven = 7 * (p // 2 + 1)                                      # (frames per row odd at even p: chunk borders fall inside rows)
    three = 3 * ((7 * p // 2) // 3) + 3
    spec = [  # name, total, rows (None: rows_for), n_fft, hop, keyword arguments, strided rows
        ('p-1', p - 1, None, 64, 16, dict(pad_mode='reflect'), False),
        ('p', p, None, 64, 16, dict(pad_mode='constant', win_length=48), False),
        ('p+1', p + 1, None, 64, 16, dict(pad_mode='replicate', normalized=True), False),
        ('2p+3', 2 * p + 3, None, 64, 16, dict(pad_mode='circular', onesided=False), False),
        ('3.5p/7rows', seven, 7, 64, 16, dict(center=False), True),
        ('3.5p/3rows', three, 3, 64, 16, dict(pad_mode='reflect', win_length=40, normalized=True), True),
        ('p+1/400', p + 1, None, 400, 160, dict(win_length=320), False),
        ('2p+3/300', 2 * p + 3, None, 300, 75, dict(pad_mode='constant'), False),
        ('p+1/77', p + 1, None, 77, 20, dict(pad_mode='replicate'), False),
        ('p+1/2048', p + 1, None, 2048, 512, dict(pad_mode='reflect'), False),
    ]
    out = []
    for i, (name, total, rows, n_fft, hop, kw, strided) in enumerate(spec):
        rows = rows_for(total) if rows is None else rows
        assert total % rows == 0, (name, total, rows)
        kw = dict(dict(win_length=n_fft, center=True, pad_mode='reflect', normalized=False, onesided=True), **kw)
        n_frames = total // rows
        length = length_for(n_frames, n_fft, hop, kw['center'], 5 + i)
        out.append(dict(name=name, total=total, rows=rows, n_frames=n_frames, n_fft=n_fft, hop=hop, kw=kw, strided=strided,
                        length=length, seed=700 + i))
    return out


def frames_of_length(length, n_fft, hop, center):
    return 1 + (length + (2 * (n_fft // 2) if center else 0) - n_fft) // hop


def window_chunk(total, p):
    """(partial rows the entry point asks for, consecutive frames a workgroup owns)."""
    parts = min(total, p)
    return parts, -(-total // parts)


def window_probe_frames(case, p):
    """Flattened (row, frame) indices of the one-hot probes: the first and the last frame, the frames on either side of a
    workgroup's chunk border and of a row border."""
    total, n_frames, rows = case['total'], case['n_frames'], case['rows']
    parts, per = window_chunk(total, p)
    used = -(-total // per)                                            # workgroups whose chunk is not empty
    picks = [0, total - 1]
    c = max(1, used // 2)
    if c * per < total:
        picks += [c * per - 1, c * per]
    if rows >= 2:
        r = rows - 1
        picks += [r * n_frames - 1, r * n_frames]
    return sorted(set(picks))


def window_waves(case):
    """(dense waveform with silence and a silent row, waveform without silence for the one-hot probes), float32 (rows, length)."""
    shape = (case['rows'], case['length'])
    x = signals.gained_with_silence(shape, case['seed'], case['n_fft'], case['hop'])
    plain = signals.uniform(shape, case['seed'] + 50) * (2.0 ** -(np.arange(case['rows']) % 13)).astype(np.float32)[:, None]
    return x, plain


def window_of(case):
    wl = case['kw']['win_length']
    return (np.hanning(wl + 2)[1:-1] + 0.1 + 0.05 * signals.uniform((wl,), case['seed'] + 90)).astype(np.float32)


def window_grad_terms(x64, w64, g64, n_fft, hop, win_length, center, pad_mode, normalized, onesided):
    """The window gradient as the sum the kernel forms, in float64: with gfr the gradient w.r.t. the windowed frames,
    g_window[n] = sum over (row, frame) of gfr[row][t][n] * padded[row][t hop + n].  Returns (that sum, the sum of the terms'
    absolute values), both cut to the window's ``win_length`` samples."""
    rows = x64.reshape(-1, x64.shape[-1])
    if center:
        pad = n_fft // 2
        rows = torch.nn.functional.pad(rows[:, None], (pad, pad), mode=pad_mode)[:, 0]
    xf = rows.unfold(-1, n_fft, hop)                                   # (rows, frames, n_fft)
    off = (n_fft - win_length) // 2
    wfull = torch.zeros(n_fft, dtype=torch.float64)
    wfull[off:off + win_length] = w64
    fw = (xf * wfull).detach().requires_grad_(True)
    z = torch.fft.rfft(fw, dim=-1) if onesided else torch.fft.fft(fw, dim=-1)
    if normalized:
        z = z * n_fft ** -0.5
    y = torch.view_as_real(z).permute(0, 2, 1, 3)                      # (rows, bins, frames, 2)
    (gfr,) = torch.autograd.grad(y, fw, g64.reshape(y.shape))
    terms = gfr * xf
    return terms.sum((0, 1))[off:off + win_length], terms.abs().sum((0, 1))[off:off + win_length]


def _stft_kwargs(case):
    kw = case['kw']
    return dict(win_length=kw['win_length'], center=kw['center'], pad_mode=kw['pad_mode'], normalized=kw['normalized'],
                onesided=kw['onesided'])


def _strided_rows(device, x, strided):
    """``x`` (rows, length) on the device; ``strided``: as a slice of a wider buffer (row_stride = length + 37)."""
    if not strided:
        return to(device, x)
    wide = torch.full((x.shape[0], x.shape[1] + 37), 3.0, dtype=torch.float32, device=device)       # (what lies between rows is not silence)
    wide[:, :x.shape[1]] = to(device, x)
    return wide[:, :x.shape[1]]


def window_case_body(tac, device, case, p, test='window_grad'):
    """The three probes of one window-gradient case.  Returns (kernel acc measure, float32-CPU acc measure) of the dense probe."""
    n_fft, hop, rows, n_frames = case['n_fft'], case['hop'], case['rows'], case['n_frames']
    kw = _stft_kwargs(case)
    assert frames_of_length(case['length'], n_fft, hop, kw['center']) == n_frames, case
    gpu = on_gpu(device)
    x_np, plain_np = window_waves(case)
    w_np = window_of(case)
    n_bins = n_fft // 2 + 1 if kw['onesided'] else n_fft
    tag = (case['name'], n_fft, hop, rows, n_frames, tuple(sorted(kw.items())), case['strided'])

    def graphs(wave_np):
        w64 = torch.from_numpy(w_np).double().requires_grad_(True)
        y64 = torch_ref.stft(torch.from_numpy(wave_np).double(), n_fft, hop, window=w64, **kw)
        w = to(device, w_np).requires_grad_(True)
        xd = _strided_rows(device, wave_np, case['strided'])
        if case['strided']:
            assert xd.stride(0) != xd.shape[1]
        y = tac.stft(xd, n_fft, hop_length=hop, window=w, **kw)
        assert tuple(y.shape) == tuple(y64.shape) == (rows, n_bins, n_frames, 2), (tag, y.shape, y64.shape)
        return w64, y64, w, y

    def grads(w64, y64, w, y, g_np, count=True):
        (want,) = torch.autograd.grad(y64, w64, torch.from_numpy(g_np).double(), retain_graph=True)
        before = dict(tac._hip.launches) if gpu else None
        (got,) = torch.autograd.grad(y, w, to(device, g_np), retain_graph=True)
        if gpu and count:
            ran = launched_since(tac, before)
            assert ran.get('tac_window_grad_f32') == 1 and ran.get('tac_sum_slabs_f32') == 1, (tag, ran)
            assert 'tac_overlap_add_f32' not in ran, (tag, ran)               # (the waveform's gradient was not asked for)
        return got, want

    # one-hot: only one (row, frame) carries gradient, on a waveform without silence
    w64, y64, w, y = graphs(plain_np)
    for fi in window_probe_frames(case, p):
        r, t = divmod(fi, n_frames)
        g_np = np.zeros((rows, n_bins, n_frames, 2), dtype=np.float32)
        g_np[r, :, t, :] = signals.uniform((n_bins, 2), seed=case['seed'] + 7 * fi + 1)
        got, want = grads(w64, y64, w, y, g_np)
        assert float(want.abs().max()) > 0, (tag, fi)
        err = rel_err(host(got), want.numpy())
        fbnd.report(test, tag + ('one-hot', fi), n_fft, 'window_onehot', err, 1e-5)
        assert err < 1e-5, '%s %r: one-hot (row %d, frame %d) is %.3e of the reference maximum off' % (test, tag, r, t, err)
    # dense, silent row, repeatability: the waveform with silence
    w64, y64, w, y = graphs(x_np)
    g_np = signals.uniform((rows, n_bins, n_frames, 2), seed=case['seed'] + 3)
    got, want = grads(w64, y64, w, y, g_np)
    again, _ = grads(w64, y64, w, y, g_np)
    assert torch.equal(got, again), '%s %r: two runs differ (the partial rows are added in a fixed order)' % (test, tag)
    if rows >= 3:
        assert not x_np[1].any()
        g_quiet = g_np.copy()
        g_quiet[1] = 0.0
        quiet, _ = grads(w64, y64, w, y, g_quiet)
        assert torch.equal(got, quiet), '%s %r: the silent row contributed to the window gradient' % (test, tag)
    err = rel_err(host(got), want.numpy())
    fbnd.report(test, tag + ('dense',), n_fft, 'window_dense', err, 1e-4)
    assert err < 1e-4, '%s %r: dense window gradient %.3e of the reference maximum off' % (test, tag, err)
    ref_sum, abs_sum = window_grad_terms(torch.from_numpy(x_np).double(), torch.from_numpy(w_np).double(),
                                         torch.from_numpy(g_np).double(), n_fft, hop, **kw)
    assert float((ref_sum - want).abs().max()) <= 1e-12 * float(want.abs().max()), tag       # the restatement IS the reference
    w32 = torch.from_numpy(w_np).requires_grad_(True)
    (cpu32,) = torch.autograd.grad(torch_ref.stft(torch.from_numpy(x_np), n_fft, hop, window=w32, **kw), w32, torch.from_numpy(g_np))
    k = rows * n_frames
    m = check_acc(got, want.detach(), abs_sum, k, test, tag, cpu32=cpu32)
    return m, acc_measure(cpu32, want.detach(), abs_sum)


# ----------------------------------------------------------------------------- 2. filterbank gradient
FB_K = (1, 31, 32, 33, 4097, 70001)
FB_FREQS = (201, 257, 1025)
FB_MELS = (1, 23, 128, 130)


def fb_freqs_at(k):
    return FB_FREQS[:2] if k >= 70001 else FB_FREQS                  # (1025 bins at the longest K would take tens of seconds)


FB_SWEEP = [(k, f) for k in FB_K for f in fb_freqs_at(k)]


def fb_row_modes(k):
    """(rows, frames per row): ``k`` frames as one row and as several rows (the smallest divisor above one; a prime k is k rows
    of one frame)."""
    if k == 1:
        return [(1, 1)]
    d = next((d for d in range(2, int(math.isqrt(k)) + 1) if k % d == 0), k)
    return [(1, k), (d, k // d)]


def fb_inputs(k, rows, n_frames, n_freqs, seed):
    """(spectrogram (rows, F, T) >= 0 with frame gains 2^0 .. 2^-12, runs of zero bins and a silent frame, incoming gradient
    (rows, 130, T)), float32."""
    spec = np.abs(signals.gained_with_silence((rows, n_frames, n_freqs), seed, max(1, n_freqs // 8), 1))
    g = signals.uniform((rows, max(FB_MELS), n_frames), seed=seed + 1)
    return np.ascontiguousarray(np.swapaxes(spec, -1, -2)), g


def fb_probe_indices(k, rng):
    picks = [0, 31, 32, k - 33, k - 1, int(rng.integers(0, k))]
    return sorted(set(i for i in picks if 0 <= i < k))


def fb_body(tac, device, k, n_freqs, test='filterbank_grad'):
    """Every row mode, n_mels and layout at one (K, n_freqs).  Returns {n_mels: (worst kernel measure, worst float32-CPU measure)}."""
    gpu = on_gpu(device)
    rng = np.random.default_rng(4200 + k + 7919 * SEED)
    worst = {}
    for rows, n_frames in fb_row_modes(k):
        spec_np, g_np = fb_inputs(k, rows, n_frames, n_freqs, 4300 + k + n_freqs)
        s64, g64 = torch.from_numpy(spec_np).double(), torch.from_numpy(g_np).double()
        ref = torch.einsum('rft,rmt->fm', s64, g64)
        abs_sum = torch.einsum('rft,rmt->fm', s64.abs(), g64.abs())
        cpu32 = torch.einsum('rft,rmt->fm', torch.from_numpy(spec_np), torch.from_numpy(g_np))
        probes = fb_probe_indices(k, rng)
        g_dev = to(device, g_np)
        layouts = (('bin-major', to(device, spec_np)),
                   ('frame-major', to(device, np.swapaxes(spec_np, -1, -2)).transpose(-1, -2)))
        for n_mels in FB_MELS:
            bank = to(device, signals.uniform((n_freqs, n_mels), seed=4400 + n_mels)).requires_grad_(True)
            for name, spec in layouts:
                tag = (k, rows, n_frames, n_freqs, n_mels, name)
                y = tac.apply_filterbank(spec, bank)
                before = dict(tac._hip.launches) if gpu else None
                (got,) = torch.autograd.grad(y, bank, g_dev[:, :n_mels], retain_graph=True)
                if gpu:
                    assert launched_since(tac, before) == {'tac_apply_filterbank_f32': 1}, tag
                assert tuple(got.shape) == (n_freqs, n_mels), tag
                m = check_acc(got, ref[:, :n_mels], abs_sum[:, :n_mels], k, test, tag, cpu32=cpu32[:, :n_mels])
                c = acc_measure(cpu32[:, :n_mels], ref[:, :n_mels], abs_sum[:, :n_mels])
                worst[n_mels] = (max(m, worst.get(n_mels, (0, 0))[0]), max(c, worst.get(n_mels, (0, 0))[1]))
                # one-hot: one frame of the incoming gradient; the result is the outer product of two float32 vectors
                hot = torch.zeros_like(g_dev[:, :n_mels])
                for ki in probes:
                    r, t = divmod(ki, n_frames)
                    hot[r, :, t] = g_dev[r, :n_mels, t]
                    (one,) = torch.autograd.grad(y, bank, hot, retain_graph=True)
                    hot[r, :, t] = 0.0
                    want = torch.outer(s64[r, :, t], g64[r, :n_mels, t])
                    d = (one.detach().cpu().double() - want).abs()
                    ok = d <= 2.0 ** -23 * want.abs()
                    assert bool(ok.all()), '%s %r: the one-hot frame at K index %d is not the outer product (%d elements, worst %.3e relative)' % (
                        test, tag, ki, int((~ok).sum()), float((d / want.abs().clamp(min=1e-300))[~ok].max()))
                    assert ki == 1 or float(want.abs().max()) > 0, (tag, ki)
    return worst


def fb_fused_mel_body(tac, device, test='filterbank_grad_fused_mel'):
    """The fused ``melspectrogram`` op with a learnable bank at fft_length 512: ``filterbank_grad`` on a recomputed spectrogram,
    held to the 1e-4 of test_general_gradient_routes_under_strict against a float64 einsum."""
    n_fft, hop, mels = 512, 128, 23
    x_np = signals.gained_with_silence((3, 2, 40 * hop + 77), 4500, n_fft, hop)
    mel = tac.Melspectrogram(num_mels=mels, sample_rate=16000, fft_length=n_fft, hop_length=hop).to(device)
    mel[2].filterbank.requires_grad_(True)
    g_np = signals.uniform((3, 2, mels, frames_of_length(x_np.shape[-1], n_fft, hop, True)), seed=4501)
    before = dict(tac._hip.launches)
    (got,) = torch.autograd.grad(tac.realize(mel(to(device, x_np))), mel[2].filterbank, to(device, g_np))
    if on_gpu(device):
        ran = launched_since(tac, before)
        assert ran.get('tac_apply_filterbank_f32') == 1 and 'tac_window_grad_f32' not in ran, ran
    p64 = fbnd.ref64(x_np, n_fft, hop, mel[0].window, 2.0)
    want = torch.einsum('abft,abmt->fm', p64, torch.from_numpy(g_np).double())
    err = rel_err(host(got), want.numpy())
    fbnd.report(test, 'fft512', n_fft, 'fb_grad', err, 1e-4)
    assert err < 1e-4, err


def fb_stretch_mel_body(tac, device, test='filterbank_grad_stretch_mel'):
    """``stretch_mel`` with a learnable bank: ``filterbank_grad`` on the recomputed stretched rows, to the 2e-5 of
    tests/test_stretch_gpu.py::test_gradients against a float64 einsum."""
    rng = np.random.default_rng(4600)
    mag_np = (np.abs(rng.standard_normal((3, 2, 129, 61))) + 0.05).astype(np.float32)
    bank_np = np.abs(rng.standard_normal((129, 23))).astype(np.float32)
    rows64 = interpolated(torch.from_numpy(mag_np).double(), 1.3, 2.0)
    g_np = rng.standard_normal((3, 2, 23, rows64.shape[-1])).astype(np.float32)
    want = torch.einsum('abft,abmt->fm', rows64, torch.from_numpy(g_np).double())
    bank = to(device, bank_np).requires_grad_(True)
    out = torch.ops.tac_amd.stretch_mel(to(device, mag_np), bank, 1.3, 2.0, False, 1.0, 1e-7)
    before = dict(tac._hip.launches)                                   # (a dense bank: the forward ran the GEMM as well)
    (got,) = torch.autograd.grad(out, bank, to(device, g_np))
    if on_gpu(device):
        ran = launched_since(tac, before)
        assert ran.get('tac_apply_filterbank_f32') == 1 and ran.get('tac_stretch_norm_f32') == 1, ran
    err = float(fbnd.row_errors(got.cpu().reshape(1, -1), want.reshape(1, -1)).max())
    fbnd.report(test, 'rate1.3', 129, 'fb_grad', err, 2e-5)
    assert err <= 2e-5, err


# ----------------------------------------------------------------------------- 4. hpss gradient
HPSS_WIDTHS = (1, 3, 5, 11, 31, 33, 63)


def hpss_unequal(mag, kernel_f, kernel_t, power, hard=False):
    """``hpss`` with unequal widths, the documented behaviour restated with torch ops: the percussive median over ``kernel_f``
    bins, the harmonic one over ``kernel_t`` frames of the reflect-padded spectrogram (*, F, T); differentiable."""
    shape = mag.shape
    x = mag.reshape((-1, 1) + tuple(shape[-2:]))
    pf = torch.nn.functional.pad(x, (0, 0, kernel_f // 2, kernel_f // 2), mode='reflect')
    pt = torch.nn.functional.pad(x, (kernel_t // 2, kernel_t // 2, 0, 0), mode='reflect')
    perc = pf.unfold(2, kernel_f, 1).median(dim=-1)[0]
    harm = pt.unfold(3, kernel_t, 1).median(dim=-1)[0]
    if power != 1.0:
        perc, harm = perc.pow(power), harm.pow(power)
    if hard:
        mh, mp = harm > perc, harm < perc
    else:
        mh, mp = (harm + 1e-6) / (harm + perc + 1e-6), (perc + 1e-6) / (harm + perc + 1e-6)
    return tuple(o.reshape(shape) for o in (x * mh, x * mp, mh, mp))


def hpss_plane(rng, rows, n_freqs, n_frames, first_gain):
    """float32 (rows, F, T) with no two equal values in a row: a permutation of 1 .. F T times 2^-15, times the row's gain
    2^-(first_gain + 5 r mod 13) — all exact in float32."""
    n = n_freqs * n_frames
    out = np.empty((rows, n_freqs, n_frames), dtype=np.float32)
    for r in range(rows):
        gain = np.float32(2.0 ** -((first_gain + 5 * r) % 13))
        out[r] = ((rng.permutation(n) + 1).astype(np.float32) * np.float32(2.0 ** -15) * gain).reshape(n_freqs, n_frames)
    return out


def hpss_cases(n_cases=None):
    """About two dozen drawn cases (scaled by TAC_FUZZ_CASES): rows 1 .. 3, F / T in 8 .. 150, widths from HPSS_WIDTHS equal and
    unequal, clipped so that width // 2 < n, every fourth case exactly at width // 2 == n - 1 along one axis; both layouts,
    powers, soft / hard masks, a random non-empty subset of the outputs given a gradient, the masks-only op."""
    n_cases = max(8, (3 * CASES) // 4) if n_cases is None else n_cases
    rng = np.random.default_rng(11000 + SEED)
    out = []
    for case in range(n_cases):
        rows = int(rng.integers(1, 4))
        n_freqs, n_frames = int(rng.integers(8, 151)), int(rng.integers(8, 151))
        if rng.random() < 0.5:
            kf = kt = int(rng.choice(HPSS_WIDTHS))
        else:
            kf, kt = int(rng.choice(HPSS_WIDTHS)), int(rng.choice(HPSS_WIDTHS))
        if case % 4 == 1:                                          # every window along that axis reflects
            kf = int(rng.choice([5, 11, 31, 33, 63]))
            n_freqs = kf // 2 + 1
        elif case % 4 == 3:
            kt = int(rng.choice([5, 11, 31, 33, 63]))
            n_frames = kt // 2 + 1
        while kf // 2 >= n_freqs:
            kf = HPSS_WIDTHS[HPSS_WIDTHS.index(kf) - 1]
        while kt // 2 >= n_frames:
            kt = HPSS_WIDTHS[HPSS_WIDTHS.index(kt) - 1]
        hard = bool(rng.random() < 0.25)
        mask_only = bool(not hard and rng.random() < 0.25)
        pool = (2, 3) if mask_only else ((0, 1) if hard else (0, 1, 2, 3))
        keep = [i for i in pool if rng.random() < 0.5] or [int(rng.choice(pool))]
        out.append(dict(case=case, rows=rows, n_freqs=n_freqs, n_frames=n_frames, kf=kf, kt=kt, hard=hard, mask_only=mask_only,
                        outputs=tuple(keep), frame_major=bool(rng.random() < 0.5), power=float(rng.choice([1.0, 2.0, 0.7])),
                        first_gain=int(rng.integers(0, 13)), seed=int(rng.integers(1 << 30)),
                        silent_grad=bool(rows >= 2 and rng.random() < 0.5)))
    return out


def hpss_case_body(tac, device, c, test='hpss_grad'):
    rng = np.random.default_rng(c['seed'])
    rows, n_freqs, n_frames, kf, kt = c['rows'], c['n_freqs'], c['n_frames'], c['kf'], c['kt']
    s = hpss_plane(rng, rows, n_freqs, n_frames, c['first_gain'])
    tag = tuple(sorted((k, v) for k, v in c.items() if k != 'seed'))
    g_np = {i: rng.standard_normal(s.shape).astype(np.float32) for i in c['outputs']}
    silent = ()
    if c['silent_grad']:
        silent = (rows - 1,)
        for g in g_np.values():
            g[rows - 1] = 0.0
    mr = torch.from_numpy(s).double().requires_grad_(True)
    if kf == kt:
        outs_r = tuple(o[:, 0] for o in torch_ref.hpss(mr[:, None], kf, c['power'], c['hard']))
    else:
        outs_r = hpss_unequal(mr, kf, kt, c['power'], c['hard'])
    (want,) = torch.autograd.grad([outs_r[i] for i in c['outputs']], mr, [torch.from_numpy(g_np[i]).double() for i in c['outputs']])
    m = (to(device, s.transpose(0, 2, 1)).transpose(1, 2) if c['frame_major'] else to(device, s)).requires_grad_(True)
    before = dict(tac._hip.launches)
    outs = tac.hpss(m, kf if kf == kt else (kf, kt), c['power'], c['hard'], mask_only=c['mask_only'])
    (got,) = torch.autograd.grad([outs[i] for i in c['outputs']], m, [to(device, g_np[i]) for i in c['outputs']])
    if on_gpu(device):
        assert launched_since(tac, before).get('tac_hpss_backward_f32') == 1, tag
    assert tuple(got.shape) == s.shape, tag
    return fbnd.check_rows(got.detach().cpu().reshape(rows, -1), want.reshape(rows, -1), 1e-4, test, tag, 0, kind='hpss_grad',
                           silent_rows=silent)


# ----------------------------------------------------------------------------- 5. phase_vocoder and stretch gradients
PV_RATES = (0.5, 0.7, 0.9, 1.1, 1.3, 1.5, 2.0, 2.7)
PV_STEP = 1e-7              # the kernel's documented rounding of the running phase: 1e-7 rad per step (csrc/phase_vocoder.hip)


def pv_cases(n_cases=None):
    """The forward fuzz's ranges: lead dims 1 .. 3 by 1 .. 3, F 3 .. 200, T 2 .. 120 (exactly 2 and 3 in some cases), its rates
    plus 1.0, an integer rate and a rate above T (one output frame), both layouts; the first case has 606 series of 101 bins
    (no multiple of the 256-thread workgroup, which therefore straddles rows at offsets that differ from row to row)."""
    n_cases = max(8, (3 * CASES) // 4) if n_cases is None else n_cases
    rng = np.random.default_rng(12000 + SEED)
    out = []
    for case in range(n_cases):
        lead = (int(rng.integers(1, 4)), int(rng.integers(1, 4)))
        n_freqs, n_frames = int(rng.integers(3, 201)), int(rng.integers(2, 121))
        if case == 0:
            lead, n_freqs = (3, 2), 101
        if case % 6 == 2:
            n_frames = 2
        elif case % 6 == 4:
            n_frames = 3
        kind = case % 5
        if kind == 1:
            rate = 1.0
        elif kind == 2:
            rate = float(rng.choice([2.0, 3.0]))
        elif kind == 3 and case % 2:
            rate = float(n_frames) + 0.5
        else:
            rate = float(rng.choice(PV_RATES)) if rng.random() < 0.7 else float(rng.uniform(0.3, 3.0))
        out.append(dict(case=case, lead=lead, n_freqs=n_freqs, n_frames=n_frames, rate=rate, frame_major=bool(rng.random() < 0.5),
                        advance=float([0.0, math.pi * 16, math.pi * 128, rng.uniform(0, 2000.0)][int(rng.integers(0, 4))]), seed=int(rng.integers(1 << 30))))
    return out


def pv_input(c):
    """(lead, F, T, 2) float32: magnitudes uniform in [0.5, 2], phases uniform — the 1 / |z| of the gradient is bounded."""
    rng = np.random.default_rng(c['seed'])
    shape = c['lead'] + (c['n_freqs'], c['n_frames'])
    mag, ph = rng.uniform(0.5, 2.0, shape), rng.uniform(-math.pi, math.pi, shape)
    return np.stack([mag * np.cos(ph), mag * np.sin(ph)], -1).astype(np.float32), rng


def pv_reference(z_np, rate, adv_np, g_np, dtype):
    z = torch.from_numpy(z_np).to(dtype).requires_grad_(True)
    adv = torch.from_numpy(adv_np).to(dtype).requires_grad_(True)
    return torch.autograd.grad(torch_ref.phase_vocoder(z, rate, adv), [z, adv], torch.from_numpy(g_np).to(dtype))


def pv_bound(n_out, class_err):
    """Per source frame: 4 x the worst per-frame error of the float32 CPU autograd of the oracle against its float64 run on the
    same inputs (``class_err``: the accuracy class, never the kernel), not below the kernel's documented rounding of the running
    phase summed over the series.  The float32 oracle accumulates the UNWRAPPED phase, so its error grows with phase_advance x
    n_out (1e-2 at an advance of 2000 rad over 400 steps); the cases with a small advance are the tight ones."""
    return max(4.0 * class_err, PV_STEP * n_out)


def pv_case_body(tac, device, c, test='phase_vocoder_grad'):
    """Returns (worst per-frame error of the route under test, of the float32 CPU autograd of the oracle)."""
    z_np, rng = pv_input(c)
    n_freqs, n_frames, rate = c['n_freqs'], c['n_frames'], c['rate']
    adv_np = (c['advance'] * np.linspace(0, 1, n_freqs)).astype(np.float32)[:, None]
    n_out = len(grid(n_frames, rate)[0])
    g_np = rng.standard_normal(c['lead'] + (n_freqs, n_out, 2)).astype(np.float32)
    want, want_adv = pv_reference(z_np, rate, adv_np, g_np, torch.float64)
    assert float(want_adv.abs().max()) < 1e-9 * max(1.0, float(want.abs().max()))
    cpu32, _ = pv_reference(z_np, rate, adv_np, g_np, torch.float32)
    z = (to(device, np.swapaxes(z_np, -3, -2)).transpose(-3, -2) if c['frame_major'] else to(device, z_np)).requires_grad_(True)
    adv = to(device, adv_np).requires_grad_(True)
    tag = tuple(sorted((k, v) for k, v in c.items() if k != 'seed'))
    before = dict(tac._hip.launches)
    out = tac.phase_vocoder(z, rate, adv)
    assert tuple(out.shape) == g_np.shape, (tag, out.shape)
    got, got_adv = torch.autograd.grad(out, [z, adv], to(device, g_np))
    if on_gpu(device):
        assert launched_since(tac, before).get('tac_phase_vocoder_backward_f32') == 1, tag
        assert float(got_adv.abs().max()) == 0.0, tag
    else:
        assert float(got_adv.abs().max()) <= 1e-5 * float(want.abs().max()), tag   # (autograd through round(): zero up to the sums' rounding)
    class_err = float(fbnd.linear_frame_errors(fbnd.as_frames(cpu32, 'complex'), fbnd.as_frames(want, 'complex')).max())
    fbnd.report(test, tag, n_freqs, 'pv_grad_cpu32', class_err, pv_bound(n_out, class_err))
    worst = fbnd.check_frames(got, want, 'complex', pv_bound(n_out, class_err), test, tag, n_freqs)
    return worst, class_err


def pv_gaussian_body(tac, device):
    """The input of test_phase_vocoder_gradient_kernel (Gaussian components: bins near zero, where 1 / |z| amplifies float32
    rounding) under its 2e-4 of the tensor maximum."""
    rng = np.random.default_rng(91)
    z_np = rng.standard_normal((2, 3, 65, 47, 2)).astype(np.float32)
    adv_np = np.linspace(0, np.pi * 32, 65, dtype=np.float32)[:, None]
    for rate in (0.6, 1.3):
        n_out = len(grid(47, rate)[0])
        g_np = rng.standard_normal((2, 3, 65, n_out, 2)).astype(np.float32)
        want, _ = pv_reference(z_np, rate, adv_np, g_np, torch.float64)
        z = to(device, z_np).requires_grad_(True)
        (got,) = torch.autograd.grad(tac.phase_vocoder(z, rate, to(device, adv_np)), z, to(device, g_np))
        assert rel_err(host(got), want.numpy()) < 2e-4, rate


STRETCH_RATES = (0.6, 1.0, 1.3, 2.5)


def stretch_cases(n_cases=None):
    n_cases = max(8, (3 * CASES) // 4) if n_cases is None else n_cases
    rng = np.random.default_rng(13000 + SEED)
    out = []
    for case in range(n_cases):
        lead = (int(rng.integers(1, 4)), int(rng.integers(1, 4)))
        n_freqs, n_frames = int(rng.integers(3, 201)), int(rng.integers(2, 121))
        if case % 6 == 2:
            n_frames = 2
        elif case % 6 == 4:
            n_frames = 3
        rate = STRETCH_RATES[case % 5] if case % 5 < 4 else float(rng.uniform(0.3, 3.0))
        out.append(dict(case=case, lead=lead, n_freqs=n_freqs, n_frames=n_frames, rate=rate, power=(1.0, 2.0, 0.7)[case % 3],
                        db=bool(rng.random() < 0.5), mel=bool(case % 2), bank_grad=bool(rng.random() < 0.6),
                        n_mels=int(rng.choice([1, 12, 40])), frame_major=bool(rng.random() < 0.5), seed=int(rng.integers(1 << 30))))
    return out


def stretch_case_body(tac, device, c, test='stretch_grad'):
    rng = np.random.default_rng(c['seed'])
    shape = c['lead'] + (c['n_freqs'], c['n_frames'])
    n_rows = c['lead'][0] * c['lead'][1]
    mag_np = (np.abs(rng.standard_normal(shape)) + 0.05).astype(np.float32)
    bank_np = (np.abs(rng.standard_normal((c['n_freqs'], c['n_mels']))) + 0.01).astype(np.float32)
    rate, power, db = c['rate'], c['power'], c['db']
    tag = tuple(sorted((k, v) for k, v in c.items() if k != 'seed'))
    mr = torch.from_numpy(mag_np).double().requires_grad_(True)
    br = torch.from_numpy(bank_np).double().requires_grad_(c['bank_grad'])
    outr = interpolated(mr, rate, power)
    if c['mel']:
        outr = torch_ref.apply_filterbank(outr, br)
    if db:
        outr = torch_ref.amplitude_to_db(outr, 1.0, 1e-7)
    g_np = rng.standard_normal(tuple(outr.shape)).astype(np.float32)
    m = (to(device, np.swapaxes(mag_np, -1, -2)).transpose(-1, -2) if c['frame_major'] else to(device, mag_np)).requires_grad_(True)
    b = to(device, bank_np).requires_grad_(c['bank_grad'])
    ins_r, ins = ([mr, br], [m, b]) if (c['mel'] and c['bank_grad']) else ([mr], [m])
    want = torch.autograd.grad(outr, ins_r, torch.from_numpy(g_np).double())
    before = dict(tac._hip.launches)
    if c['mel']:
        out = torch.ops.tac_amd.stretch_mel(m, b, rate, power, db, 1.0, 1e-7)
    else:
        out = torch.ops.tac_amd.stretch_norm(m, rate, power, db, 1.0, 1e-7)
    got = torch.autograd.grad(out, ins, to(device, g_np))
    if on_gpu(device):
        ran = launched_since(tac, before)
        assert ran.get('tac_stretch_norm_backward_f32') == 1, (tag, ran)
        assert len(ins) == 1 or ran.get('tac_apply_filterbank_f32', 0) >= 1, (tag, ran)
    worst = fbnd.check_rows(got[0].detach().cpu().reshape(n_rows, -1), want[0].reshape(n_rows, -1), 2e-5, test, tag, c['n_freqs'],
                            kind='stretch_grad')
    if len(ins) == 2:
        worst = max(worst, fbnd.check_rows(got[1].detach().cpu().reshape(1, -1), want[1].reshape(1, -1), 2e-5, test, tag, c['n_freqs'],
                                           kind='stretch_bank_grad'))
    return worst
