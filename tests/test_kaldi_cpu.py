"""``kaldi_fbank`` / ``KaldiFbank`` / ``kaldi.fbank`` without a device: the CPU route (torch operators) under the rule of
tests/kaldi_rules.py for every option, frame counts and the empty result, the windows, the bank, the torchaudio-shaped wrapper,
argument errors, tracing, and the C ABI surface.  The signals of the GPU tests (tests/test_kaldi_gpu.py) are checked here for the
condition their log rule needs: at least 99 % of the elements above the floor held."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import kaldi_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OPTIONS = R.GEOMETRIES + R.OPTIONS
ident = R.ident
waveform = R.waveform


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


# ----------------------------------------------------------------------------- the CPU route under the rule
@pytest.mark.parametrize('kw', OPTIONS, ids=ident)
def test_cpu_float32_within_the_rule(tac, kw):
    o = R.options(**kw)
    w, s, n = R.sizes(o)
    x = waveform(3, w + 5 * s + 7, seed=len(ident(kw)), kw=kw)
    got = tac.kaldi_fbank(torch.from_numpy(x), **kw)
    r = R.reference(x, o)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 6 if o['snip_edges'] else R.num_frames(x.shape[1], w, s, False), r.cols)
    print('cpu %s: %r' % (ident(kw), R.check(got.numpy(), r, o, 'cpu ' + ident(kw))))


def test_cpu_subtract_mean_and_float64(tac):
    x = waveform(2, 400 + 160 * 7, seed=5)
    plain = tac.kaldi_fbank(torch.from_numpy(x), use_energy=True)
    sub = tac.kaldi_fbank(torch.from_numpy(x), use_energy=True, subtract_mean=True)
    R.check_subtracted(sub.numpy(), plain.numpy(), 'cpu')
    o = R.options(use_energy=True, subtract_mean=True, num_mel_bins=40)
    got = tac.kaldi_fbank(torch.from_numpy(x).double(), use_energy=True, subtract_mean=True, num_mel_bins=40)
    assert got.dtype == torch.float64
    assert np.abs(got.numpy() - R.reference(x, o).out).max() < 1e-9


def test_special_frames_on_the_cpu(tac):
    """an all-zero frame gives log(eps) in every bin and in the energy; so does a frame at 1e-30 scale"""
    x = waveform(1, 400 + 160 * 6, seed=9)
    x[0, 160:560] = 0.0
    x[0, 800:1200] *= np.float32(1e-30)
    got = tac.kaldi_fbank(torch.from_numpy(x), use_energy=True, energy_floor=0.0).numpy()
    assert (got[0, 1] == R.LOG_EPS32).all() and (got[0, 5] == R.LOG_EPS32).all()
    o = R.options(use_energy=True, energy_floor=0.0)
    R.check(got, R.reference(x, o), o, 'cpu special frames')


# ----------------------------------------------------------------------------- frame counts
def test_frame_counts_and_the_empty_result(tac):
    w, s = 400, 160
    for length, frames in ((w - 1, 0), (w, 1), (w + s - 1, 1), (w + s, 2), (0, 0)):
        got = tac.kaldi_fbank(torch.randn(2, 3, length), num_mel_bins=40, use_energy=True)
        assert tuple(got.shape) == (2, 3, frames, 41), (length, got.shape)
        assert R.num_frames(length, w, s, True) == frames == tac._kaldi.num_frames(length, w, s, True)
    for length in (1, 79, 80, 239, 240, 400, 1000, 1681):
        frames = (length + s // 2) // s
        assert tac._kaldi.num_frames(length, w, s, False) == R.num_frames(length, w, s, False) == frames
    assert tuple(tac.kaldi_fbank(torch.randn(2, 1000), snip_edges=False).shape) == (2, 6, 23)
    assert tuple(tac.kaldi_fbank(torch.zeros(0, 1000)).shape) == (0, 4, 23)


def test_mirrored_indices_at_both_ends(tac):
    w, s, length = 400, 160, 1000
    m = tac._kaldi.num_frames(length, w, s, False)
    idx = tac._kaldi.mirror_index(length, w, s, m)
    assert tuple(idx.shape) == (m, w)
    pad = w // 2 - s // 2
    assert idx[0, :pad].tolist() == list(range(pad - 1, -1, -1)) and idx[0, pad:].tolist() == list(range(w - pad))
    last = [R.frame_indices(length, w, s, m - 1, False)]
    assert idx[m - 1].tolist() == last[0] and max(last[0]) == length - 1 and last[0][-1] == 2 * length - 1 - ((m - 1) * s - pad + w - 1)
    for t in range(m):
        assert idx[t].tolist() == R.frame_indices(length, w, s, t, False)
    x = torch.arange(length, dtype=torch.float64)[None]
    got = tac.kaldi_fbank(x, snip_edges=False, num_mel_bins=8)
    assert np.abs(got.numpy() - R.reference(x.numpy(), R.options(snip_edges=False, num_mel_bins=8)).out).max() < 1e-8
    with pytest.raises(ValueError):
        tac.kaldi_fbank(torch.randn(1, 100), snip_edges=False)            # one mirror does not reach: the definition ends there


# ----------------------------------------------------------------------------- windows and bank
@pytest.mark.parametrize('w', (200, 400, 551))
def test_windows(tac, w):
    K = tac._kaldi
    hann = K.window64('hanning', w)
    for kind in K.WINDOWS:
        win = K.window64(kind, w, 0.42)
        assert win.dtype == torch.float64 and tuple(win.shape) == (w,)
        assert torch.allclose(win, win.flip(0), rtol=0, atol=1e-14), kind
        assert np.abs(win.numpy() - R.window64(kind, w, 0.42)).max() < 1e-14
    assert abs(float(hann[0])) < 1e-15 and abs(float(hann[-1])) < 1e-15
    assert abs(float(K.window64('hamming', w)[0]) - 0.08) < 1e-15
    for a in (0.42, 0.3):                                       # a - 0.5 + (0.5 - a) at the ends, a + 0.5 cos(pi/2) - (0.5 - a) a quarter in
        black = K.window64('blackman', 4 * (w // 4) + 1, a)
        assert abs(float(black[0])) < 1e-15 and abs(float(black[-1])) < 1e-15 and abs(float(black[w // 4]) - (2.0 * a - 0.5)) < 1e-14
    assert bool((K.window64('rectangular', w) == 1).all())
    assert torch.allclose(K.window64('povey', w), hann.pow(0.85), rtol=0, atol=1e-15)
    assert abs(float(hann[(w - 1) // 2]) - 1.0) < 1e-4


@pytest.mark.parametrize('rate,bins', [(16000.0, 23), (16000.0, 40), (16000.0, 80), (16000.0, 128), (8000.0, 23), (8000.0, 40)])
def test_bank_properties(tac, rate, bins):
    K = tac._kaldi
    w, s, n = K.sizes(rate, 25.0, 10.0, True)
    bank = K.mel_bank64(bins, n, rate, 20.0, 0.0)
    assert tuple(bank.shape) == (bins, n // 2 + 1) and bank.dtype == torch.float64
    assert np.abs(bank.numpy() - R.bank64(bins, n, rate, 20.0, 0.0)).max() < 1e-12
    assert bool((bank[:, -1] == 0).all())                       # the Nyquist column
    # every band is non-zero — except, at 128 bins, band 3: it spans 62.96 .. 93.01 Hz, between the bins at 62.5 and 93.75 Hz, and
    # holds no FFT bin.  By the definition a band is empty exactly when no bin lies strictly inside it; that is asserted per band
    inside = [any(R.mel(20.0) + b * delta < R.mel(k * rate / n) < R.mel(20.0) + (b + 2) * delta for k in range(n // 2))
              for b in range(bins) for delta in [(R.mel(rate / 2) - R.mel(20.0)) / (bins + 1)]]
    assert (bank.sum(1) > 0).tolist() == inside
    assert [b for b in range(bins) if not inside[b]] == ([3] if bins == 128 else [])
    assert float(bank.max()) <= 1.0 and float(bank.min()) >= 0.0
    for b in range(bins):                                       # one interval per band
        nz = torch.nonzero(bank[b]).reshape(-1)
        assert nz.numel() == 0 or int(nz[-1]) - int(nz[0]) + 1 == nz.numel()
    weights, table = K.packed_runs(bank.to(torch.float32))
    assert tuple(table.shape) == (3, bins) and table.dtype == torch.int32 and weights.dtype == torch.float32
    rebuilt = torch.zeros(bins, n // 2 + 1)
    for b in range(bins):
        lo, cnt, off = (int(v) for v in table[:, b])
        assert (cnt > 0) == inside[b] and lo + cnt <= n // 2 and off + cnt <= weights.numel()
        rebuilt[b, lo:lo + cnt] = weights[off:off + cnt]
    assert torch.equal(rebuilt, bank.to(torch.float32)) and weights.numel() <= n


# ----------------------------------------------------------------------------- kaldi.fbank
def test_wrapper_has_torchaudio_signature(tac):
    sig = inspect.signature(tac.kaldi.fbank)
    want = dict(blackman_coeff=0.42, channel=-1, dither=0.0, energy_floor=1.0, frame_length=25.0, frame_shift=10.0, high_freq=0.0,
                htk_compat=False, low_freq=20.0, min_duration=0.0, num_mel_bins=23, preemphasis_coefficient=0.97, raw_energy=True,
                remove_dc_offset=True, round_to_power_of_two=True, sample_frequency=16000.0, snip_edges=True, subtract_mean=False,
                use_energy=False, use_log_fbank=True, use_power=True, vtln_high=-500.0, vtln_low=100.0, vtln_warp=1.0,
                window_type='povey')
    names = list(sig.parameters)
    assert names[0] == 'waveform' and names[1:] == list(want)
    assert {k: sig.parameters[k].default for k in want} == want


def test_wrapper_channel_min_duration_and_column_order(tac):
    x = torch.from_numpy(waveform(3, 400 + 160 * 4, seed=2))
    rows = [tac.kaldi_fbank(x[c], num_mel_bins=40) for c in range(3)]
    assert tuple(rows[0].shape) == (5, 40) and not torch.equal(rows[0], rows[2])
    assert torch.equal(tac.kaldi.fbank(x, num_mel_bins=40), rows[0])                  # channel -1 -> 0
    assert torch.equal(tac.kaldi.fbank(x, num_mel_bins=40, channel=0), rows[0])
    assert torch.equal(tac.kaldi.fbank(x, num_mel_bins=40, channel=2), rows[2])
    dur = x.shape[1] / 16000.0
    assert tuple(tac.kaldi.fbank(x, num_mel_bins=40, min_duration=dur + 1e-3).shape) == (0, 40)
    assert tuple(tac.kaldi.fbank(x, num_mel_bins=40, min_duration=dur).shape) == (5, 40)
    assert tuple(tac.kaldi.fbank(x[:, :399], use_energy=True).shape) == (0, 24)
    first = tac.kaldi.fbank(x, use_energy=True)
    last = tac.kaldi.fbank(x, use_energy=True, htk_compat=True)
    assert tuple(first.shape) == tuple(last.shape) == (5, 24)
    assert torch.equal(first[:, 0], last[:, -1]) and torch.equal(first[:, 1:], last[:, :-1])
    assert torch.equal(first[:, 1:], tac.kaldi.fbank(x))
    with pytest.raises(ValueError):
        tac.kaldi.fbank(x[0])


# ----------------------------------------------------------------------------- errors
def test_argument_errors(tac):
    x = torch.randn(2, 2000)
    for kw in (dict(num_mel_bins=3), dict(num_mel_bins=0), dict(window_type='hann'), dict(window_type='kaiser'),
               dict(frame_length=0.1), dict(frame_shift=0.05), dict(low_freq=-1.0), dict(low_freq=9000.0),
               dict(high_freq=8001.0), dict(low_freq=4000.0, high_freq=3000.0), dict(high_freq=-7990.0), dict(low_freq=8000.0)):
        with pytest.raises(ValueError):
            tac.kaldi_fbank(x, **kw)
        with pytest.raises(ValueError):
            tac.KaldiFbank(**kw)
    with pytest.raises(NotImplementedError, match='vtln_warp'):
        tac.kaldi_fbank(x, vtln_warp=1.1)
    with pytest.raises(NotImplementedError, match='vtln_warp'):
        tac.kaldi.fbank(x, vtln_warp=0.9)
    with pytest.raises(TypeError):
        tac.kaldi_fbank([1.0, 2.0])
    with pytest.raises(TypeError):
        tac.KaldiFbank(channel=0)
    with pytest.raises(RuntimeError):
        tac.kaldi_fbank(torch.zeros(2, 2000, dtype=torch.int16))
    with pytest.raises(RuntimeError):
        tac.kaldi_fbank(torch.tensor(1.0))


# ----------------------------------------------------------------------------- routes on the CPU, tracing, the layer
def test_cpu_options_outside_the_kernel_and_dither(tac):
    """what the kernel does not cover is the same definition on the CPU: N = 2048, no rounding to a power of two, 200 bins"""
    x = waveform(2, 3000, seed=4)
    for kw in (dict(sample_frequency=48000.0), dict(round_to_power_of_two=False), dict(num_mel_bins=200)):
        o = R.options(**kw)
        got = tac.kaldi_fbank(torch.from_numpy(x).double(), **kw)
        assert np.abs(got.numpy() - R.reference(x, o).out).max() < 1e-8, kw
    torch.manual_seed(0)
    a = tac.kaldi_fbank(torch.from_numpy(x), dither=1.0)
    b = tac.kaldi_fbank(torch.from_numpy(x), dither=1.0)
    assert tuple(a.shape) == (2, 17, 23) and not torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_gradient_on_the_cpu(tac):
    x = torch.from_numpy(waveform(2, 200 + 80 * 2 + 3, seed=6)).double().requires_grad_(True)
    kw = dict(sample_frequency=8000.0, num_mel_bins=6, use_energy=True, energy_floor=0.0)
    assert torch.autograd.gradcheck(lambda t: tac.kaldi_fbank(t, **kw), (x,), atol=1e-6)
    g = np.random.default_rng(0).standard_normal((2, 3, 7))
    tac.kaldi_fbank(x, **kw).backward(torch.from_numpy(g))
    want = R.row_gradient(x.detach().numpy(), R.options(**kw), g)
    assert np.abs(x.grad.numpy() - want).max() <= 1e-9 * np.abs(want).max()


def test_fake_kernel_shape_under_compile(tac):
    seen = []

    def capture(gm, example_inputs):
        seen.extend(n.target for n in gm.graph.nodes if n.op == 'call_function')
        return gm.forward

    torch._dynamo.reset()
    layer = tac.KaldiFbank(num_mel_bins=80, use_energy=True)
    x = torch.randn(2, 3, 2000)
    out = torch.compile(layer, backend=capture, fullgraph=True)(x)
    names = [str(t) for t in seen]
    assert sum('tac_amd.kaldi_fbank' in n for n in names) == 1 and len(names) == 1, names
    eager = layer(x)
    assert torch.equal(out, eager)
    from torch._subclasses.fake_tensor import FakeTensorMode
    p = tac._kaldi.Params(**R.options(num_mel_bins=80, use_energy=True, snip_edges=False))
    with FakeTensorMode() as mode:
        fake = torch.ops.tac_amd.kaldi_fbank(mode.from_tensor(x), *p)
    assert tuple(fake.shape) == (2, 3, 13, 81) and fake.dtype == torch.float32 and fake.stride() == (3 * 13 * 81, 13 * 81, 81, 1)
    assert tuple(eager.shape) == (2, 3, 11, 81) and eager.is_contiguous()
    torch.library.opcheck(torch.ops.tac_amd.kaldi_fbank.default, (torch.randn(2, 1000),) + tuple(tac._kaldi.Params(**R.options())),
                          test_utils=('test_schema', 'test_faketensor'))


def test_layer_and_names(tac):
    m = tac.KaldiFbank(num_mel_bins=80, frame_shift=10.0)
    assert repr(m) == 'KaldiFbank(num_mel_bins=80, frame_shift=10.0)' and repr(tac.KaldiFbank()) == 'KaldiFbank()'
    assert m.state_dict() == {} and list(m.named_buffers()) == []
    x = torch.from_numpy(waveform(2, 2000, seed=8))
    assert torch.equal(m(x), tac.kaldi_fbank(x, num_mel_bins=80))
    chain = torch.nn.Sequential(tac.Resample(48000, 16000), tac.Preemphasis(), tac.KaldiFbank(num_mel_bins=40))
    assert tuple(chain(torch.randn(2, 6000)).shape) == (2, 11, 40)
    assert 'kaldi_fbank' in tac.functional.__all__ and tac.kaldi_fbank is tac.functional.kaldi_fbank
    assert tac.KaldiFbank is tac.layers.KaldiFbank and tac.kaldi.fbank.__module__ == 'torchaudio_contrib_amd.kaldi'
    assert 'kaldi_fbank' in tac._ops.cuda_kernels and hasattr(torch.ops.tac_amd, 'kaldi_fbank')


def test_entry_point_is_declared_and_exported(tac):
    header = open(os.path.join(ROOT, 'include', 'tac_amd.h')).read()
    assert re.search(r'\bint\s+tac_kaldi_fbank_f32\s*\(', header) and '(18)' in header
    assert 'tac_kaldi_fbank_f32' in tac._native.EXPORTS and 'tac_kaldi_num_frames' in tac._native.EXPORTS
    assert 'kaldi_fbank.hip' in open(os.path.join(ROOT, 'torchaudio-contrib_amd', 'csrc', 'Makefile')).read()
    if not os.path.exists(tac._native.LIB_PATH):
        tac.build_native()
    h = tac._native.lib()
    assert h.tac_abi_version() == 5
    for length in (0, 399, 400, 559, 560, 16000):
        for snip in (0, 1):
            assert h.tac_kaldi_num_frames(length, 400, 160, snip) == R.num_frames(length, 400, 160, bool(snip))
    for name, bit in tac._hip._KALDI_FLAGS.items():
        macro = {'snip_edges': 'SNIP_EDGES', 'remove_dc_offset': 'REMOVE_DC', 'raw_energy': 'RAW_ENERGY', 'use_energy': 'USE_ENERGY',
                 'htk_compat': 'HTK', 'use_log_fbank': 'LOG', 'use_power': 'POWER'}[name]
        assert re.search(r'#define TAC_KALDI_%s %d\b' % (macro, bit), header), name
    # argument checks of the launcher need no device: nothing is launched for these
    assert h.tac_kaldi_fbank_f32(None, 1, 1000, 1000, None, None, None, 512, 400, 160, 23, 100, 0, 0.97, 1.0, None, None) == tac._native.TAC_E_INVALID


def test_the_gpu_tests_signals_meet_the_mask_condition():
    """The 99 % condition of the log rule is a property of the signal and the bound, not of the code under test: established
    here, on the CPU, for the waveforms tests/test_kaldi_gpu.py builds (``kaldi_rules.waveform`` at 4 G + 1 frames, 3 rows) at
    every geometry and option."""
    for kw in OPTIONS:
        o = R.options(**kw)
        w, s, n = R.sizes(o)
        g = 64 // (n // 32)
        x = waveform(3, R.length_for(4 * g + 1, w, s, o['snip_edges']), seed=11, kw=kw)
        r = R.reference(x, o)
        assert r.value.shape[1] == 4 * g + 1
        above, held = r.value > R.EPS, (r.value - r.bound) > R.EPS
        assert held.sum() >= R.KEEP * above.sum(), (kw, held.sum(), above.sum())
