"""``kaldi_mfcc`` / ``kaldi_spectrogram`` (``KaldiMfcc`` / ``KaldiSpectrogram``, ``kaldi.mfcc`` / ``kaldi.spectrogram``) without a
device: the CPU route (torch operators) under the rules of tests/kaldi_mfcc_rules.py, the invariants of the definition on
float64 rows, the torchaudio-shaped wrappers, argument errors, tracing, and the C ABI surface.  The signals of the GPU tests
(tests/test_kaldi_mfcc_gpu.py) are checked here for the conditions their rules need: 99 % of the bins above the floor held and
the Nyquist bin held in half of the frames (spectrogram), 90 % of the frames with every band held or deep (MFCC)."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import kaldi_mfcc_rules as MR
import kaldi_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ident = R.ident


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


def signal(kw, rows=3, frames=13, seed=5):
    """the waveform of the GPU tests: ``rows`` x 13 frames off the frame grid (``kaldi_rules.waveform``, seed 5)"""
    o = R.options(**{k: v for k, v in kw.items() if k in R.DEFAULTS})
    w, s, n = R.sizes(o)
    return R.waveform(rows, R.length_for(frames, w, s, o['snip_edges']), seed=seed, kw=MR.waveform_kw(kw))


# ----------------------------------------------------------------------------- the CPU route under the rules
@pytest.mark.parametrize('kw', R.GEOMETRIES + MR.SPECTROGRAM_OPTIONS, ids=ident)
def test_cpu_spectrogram_within_the_rule(tac, kw):
    o = MR.spectrogram_options(**kw)
    x = signal(kw)
    ref = MR.spectrogram_reference(x, o)
    got = tac.kaldi_spectrogram(torch.from_numpy(x), **kw)
    n = R.sizes(R.options(**kw))[2]
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 13, n // 2 + 1) and got.is_contiguous()
    print('cpu spectrogram %s: %r' % (ident(kw), MR.check_spectrogram(got.numpy(), ref, o, 'cpu ' + ident(kw))))
    wide = tac.kaldi_spectrogram(torch.from_numpy(x).double(), **kw)
    assert wide.dtype == torch.float64 and np.abs(wide.numpy() - ref.out).max() < 1e-8


@pytest.mark.parametrize('kw', R.GEOMETRIES + MR.MFCC_OPTIONS, ids=ident)
def test_cpu_mfcc_within_the_rule(tac, kw):
    o = MR.mfcc_options(**kw)
    x = signal(kw)
    ref = MR.mfcc_reference(x, o)
    got = tac.kaldi_mfcc(torch.from_numpy(x), **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 13, o['num_ceps']) and got.is_contiguous()
    print('cpu mfcc %s: %r' % (ident(kw), MR.check_mfcc(got.numpy(), ref, o, 'cpu ' + ident(kw))))
    wide = tac.kaldi_mfcc(torch.from_numpy(x).double(), **kw)
    assert wide.dtype == torch.float64 and np.abs(wide.numpy() - ref.out).max() < 1e-8


def test_cpu_mfcc_80_bins_on_the_two_row_waveform(tac):
    """80 bins with 40 coefficients run on the two rows without the offset row, whose narrow low bands are the hardest to hold;
    every frame of these two rows is checked"""
    kw = MR.MFCC_TWO_ROWS
    o = MR.mfcc_options(**kw)
    x = signal(kw, rows=2)
    ref = MR.mfcc_reference(x, o)
    res = MR.check_mfcc(tac.kaldi_mfcc(torch.from_numpy(x), **kw).numpy(), ref, o, 'cpu 80 / 40')
    print('cpu mfcc 80 / 40: %r' % res)
    assert res['frames'] == 1.0


def test_cpu_subtract_mean(tac):
    x = torch.from_numpy(signal(dict(), rows=2, frames=9))
    for fn, kw in ((tac.kaldi_mfcc, dict(use_energy=True)), (tac.kaldi_spectrogram, dict())):
        R.check_subtracted(fn(x, subtract_mean=True, **kw).numpy(), fn(x, **kw).numpy(), 'cpu ' + fn.__name__)
    o = MR.mfcc_options(subtract_mean=True, htk_compat=True)
    got = tac.kaldi_mfcc(x.double(), subtract_mean=True, htk_compat=True)
    assert np.abs(got.numpy() - MR.mfcc_reference(x.numpy(), o).out).max() < 1e-9
    o = MR.spectrogram_options(subtract_mean=True)
    got = tac.kaldi_spectrogram(x.double(), subtract_mean=True)
    assert np.abs(got.numpy() - MR.spectrogram_reference(x.numpy(), o).out).max() < 1e-9


# ----------------------------------------------------------------------------- invariants of the definition, float64
@pytest.mark.parametrize('bins', (4, 23, 40, 128))
def test_dct_matrix_and_lifter(tac, bins):
    K = tac._kaldi
    d = K.dct64(bins, bins)
    assert d.dtype == torch.float64 and np.abs(d.numpy() - MR.dct64(bins, bins)).max() < 1e-14
    assert bool((d[:, 0] == math.sqrt(1.0 / bins)).all())
    assert np.abs((d.t() @ d).numpy() - np.eye(bins)).max() < 1e-13             # orthonormal
    assert torch.equal(K.dct64(bins, 3), d[:, :3])
    for q in (0.0, 22.0, 10.5):
        lift = K.lifter64(bins, q)
        assert float(lift[0]) == 1.0 and np.abs(lift.numpy() - MR.lifter64(bins, q)).max() < 1e-14
    assert bool((K.lifter64(bins, 0.0) == 1).all())


def test_transposed_matrix_returns_the_fbank_rows(tac):
    x = torch.from_numpy(signal(dict(), rows=2, frames=5)).double()
    logmel = tac.kaldi_fbank(x, num_mel_bins=23)
    ceps = tac.kaldi_mfcc(x, num_mel_bins=23, num_ceps=23, cepstral_lifter=0.0)
    back = ceps @ tac._kaldi.dct64(23, 23).t()
    assert float((back - logmel).abs().max()) <= 1e-12 * float(logmel.abs().max())


def test_constant_log_mel_row_gives_c0_only(tac):
    K = tac._kaldi
    for bins in (4, 23, 80):
        row = torch.full((bins,), -3.25, dtype=torch.float64)
        c = row @ K.dct64(bins, bins)
        assert abs(float(c[0]) - math.sqrt(bins) * -3.25) < 1e-12 and float(c[1:].abs().max()) < 1e-12


def test_energy_htk_order_and_sqrt_two(tac):
    x = torch.from_numpy(signal(dict(), rows=2, frames=5)).double()
    plain = tac.kaldi_mfcc(x)
    energy = tac.kaldi_fbank(x, use_energy=True)[..., 0]
    with_e = tac.kaldi_mfcc(x, use_energy=True)
    assert torch.equal(with_e[..., 0], energy) and torch.equal(with_e[..., 1:], plain[..., 1:])
    htk = tac.kaldi_mfcc(x, htk_compat=True)
    assert torch.equal(htk[..., :-1], plain[..., 1:])
    assert float((htk[..., -1] - math.sqrt(2.0) * plain[..., 0]).abs().max()) <= 1e-14 * float(plain[..., 0].abs().max())
    htk_e = tac.kaldi_mfcc(x, htk_compat=True, use_energy=True)
    assert torch.equal(htk_e[..., -1], energy) and torch.equal(htk_e[..., :-1], plain[..., 1:])       # no sqrt 2 on the energy
    unlifted = tac.kaldi_mfcc(x, cepstral_lifter=0.0)
    lift = tac._kaldi.lifter64(13, 22.0)
    assert float((plain - unlifted * lift).abs().max()) <= 1e-13 * float(plain.abs().max())
    spec = tac.kaldi_spectrogram(x)
    assert torch.equal(spec[..., 0], energy)
    assert torch.equal(tac.kaldi_spectrogram(x, raw_energy=False)[..., 0], tac.kaldi_fbank(x, use_energy=True, raw_energy=False)[..., 0])
    quiet = x * 1e-3                                            # frame energies below 1: the floor log 1 = 0 takes them
    assert float(tac.kaldi_spectrogram(quiet, energy_floor=0.0)[..., 0].max()) < 0.0
    assert bool((tac.kaldi_spectrogram(quiet)[..., 0] == 0.0).all()) and bool((tac.kaldi_mfcc(quiet, use_energy=True)[..., 0] == 0.0).all())


def test_spectrogram_bins_are_the_power_spectrum(tac):
    """every bin but the DC one, the Nyquist bin included, against numpy's transform of the definition's frame"""
    x = signal(dict(), rows=1, frames=2)
    got = tac.kaldi_spectrogram(torch.from_numpy(x).double()).numpy()
    win = R.window64('povey', 400)
    for t in range(2):
        f = x[0, 160 * t:160 * t + 400].astype(np.float64)
        f = f - f.mean()
        f = (f - 0.97 * np.concatenate([f[:1], f[:-1]])) * win
        power = np.abs(np.fft.rfft(f, 512)) ** 2
        assert power.shape == (257,) and np.abs(got[0, t, 1:] - np.log(np.maximum(power[1:], R.EPS))).max() < 1e-9


# ----------------------------------------------------------------------------- wrappers, shapes, errors
def test_wrappers_have_torchaudio_signatures(tac):
    want = dict(blackman_coeff=0.42, cepstral_lifter=22.0, channel=-1, dither=0.0, energy_floor=1.0, frame_length=25.0,
                frame_shift=10.0, high_freq=0.0, htk_compat=False, low_freq=20.0, num_ceps=13, min_duration=0.0, num_mel_bins=23,
                preemphasis_coefficient=0.97, raw_energy=True, remove_dc_offset=True, round_to_power_of_two=True,
                sample_frequency=16000.0, snip_edges=True, subtract_mean=False, use_energy=False, vtln_high=-500.0, vtln_low=100.0,
                vtln_warp=1.0, window_type='povey')
    sig = inspect.signature(tac.kaldi.mfcc)
    assert list(sig.parameters) == ['waveform'] + list(want) and {k: sig.parameters[k].default for k in want} == want
    want = dict(blackman_coeff=0.42, channel=-1, dither=0.0, energy_floor=1.0, frame_length=25.0, frame_shift=10.0, min_duration=0.0,
                preemphasis_coefficient=0.97, raw_energy=True, remove_dc_offset=True, round_to_power_of_two=True,
                sample_frequency=16000.0, snip_edges=True, subtract_mean=False, window_type='povey')
    sig = inspect.signature(tac.kaldi.spectrogram)
    assert list(sig.parameters) == ['waveform'] + list(want) and {k: sig.parameters[k].default for k in want} == want
    assert tac.kaldi.__all__ == ['fbank', 'mfcc', 'spectrogram']


def test_shapes_channel_and_min_duration(tac):
    x = torch.from_numpy(signal(dict(), rows=3, frames=5))
    assert tuple(tac.kaldi_mfcc(x.reshape(3, 1, -1).expand(3, 2, -1), num_ceps=7).shape) == (3, 2, 5, 7)
    assert tuple(tac.kaldi_spectrogram(x.reshape(1, 3, -1), sample_frequency=8000.0).shape) == (1, 3, 12, 129)
    assert tuple(tac.kaldi_mfcc(x, snip_edges=False).shape) == (3, 7, 13)
    for length, frames in ((399, 0), (400, 1), (0, 0)):
        assert tuple(tac.kaldi_mfcc(torch.randn(2, length)).shape) == (2, frames, 13)
        assert tuple(tac.kaldi_spectrogram(torch.randn(2, length)).shape) == (2, frames, 257)
    rows = [tac.kaldi_mfcc(x[c]) for c in range(3)]
    assert not torch.equal(rows[0], rows[2])
    assert torch.equal(tac.kaldi.mfcc(x), rows[0]) and torch.equal(tac.kaldi.mfcc(x, channel=2), rows[2])
    assert torch.equal(tac.kaldi.spectrogram(x, channel=1), tac.kaldi_spectrogram(x[1]))
    dur = x.shape[1] / 16000.0
    assert tuple(tac.kaldi.mfcc(x, min_duration=dur + 1e-3).shape) == (0, 13) and tuple(tac.kaldi.mfcc(x, min_duration=dur).shape) == (5, 13)
    assert tuple(tac.kaldi.spectrogram(x, min_duration=dur + 1e-3).shape) == (0, 257)
    for fn in (tac.kaldi.mfcc, tac.kaldi.spectrogram):
        with pytest.raises(ValueError):
            fn(x[0])


def test_argument_errors(tac):
    x = torch.randn(2, 2000)
    for kw in (dict(num_ceps=24), dict(num_mel_bins=10, num_ceps=11), dict(num_ceps=0), dict(num_mel_bins=3, num_ceps=2),
               dict(window_type='hann'), dict(frame_length=0.1), dict(frame_shift=0.05), dict(low_freq=-1.0), dict(high_freq=8001.0)):
        with pytest.raises(ValueError):
            tac.kaldi_mfcc(x, **kw)
        with pytest.raises(ValueError):
            tac.KaldiMfcc(**kw)
    for kw in (dict(window_type='hann'), dict(frame_length=0.1), dict(frame_shift=0.05)):
        with pytest.raises(ValueError):
            tac.kaldi_spectrogram(x, **kw)
        with pytest.raises(ValueError):
            tac.KaldiSpectrogram(**kw)
    with pytest.raises(NotImplementedError, match='vtln_warp'):
        tac.kaldi_mfcc(x, vtln_warp=1.1)
    with pytest.raises(NotImplementedError, match='vtln_warp'):
        tac.kaldi.mfcc(x, vtln_warp=0.9)
    for fn, layer in ((tac.kaldi_mfcc, tac.KaldiMfcc), (tac.kaldi_spectrogram, tac.KaldiSpectrogram)):
        with pytest.raises(TypeError):
            fn([1.0, 2.0])
        with pytest.raises(TypeError):
            layer(channel=0)
        with pytest.raises(RuntimeError):
            fn(torch.zeros(2, 2000, dtype=torch.int16))
        with pytest.raises(RuntimeError):
            fn(torch.tensor(1.0))
    with pytest.raises(TypeError):
        tac.KaldiSpectrogram(num_mel_bins=23)
    with pytest.raises(ValueError):
        tac.kaldi_mfcc(torch.randn(1, 100), snip_edges=False)   # one mirror does not reach, as for kaldi_fbank


def test_cpu_options_outside_the_kernel(tac):
    """N = 2048, no rounding to a power of two, and a table beyond the launch's LDS are the same definition on the CPU"""
    x = signal(dict(), rows=2, frames=7)[:, :3000]
    for kw in (dict(sample_frequency=48000.0), dict(round_to_power_of_two=False), dict(num_mel_bins=80, num_ceps=80)):
        got = tac.kaldi_mfcc(torch.from_numpy(x).double(), **kw)
        assert np.abs(got.numpy() - MR.mfcc_reference(x, MR.mfcc_options(**kw)).out).max() < 1e-8, kw
    got = tac.kaldi_spectrogram(torch.from_numpy(x).double(), sample_frequency=48000.0)
    assert tuple(got.shape) == (2, 1, 1025)
    assert np.abs(got.numpy() - MR.spectrogram_reference(x, MR.spectrogram_options(sample_frequency=48000.0)).out).max() < 1e-8
    torch.manual_seed(0)
    a, b = tac.kaldi_mfcc(torch.from_numpy(x), dither=1.0), tac.kaldi_mfcc(torch.from_numpy(x), dither=1.0)
    assert not torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_gradient_on_the_cpu(tac):
    x = torch.from_numpy(signal(dict(sample_frequency=8000.0), rows=2, frames=3)).double().requires_grad_(True)
    kw = dict(sample_frequency=8000.0, num_mel_bins=6, num_ceps=4, use_energy=True, energy_floor=0.0, htk_compat=True)
    assert torch.autograd.gradcheck(lambda t: tac.kaldi_mfcc(t, **kw), (x,), atol=1e-6)
    g = np.random.default_rng(0).standard_normal((2, 3, 4))
    tac.kaldi_mfcc(x, **kw).backward(torch.from_numpy(g))
    want = MR.row_gradient(x.detach().numpy(), MR.mfcc_options(**kw), g, 'mfcc')
    assert np.abs(x.grad.numpy() - want).max() <= 1e-9 * np.abs(want).max()
    x.grad = None
    kw = dict(sample_frequency=8000.0, energy_floor=0.0)
    g = np.random.default_rng(1).standard_normal((2, 3, 129))
    tac.kaldi_spectrogram(x, **kw).backward(torch.from_numpy(g))
    want = MR.row_gradient(x.detach().numpy(), MR.spectrogram_options(**kw), g, 'spectrogram')
    assert np.abs(x.grad.numpy() - want).max() <= 1e-9 * np.abs(want).max()


def test_fake_kernel_shapes_under_compile(tac):
    from torch._subclasses.fake_tensor import FakeTensorMode
    x = torch.randn(2, 3, 2000)
    for layer, op, cols in ((tac.KaldiMfcc(num_mel_bins=40, num_ceps=20), 'kaldi_mfcc', 20), (tac.KaldiSpectrogram(), 'kaldi_spectrogram', 257)):
        seen = []

        def capture(gm, example_inputs):
            seen.extend(n.target for n in gm.graph.nodes if n.op == 'call_function')
            return gm.forward

        torch._dynamo.reset()
        out = torch.compile(layer, backend=capture, fullgraph=True)(x)
        names = [str(t) for t in seen]
        assert sum('tac_amd.' + op in n for n in names) == 1 and len(names) == 1, names
        eager = layer(x)
        assert torch.equal(out, eager) and tuple(eager.shape) == (2, 3, 11, cols) and eager.is_contiguous()
    pm = tac._kaldi.MfccParams(**MR.mfcc_options(num_mel_bins=40, num_ceps=20, snip_edges=False))
    ps = tac._kaldi.SpectrogramParams(**MR.spectrogram_options(snip_edges=False, sample_frequency=8000.0))
    with FakeTensorMode() as mode:
        fm = torch.ops.tac_amd.kaldi_mfcc(mode.from_tensor(x), *pm)
        fs = torch.ops.tac_amd.kaldi_spectrogram(mode.from_tensor(x), *ps)
    assert tuple(fm.shape) == (2, 3, 13, 20) and fm.dtype == torch.float32 and fm.stride() == (3 * 13 * 20, 13 * 20, 20, 1)
    assert tuple(fs.shape) == (2, 3, 25, 129) and fs.stride() == (3 * 25 * 129, 25 * 129, 129, 1)
    torch.library.opcheck(torch.ops.tac_amd.kaldi_mfcc.default, (torch.randn(2, 1000),) + tuple(tac._kaldi.MfccParams(**MR.mfcc_options())),
                          test_utils=('test_schema', 'test_faketensor'))
    torch.library.opcheck(torch.ops.tac_amd.kaldi_spectrogram.default,
                          (torch.randn(2, 1000),) + tuple(tac._kaldi.SpectrogramParams(**MR.spectrogram_options())),
                          test_utils=('test_schema', 'test_faketensor'))


def test_layers_and_names(tac):
    m = tac.KaldiMfcc(num_mel_bins=40, num_ceps=20)
    assert repr(m) == 'KaldiMfcc(num_mel_bins=40, num_ceps=20)' and repr(tac.KaldiSpectrogram()) == 'KaldiSpectrogram()'
    assert m.state_dict() == {} and list(m.named_buffers()) == []
    x = torch.from_numpy(signal(dict(), rows=2, frames=4))
    assert torch.equal(m(x), tac.kaldi_mfcc(x, num_mel_bins=40, num_ceps=20))
    assert torch.equal(tac.KaldiSpectrogram(window_type='hamming')(x), tac.kaldi_spectrogram(x, window_type='hamming'))
    for name in ('kaldi_mfcc', 'kaldi_spectrogram'):
        assert name in tac.functional.__all__ and getattr(tac, name) is getattr(tac.functional, name)
        assert name in tac._ops.cuda_kernels and hasattr(torch.ops.tac_amd, name)
    assert tac.KaldiMfcc is tac.layers.KaldiMfcc and tac.KaldiSpectrogram is tac.layers.KaldiSpectrogram
    assert tac.kaldi.mfcc.__module__ == tac.kaldi.spectrogram.__module__ == 'torchaudio_contrib_amd.kaldi'


# ----------------------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_and_exported(tac):
    header = open(os.path.join(ROOT, 'include', 'tac_amd.h')).read()
    for name in ('tac_kaldi_mfcc_f32', 'tac_kaldi_spectrogram_f32', 'tac_kaldi_mfcc_table_limit'):
        assert re.search(r'\b%s\s*\(' % name, header) and name in tac._native.EXPORTS
    if not os.path.exists(tac._native.LIB_PATH):
        tac.build_native()
    h = tac._native.lib()
    assert h.tac_abi_version() == 5
    inv, uns = tac._native.TAC_E_INVALID, tac._native.TAC_E_UNSUPPORTED
    # argument checks of the launchers need no device: nothing is launched for these
    assert h.tac_kaldi_mfcc_f32(None, 1, 1000, 1000, None, None, None, None, 512, 400, 160, 23, 100, 13, 0, 0.97, 1.0, None, None) == inv
    assert h.tac_kaldi_spectrogram_f32(None, 1, 1000, 1000, None, 512, 400, 160, 0, 0.97, 1.0, None, None) == inv
    p = ctypes_buffer()
    assert h.tac_kaldi_mfcc_f32(p, 1, 1000, 1000, p, p, p, p, 512, 400, 160, 23, 100, 24, 1, 0.97, 1.0, p, None) == inv     # num_ceps > n_mels
    assert h.tac_kaldi_mfcc_f32(p, 1, 1000, 1000, p, p, p, p, 512, 400, 160, 23, 100, 0, 1, 0.97, 1.0, p, None) == inv
    assert h.tac_kaldi_mfcc_f32(p, 1, 1000, 1000, p, p, p, p, 2048, 400, 160, 23, 100, 13, 1, 0.97, 1.0, p, None) == uns
    assert h.tac_kaldi_mfcc_f32(p, 1, 1000, 1000, p, p, p, p, 512, 400, 160, 129, 100, 13, 1, 0.97, 1.0, p, None) == uns
    assert h.tac_kaldi_mfcc_f32(p, 1, 1000, 1000, p, p, p, p, 512, 400, 160, 80, 501, 80, 1, 0.97, 1.0, p, None) == uns     # the table
    assert h.tac_kaldi_mfcc_f32(p, 1, 300, 300, p, p, p, p, 512, 400, 160, 23, 100, 13, 1, 0.97, 1.0, p, None) == inv       # no frame
    assert h.tac_kaldi_spectrogram_f32(p, 1, 1000, 1000, p, 2048, 400, 160, 1, 0.97, 1.0, p, None) == uns
    assert h.tac_kaldi_spectrogram_f32(p, 1, 1000, 1000, p, 256, 400, 160, 1, 0.97, 1.0, p, None) == uns                   # W > N
    assert h.tac_kaldi_spectrogram_f32(p, 2, 1000, 0, p, 512, 400, 160, 1, 0.97, 1.0, p, None) == inv                      # row stride
    assert h.tac_kaldi_spectrogram_f32(p, 1, 300, 300, p, 512, 400, 160, 0, 0.97, 1.0, p, None) == uns                     # short mirrored row


def ctypes_buffer():
    import ctypes
    ctypes_buffer.keep = ctypes.create_string_buffer(64)
    return ctypes.cast(ctypes_buffer.keep, ctypes.c_void_p)


def test_table_limit_is_the_launchers_formula(tac):
    """64 KB less the four waves' areas, the window, the packed bank and its table, in floats — the Python route asks this entry
    point before launching, so the numbers the route and the launcher go by are the same"""
    if not os.path.exists(tac._native.LIB_PATH):
        tac.build_native()
    h = tac._native.lib()
    for n, frames_per_wave in ((256, 8), (512, 4), (1024, 2)):
        nc = n // 2
        slots = ((frames_per_wave * (nc + nc // 16 + 1) + 1) // 2) * 2
        for bins, w_total in ((23, 480), (80, 501), (128, 504), (4, 1)):
            want = (64 * 1024 - (4 * slots * 8 + 4 * (n + w_total + 3 * bins))) // 4
            assert h.tac_kaldi_mfcc_table_limit(n, bins, w_total) == want and want > 5000
    assert h.tac_kaldi_mfcc_table_limit(2048, 23, 480) == 0 and h.tac_kaldi_mfcc_table_limit(512, 129, 480) == 0
    assert h.tac_kaldi_mfcc_table_limit(512, 3, 480) == 0 and h.tac_kaldi_mfcc_table_limit(512, 23, 0) == 0
    K = tac._kaldi
    for bins, ceps, fits in ((23, 13, True), (80, 40, True), (128, 40, True), (80, 80, False), (128, 128, False)):
        p = K.MfccParams(**MR.mfcc_options(num_mel_bins=bins, num_ceps=ceps))
        limit = tac._hip.kaldi_mfcc_table_limit(p, 400, 512, torch.device('cpu'))
        assert (bins * ceps <= limit) == fits, (bins, ceps, limit)
