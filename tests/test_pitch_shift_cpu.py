"""not-gpu: ``pitch_shift`` / ``PitchShift`` / ``tac_amd::resample_fit`` where no device is needed — the rates, the host plan of the
wide polyphase kernel (``_hip.resample_wide_plan``), the compact composite (``_composite.resample_compact``) and the whole chain on
CPU float64 against the independent restatement of tests/pitch_shift_rules.py."""
import os

import numpy as np
import pytest
import torch

import pitch_shift_rules as PS
import resample_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


# ----------------------------------------------------------------------------- rates
@pytest.mark.parametrize('sample_rate, n_steps, source, pair', [
    (16000, 4, 20158, (10079, 8000)), (16000, -4, 12699, (12699, 16000)), (44100, 2, 49500, (55, 49)),
    (48000, -2, 42763, (42763, 48000)), (16000, 12, 32000, (2, 1)), (44100, -12, 22050, (1, 2)), (22050, 12, 44100, (2, 1))])
def test_rates(tac, sample_rate, n_steps, source, pair):
    rate, got = tac._augment.pitch_rates(sample_rate, n_steps, 12)
    assert rate == 2.0 ** (-n_steps / 12) and got == source
    assert tac._resample.constants(got, sample_rate)[:2] == pair
    assert PS.rates(sample_rate, n_steps)[1:] == (source, pair)


# ----------------------------------------------------------------------------- the plan
@pytest.mark.parametrize('pair', [(2000, 2001), (1873, 1575), (10079, 8000), (42763, 48000), (44101, 16000)], ids=str)
def test_plan_is_the_brute_force_span(tac, pair):
    key = tac._resample.constants(*pair)
    for b in (tac._resample.bank(*key), tac._resample.adjoint_bank(*key)):
        assert PS.monotone(b.off, b.phases, b.step)
        start = tac._hip.resample_wide_starts(b)
        assert bool((start[1:] >= start[:-1]).all())
        plan = tac._hip.resample_wide_plan(b)
        assert plan is not None
        span, tile = plan
        assert tile in (1024, 512, 256) and span == PS.brute_span(b.off, b.run, b.phases, b.step, tile)
        assert span <= tac._hip.RESAMPLE_WIDE_SPAN_MAX
        assert tac._hip.resample_wide_plan(b) is plan                         # cached
    if pair == (44101, 16000):
        assert tac._hip.resample_wide_plan(tac._resample.bank(*key)) == (2854, 1024)


def test_plan_refusals(tac):
    key = tac._resample.constants(96001, 96000)
    b = tac._resample.bank(*key)
    assert b.phases * b.K > tac._hip.RESAMPLE_WIDE_MAX_BANK == 1 << 20
    assert tac._hip.resample_wide_plan(b) is None and tac._hip.resample_wide_plan(tac._resample.adjoint_bank(*key)) is None
    assert not tac._hip.resample_fit_covers(key, 1000, 1000)
    good = tac._resample.bank(*tac._resample.constants(1873, 1575))
    assert tac._hip.resample_wide_plan(good) is not None
    off = list(good.off)
    off[700] = off[699] - 1                                                 # one start before its predecessor's
    broken = tac._resample.Bank(good.phases, good.step, good.taps, off, good.run)
    assert not PS.monotone(broken.off, broken.phases, broken.step) and tac._hip.resample_wide_plan(broken) is None
    off = list(good.off)
    off[0] = off[-1] - good.step - 1                                        # ... and across the wrap: start(P) < start(P - 1)
    assert all(b >= a for a, b in zip(off, off[1:]))
    assert tac._hip.resample_wide_plan(tac._resample.Bank(good.phases, good.step, good.taps, off, good.run)) is None
    wide = tac._resample.Bank(2, 3, torch.zeros(2, 65, dtype=torch.float64), [0, 1], [65, 65])
    assert tac._hip.resample_wide_plan(wide) is None                        # K > 64


def test_the_launcher_text_the_grid_rule_restates():
    name, lines = PS.WIDE
    text = open(os.path.join(ROOT, 'torchaudio-contrib_amd', 'csrc', name)).read()
    for line in lines:
        assert line in text, line
    for cus in (256, 304):
        rows = PS.wrap_shape(cus, 1553, 19, 1024, 1500)
        units, grid = PS.wide_launch(cus, rows, 1500, 1553, 19, 1024)
        assert grid % cus == 0 and 0 < units - 2 * grid < grid and rows % PS.WIDE_ROWS
        assert rows * 2250 * 4 <= PS.MAX_TENSOR_BYTES


# ----------------------------------------------------------------------------- the compact composite
@pytest.mark.parametrize('pair', [(2000, 2001), (1873, 1575)], ids=str)
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=str)
def test_compact_composite_within_the_bound(tac, pair, dtype):
    key = tac._resample.constants(*pair)
    x = R.waveform((2, 2600), seed=pair[0])
    n_out = R.out_length(2600, *pair)
    for out_len in (n_out - 11, n_out, n_out + 13):
        got = tac._composite.resample_compact(torch.from_numpy(x).to(dtype), *key, out_len)
        assert got.dtype == dtype and tuple(got.shape) == (2, out_len) and got.is_contiguous()
        ref, bound = PS.fit_reference(x, pair[0], pair[1], out_len)
        R.assert_close(got, ref, bound if dtype == torch.float32 else bound * 1e-8 + 1e-300, 'compact %s %s' % (pair, dtype))
        assert not bool(got[:, n_out:].any())                               # the padded tail: exactly zero
        via_op = torch.ops.tac_amd.resample_fit(torch.from_numpy(x).to(dtype), *key, out_len)
        assert torch.equal(via_op, got)


def test_compact_composite_against_the_conv1d_composite(tac):
    orig, new = 441, 160
    key = tac._resample.constants(orig, new)
    x = R.waveform((3, 3000), seed=4)
    n_out = R.out_length(3000, orig, new)
    _, width, _ = R.filter_constants(orig, new, 6, 0.99)
    k_min = min(len(R.phase_taps(orig, new, p)[0]) for p in range(new))
    ref, bound = R.reference(x, orig, new)
    full = tac._composite.resample(torch.from_numpy(x), *key)
    compact = tac._composite.resample_compact(torch.from_numpy(x), *key, n_out)
    # the conv1d sums all 2 width + orig taps of a phase, zeros included: its own bound counts every one of them
    R.assert_close(full, ref, bound * (2 * width + orig + 2) / (k_min + 2), 'conv1d composite')
    R.assert_close(compact, ref, bound, 'compact composite')
    R.assert_close(compact, full.double().numpy(), bound * (1 + (2 * width + orig + 2) / (k_min + 2)), 'compact against conv1d')


def test_compact_composite_gradcheck(tac):
    key = tac._resample.constants(7, 5)
    length = 40
    n_out = R.out_length(length, 7, 5)
    for out_len in (n_out - 4, n_out, n_out + 5):
        x = torch.from_numpy(R.waveform((2, length), seed=out_len)).double().requires_grad_(True)
        assert torch.autograd.gradcheck(lambda t: tac._composite.resample_compact(t, *key, out_len), (x,))
        assert torch.autograd.gradcheck(lambda t: torch.ops.tac_amd.resample_fit(t, *key, out_len), (x,))
        g = R.waveform((2, out_len), seed=1)
        (gx,) = torch.autograd.grad(torch.ops.tac_amd.resample_fit(x, *key, out_len), x, torch.from_numpy(g).double())
        aref, abound = PS.fit_adjoint_reference(g, length, 7, 5)
        R.assert_close(gx, aref, abound * 1e-8 + 1e-300, 'gradient, out_len %d' % out_len)


# ----------------------------------------------------------------------------- the chain on CPU float64
def _close(got, want, what):
    got = got.detach().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.abs(got - want).max())
    assert err <= 1e-10 * float(np.abs(want).max()), '%s: max |err| %.3g against a peak of %.3g' % (what, err, float(np.abs(want).max()))


@pytest.fixture(scope='module')
def wave():
    return torch.from_numpy(np.random.default_rng(21).standard_normal((2, 3, 4000)))


@pytest.mark.parametrize('n_steps', [4, -3, 0])
def test_pitch_shift_is_the_restatement(tac, wave, n_steps):
    got = tac.pitch_shift(wave, 16000, n_steps)
    assert tuple(got.shape) == (2, 3, 4000) and got.dtype == torch.float64
    _close(got, PS.pitch_shift_reference(wave, 16000, n_steps), 'n_steps %d' % n_steps)


def test_pitch_shift_other_geometry_and_the_layer(tac, wave):
    x = wave[0]
    kw = dict(n_fft=256, hop_length=64, win_length=200)
    got = tac.pitch_shift(x, 16000, 4, **kw)
    _close(got, PS.pitch_shift_reference(x, 16000, 4, **kw), 'n_fft 256, hop 64, win 200')
    layer = tac.PitchShift(16000, 4, wkwargs=dict(dtype=torch.float64), **kw)     # (the functional's own float64 Hann)
    assert layer.window.dtype == torch.float64 and not layer.state_dict()
    assert torch.equal(layer(x), got)
    window = torch.hamming_window(200, dtype=torch.float64)
    got = tac.pitch_shift(x, 16000, -3, window=window, **kw)
    _close(got, PS.pitch_shift_reference(x, 16000, -3, window=window, **kw), 'a Hamming window')
    layer = tac.PitchShift(16000, -3, window_fn=torch.hamming_window, wkwargs=dict(dtype=torch.float64), **kw)
    assert torch.equal(layer(x), got)
    assert torch.equal(tac.PitchShift(16000, 5, bins_per_octave=24, wkwargs=dict(dtype=torch.float64))(x),
                       tac.pitch_shift(x, 16000, 5, bins_per_octave=24))
    # it is differentiable end to end
    xg = x[:1, :1500].clone().requires_grad_(True)
    tac.pitch_shift(xg, 16000, 4).square().sum().backward()
    assert bool(torch.isfinite(xg.grad).all()) and bool(xg.grad.any())


def test_fake_kernel_shapes(tac):
    from torch._subclasses.fake_tensor import FakeTensorMode
    key = tac._resample.constants(10079, 8000)
    with FakeTensorMode():
        x = torch.empty(2, 3, 4000)
        assert tuple(torch.ops.tac_amd.resample_fit(x, *key, 4321).shape) == (2, 3, 4321)
        assert tuple(torch.ops.tac_amd.resample_fit(x.half(), *key, 17).shape) == (2, 3, 17)
        got = tac.pitch_shift(x, 16000, 4)
        assert tuple(got.shape) == (2, 3, 4000) and got.dtype == torch.float32


def test_argument_errors(tac):
    x = torch.zeros(2, 2000)
    for bad in (16000.0, True, '16000'):
        with pytest.raises(ValueError, match='sample_rate'):
            tac.pitch_shift(x, bad, 4)
        with pytest.raises(ValueError, match='sample_rate'):
            tac.PitchShift(bad, 4)
    with pytest.raises(ValueError, match='bins_per_octave'):
        tac.pitch_shift(x, 16000, 4, bins_per_octave=0)
    with pytest.raises(ValueError, match='leaves no sample rate'):
        tac.pitch_shift(x, 8, -48)                                          # int(8 / 16) == 0
    with pytest.raises(ValueError, match='leaves no sample rate'):
        tac.PitchShift(8, -48)
    with pytest.raises(RuntimeError, match='floating-point'):
        tac.pitch_shift(torch.zeros(2, 2000, dtype=torch.int64), 16000, 4)
    with pytest.raises(TypeError):
        tac.pitch_shift([0.0] * 2000, 16000, 4)
    assert 'pitch_shift' in tac.functional.__all__ and tac.PitchShift is tac.layers.PitchShift
