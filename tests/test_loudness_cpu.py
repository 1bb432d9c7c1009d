"""Not gpu: ``loudness`` / ``Loudness`` and the two shelving biquads on the CPU route (``_composite.loudness``: the definition in torch
operators with the package's own biquads), the argument checks, the routing decisions and the C entry's refusals.

Reference and bounds: tests/loudness_rules.py.  float64 input is held to 1e-9 dB of the scipy reference; float32 input to the bound
derived there for two roundings per sample and float32 sums (``f32_bound``), with the inputs' margins to both gates asserted above
that bound first.  Sizes: 4410 Hz (a block of 1764 samples, a hop of 441), one to four blocks — the CPU route is a loop over time."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import lfilter_rules
import loudness_rules as R

SR = 4410
GATE, STEP = 1764, 441


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    if not os.path.exists(t._native.LIB_PATH):
        t.build_native()
    return t


# ----------------------------------------------------------------------------- the designs and the two functionals
SETTINGS = ((16000, 4.0, 1500.0, 1.0 / np.sqrt(2.0)), (48000, -6.0, 3000.0, 0.707), (44100, 12.5, 100.0, 0.5), (8000, 0.0, 250.0, 2.0))


def test_shelf_designs_match_the_closed_forms(tac):
    for sr, gain, f, q in SETTINGS:
        for mine, closed in ((tac._filters.treble, R.treble_closed_form), (tac._filters.bass, R.bass_closed_form)):
            (b, a), (cb, ca) = mine(sr, gain, f, q), closed(sr, gain, f, q)
            assert len(b) == len(a) == 3 and all(isinstance(v, float) for v in b + a)
            np.testing.assert_allclose(np.array(b + a), np.array(cb + ca), rtol=1e-14, atol=0.0)
    # torchaudio's defaults, and 0 dB is the identity up to the common factor
    assert tac._filters.treble(16000, 3.0) == tac._filters.treble(16000, 3.0, 3000, 0.707)
    assert tac._filters.bass(16000, 3.0) == tac._filters.bass(16000, 3.0, 100, 0.707)
    b, a = tac._filters.treble(8000, 0.0, 250.0, 2.0)
    np.testing.assert_allclose(np.array(b) / a[0], np.array(a) / a[0], rtol=1e-14, atol=1e-15)
    # the K-weighting is torchaudio's pair
    (b1, a1), (b2, a2) = tac._filters.k_weighting(48000)
    np.testing.assert_allclose(np.array(b1 + a1 + b2 + a2), np.array(sum(map(tuple, sum(R.k_weighting(48000), ())), ())), rtol=1e-14)
    with pytest.raises(ValueError):
        tac._filters.treble(0, 4.0)
    with pytest.raises(ValueError):
        tac._filters.bass(16000, 4.0, Q=0.0)


@pytest.mark.parametrize('name', ['treble_biquad', 'bass_biquad'])
def test_shelf_biquads_on_the_cpu_route(tac, name):
    x = lfilter_rules.waveform((3, 301), seed=5) * np.float32(0.4)
    closed = R.treble_closed_form if name == 'treble_biquad' else R.bass_closed_form
    for sr, gain, f, q in SETTINGS:
        got = getattr(tac.functional, name)(torch.from_numpy(x), sr, gain, f, q)
        b, a = closed(sr, gain, f, q)
        ref, bound = lfilter_rules.reference(x, b, a, clamp=True)
        ratio = lfilter_rules.assert_close(got, ref, bound, '%s %r' % (name, (sr, gain, f, q)))
        print('%s %r: worst |err| / bound %.3g' % (name, (sr, gain, f, q), ratio))
    assert got.dtype == torch.float32 and got.shape == x.shape
    assert callable(getattr(tac.functional, name)) and not hasattr(tac, name)     # (tests/test_lfilter_cpu.py pins the top level)


# ----------------------------------------------------------------------------- values
CASES = [(c, n) for c in (1, 2, 5) for n in (GATE, GATE + STEP - 1, GATE + 3 * STEP + 5)]


@pytest.mark.parametrize('channels,length', CASES)
def test_cpu_route_matches_the_reference(tac, channels, length):
    case = R.levels(SR, channels, length)
    x = torch.from_numpy(case.x)
    got64 = tac.loudness(x.double(), SR)
    assert got64.dtype == torch.float64 and tuple(got64.shape) == (3,)
    R.assert_close(got64, case.want, 1e-9, case.what + ', float64')
    limit = R.f32_bound(case.x, SR, case.want)
    assert min(case.margins) > 2.0 * float(limit.max()), (case.margins, limit)
    got32 = tac.loudness(x, SR)
    assert got32.dtype == torch.float32
    R.assert_close(got32, case.want, limit, case.what + ', float32')


def test_both_gates_and_the_clip_on_the_cpu_route(tac):
    case = R.three_level(SR, 2, 4)
    assert case.removed == (1, 4, 4)
    R.assert_close(tac.loudness(torch.from_numpy(case.x).double(), SR), case.want, 1e-9, case.what)
    limit = R.f32_bound(case.x, SR, case.want)
    assert min(case.margins) > 2.0 * float(limit.max())
    R.assert_close(tac.Loudness(SR)(torch.from_numpy(case.x)), case.want, limit, case.what + ', float32')
    tone = R.loud()
    R.assert_close(tac.loudness(torch.from_numpy(tone.x).double(), tone.sample_rate), tone.want, 1e-9, tone.what)


# ----------------------------------------------------------------------------- shapes and errors
def test_shapes(tac):
    for channels in (1, 2, 3, 4, 5):
        base = torch.from_numpy(R.noise((6, channels, GATE), 0.1, channels))
        flat = tac.loudness(base, SR)
        assert tuple(flat.shape) == (6,)
        one = tac.loudness(base[0], SR)
        assert tuple(one.shape) == () and torch.equal(one, flat[0])
        nested = tac.loudness(base.reshape(2, 3, channels, GATE), SR)
        assert tuple(nested.shape) == (2, 3) and torch.equal(nested.reshape(-1), flat)
    empty = tac.loudness(torch.zeros(0, 2, GATE), SR)
    assert tuple(empty.shape) == (0,) and empty.dtype == torch.float32
    with pytest.raises(ValueError, match='no channel'):
        tac.loudness(torch.zeros(3, 0, GATE), SR)


def test_errors_come_before_any_work(tac):
    x = torch.zeros(2, GATE)
    with pytest.raises(ValueError, match='channels, time'):
        tac.loudness(torch.zeros(GATE), SR)
    with pytest.raises(ValueError, match='Only up to 5 channels are supported.'):
        tac.loudness(torch.zeros(6, GATE), SR)
    with pytest.raises(ValueError, match='floating-point'):
        tac.loudness(torch.zeros(2, GATE, dtype=torch.int16), SR)
    for rate in (0, -8000, 4410.0, '4410', None, True):
        with pytest.raises(ValueError, match='positive int'):
            tac.loudness(x, rate)
    with pytest.raises(ValueError, match='positive int'):
        tac.Loudness(16000.0)
    with pytest.raises(ValueError, match='shorter than one block of 400 ms'):
        tac.loudness(torch.zeros(2, GATE - 1), SR)
    with pytest.raises(ValueError, match='shorter than one block'):
        torch.ops.tac_amd.loudness(torch.zeros(2, GATE - 1), SR)           # the op itself checks too
    with pytest.raises(TypeError):
        tac.loudness(np.zeros((2, GATE)), SR)


def test_silence_is_nan_and_a_nan_stays_in_its_entry(tac):
    assert torch.isnan(tac.loudness(torch.zeros(2, 2, GATE + STEP), SR)).all()
    x = torch.from_numpy(R.noise((3, 2, GATE + STEP), 0.1, 3))
    clean = tac.loudness(x, SR)
    for bad in (float('nan'), float('inf')):
        y = x.clone()
        y[1, 0, 40] = bad
        got = tac.loudness(y, SR)
        assert torch.isnan(got[1]) and torch.equal(got[[0, 2]], clean[[0, 2]]), (bad, got, clean)


# ----------------------------------------------------------------------------- routing
def test_blocks_of_the_common_rates(tac):
    for rate, (gate, step) in R.COMMON_RATES.items():
        assert tac._filters.loudness_blocks(rate) == (gate, step) == R.blocks(rate) and gate == 4 * step
    assert tac._filters.loudness_blocks(4410) == (GATE, STEP) and tac._filters.loudness_blocks(11025) == (4410, 1102)


def test_routing_decisions(tac):
    reason = tac._ops.loudness_reason
    x = torch.zeros(3, 2, 40000)
    for rate in R.COMMON_RATES:
        assert reason(x, *R.blocks(rate)) is None
    assert reason(x, 4410, 1102) == 'a sample rate whose block of 4410 samples is not four hops of 1102'
    assert reason(x.double(), 3200, 800) == 'dtype float64'
    assert reason(x[:1].expand(3, 2, 40000), 3200, 800) == 'non-positive strides'
    assert reason(x[:, :1].expand(3, 2, 40000), 3200, 800) == 'non-positive strides'
    assert reason(x[:, 1:, 3:], 3200, 800) is None and reason(x.half(), 3200, 800) is None
    assert reason(x, 40, 10).startswith('a hop of 10 samples') and tac._hip.LOUDNESS_MIN_STEP == R.MIN_STEP


def test_fake_kernel_layer_and_exports(tac):
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode() as mode:
        fake = torch.ops.tac_amd.loudness(mode.from_tensor(torch.zeros(2, 3, 2, GATE)), SR)
    assert tuple(fake.shape) == (2, 3) and fake.dtype == torch.float32
    m = tac.Loudness(SR)
    assert m.state_dict() == {} and list(m.named_buffers()) == [] and list(m.parameters()) == [] and repr(m) == 'Loudness(sample_rate=4410)'
    assert 'loudness' in tac.functional.__all__ and tac.loudness is tac.functional.loudness and tac.Loudness is tac.layers.Loudness
    x = torch.from_numpy(R.noise((2, GATE), 0.1, 1))
    assert torch.equal(m(x), tac.loudness(x, SR))


def test_gradient_on_the_cpu_route(tac):
    """differentiable through the composite: the gradient of the float64 result agrees with a central difference"""
    x = torch.from_numpy(R.noise((1, GATE), 0.1, 2)).double().requires_grad_(True)
    tac.loudness(x, SR).backward()
    probe = torch.zeros_like(x)
    probe[0, 100], h = 1.0, 1e-6
    with torch.no_grad():
        fd = (tac.loudness(x + h * probe, SR) - tac.loudness(x - h * probe, SR)) / (2 * h)
    assert abs(float(x.grad[0, 100]) - float(fd)) <= 1e-5 * max(1.0, abs(float(fd)))


# ----------------------------------------------------------------------------- the launcher and the C ABI
def test_quoted_launcher_expressions_are_in_the_source(tac):
    name, quotes = R.QUOTED
    with open(os.path.join(os.path.dirname(os.path.abspath(tac.__file__)), 'csrc', name)) as f:
        text = f.read()
    for q in quotes:
        assert q in text, '%s no longer holds %r: tests/loudness_rules.py restates a launcher that has changed' % (name, q)
    assert R.TILE == tac._hip.LOUDNESS_TILE == 1024 * 16
    for cus in R.CU_COUNTS:
        assert R.grid(cus, 3, 2) == (6, 3) and R.grid(cus, R.wrap_rows(cus), 1) == (cus, 2 * cus + 5)
        assert R.grid(cus, 256, 5) == (cus, 256) and R.grid(cus, 10 * cus, 1) == (cus, 8 * cus)


def test_c_abi_surface(tac):
    h = tac._native.lib()
    assert h.tac_abi_version() == 5
    for name in ('tac_loudness_tile', 'tac_loudness_work_bytes', 'tac_loudness_f32'):
        assert name in tac._native.EXPORTS
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tac_amd.h')) as f:
        assert 'int tac_loudness_f32(' in f.read()
    assert h.tac_loudness_tile() == R.TILE
    assert h.tac_loudness_work_bytes(3, 2, GATE, GATE, STEP) == 8 * 3 * 2 * 4
    assert h.tac_loudness_work_bytes(3, 5, GATE + 2 * STEP + 440, GATE, STEP) == 8 * 3 * 5 * 6
    assert h.tac_loudness_work_bytes(256, 1, 160000, 6400, 1600) == 8 * 256 * 100
    for bad in ((0, 2, GATE, GATE, STEP), (3, 0, GATE, GATE, STEP), (3, 6, GATE, GATE, STEP), (3, 2, GATE - 1, GATE, STEP),
                (3, 2, 9000, 4410, 1102), (3, 2, 100, 40, 10)):
        assert h.tac_loudness_work_bytes(*bad) == 0, bad
    # argument errors are refused before anything is launched (no device is touched)
    one = ctypes.c_void_p(16)
    coeffs = (ctypes.c_double * 12)(*[v for b, a in tac._filters.k_weighting(SR) for v in b + a])
    invalid, unsupported, short = tac._native.TAC_E_INVALID, tac._native.TAC_E_UNSUPPORTED, tac._native.TAC_E_SHORT_INPUT
    ok = (one, 3, 2, 4000, 8000, 4000, GATE, STEP, coeffs, one, one, None)

    def call(**change):
        names = ('waveform', 'entries', 'channels', 'length', 'stride_b', 'stride_c', 'gate', 'step', 'coeffs', 'work', 'out', 'stream')
        return h.tac_loudness_f32(*[change.get(n, v) for n, v in zip(names, ok)])

    for name in ('waveform', 'coeffs', 'work', 'out'):
        assert call(**{name: None}) == invalid, name
    for name in ('entries', 'channels', 'length', 'gate', 'step'):
        assert call(**{name: 0}) == invalid, name
    assert call(channels=6) == invalid and call(stride_b=0) == invalid and call(stride_c=-4000) == invalid
    assert call(length=GATE - 1) == short
    assert call(gate=4410, step=1102, length=9000) == unsupported and call(gate=GATE + 1) == unsupported
    assert call(gate=40, step=10) == unsupported
    zero_a0 = (ctypes.c_double * 12)(*([1.0, 0.0, 0.0, 0.0, 0.0, 0.0] * 2))
    assert call(coeffs=zero_a0) == invalid
