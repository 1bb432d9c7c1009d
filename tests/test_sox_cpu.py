"""not-gpu: the SoX effects ``overdrive`` / ``phaser`` / ``flanger`` — the LFO tables against hand-checked values, the closed and
blocked forms the kernels rest on against the literal loops (tests/sox_rules.py), the CPU route against the float32 literal loops
within ``bound32``, argument checks, exports, ``overdrive``'s gradient and the host-side routing predicates."""
import math
import warnings

import numpy as np
import pytest
import torch

import sox_rules as R


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


# ----------------------------------------------------------------------------- tables
def test_sine_table_by_hand():
    # n = 8 (divisible by 4), phase pi / 2: off = int(0.25 * 8 + 0.5) = 2, p = 2 3 4 5 6 7 0 1
    got = R.wave_table(R.SINE, R.FLOAT, 8, 0.0, 1.0, math.pi / 2)
    r = math.sqrt(0.5)
    want = [(s + 1) / 2 for s in (1.0, r, 0.0, -r, -1.0, -r, 0.0, r)]
    assert got.dtype == np.float32 and np.allclose(got, want, atol=1e-7)
    assert got[0] == 1.0                                                   # the exact peak: sin(pi / 2) == 1 in float64
    # n = 6 (not divisible by 4), phase 0, scaled to [2, 5]
    got = R.wave_table(R.SINE, R.FLOAT, 6, 2.0, 5.0, 0.0)
    want = [(math.sin(2 * math.pi * p / 6) + 1) / 2 * 3 + 2 for p in range(6)]
    assert np.allclose(got, want, atol=1e-6)


def test_triangle_table_by_hand():
    # n = 8: d = p / 4, v = p // 2: 0.5 0.75 | 1.0 0.75 0.5 0.25 | 0.0 0.25
    got = R.wave_table(R.TRIANGLE, R.FLOAT, 8, 0.0, 1.0, 0.0)
    assert np.array_equal(got, np.float32([0.5, 0.75, 1.0, 0.75, 0.5, 0.25, 0.0, 0.25]))
    # n = 6: d = p / 3, v = (4 p) // 6 = 0 0 1 2 2 3: 0.5 5/6 5/6 0.5 1/6 1/6
    got = R.wave_table(R.TRIANGLE, R.FLOAT, 6, 0.0, 1.0, 0.0)
    assert np.allclose(got, [0.5, 5 / 6, 5 / 6, 0.5, 1 / 6, 1 / 6], atol=1e-7)
    # INT: d + 0.5 truncated; scaled to [1, 4]: 2.5 3.25 4 3.25 2.5 1.75 1 1.75 -> 3 3 4 3 3 2 1 2
    got = R.wave_table(R.TRIANGLE, R.INT, 8, 1.0, 4.0, 0.0)
    assert got.dtype == np.int32 and got.tolist() == [3, 3, 4, 3, 3, 2, 1, 2]
    # phase 3 pi / 2: off = int(0.75 * 8 + 0.5) = 6: the table starts at its minimum
    assert R.wave_table(R.TRIANGLE, R.FLOAT, 8, 0.0, 1.0, 3 * math.pi / 2)[0] == 0.0


@pytest.mark.parametrize('kind', [R.SINE, R.TRIANGLE])
@pytest.mark.parametrize('n, L', [(4000, 24), (16001, 2), (37, 40), (8, 1)])
def test_int_tables_stay_in_range_and_match_the_package(tac, kind, n, L):
    m = R.wave_table(kind, R.INT, n, 1.0, float(L), math.pi / 2)
    assert m.min() >= 1 and m.max() <= L and (n < 4000 or (m.min() == 1 and m.max() == L))
    for data_type, lo, hi in ((R.INT, 1.0, float(L)), (R.FLOAT, 3.0, L + 3.5)):
        ours = tac._sox.wave_table(kind, data_type, n, lo, hi, 3 * math.pi / 2)
        assert np.array_equal(ours, R.wave_table(kind, data_type, n, lo, hi, 3 * math.pi / 2))


def test_plans_match_the_rules(tac):
    L, P, table = tac._sox.phaser_plan(8000, 3.0, 2.0, False)
    rl, rp, rm = R.phaser_plan(8000, 3.0, 2.0, False)
    assert (L, P) == (rl, rp) == (24, 4000) and table.dtype == torch.int32 and np.array_equal(table.numpy(), rm)
    q = tac._sox.flanger_plan(8000, 5.0, 3.0, 50.0, 71.0, 10.0, 25.0, 'triangular', 'quadratic', 3)
    r = R.flanger_plan(8000, 5.0, 3.0, 50.0, 71.0, 10.0, 25.0, 'triangular', 'quadratic', 3)
    assert (q.Lb, q.P, q.tmin, q.W) == (r.Lb, r.P, r.tmin, 41) == (66, 800, 40, 41)
    assert np.array_equal(q.lfo.numpy(), r.lfo) and list(q.phases) == list(r.phases) == [0, 200, 400]
    assert (q.fb, q.in_gain, q.delay_gain) == (r.fb, r.in_gain, r.delay_gain)
    assert q.lfo.min() >= q.tmin and q.lfo.max() <= q.Lb - 2
    assert tac._sox.flanger_plan(8000, 0.0, 0.0, 0.0, 71.0, 10.0, 25.0, 'sinusoidal', 'linear', 1).Lb == 2
    assert tac._sox.flanger_plan(8000, 30.0, 0.0, 0.0, 71.0, 10.0, 25.0, 'sinusoidal', 'linear', 1).W == 64


# ----------------------------------------------------------------------------- the forms the kernels rest on
PHASER_SETS = [dict(sample_rate=8000, mod_speed=2.0, delay_ms=3.0, decay=0.4), dict(sample_rate=8000, mod_speed=2.0, delay_ms=0.25, decay=0.99),
               dict(sample_rate=8000, mod_speed=1.7, delay_ms=5.0, decay=0.0, sinusoidal=False),
               dict(sample_rate=16000, mod_speed=0.5, delay_ms=3.0, decay=0.4, gain_in=1.0, sinusoidal=False)]


@pytest.mark.parametrize('kw', PHASER_SETS)
def test_phaser_closed_form_and_pointer_jumping_are_the_literal_loop(kw):
    x = R.waveform((3, 9001), seed=1)
    lit = R.phaser_literal(x, **kw)
    closed = R.phaser_closed(x, **kw)
    scale = np.abs(lit).max()
    assert np.abs(closed - lit).max() <= 1e-14 * scale
    jumped, rounds = R.phaser_jumped(x, **kw)
    assert rounds <= 14 and np.abs(jumped - lit).max() <= 1e-13 * scale
    ref, bound, _ = R.phaser(x, **kw)
    R.assert_close(np.clip(kw.get('gain_out', 0.74) * jumped, -1, 1), ref, bound, 'pointer jumping within the bound')


@pytest.mark.parametrize('W, delay', [(1, 0.0), (41, 5.0), (64, 30.0)])
@pytest.mark.parametrize('interpolation', ['linear', 'quadratic'])
def test_flanger_blocked_form_is_the_literal_loop(tac, W, delay, interpolation):
    plan = R.flanger_plan(8000, delay, 2.0, 50.0, 71.0, 10.0, 25.0, 'sinusoidal', interpolation, channels=2)
    assert min(64, 1 + plan.tmin) == W and plan.P % 4 == 0
    x = R.waveform((2, 2, 2500), seed=2)
    raw, _, _ = R.flanger_literal(x, plan)
    assert np.array_equal(R.flanger_blocked(x, plan, W), raw)             # bit-equal in float64
    if interpolation == 'quadratic':                                       # the wrap tap k + 2 == Lb occurs, with fr == 0
        k = np.floor(plan.lfo)
        assert ((k + 2 == plan.Lb) & (plan.lfo == k)).any() and not ((k + 2 >= plan.Lb) & (plan.lfo != k)).any()


# ----------------------------------------------------------------------------- the CPU route
def _cpu(fn, x, *args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        return fn(torch.from_numpy(x), *args, **kw)


@pytest.mark.parametrize('gain, colour, scale', [(20, 20, 0.3), (0, 0, 4.0), (100, 100, 1.0), (37.5, 5, 0.05)])
def test_overdrive_cpu_route(tac, gain, colour, scale):
    x = R.waveform((3, 700), seed=3, scale=scale)
    got = _cpu(tac.overdrive, x, gain, colour)
    assert got.dtype == torch.float32 and got.shape == (3, 700)
    ref, _, mass = R.overdrive(x, gain, colour)
    lit = np.clip(R.overdrive_literal(x, gain, colour, np.float32)[0], -1, 1)
    print('overdrive cpu: %.3f, literal32: %.3f' % (R.assert_close(got, ref, R.bound32(mass), 'CPU route'),
                                                   R.assert_close(lit, ref, R.bound32(mass), 'float32 literal')))
    r64, b64, _ = R.overdrive(x, gain, colour)
    R.assert_close(_cpu(tac.overdrive, x.astype(np.float64), gain, colour), r64, b64, 'float64 CPU route')
    layer = tac.Overdrive(gain, colour)
    assert torch.equal(layer(torch.from_numpy(x)), got)


@pytest.mark.parametrize('kw', PHASER_SETS)
def test_phaser_cpu_route(tac, kw):
    x = R.waveform((3, 1200), seed=4)
    got = _cpu(tac.phaser, x, **kw)
    assert got.dtype == torch.float32 and got.shape == (3, 1200)
    ref, _, mass = R.phaser(x, **kw)
    lit = np.clip(np.float32(kw.get('gain_out', 0.74)) * R.phaser_literal(x, dtype=np.float32, **kw), -1, 1)
    print('phaser cpu: %.3f, literal32: %.3f' % (R.assert_close(got, ref, R.bound32(mass), 'CPU route'),
                                                R.assert_close(lit, ref, R.bound32(mass), 'float32 literal')))
    full = dict(dict(gain_in=0.4, gain_out=0.74, delay_ms=3.0, decay=0.4, mod_speed=0.5, sinusoidal=True), **kw)
    assert torch.equal(tac.Phaser(**full)(torch.from_numpy(x)), got)


@pytest.mark.parametrize('regen', [0.0, -50.0, 95.0])
@pytest.mark.parametrize('interpolation', ['linear', 'quadratic'])
def test_flanger_cpu_route(tac, regen, interpolation):
    kw = dict(sample_rate=8000, delay=1.0, depth=2.0, regen=regen, width=71.0, speed=10.0, phase=25.0, modulation='triangular',
              interpolation=interpolation)
    x = R.waveform((2, 3, 900), seed=5, scale=0.5)
    got = _cpu(tac.flanger, x, **kw)
    assert got.dtype == torch.float32 and got.shape == (2, 3, 900)
    plan = R.flanger_plan(channels=3, **kw)
    ref, _, mass = R.flanger(x, plan)
    lit = np.clip(R.flanger_literal(x, plan, np.float32)[0], -1, 1)
    print('flanger cpu: %.3f, literal32: %.3f' % (R.assert_close(got, ref, R.bound32(mass), 'CPU route'),
                                                 R.assert_close(lit, ref, R.bound32(mass), 'float32 literal')))
    assert torch.equal(tac.Flanger(**kw)(torch.from_numpy(x)), got)


# ----------------------------------------------------------------------------- arguments, exports
def test_argument_checks(tac):
    x = torch.zeros(2, 2, 64)
    with pytest.raises(ValueError, match='4 channels'):
        tac.flanger(torch.zeros(1, 5, 64), 8000)
    with pytest.raises(ValueError, match='modulation'):
        tac.flanger(x, 8000, modulation='square')
    with pytest.raises(ValueError, match='interpolation'):
        tac.flanger(x, 8000, interpolation='cubic')
    with pytest.raises(ValueError):
        tac.flanger(x, 0)
    with pytest.raises(ValueError):
        tac.flanger(x, 8000, speed=10000.0)                 # P < 1
    with pytest.raises(ValueError):
        tac.flanger(torch.zeros(64), 8000)
    with pytest.raises(ValueError):
        tac.phaser(x, 8000, delay_ms=0.0)                   # L < 1
    with pytest.raises(ValueError):
        tac.phaser(x, 0)
    with pytest.raises(ValueError):
        tac.phaser(x, -8000)
    with pytest.raises(ValueError):
        tac.phaser(x, 8000, mod_speed=20000.0)              # P < 1
    with pytest.raises(ValueError):
        tac.Phaser(8000, delay_ms=0.0)
    with pytest.raises(ValueError):
        tac.Flanger(8000, modulation='square')
    with pytest.raises(RuntimeError):
        tac.overdrive(torch.zeros(4, dtype=torch.int32))
    for fn, args in ((tac.overdrive, ()), (tac.phaser, (8000,)), (tac.flanger, (8000,))):
        assert tuple(fn(x[..., :0], *args).shape) == (2, 2, 0)


def test_names_are_exported(tac):
    for name in ('overdrive', 'phaser', 'flanger'):
        assert name in tac.functional.__all__ and getattr(tac, name) is getattr(tac.functional, name)
        assert hasattr(torch.ops.tac_amd, name)
    for name in ('Overdrive', 'Phaser', 'Flanger'):
        assert getattr(tac, name) is getattr(tac.layers, name)


# ----------------------------------------------------------------------------- gradient
def test_overdrive_gradcheck_and_the_rules_gradient(tac):
    rng = np.random.default_rng(6)
    for gain, colour, scale in ((10.0, 30.0, 0.5), (0.0, 0.0, 2.0), (30.0, 100.0, 0.1)):
        x = torch.from_numpy(scale * rng.standard_normal((2, 40))).requires_grad_(True)
        assert torch.autograd.gradcheck(lambda v: tac.overdrive(v, gain, colour), (x,), eps=1e-7, atol=1e-6)
        gy = rng.standard_normal((2, 40))
        (gx,) = torch.autograd.grad(tac.overdrive(x, gain, colour), x, grad_outputs=torch.from_numpy(gy))
        want, mass, _ = R.overdrive_gradient(x.detach().numpy(), gy, gain, colour)
        assert np.abs(gx.numpy() - want).max() <= 1e-12 * mass.max()


# ----------------------------------------------------------------------------- routing predicates
def test_routing_predicates(tac):
    S, H = tac._sox, tac._hip
    assert S.inside(S.OVERDRIVE_RANGES, gain=0.0, colour=100.0) is None
    assert 'gain' in S.inside(S.OVERDRIVE_RANGES, gain=100.5, colour=20.0)
    assert 'colour' in S.inside(S.OVERDRIVE_RANGES, gain=20.0, colour=-1.0)
    assert S.inside(S.PHASER_RANGES, gain_in=1.0, delay_ms=5.0, decay=0.99, mod_speed=0.1) is None
    assert 'decay' in S.inside(S.PHASER_RANGES, gain_in=1.0, delay_ms=5.0, decay=0.995, mod_speed=0.1)
    assert 'mod_speed' in S.inside(S.PHASER_RANGES, gain_in=1.0, delay_ms=5.0, decay=0.5, mod_speed=float('nan'))
    assert S.inside(S.FLANGER_RANGES, delay=30.0, depth=10.0, regen=-95.0, width=100.0, speed=0.1, phase=100.0) is None
    assert 'regen' in S.inside(S.FLANGER_RANGES, delay=30.0, depth=10.0, regen=96.0, width=100.0, speed=0.1, phase=100.0)
    h = tac._native.lib()
    ok, unsupported, invalid = tac._native.TAC_OK, tac._native.TAC_E_UNSUPPORTED, tac._native.TAC_E_INVALID
    assert h.tac_overdrive_supported(10.0, 0.1) == ok and h.tac_overdrive_supported(float('inf'), 0.1) == invalid
    assert h.tac_phaser_supported(1, 1) == ok and h.tac_phaser_supported(H.PHASER_MAX_DELAY, 4000) == ok
    assert h.tac_phaser_supported(H.PHASER_MAX_DELAY + 1, 4000) == unsupported and h.tac_phaser_supported(0, 4000) == invalid
    assert h.tac_flanger_supported(2, 800, 1, 1) == ok and h.tac_flanger_supported(H.FLANGER_MAX_DELAY, 800, 64, 4) == ok
    assert h.tac_flanger_supported(H.FLANGER_MAX_DELAY + 1, 800, 64, 4) == unsupported
    assert h.tac_flanger_supported(66, 800, 65, 1) == unsupported and h.tac_flanger_supported(66, 800, 41, 5) == unsupported
    assert h.tac_flanger_supported(1, 800, 1, 1) == invalid and h.tac_flanger_supported(66, 0, 1, 1) == invalid
    assert (h.tac_overdrive_tile(), h.tac_phaser_tile(), h.tac_flanger_tile(), h.tac_flanger_chunk(), h.tac_flanger_max_block()) == (
        H.OVERDRIVE_TILE, H.PHASER_TILE, H.FLANGER_TILE, H.FLANGER_CHUNK, H.FLANGER_MAX_BLOCK)
    assert H.FLANGER_MAX_BLOCK == S.FLANGER_MAX_BLOCK == 64
    assert H.phaser_covers(24, 4000) and not H.phaser_covers(2000, 4000)
    plan = S.flanger_plan(8000, 5.0, 3.0, 50.0, 71.0, 10.0, 25.0, 'sinusoidal', 'linear', 2)
    assert H.flanger_covers(plan, 2)
    assert not H.flanger_covers(S.flanger_plan(192000, 30.0, 10.0, 50.0, 71.0, 10.0, 25.0, 'sinusoidal', 'linear', 2), 2)
