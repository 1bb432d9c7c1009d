"""not-gpu: the checker of the elementwise kernels (tests/elementwise_rules.py) checked itself — the float64 reference rounded once
passes every helper near 1 u, each planted error is caught (one of them while the old per-tensor bar still passes), the generators
hold what they promise, and the float32 composite routes (``_composite.py``, what a CPU tensor takes) go through the same helpers:
their error is printed, and they are held to the edge table's classes."""
import numpy as np
import pytest
import torch

import elementwise_rules as R

F32 = np.float32


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


def rounded(want):
    with np.errstate(all='ignore'):
        return np.asarray(want, dtype=np.float64).astype(F32)


# ----------------------------------------------------------------------------- 1. the reference, rounded once, passes
def test_rounded_reference_passes_every_helper():
    z = R.pair_sweep()
    w = R.grad_weights(R.N_PAIRS, 1)
    w2 = R.grad_weights(R.N_PAIRS, 2)
    for p in R.POWERS:
        frac = R.assert_forward('norm', rounded(R.n_forward('norm', z, p)), z, p, what='rounded |z|^%g' % p)
        assert frac <= 1.0 / min(2.0, 2.0 * abs(p) + R.LIB) + 1e-9               # one rounding: u of a bound of >= 2 u
        want, _ = R.grad_reference('norm', z, w, p)
        assert R.assert_grad('norm', rounded(want), z, w, p, what='rounded d|z|^%g' % p) <= 0.5
        want, _ = R.grad_reference('magphase', z, w, p, second=w2)
        assert R.assert_grad('magphase', rounded(want), z, w, p, second=w2, what='rounded d magphase(%g)' % p) <= 1.0
    assert R.assert_forward('angle', rounded(R.n_forward('angle', z)), z, what='rounded angle') <= 1.0 / R.LIB + 1e-9
    want, _ = R.grad_reference('magphase', z, None, 1.0, second=w2)
    assert R.assert_grad('magphase', rounded(want), z, None, 1.0, second=w2, what='rounded d angle') <= 0.25
    for ref, amin in R.DB_CASES + (R.DB_EQUALITY_CASE,):
        x = R.db_sweep(amin)
        g = R.grad_weights(x.numel(), 3)
        assert R.assert_forward('to_db', rounded(R.n_forward('to_db', x, ref, amin)), x, ref, amin,
                                what='rounded to_db %r' % ((ref, amin),)) <= 1.0
        want, _ = R.grad_reference('to_db', x, g, ref, amin)
        assert R.assert_grad('to_db', rounded(want), x, g, ref, amin, what='rounded d to_db %r' % ((ref, amin),)) <= 1.0 / 3 + 1e-9
    x = R.undb_sweep()
    g = R.grad_weights(x.numel(), 4)
    for ref in R.UNDB_REFS:
        assert R.assert_forward('from_db', rounded(R.n_forward('from_db', x, ref)), x, ref, what='rounded from_db %g' % ref) <= 1.0 / R.LIB
        want, _ = R.grad_reference('from_db', x, g, ref)
        assert R.assert_grad('from_db', rounded(want), x, g, ref, what='rounded d from_db %g' % ref) <= 1.0 / R.LIB


@pytest.mark.skipif(not R.longdouble_ok(), reason='numpy.longdouble has no more mantissa bits than float64 here')
def test_rounded_longdouble_reference_passes():
    z = R.pair_sweep(np.float64)
    for p in R.POWERS:
        want = R.n_forward('norm', z, p)
        assert want.dtype == np.longdouble
        assert R.assert_forward('norm', want.astype(np.float64), z, p, what='float64 rounded |z|^%g' % p) <= 0.5 + 1e-9
    assert R.assert_forward('angle', R.n_forward('angle', z).astype(np.float64), z, what='float64 rounded angle') <= 0.126
    for ref, amin in R.DB_CASES:
        x = R.db_sweep(amin, np.float64)
        assert R.assert_forward('to_db', R.n_forward('to_db', x, ref, amin).astype(np.float64), x, ref, amin, what='float64 rounded to_db') <= 1.0
    x = R.undb_sweep(np.float64)
    for ref in R.UNDB_REFS:
        assert R.assert_forward('from_db', R.n_forward('from_db', x, ref).astype(np.float64), x, ref, what='float64 rounded from_db') <= 0.2
    # a float64 reference could not judge a float64 kernel: the longdouble one sees a single float64 rounding as 1 u
    want = R.n_forward('from_db', x, 1.0)
    err = np.abs(want.astype(np.float64).astype(np.longdouble) - want) / np.abs(want)
    assert 0.2 * 2.0 ** -53 < float(err.max()) <= 2.0 ** -53


# ----------------------------------------------------------------------------- 2. planted errors
def test_plant_exp2_log2_for_pow():
    """``exp2(p * log2 m)`` step by step in float32: the product ``p log2 m`` is rounded at magnitude up to 42, which ``exp2``
    turns into tens of u"""
    z = R.pair_sweep()
    m = np.sqrt((z[:, 0].double() ** 2 + z[:, 1].double() ** 2).numpy()).astype(F32)
    for p in (0.7, 0.5):
        got = np.exp2(F32(p) * np.log2(m))
        assert got.dtype == F32
        with pytest.raises(AssertionError):
            R.assert_forward('norm', got, z, p, what='planted exp2(p log2 m), p %g' % p)


def test_plant_log2_times_constant_for_log10():
    """``log2(sigma) * 3.0103`` step by step in float32 with a subnormal ``sigma`` flushed to 0 before the logarithm, as the
    hardware logarithm flushes it.  (With a correctly rounded ``log2`` and a normal ``sigma`` that form stays inside the bound, whose
    ``LIB u |log10 sigma|`` term is what a library ``log10f`` is allowed: printed, not asserted.)"""
    ref, amin = R.DB_CASES[0]
    x = R.db_sweep(amin)
    xv = x.numpy()
    sigma = np.maximum(xv * xv, F32(amin))
    got = np.log2(sigma) * F32(3.0103) - F32(10.0) * F32(R.host_log10(ref))
    assert got.dtype == F32
    want = R.n_forward('to_db', x, ref, amin)
    print('log2 * 3.0103 on normal sigma: worst %.3f of the bound' % R.fractions(got, want, R.forward_bound('to_db', x, want, ref, amin)).max())
    xs = torch.tensor([1e-25, -3e-24, 1.0], dtype=torch.float32)                 # amin subnormal: sigma = amin below 1e-21
    sub = np.maximum(xs.numpy() ** 2, F32(1e-42))
    with np.errstate(all='ignore'):
        flushed = np.where(sub < F32(2.0 ** -126), F32(0), sub)
        got = (np.log2(flushed) * F32(3.0102999566)).astype(F32)
    with pytest.raises(AssertionError):
        R.assert_forward('to_db', got, xs, 1.0, 1e-42, what='planted flush of a subnormal sigma')


def test_plant_error_on_the_quiet_elements_passes_the_old_bar():
    """1e-6 max|want| added to the elements below 1e-3 max|want|: ``max|got - want| < 1e-5`` (the bar of test_complex_norm, on its
    data: uniform in (-4, 4)) still passes — which is the point — and the per-element bound does not"""
    g = torch.Generator().manual_seed(5)
    z = torch.rand((4096, 2), generator=g) * 8.0 - 4.0
    z[::4] *= 1e-4
    want = R.n_forward('norm', z, 1.0)
    top = np.abs(want).max()
    quiet = np.abs(want) < 1e-3 * top
    assert 0.2 < quiet.mean() < 0.3
    got = rounded(want + np.where(quiet, 1e-6 * top, 0.0))
    assert np.abs(got.astype(np.float64) - want).max() < 1e-5                    # the old bar
    assert np.abs(got.astype(np.float64) - want).max() / top < 1e-5             # and its relative form
    with pytest.raises(AssertionError):
        R.assert_forward('norm', got, z, 1.0, what='planted error on the quiet elements')
    assert R.assert_forward('norm', rounded(want), z, 1.0, what='the same data, unplanted') <= 0.5


def test_plant_dropped_sign_of_a_zero_imaginary_part():
    z = torch.tensor([[-1.0, -0.0], [-2.5, 0.0], [-3e10, -0.0], [1.0, -0.0]], dtype=torch.float32)
    got = np.arctan2(np.abs(z[:, 1].numpy()), z[:, 0].numpy())                   # +pi on the whole negative real axis
    with pytest.raises(AssertionError):
        R.assert_forward('angle', got, z, what='planted dropped sign')
    with pytest.raises(AssertionError):
        R.assert_edges('angle', got, z, what='planted dropped sign, by class')
    R.assert_edges('angle', np.arctan2(z[:, 1].numpy(), z[:, 0].numpy()), z)


def test_plant_gradient_through_the_clamp():
    ref, amin = R.DB_CASES[1]
    x = R.db_sweep(amin)
    g = R.grad_weights(x.numel(), 3)
    below, equal, above = R.clamp_sides(x, amin)
    assert below and above
    got = (g.numpy() * (F32(8.6858896380650366) / x.numpy())).astype(F32)
    with pytest.raises(AssertionError):
        R.assert_grad('to_db', got, x, g, ref, amin, what='planted gradient through the clamp')
    passes = R.t_passes(x, amin).numpy()
    assert R.assert_grad('to_db', np.where(passes, got, F32(0)), x, g, ref, amin, what='the closed form, clamped') <= 1.0


def test_plant_wrong_side_at_equality():
    """the clamp passes the gradient AT equality (torch's ``clamp`` backward does); a kernel with ``>`` is caught"""
    ref, amin = R.DB_EQUALITY_CASE
    x = R.db_sweep(amin)
    g = R.grad_weights(x.numel(), 3)
    xv = x.numpy()
    assert R.clamp_sides(x, amin)[1] >= 2
    got = np.where(xv * xv > F32(amin), g.numpy() * (F32(8.6858896380650366) / xv), F32(0)).astype(F32)
    with pytest.raises(AssertionError):
        R.assert_grad('to_db', got, x, g, ref, amin, what='planted > for >=')


# ----------------------------------------------------------------------------- 3. the generators
def test_pair_sweep_holds_what_it_promises():
    for dtype in (np.float32, np.float64):
        z = R.pair_sweep(dtype)
        assert tuple(z.shape) == (R.N_PAIRS, 2) and R.N_PAIRS == int(np.prod(R.PAIR_SHAPE))
        mag = np.hypot(z[:, 0].double().numpy(), z[:, 1].double().numpy())
        assert R.binades(mag) >= set(R.PAIR_BINADES) and R.binades(mag) <= set(range(-51, 62))
        s = (z[:, 0] * z[:, 0] + z[:, 1] * z[:, 1]).float()
        assert bool(torch.isfinite(s).all()) and float(s.min()) >= 2.0 ** -126       # re^2 + im^2 normal and finite in float32
        re, im = z[:, 0].double(), z[:, 1].double()
        on_axis = (re == 0) | (im == 0)
        assert float(on_axis.double().mean()) == R.AXIS_SHARE
        for mask in ((im == 0) & (re > 0), (im == 0) & (re < 0), (re == 0) & (im > 0), (re == 0) & (im < 0)):
            assert float(mask.double().mean()) == R.AXIS_SHARE / 4
        ratio = torch.where(on_axis, torch.ones_like(re), torch.maximum(re.abs(), im.abs()) / torch.minimum(re.abs(), im.abs()).clamp(min=1e-300))
        lopsided = ratio == 2.0 ** 30
        assert float(lopsided.double().mean()) == R.LOPSIDED_SHARE
        assert bool((lopsided & (re.abs() > im.abs())).any()) and bool((lopsided & (re.abs() < im.abs())).any())
        k = np.floor(np.log2(mag)).astype(int)
        for kind in (on_axis.numpy(), lopsided.numpy()):
            assert set(k[kind].tolist()) >= set(range(-49, 60))                      # every binade gets every kind
        assert torch.equal(z, R.pair_sweep(dtype))                                   # deterministic


def test_db_sweeps_hold_what_they_promise():
    equal_somewhere = 0
    for ref, amin in R.DB_CASES + (R.DB_EQUALITY_CASE,):
        for dtype in (np.float32, np.float64):
            x = R.db_sweep(amin, dtype)
            assert x.numel() == R.N_DB + 18
            assert R.binades(x[:R.N_DB]) >= set(R.DB_BINADES)
            assert bool((x[:R.N_DB] > 0).any()) and bool((x[:R.N_DB] < 0).any())
            near = x[R.N_DB:]
            below, equal, above = R.clamp_sides(near, amin)
            assert below >= 2 and above >= 2, (amin, below, equal, above)
            root = float(np.sqrt(np.dtype(dtype).type(amin)))
            assert float((near.abs().double() - root).abs().max()) <= 4.5 * float(np.spacing(np.dtype(dtype).type(root)))
            if dtype is np.float32:
                equal_somewhere += equal
                if (ref, amin) == R.DB_EQUALITY_CASE:
                    assert equal >= 2, equal                                         # both signs of the exact root
    assert equal_somewhere >= 2
    x = R.undb_sweep()
    assert float(x.abs().max()) <= 300.0 and float(x.abs().max()) > 299.0 and bool((x < 0).any())


# ----------------------------------------------------------------------------- 4. the float32 composite routes
def test_composite_routes_through_the_helpers(tac):
    """What a CPU tensor takes (``_composite.py``): stock float32 torch operators.  Their error is torch's, not this project's: it
    is printed as a fraction of the kernels' bound and not asserted; the classes of the edge table are."""
    z = R.pair_sweep()
    worst = {}
    for p in R.POWERS:
        want = R.n_forward('norm', z, p)
        worst['|z|^%g' % p] = R.fractions(tac.complex_norm(z, p).numpy(), want, R.forward_bound('norm', z, want, p)).max()
    want = R.n_forward('angle', z)
    worst['angle'] = R.fractions(tac.angle(z).numpy(), want, R.forward_bound('angle', z, want)).max()
    mag, phase = tac.magphase(z, 2.0)
    assert torch.equal(mag, tac.complex_norm(z, 2.0)) and torch.equal(phase, tac.angle(z))
    for ref, amin in R.DB_CASES:
        x = R.db_sweep(amin)
        want = R.n_forward('to_db', x, ref, amin)
        worst['to_db %r' % ((ref, amin),)] = R.fractions(tac.amplitude_to_db(x, ref, amin).numpy(), want,
                                                        R.forward_bound('to_db', x, want, ref, amin)).max()
    x = R.undb_sweep()
    for ref in R.UNDB_REFS:
        want = R.n_forward('from_db', x, ref)
        worst['from_db %g' % ref] = R.fractions(tac.db_to_amplitude(x, ref).numpy(), want, R.forward_bound('from_db', x, want, ref)).max()
    for name, frac in worst.items():
        print('float32 torch evaluation, %s: worst error %.3f of the kernels\' bound' % (name, frac))
    assert all(np.isfinite(f) for f in worst.values())                               # no class ever differs on the sweep

    def class_equal(got, op, rows, *params):
        expect, _ = R.edge_expectation(op, rows, *params)
        plain = R._oracle_f32(op, rows, *params).numpy()
        assert np.array_equal(R.classes(got.numpy()), R.classes(plain)), (op, params)
        return expect

    ze = R.pair_edges()
    for p in R.POWERS:
        class_equal(tac.complex_norm(ze, p), 'norm', ze, p)
    class_equal(tac.angle(ze), 'angle', ze)
    xe = torch.tensor(R.DB_EDGE_X, dtype=torch.float32)
    for ref in R.DB_EDGE_REF:
        for amin in R.DB_EDGE_AMIN:
            class_equal(tac.amplitude_to_db(xe, ref, amin), 'to_db', xe, ref, amin)
    ue = torch.tensor(R.UNDB_EDGE_X, dtype=torch.float32)
    for ref in R.UNDB_EDGE_REF:
        class_equal(tac.db_to_amplitude(ue, ref), 'from_db', ue, ref)


def test_every_deviation_is_used_and_named():
    """each entry of DEVIATIONS replaces at least one row of the edge tables, and nothing replaces a row under another name"""
    used = set()
    ze = R.pair_edges()
    g = R.grad_weights(ze.shape[0], 6)
    for p in R.POWERS:
        used |= set(R.edge_expectation('norm', ze, p, g=g)[1])
    used |= set(R.edge_expectation('angle', ze, g=g)[1])
    xe = torch.tensor(R.DB_EDGE_X, dtype=torch.float32)
    gx = R.grad_weights(xe.numel(), 7)
    for amin in R.DB_EDGE_AMIN:
        used |= set(R.edge_expectation('to_db', xe, 1.0, amin, g=gx)[1])
    ue = torch.tensor(R.UNDB_EDGE_X, dtype=torch.float32)
    used |= set(R.edge_expectation('from_db', ue, 1.0)[1])
    used |= set(R.edge_expectation('from_db', ue, 1.0, g=R.grad_weights(ue.numel(), 8))[1])
    assert used | {'gradient zero sign'} == set(R.DEVIATIONS), set(R.DEVIATIONS) ^ used
    assert all(len(reason) > 40 for reason in R.DEVIATIONS.values())
