"""-m gpu: ``cqt`` on the gfx950 kernel of csrc/cqt.hip — strict mode and poisoned outputs on, one counted ``tac_cqt_f32`` launch per
call, every element held to the bound of tests/cqt_rules.py.  Shapes: the smallest that reach one group plus a ragged one, one
chunk and several, one frame tile and a ragged second one, both skew parities of the staged window, and more units than the grid."""
import warnings

import numpy as np
import pytest
import torch

import cqt_rules as R

pytestmark = pytest.mark.gpu

ENTRY = 'tac_cqt_f32'
dev = R.dev
TINY = dict(sr=4000.0, hop_length=64, fmin=250.0, n_bins=9, bins_per_octave=4)            # N_0 = 85: groups of 8 + 1, one chunk
FULL = dict(sr=22050.0, hop_length=512, fmin=32.70, n_bins=84, bins_per_octave=12)         # N_0 = 11341: 11 groups, six chunks


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    assert torch.cuda.is_available(), 'these tests need the MI355X'
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


def run(tac_, x, kw):
    """one call on the kernel route: no announcement, exactly one launch"""
    kw = dict(kw)
    before = dict(tac_._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac_.CompositeRouteWarning)
        got = tac_.cqt(x, kw.pop('sr'), **kw)
    now = tac_._hip.launches
    assert {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)} == {ENTRY: 1}
    assert got.dtype == torch.float32 and got.is_contiguous()
    return got


def check(tac_, x, kw, what, view=None):
    got = run(tac_, dev(x) if view is None else view, kw)
    ratio = R.assert_close(got, *R.cqt(x, **kw), what)
    print('%s: worst |err| / bound %.3f' % (what, ratio))


@pytest.mark.parametrize('kw, length', [(dict(TINY, center=c), (f - 1) * 64 + (43 if c else 85)) for c in (True, False) for f in (1, 32, 33)]
                         + [(FULL, 22050)], ids=lambda v: str(v if isinstance(v, int) else v.get('center', 'default bank')))
def test_one_frame_one_tile_a_ragged_second_and_the_default_bank(tac, kw, length):
    for name, x in zip(('dense', 'sparse'), R.signals(length, kw['sr'], kw['hop_length'], length)):
        check(tac, x, kw, '%s, %d samples, center=%s, %d bins' % (name, length, kw.get('center', True), kw['n_bins']))


@pytest.mark.parametrize('extra', [dict(hop_length=260), dict(hop_length=4), dict(hop_length=8), dict(bins_per_octave=24, n_bins=30), dict(gamma=20.0), dict(norm=2), dict(norm=None), dict(scale=False),
                                   dict(filter_scale=0.5), dict(pad_mode='constant'), dict(power=1.0), dict(power=2.0)],
                         ids=lambda e: ','.join('%s=%s' % kv for kv in e.items()))
def test_argument_variants_and_both_skew_parities(tac, extra):
    kw = dict(TINY, **extra)                     # (hop / 4 odd: 260 and 4, unskewed; even: 64 and 8, skewed)
    for name, x in zip(('dense', 'sparse'), R.signals(2301, 4000.0, kw['hop_length'], 7)):
        check(tac, x, kw, '%r, %s' % (extra, name))
    if 'power' in extra:
        check(tac, R.signals(22050, 22050.0, 512, 11)[0], dict(FULL, **extra), 'default bank, %r' % extra)
    layer = tac.CQT(kw.pop('sr'), **kw)
    assert torch.equal(layer(dev(x)), tac.cqt(dev(x), 4000.0, **kw))


def test_layouts(tac):
    r = np.random.default_rng(5)
    x = r.standard_normal((2, 3, 700)).astype(np.float32)
    check(tac, x, TINY, 'leading dims (2, 3)')
    check(tac, x[:, 1:3], TINY, 'a channel slice', dev(x)[:, 1:3])
    check(tac, x[..., ::2], TINY, 'time stride 2', dev(x)[..., ::2])
    for off in (1, 2, 3):
        check(tac, x[0, 0, off:off + 601], TINY, 'offset %d' % off, dev(x)[0, 0, off:off + 601])
    half = x.astype(np.float16)
    check(tac, half.astype(np.float32), TINY, 'float16 input', dev(half))


def test_non_finite_samples_stay_in_their_groups(tac):
    """a non-finite sample reaches all 8 bins of every group whose span of the tap axis covers it in a frame — the
    zero fill of a group multiplies it —, which contains every element the definition makes non-finite, and nothing else"""
    from torchaudio_contrib_amd import _cqt
    x = R.signals(22050, 22050.0, 512, 11)[0]
    x[6001], x[15000] = np.nan, np.inf
    got = run(tac, dev(x), FULL).cpu().numpy()
    value, bound = R.cqt(x, **FULL)
    plan = _cqt.plan(22050.0, 32.70, 84, 12, 1.0, 0.0, 1, True)
    bad = np.flatnonzero(~np.isfinite(x))
    expected = np.zeros(value.shape, bool)
    for g, (E, steps, _, bins) in enumerate(plan.groups.tolist()):
        first = 512 * np.arange(value.shape[-1]) - plan.c0 + E          # (far from both ends: the mirror does not reach them)
        hit = ((bad[None, :] >= first[:, None]) & (bad[None, :] < first[:, None] + 16 * steps)).any(1)
        expected[8 * g:8 * g + bins] = hit
    assert np.array_equal(~np.isfinite(got).all(-1), expected) and not (~np.isfinite(value) & ~expected).any()
    err = np.hypot(got[..., 0] - value.real, got[..., 1] - value.imag)
    assert np.all(err[~expected] <= bound[~expected])


def test_more_units_than_the_grid(tac):
    """2 x grid + 6 units of one tile each, every row different: the rows of a workgroup's second and third unit have the bits of
    the same rows run alone"""
    grid = torch.cuda.get_device_properties(0).multi_processor_count * tac._native.lib().tac_cqt_blocks_per_cu()
    rows = 2 * grid + 6
    x = dev(np.random.default_rng(9).standard_normal((rows, 300)).astype(np.float32))
    got = run(tac, x, TINY)
    for i in (0, grid - 1, grid, 2 * grid - 1, 2 * grid, rows - 1):
        assert torch.equal(got[i], run(tac, x[i], TINY)), 'row %d' % i
    R.assert_close(got[-3:], *R.cqt(x[-3:].cpu().numpy(), **TINY), 'the last rows')


@pytest.mark.parametrize('route', ['hop', 'float64', 'backward'])
def test_other_routes_are_announced_and_refused_under_strict(tac, route):
    x = dev(R.signals(2301, 4000.0, 64, 7)[0])
    kw = dict(TINY, hop_length=510) if route == 'hop' else dict(TINY)
    sr = kw.pop('sr')
    x = x.double() if route == 'float64' else x
    if route == 'backward':
        x.requires_grad_(True)
        call = lambda: tac.cqt(x, sr, power=2.0, **kw).sum().backward()
    else:
        call = lambda: tac.cqt(x, sr, **kw)
    with pytest.raises(RuntimeError, match='strict mode forbids'):
        call()
    tac.set_strict(False)
    try:
        tac._ops._warned.clear()
        with pytest.warns(tac.CompositeRouteWarning, match='cqt'):
            call()
        if route == 'backward':
            assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    finally:
        tac.set_strict(True)
