"""-m gpu: ``vad`` / ``vad_start`` / ``Vad`` on the gfx950 kernels (csrc/vad.hip behind ``tac_spectrogram_f32``) — strict mode and
poisoned outputs on, as in tests/test_pitch_gpu.py.

Reference and rules: tests/vad_rules.py — the float64 restatement of the same float32 samples, the bound ``DELTA`` (4 times the
float32 restatement's own deviation over the case table) every measure is held to, and the decision-stability rule under which
the kernels must give the restatement's ``(start, triggered)``.  Signals: ``(2, 3, 2.5 s + 37)`` at 8, 16, 22.05, 44.1 and 48 kHz, one
restatement per case, computed once.

A call of ``vad_start`` is ONE ``tac_spectrogram_f32`` launch and ONE ``tac_vad_start_f32`` entry of two launches; the int64 starts
and the float32 measures between the launches are poisoned before the entry and checked after it."""
import warnings

import pytest
import torch

import vad_rules as R

pytestmark = pytest.mark.gpu

SPEC_ENTRY, START_ENTRY, MEASURE_ENTRY = 'tac_spectrogram_f32', 'tac_vad_start_f32', 'tac_vad_measures_f32'


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
    t.set_lazy_fusion(True)


@pytest.fixture(autouse=True)
def every_output_written(tac):
    tac._hip.poison_report()
    yield
    left = tac._hip.poison_report()
    assert not left, 'kernel outputs left unwritten (poisoned elements per entry point): %r' % left


def launched_since(tac_, before):
    now = tac_._hip.launches
    return {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)}


def package_plan(tac_, rate, **kw):
    return tac_._vad.plan(rate, *tac_._vad.resolve(R.arguments(**kw)))


def measured(tac_, x, p, what):
    """launches 1 and 2 alone: one entry each, float32 of the frames' shape"""
    before = dict(tac_._hip.launches)
    got = tac_._hip.vad_measures(x, p)
    frames = R.n_frames(x.shape[-1], p)
    assert launched_since(tac_, before) == ({SPEC_ENTRY: 1, MEASURE_ENTRY: 1} if frames and got.numel() else {}), what
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(x.shape[:-1]) + (frames,), what
    return got


# ----------------------------------------------------------------------------- 1. the measures against the float64 restatement
@pytest.mark.parametrize('rate', R.RATES)
def test_measures(tac, rate):
    c = R.case(rate)
    p = package_plan(tac, rate)
    assert tuple(p) == tuple(c.plan) and p.dft == R.DFT[rate]
    xd = c.x.cuda()
    got = measured(tac, xd, p, '%d Hz' % rate)
    R.assert_measures(got, c, 'kernels, %d Hz (dft %d, bins [%d, %d), cepstrum [%d, %d))' % (rate, p.dft, p.s0, p.s1, p.c0, p.c1))
    assert bool((got[..., :p.boot_max + 1] == 0).all())                       # the boot frames: exactly 0
    again = measured(tac, xd, p, 'again')
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), 'two calls differ'


# ----------------------------------------------------------------------------- 2. launches, groupings and the slice
@pytest.mark.parametrize('rate', R.RATES)
def test_launches_and_starts(tac, rate):
    c = R.case(rate)
    xd = c.x.cuda()
    for joint, lead in (('all', ()), ('channel', (2,)), ('none', (2, 3))):
        before = dict(tac._hip.launches)
        with warnings.catch_warnings():
            warnings.simplefilter('error', tac.CompositeRouteWarning)
            start, triggered = tac.vad_start(xd, rate, joint=joint)
        assert launched_since(tac, before) == {SPEC_ENTRY: 1, START_ENTRY: 1}, joint
        assert start.is_cuda and triggered.is_cuda and tuple(start.shape) == tuple(triggered.shape) == lead
        R.assert_starts(start, triggered, c, joint, '%d Hz, joint %s' % (rate, joint))
    flat = xd.reshape(6, -1)
    before = dict(tac._hip.launches)
    out = tac.vad(flat, rate)
    assert launched_since(tac, before) == {SPEC_ENTRY: 1, START_ENTRY: 1}
    want = R.verdicts(c, 'all')[0].decision.start
    assert tuple(out.shape) == (6, flat.shape[-1] - want) and torch.equal(out, flat[:, want:])
    assert out.data_ptr() == flat[:, want:].data_ptr() and out.stride() == flat.stride()          # the slice itself …
    assert torch.equal(flat.cpu(), c.x.reshape(6, -1))                                            # … of an input left as it was
    one = xd[1, 2]
    assert torch.equal(tac.Vad(rate)(one), one[R.verdicts(c, 'none')[5].decision.start:])


@pytest.mark.parametrize('gain', R.GAINS)
def test_level_dependence(tac, gain):
    c = R.case(16000, gain)
    xd = c.x.cuda()
    R.assert_measures(measured(tac, xd, package_plan(tac, 16000), 'gain %g' % gain), c, 'kernels, gain %g' % gain)
    for joint in ('all', 'channel', 'none'):
        R.assert_starts(*tac.vad_start(xd, 16000, joint=joint), c, joint, 'gain %g, joint %s' % (gain, joint))


# ----------------------------------------------------------------------------- 3. edge shapes and layouts
def test_edge_lengths(tac):
    rate = 8000
    c = R.case(rate)
    p = package_plan(tac, rate)
    bound = R.delta()[0]
    for time in (p.mlen - 1, p.mlen, p.mlen + p.period - 1, p.mlen + p.period, p.mlen + (p.boot_max + 1) * p.period):
        x = c.x[:, :, 4200:4200 + time].contiguous()                    # the first voice sets in at sample 3000: frame boot_max + 1
        frames = R.n_frames(time, p)
        want = R.measures(x, p, torch.float64)
        got = measured(tac, x.cuda(), p, '%d samples' % time)
        assert tuple(got.shape) == (2, 3, frames) == tuple(want.meas.shape)
        if frames:
            assert float((got.cpu().double() - want.meas).abs().max()) <= bound, '%d samples' % time
        start, triggered = tac.vad_start(x.cuda(), rate, joint='none')
        assert not bool(triggered.any()) and start.tolist() == [[max(time - p.keep, 0)] * 3] * 2
    assert frames == p.boot_max + 2 and bool((want.meas[:, 0, -1] > 0).all()) and bool((got[:, 0, -1] > 0).all())


def test_layouts(tac):
    rate = 16000
    c = R.case(rate)
    p = package_plan(tac, rate)
    xd = c.x.cuda()
    time = xd.shape[-1]
    plain = measured(tac, xd, p, 'contiguous')
    want = tac.vad_start(xd, rate, joint='channel')
    store = torch.full((2, 5, time + 8), float('nan'), device='cuda')                       # a channel slice of a padded batch
    store[:, 1:4, 3:time + 3] = xd
    view = store[:, 1:4, 3:time + 3]
    assert not view.is_contiguous()
    assert torch.equal(measured(tac, view, p, 'channel slice'), plain)
    got = tac.vad_start(view, rate, joint='channel')
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    turned = xd.reshape(6, time).t().contiguous().t()                                       # a transposed (time, rows) view
    assert turned.stride() == (1, 6)
    assert torch.equal(measured(tac, turned, p, 'transposed').reshape(2, 3, -1), plain)
    store = torch.full((6 * time + 5,), float('nan'), device='cuda')                        # an odd storage offset
    late = store[3:3 + 6 * time].view(2, 3, time)
    late.copy_(xd)
    assert late.data_ptr() % 16 == 12
    assert torch.equal(measured(tac, late, p, 'offset 3'), plain)
    one = xd[1, 0]                                                                          # one dimension
    assert torch.equal(measured(tac, one, p, 'one dimension'), plain[1, 0])
    start, triggered = tac.vad_start(one, rate)
    assert tuple(start.shape) == () and int(start) == R.verdicts(c, 'none')[3].decision.start and bool(triggered)


def test_rows_beyond_the_grid(tac):
    """launch 2 is persistent: every workgroup takes a second row, and three of them a third"""
    rate, time = 8000, 4000
    p = package_plan(tac, rate)
    assert R.n_frames(time, p) == 9
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    limits = tac._hip.vad_limits(p)
    assert limits[4] == R.VAD_PER_CU and limits[3] >= p.n
    rows = 2 * cus * R.VAD_PER_CU + 3
    work, grid = R.measure_grid(cus, rows)
    assert work == 2 * grid + 3 and grid == cus * R.VAD_PER_CU
    base = []                                                            # 5 distinct rows, each voice setting in behind the boot frames
    for i, (group, which) in enumerate(((0, 0), (0, 1), (0, 2), (1, 0), (1, 1))):
        at = int(R.ONSET[which] * rate) - 3000 - 50 * i
        base.append(R.case(rate).x[group, which, at:at + time])
    base = torch.stack(base).cuda()
    alone = torch.stack([measured(tac, base[i], p, 'row %d alone' % i) for i in range(5)])
    assert len({tuple(r.tolist()) for r in alone.cpu()}) == 5 and bool((alone[:, -2:] > 0).any(-1).all())
    index = (torch.arange(rows) % 5).cuda()
    big = measured(tac, base[index].contiguous(), p, '%d rows on a grid of %d' % (rows, grid))
    assert torch.equal(big.view(torch.int32), alone[index].view(torch.int32))


# ----------------------------------------------------------------------------- 4. other arguments and the refused calls
def test_custom_arguments_and_routes(tac):
    rate = 16000
    c = R.case(rate)
    xd = c.x.cuda()
    kw = dict(measure_duration=0.05, lp_filter_freq=3000.0, trigger_level=6.0, pre_trigger_time=0.01)
    p = package_plan(tac, rate, **kw)
    q = R.plan(rate, **kw)
    assert tuple(p) == tuple(q) and (p.dft, p.s0, p.s1) == (1024, 3, 192) != (c.plan.dft, c.plan.s0, c.plan.s1)
    want = R.measures(c.x, q, torch.float64)
    got = measured(tac, xd, p, 'custom arguments')
    assert float((got.cpu().double() - want.meas).abs().max()) <= R.delta()[0]
    start, triggered = tac.vad_start(xd, rate, joint='channel', **kw)
    for g in range(2):
        v = R.judge(R.Measures(want.meas[g], want.raw[g], want.r[g]), q, xd.shape[-1], R.delta()[0])
        assert v.stable and int(start[g]) == v.decision.start and bool(triggered[g]) == v.decision.triggered
    # float16 is widened and takes the kernels
    before = dict(tac._hip.launches)
    start, _ = tac.vad_start(xd.half(), rate, joint='none')
    assert launched_since(tac, before) == {SPEC_ENTRY: 1, START_ENTRY: 1} and tuple(start.shape) == (2, 3)
    # empty leading shapes launch nothing
    before = dict(tac._hip.launches)
    start, triggered = tac.vad_start(torch.zeros(0, 3, 20000, device='cuda'), rate, joint='channel')
    assert tuple(start.shape) == (0,) and start.is_cuda and launched_since(tac, before) == {}
    # refused calls: an error under strict mode, the composite without it
    with pytest.raises(RuntimeError, match='dtype float64'):
        tac.vad_start(xd.double(), rate)
    with pytest.raises(RuntimeError, match='expanded or non-positive strides'):
        tac.vad_start(xd[:1].expand(4, -1, -1), rate)
    with pytest.raises(RuntimeError, match='a search of 1025 measures'):
        tac.vad_start(xd, rate, search_time=51.25)
    with pytest.raises(ValueError):
        tac.vad_start(xd, rate, hp_lifter_freq=2500.0)
    assert launched_since(tac, before) == {}
    tac.set_strict(False)
    try:
        for key in [k for k in tac._ops._warned if k[0] in ('vad_start', 'vad_measures')]:
            tac._ops._warned.discard(key)
        with pytest.warns(tac.CompositeRouteWarning):
            start, triggered = tac.vad_start(xd.double(), rate, joint='none')
        assert launched_since(tac, before) == {} and start.is_cuda
        R.assert_starts(start, triggered, c, 'none', 'float64 on the device')
    finally:
        tac.set_strict(True)
