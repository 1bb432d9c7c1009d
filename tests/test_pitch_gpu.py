"""-m gpu: ``detect_pitch_frequency`` / ``PitchFrequency`` on the gfx950 kernels (csrc/pitch.hip) — strict mode and poisoned outputs on, as
in tests/test_loudness_gpu.py.

Reference and rule: tests/pitch_rules.py — the float64 restatement of the same float32 samples and its decision-stability rule.  The
first launch (``pitch_lags``) must give every stable frame the restatement's lag, every all-zero frame ``lag_min + 1`` and every other
frame a near-maximum; the second (``pitch_smooth``) must equal the torch form bit for bit, division included; the op must equal
``pitch_smooth`` of the restatement's lags wherever a median window holds no unstable frame.  Signals: six rows of 0.62 s + 37
samples at 8, 16, 44.1 and 48 kHz (``F`` 80 … 480, ``L`` 95 … 565, ``L > F``, odd sizes), one verdict per case, computed once.

A call of the op is ONE ``tac_pitch_frequency_f32`` entry, which makes two launches on the stream; the result and the int32 lags
between the launches are poisoned before the entry and checked after it."""
import functools
import warnings

import pytest
import torch

import pitch_rules as R

pytestmark = pytest.mark.gpu

ENTRY, LAGS_ENTRY, SMOOTH_ENTRY = 'tac_pitch_frequency_f32', 'tac_pitch_lags_f32', 'tac_pitch_smooth_i32'


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


@functools.lru_cache(maxsize=None)
def case(rate, frame_time=1e-2, freq_low=85, freq_high=3400, gain=1.0):
    """(float32 signal on the host, its verdict), computed once"""
    x = R.glide(rate) * gain
    return x, R.judge(x, rate, frame_time, freq_low, freq_high)


def lags(tac_, x, geo, what):
    """the first launch alone: exactly one entry, int32 of the frames' shape"""
    before = dict(tac_._hip.launches)
    got = tac_._hip.pitch_lags(x, geo.F, geo.L, geo.lag_min)
    assert launched_since(tac_, before) == {LAGS_ENTRY: 1}, what
    assert got.dtype == torch.int32 and tuple(got.shape) == tuple(x.shape[:-1]) + (R.ceil_div(x.shape[-1], geo.F),), what
    return got


# ----------------------------------------------------------------------------- 1. the lags against the float64 restatement
@pytest.mark.parametrize('rate', sorted(R.RATES))
def test_lags(tac, rate):
    x, verdict = case(rate)
    geo = verdict.geo
    assert (geo.F, geo.L) == R.RATES[rate] and x.shape[-1] % geo.F != 0
    assert verdict.unstable_share <= R.UNSTABLE_CAP, 'the signal leaves %.1f %% of its frames unstable' % (100 * verdict.unstable_share)
    xd = x.cuda()
    got = lags(tac, xd, geo, '%d Hz' % rate)
    differ = R.assert_lags(got, verdict, '%d Hz' % rate)
    print('%d Hz: F %d, L %d, %d frames, %.1f %% unstable, %d differ from the float64 lags' % (
        rate, geo.F, geo.L, verdict.silent.numel(), 100 * verdict.unstable_share, differ))
    assert torch.equal(got, lags(tac, xd, geo, 'again')), 'two calls differ'


@pytest.mark.parametrize('gain', [2.0 ** -12, 2.0 ** 12])
def test_gains(tac, gain):
    x, verdict = case(16000, gain=gain)
    assert verdict.unstable_share <= R.UNSTABLE_CAP
    R.assert_lags(lags(tac, x.cuda(), verdict.geo, 'gain %g' % gain), verdict, 'gain %g' % gain)


@pytest.mark.parametrize('rate,frame_time,freq_low,freq_high', R.VARIANTS)
def test_variants(tac, rate, frame_time, freq_low, freq_high):
    x, verdict = case(rate, frame_time, freq_low, freq_high)
    geo, default = verdict.geo, R.geometry(x.shape[-1], rate)
    assert (geo.F, geo.L, geo.lag_min) != (default.F, default.L, default.lag_min) and geo.lag_min < geo.half
    assert verdict.unstable_share <= R.UNSTABLE_CAP
    what = '%d Hz, frames of %d, lags %d .. %d' % (rate, geo.F, geo.lag_min + 1, geo.L)
    R.assert_lags(lags(tac, x.cuda(), geo, what), verdict, what)
    assert any(R.geometry(1, *v[:2], 30, *v[2:]).F % 4 for v in R.VARIANTS)


# ----------------------------------------------------------------------------- 2. edge shapes and layouts
def test_edge_lengths(tac):
    rate = 8000
    full, _ = case(rate)
    start = full.shape[-1] // 9 + 100                                 # behind the leading zeros
    for time in (50, 79, 80, 81, 80 * 30, 80 * 30 + 1):               # one short frame, one frame, exact multiples of F and one beyond
        x = full[:, start:start + time].contiguous()
        verdict = R.judge(x, rate)
        assert verdict.geo.N == R.ceil_div(time, 80)
        R.assert_lags(lags(tac, x.cuda(), verdict.geo, '%d samples' % time), verdict, '%d samples' % time)
    one = full[0, start:start + 500]                                  # a tensor of one dimension
    verdict = R.judge(one.reshape(1, -1), rate)
    got = lags(tac, one.cuda(), verdict.geo, 'one dimension')
    R.assert_lags(got.reshape(1, -1), verdict, 'one dimension')


def test_layouts(tac):
    rate = 16000
    x, verdict = case(rate)
    geo = verdict.geo
    rows, time = x.shape
    xd = x.cuda()
    plain = lags(tac, xd, geo, 'contiguous')
    R.assert_lags(plain, verdict, 'contiguous')
    store = torch.full((3, 4, time + 8), float('nan'), device='cuda')                       # channel slices of (B, C, T)
    store[:, 1:3, 2:time + 2] = xd.reshape(3, 2, time)
    view = store[:, 1:3, 2:time + 2]
    assert not view.is_contiguous() and all(s > 0 for s in view.stride())
    assert torch.equal(lags(tac, view, geo, 'channel slices').reshape(rows, -1), plain)
    store = torch.full((rows, 2 * time + 1), float('nan'), device='cuda')                    # time stride 2
    store[:, 1::2] = xd
    assert store[:, 1::2].stride(-1) == 2
    assert torch.equal(lags(tac, store[:, 1::2], geo, 'time stride 2'), plain)
    for off in (1, 2, 3):                                                                    # rows that start off a 16-byte boundary
        store = torch.full((rows * (time + off) + 4,), float('nan'), device='cuda')
        late = store[off:off + rows * (time + off)].view(rows, time + off)[:, :time]
        late.copy_(xd)
        assert late.data_ptr() % 16 == 4 * off
        assert torch.equal(lags(tac, late, geo, 'offset %d' % off), plain)
    nested = torch.stack([xd, xd.flip(0)]).reshape(2, 2, 3, time)                            # three leading dimensions
    got = lags(tac, nested, geo, 'three leading dimensions').reshape(2, rows, -1)
    assert torch.equal(got[0], plain) and torch.equal(got[1], plain.flip(0))


def test_units_beyond_the_grid(tac):
    """the first launch is persistent: every workgroup takes a second unit, and some a third"""
    rate, time = 8000, 22 * 80 - 3
    full, _ = case(rate)
    base = full[:5, 900:900 + time].contiguous()
    verdict = R.judge(base, rate)
    geo = verdict.geo
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    group, nbytes = tac._hip.pitch_plan(geo.N, geo.F, geo.L)
    assert (group, nbytes) == (R.plan(geo.N, geo.F, geo.L)[0], R.plan(geo.N, geo.F, geo.L)[2]) and R.ceil_div(geo.N, group) == 2
    grid = R.lags_grid(cus, 1, geo.N, geo.F, geo.L)[1]
    rows = grid + 3
    units, _ = R.lags_grid(cus, rows, geo.N, geo.F, geo.L)
    assert units == 2 * grid + 6 and units > 2 * grid
    small = lags(tac, base.cuda(), geo, 'five rows')
    R.assert_lags(small, verdict, 'five rows')
    index = (torch.arange(rows) % 5).cuda()
    big = lags(tac, base.cuda()[index].contiguous(), geo, '%d rows: %d units on a grid of %d' % (rows, units, grid))
    assert torch.equal(big, small[index])


def test_a_non_finite_sample_stays_in_its_frames(tac):
    rate = 16000
    x, verdict = case(rate)
    geo = verdict.geo
    clean = lags(tac, x.cuda(), geo, 'clean')
    R.assert_lags(clean, verdict, 'clean')
    bad = x.clone()
    spots = ((1, 5000, float('nan')), (3, 7777, float('inf')), (4, x.shape[-1] - 1, float('-inf')))
    touched = torch.zeros_like(verdict.silent)
    for row, at, value in spots:
        bad[row, at] = value
        for t in range(geo.N):
            touched[row, t] |= t * geo.F <= at < t * geo.F + geo.F + geo.L
    got = lags(tac, bad.cuda(), geo, 'NaN and Inf').cpu()
    assert 0 < int(touched.sum()) < 12
    assert torch.equal(got[~touched], clean.cpu()[~touched]), 'a frame whose span holds no non-finite sample changed'
    assert bool(((got[touched] >= geo.lag_min + 1) & (got[touched] <= geo.L)).all()), got[touched]


# ----------------------------------------------------------------------------- 3. the smoothing launch
@pytest.mark.parametrize('win', [1, 2, 3, 29, 30, 31, R.MAX_WIN])
def test_smoothing(tac, win):
    pad = (win - 1) // 2
    for n in (win - pad, win - pad + 1, 255 + win - pad, 256 + win - pad, 700):        # one output, two, a tile, a tile and one, three tiles
        table = R.lag_table(5, n, 6, 189, seed=win * 1000 + n)
        before = dict(tac._hip.launches)
        got = tac._hip.pitch_smooth(table.cuda(), win, 16000)
        assert launched_since(tac, before) == {SMOOTH_ENTRY: 1}
        want = R.smooth(table, win, 16000)
        assert got.dtype == torch.float32 and tuple(got.shape) == (5, n + pad - win + 1) == tuple(want.shape)
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), 'win_length %d over %d lags' % (win, n)
    if win == 1:
        single = torch.tensor([[80], [7]], dtype=torch.int32)                          # a single frame
        assert torch.equal(tac._hip.pitch_smooth(single.cuda(), 1, 44100).cpu(), R.smooth(single, 1, 44100))
    table = R.lag_table(2, 40, 6, 189, seed=3).reshape(2, 1, 40).expand(2, 3, 40)       # leading dimensions
    assert torch.equal(tac._hip.pitch_smooth(table.cuda(), 3, 8000).cpu(), R.smooth(table, 3, 8000))
    with pytest.raises(RuntimeError):
        tac._hip.pitch_smooth(table.cuda(), R.MAX_WIN + 1, 8000)


# ----------------------------------------------------------------------------- 4. end to end
def clean_windows(verdict, win, silent_too=True):
    """bool (rows, n_out): the outputs whose median window holds no unstable frame (and, on request, no all-zero frame, whose
    tie between equal values torch's ``max`` on a device need not break by the first index)"""
    pad = (win - 1) // 2
    firm = (verdict.stable | verdict.silent if silent_too else verdict.stable).to(torch.int64)
    firm = torch.cat([firm[:, :1]] * pad + [firm], -1) if pad else firm
    return firm.unfold(-1, win, 1).amin(-1).bool()


@pytest.mark.parametrize('rate,win', [(8000, 30), (16000, 30), (48000, 5), (16000, 1)])
def test_end_to_end(tac, rate, win):
    x, verdict = case(rate)
    want = R.smooth(verdict.lags, win, rate)
    keep = clean_windows(verdict, win)
    assert tuple(keep.shape) == tuple(want.shape) and float(keep.float().mean()) > 0.5
    xd = x.cuda().reshape(2, 3, -1)
    before = dict(tac._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac.CompositeRouteWarning)
        got = tac.detect_pitch_frequency(xd, rate, win_length=win)
    assert launched_since(tac, before) == {ENTRY: 1}                     # one entry: two launches on the stream behind it
    assert type(got) is torch.Tensor and got.dtype == torch.float32 and tuple(got.shape) == (2, 3, want.shape[-1])
    flat = got.reshape(6, -1).cpu()
    assert torch.equal(flat[keep].view(torch.int32), want[keep].view(torch.int32))
    geo = verdict.geo
    rate32 = torch.tensor(float(rate), dtype=torch.float32)
    assert bool(((flat >= rate32 / geo.L) & (flat <= rate32 / (geo.lag_min + 1))).all())
    assert torch.equal(got, tac.PitchFrequency(rate, win_length=win)(xd)), 'two calls differ'
    # the two halves by themselves give the same bits
    halves = tac._hip.pitch_smooth(tac._hip.pitch_lags(xd, geo.F, geo.L, geo.lag_min), win, rate)
    assert torch.equal(got, halves)


def test_known_answer_and_routes(tac):
    for rate, freq in ((16000, 200.0), (8000, 250.0)):
        x = R.tone(rate, freq, rate // 2 + 13).reshape(1, -1).cuda()
        got = tac.detect_pitch_frequency(x, rate)
        assert tuple(got.shape) == (1, R.geometry(x.shape[-1], rate).N - 15) and bool((got == freq).all()), got
    silence = tac.detect_pitch_frequency(torch.zeros(2, 4000, device='cuda'), 16000)
    assert bool((silence == 16000.0 / (R.geometry(4000, 16000).lag_min + 1)).all())
    x, verdict = case(8000)
    xd = x.cuda()
    ref = tac.detect_pitch_frequency(xd, 8000)
    before = dict(tac._hip.launches)
    half = tac.detect_pitch_frequency(xd.half(), 8000)
    assert half.dtype == torch.float32 and half.shape == ref.shape
    assert launched_since(tac, before) == {ENTRY: 1}                     # float16 is widened and takes the kernels
    before = dict(tac._hip.launches)
    with pytest.raises(RuntimeError, match='dtype float64'):
        tac.detect_pitch_frequency(xd.double(), 8000)
    with pytest.raises(RuntimeError, match='non-positive strides'):
        tac.detect_pitch_frequency(xd[:1].expand(3, -1), 8000)
    with pytest.raises(RuntimeError, match='a median window of 65 lags'):
        tac.detect_pitch_frequency(xd.repeat(1, 2), 8000, win_length=65)
    with pytest.raises(ValueError):
        tac.detect_pitch_frequency(xd, 8000, freq_high=170)
    empty = tac.detect_pitch_frequency(torch.zeros(0, 4000, device='cuda'), 16000)
    assert tuple(empty.shape) == (0, 10) and launched_since(tac, before) == {}
    tac.set_strict(False)
    try:
        for key in [k for k in tac._ops._warned if k[0] == 'detect_pitch_frequency']:
            tac._ops._warned.discard(key)
        with pytest.warns(tac.CompositeRouteWarning):
            got = tac.detect_pitch_frequency(xd.double(), 8000)
        assert launched_since(tac, before) == {} and got.dtype == torch.float32
        keep = clean_windows(verdict, 30, silent_too=False)
        assert int(keep.sum()) > 20 and torch.equal(got.cpu()[keep], R.smooth(verdict.lags, 30, 8000)[keep])
    finally:
        tac.set_strict(True)
