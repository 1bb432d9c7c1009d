"""-m gpu: ``kaldi_fbank`` / ``KaldiFbank`` / ``kaldi.fbank`` on the gfx950 kernel (csrc/kaldi_fbank.hip) — strict mode and poisoned
outputs on, as in tests/test_mfcc_gpu.py.

Reference and rule: tests/kaldi_rules.py — the float64 per-frame definition, the per-element linear bound (FRAME_POW on the
processed frame's spectrum through the bank, plus the float32 roundings of the raw samples through mean removal and pre-emphasis)
and the log rule on top of it; every element is checked.  That the signals keep 99 % of their elements under the log rule is
established on the CPU (tests/test_kaldi_cpu.py).  The shapes are the smallest that reach each path of the kernel: 1 / G-1 / G /
G+1 / 4G+1 frames per row (a lone frame, the edges of a wave's G frames, several units per row), 1 and 3 rows, a shift beyond the
span a wave stages at once, more units than the whole grid's waves, misaligned rows with a padded stride, and a strided time slice (copied by the route).

Worst ratios of error to allowance measured on the MI355X: DESIGN 3.14."""
import warnings

import numpy as np
import pytest
import torch

import kaldi_rules as R
from oracle import signals

pytestmark = pytest.mark.gpu

ENTRY = 'tac_kaldi_fbank_f32'
GRAD_DB = 1e-3      # per row, gradients through a logarithm (tests/test_gpu_fuzz.py)


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


def dev(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to('cuda')


def frames_per_wave(o):
    return 64 // (R.sizes(o)[2] // 32)


def run_and_check(tac_, x, kw, what, xdev=None):
    """one covered call on ``x`` (rows, n): exactly one launch, the result under the rule; returns the ratios"""
    o = R.options(**kw)
    before = dict(tac_._hip.launches)
    got = tac_.kaldi_fbank(dev(x) if xdev is None else xdev, **kw)
    assert launched_since(tac_, before) == {ENTRY: 1}, launched_since(tac_, before)
    r = R.reference(x, o)
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (x.shape[0], r.value.shape[1], r.cols)
    res = R.check(got.cpu().numpy(), r, o, what)
    print('%s: %r' % (what, res))
    return res


# ----------------------------------------------------------------------------- geometries, frame counts, rows
@pytest.mark.parametrize('rows', (1, 3))
@pytest.mark.parametrize('geo', R.GEOMETRIES, ids=R.ident)
def test_frame_counts_of_every_geometry(tac, geo, rows):
    o = R.options(**geo)
    w, s, n = R.sizes(o)
    g = frames_per_wave(o)
    assert (w, s, n, g) in ((400, 160, 512, 4), (200, 80, 256, 8), (551, 220, 1024, 2), (400, 161, 512, 4), (512, 160, 512, 4),
                            (400, 2240, 512, 4))
    for frames in sorted({1, g - 1, g, g + 1, 4 * g + 1}):
        x = R.waveform(rows, R.length_for(frames, w, s, True), seed=11, kw=geo)
        run_and_check(tac, x, geo, '%s rows=%d frames=%d' % (R.ident(geo), rows, frames))


def test_more_units_than_the_grid_has_waves(tac):
    """96 rows of 120 frames: 2880 units of four frames, more than two workgroups of four waves on each of 256 compute units —
    every wave walks its loop more than once.  The rows repeat three checked ones and must repeat their bits."""
    base = R.waveform(3, R.length_for(120, 400, 160, True), seed=12)
    small = tac.kaldi_fbank(dev(base), num_mel_bins=80)
    few = np.ascontiguousarray(base[:, :R.length_for(9, 400, 160, True)])
    run_and_check(tac, few, dict(num_mel_bins=80), 'three rows of the batch, nine frames')
    assert torch.equal(small[:, :9], tac.kaldi_fbank(dev(few), num_mel_bins=80))       # a frame depends on its own samples only
    big = tac.kaldi_fbank(dev(np.tile(base, (32, 1))), num_mel_bins=80)
    assert tuple(big.shape) == (96, 120, 80)
    assert torch.equal(big.reshape(32, 3, 120, 80), small[None].expand(32, 3, 120, 80))


def test_misaligned_rows_padded_stride_and_leading_dims(tac):
    x = R.waveform(3, R.length_for(6, 400, 160, True), seed=13)
    n = x.shape[1]
    store = torch.full((3, n + 6), float('nan'), device='cuda')
    store[:, 1:n + 1] = dev(x)
    view = store[:, 1:n + 1]                                    # rows start 4 bytes off a 16-byte line, stride n + 6
    assert view.stride() == (n + 6, 1) and view.data_ptr() % 8 == 4
    res = run_and_check(tac, x, dict(use_energy=True), 'misaligned rows', xdev=view)
    plain = tac.kaldi_fbank(dev(x), use_energy=True)
    assert torch.equal(plain, tac.kaldi_fbank(view, use_energy=True))
    lead = tac.kaldi_fbank(dev(x).reshape(3, 1, n).expand(3, 2, n)[:, :1], use_energy=True)
    assert tuple(lead.shape) == (3, 1, 6, 24) and torch.equal(lead[:, 0], plain)
    assert res['kept'] >= R.KEEP


def test_time_slice_with_stride_two(tac):
    x = R.waveform(3, 2 * R.length_for(5, 400, 160, True), seed=14)
    xd = dev(x)[:, ::2]
    assert xd.stride(1) == 2
    run_and_check(tac, np.ascontiguousarray(x[:, ::2]), dict(), 'stride-2 time slice', xdev=xd)


# ----------------------------------------------------------------------------- options
@pytest.mark.parametrize('kw', R.OPTIONS, ids=R.ident)
def test_every_option_against_the_defaults(tac, kw):
    o = R.options(**kw)
    w, s, n = R.sizes(o)
    x = R.waveform(3, R.length_for(4 * frames_per_wave(o) + 1, w, s, o['snip_edges']), seed=11, kw=kw)
    run_and_check(tac, x, kw, R.ident(kw))


def test_snip_edges_false_mirrors_at_both_ends(tac):
    """two lengths whose last frame reads past the end (and whose first reads before the start), and the shortest row covered"""
    kw = dict(snip_edges=False, use_energy=True)
    for length in (400, 1000, 1687):
        m = R.num_frames(length, 400, 160, False)
        last = R.frame_indices(length, 400, 160, m - 1, False)
        assert max(last) == length - 1 and last[-1] < length - 1 and R.frame_indices(length, 400, 160, 0, False)[0] == 119
        run_and_check(tac, R.waveform(3, length, seed=15), kw, 'snip_edges=False n=%d' % length)


def test_subtract_mean_is_a_reduction_after_the_launch(tac):
    x = dev(R.waveform(3, R.length_for(9, 400, 160, True), seed=16))
    before = dict(tac._hip.launches)
    plain = tac.kaldi_fbank(x, use_energy=True)
    sub = tac.kaldi_fbank(x, use_energy=True, subtract_mean=True)
    assert launched_since(tac, before) == {ENTRY: 2}
    R.check_subtracted(sub.cpu().numpy(), plain.cpu().numpy(), 'subtract_mean')


# ----------------------------------------------------------------------------- signals
def test_zero_frame_tiny_frame_and_offset_row(tac):
    x = R.waveform(3, R.length_for(9, 400, 160, True), seed=17)
    x[0, 320:720] = 0.0                                         # frame 2 of row 0 is all zeros
    x[1, 640:1040] *= np.float32(1e-30)                         # frame 4 of row 1 at 1e-30 scale
    assert np.abs(x[2] - 0.5).max() <= 1e-3 + 1e-9              # row 2: an offset of 0.5 under an amplitude of 1e-3
    kw = dict(use_energy=True, energy_floor=0.0)
    got = tac.kaldi_fbank(dev(x), **kw).cpu().numpy()
    assert (got[0, 2] == R.LOG_EPS32).all(), got[0, 2]
    assert (got[1, 4] == R.LOG_EPS32).all(), got[1, 4]
    o = R.options(**kw)
    r = R.reference(x, o)
    res = R.check(got, r, o, 'zero frame, tiny frame, offset row')
    # the offset row alone, so that its own worst ratio is on record
    r2 = R.reference(x[2:], o)
    print('offset row: %r; all rows: %r' % (R.check(got[2:], r2, o, 'offset row'), res))
    floored = tac.kaldi_fbank(dev(x), use_energy=True).cpu().numpy()
    assert floored[0, 2, 0] == 0.0 and floored[1, 4, 0] == 0.0  # energy_floor = 1: log 1


@pytest.mark.parametrize('geo', R.GEOMETRIES[:3], ids=R.ident)
def test_nan_reaches_exactly_the_frames_that_read_it(tac, geo):
    o = R.options(**geo)
    w, s, n = R.sizes(o)
    frames = 2 * frames_per_wave(o) + 1
    length = R.length_for(frames, w, s, True)
    x = R.waveform(2, length, seed=18)
    clean = tac.kaldi_fbank(dev(x), use_energy=True, **geo)
    assert bool(torch.isfinite(clean).all())
    # the sample just before a frame's first; a frame's first and last; one in the overlap of three frames
    for sample in (3 * s - 1, 3 * s, 2 * s + w - 1, 2 * s + w, 0, length - 1):
        y = x.copy()
        y[1, sample] = np.nan
        got = tac.kaldi_fbank(dev(y), use_energy=True, **geo)
        hit = R.frames_reading(length, o, sample)
        bad = ~torch.isfinite(got)
        for t in range(frames):
            assert bool(bad[1, t].all()) == (t in hit) and bool(bad[1, t].any()) == (t in hit), (sample, t, hit)
        assert not bool(bad[0].any())
        keep = [t for t in range(frames) if t not in hit]
        assert torch.equal(got[:, keep], clean[:, keep]) and torch.equal(got[0], clean[0])
    assert 3 not in R.frames_reading(length, o, 3 * s - 1) and 2 in R.frames_reading(length, o, 3 * s - 1)
    for kw in (dict(snip_edges=False),):
        y = x.copy()
        y[1, 0] = np.inf
        got = tac.kaldi_fbank(dev(y), **kw, **geo)
        hit = R.frames_reading(length, R.options(**kw, **geo), 0)
        bad = ~torch.isfinite(got)
        assert [t for t in range(got.shape[1]) if bool(bad[1, t].any())] == hit and not bool(bad[0].any())


# ----------------------------------------------------------------------------- determinism, routing
def test_two_runs_are_bit_identical(tac):
    x = dev(R.waveform(3, R.length_for(33, 400, 160, True), seed=19))
    a = tac.kaldi_fbank(x, num_mel_bins=80, use_energy=True)
    b = tac.kaldi_fbank(x.clone(), num_mel_bins=80, use_energy=True)
    assert torch.equal(a, b)


def test_wrapper_layer_and_half_precision_run_the_kernel(tac):
    x = dev(R.waveform(3, R.length_for(5, 400, 160, True), seed=20))
    before = dict(tac._hip.launches)
    full = tac.kaldi_fbank(x, num_mel_bins=80)
    assert torch.equal(tac.kaldi.fbank(x, num_mel_bins=80, channel=2), full[2])
    assert torch.equal(tac.KaldiFbank(num_mel_bins=80)(x), full)
    half = tac.kaldi_fbank(x.half(), num_mel_bins=80)
    assert half.dtype == torch.float16 and torch.equal(half, tac.kaldi_fbank(x.half().float(), num_mel_bins=80).half())
    assert launched_since(tac, before) == {ENTRY: 5}
    assert tuple(tac.kaldi.fbank(x, min_duration=1.0).shape) == (0, 23) and tuple(tac.kaldi_fbank(x[:, :399]).shape) == (3, 0, 23)
    assert launched_since(tac, before) == {ENTRY: 5}            # empty results launch nothing


COMPOSITE = [('float64', dict(), torch.float64, 1000), ('N=2048', dict(sample_frequency=48000.0), torch.float32, 3000),
             ('no power of two', dict(round_to_power_of_two=False), torch.float32, 1000),
             ('200 bins', dict(num_mel_bins=200), torch.float32, 1000), ('dither', dict(dither=0.5), torch.float32, 1000),
             ('expanded rows', dict(), 'expand', 1000), ('short mirrored row', dict(snip_edges=False), torch.float32, 300)]


@pytest.mark.parametrize('name,kw,dtype,length', COMPOSITE, ids=[c[0] for c in COMPOSITE])
def test_composite_cases_warn_or_raise(tac, name, kw, dtype, length):
    x = R.waveform(2, length, seed=21)
    xd = dev(x)[:1].expand(2, length) if dtype == 'expand' else dev(x).to(dtype)       # (row stride 0: not a positive stride)
    xin = np.repeat(x[:1], 2, 0) if dtype == 'expand' else x
    before = dict(tac._hip.launches)
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.kaldi_fbank(xd, **kw)
    tac.set_strict(False)
    try:
        for key in [k for k in tac._ops._warned if k[0] == 'kaldi_fbank']:
            tac._ops._warned.discard(key)
        with pytest.warns(tac.CompositeRouteWarning):
            got = tac.kaldi_fbank(xd, **kw)
    finally:
        tac.set_strict(True)
    assert launched_since(tac, before) == {}
    o = R.options(**kw)
    r = R.reference(xin, o)
    assert got.dtype == xd.dtype and tuple(got.shape) == (2, r.value.shape[1], r.cols)
    if name == 'float64':
        assert np.abs(got.cpu().numpy() - r.out).max() < 1e-9
    elif name != 'dither':
        R.check(got.cpu().numpy(), r, o, 'stock-torch route, ' + name)
    else:
        assert bool(torch.isfinite(got).all())


def test_backward_is_the_announced_composite_and_matches_float64(tac):
    kw = dict(num_mel_bins=23, use_energy=True)
    x = R.waveform(3, R.length_for(5, 400, 160, True), seed=22)
    g = np.random.default_rng(3).standard_normal((3, 5, 24)).astype(np.float32)
    xd = dev(x).requires_grad_(True)
    before = dict(tac._hip.launches)
    out = tac.kaldi_fbank(xd, **kw)
    assert launched_since(tac, before) == {ENTRY: 1}
    with pytest.raises(RuntimeError, match='strict mode'):
        out.backward(dev(g), retain_graph=True)
    tac.set_strict(True, backward=False)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', tac.CompositeRouteWarning)
            out.backward(dev(g))
    finally:
        tac.set_strict(True)
    want = R.row_gradient(x, R.options(**kw), g)
    got = xd.grad.cpu().numpy().astype(np.float64)
    ratio = np.abs(got - want).max(1) / np.abs(want).max(1)
    print('backward: worst row error / row maximum %.3e' % ratio.max())
    assert (ratio <= GRAD_DB).all(), ratio


# ----------------------------------------------------------------------------- drop-in use
def test_kaldi_fbank_behind_resample_and_preemphasis(tac):
    chain = torch.nn.Sequential(tac.Resample(48000, 16000), tac.Preemphasis(), tac.KaldiFbank(num_mel_bins=80)).to('cuda')
    x = dev(signals.audio_like((2, 3 * (400 + 160 * 8) + 11), seed=23))
    before = dict(tac._hip.launches)
    out = chain(x)
    assert launched_since(tac, before).get(ENTRY) == 1 and type(out) is torch.Tensor
    mid = chain[1](chain[0](x))
    assert tuple(out.shape) == (2, tac._kaldi.num_frames(mid.shape[-1], 400, 160, True), 80) and bool(torch.isfinite(out).all())
    assert torch.equal(out, tac.kaldi_fbank(mid, num_mel_bins=80))
    # (white noise pre-emphasised twice is too tilted for the 99 % condition of the log rule; the values are the kernel's own on
    # the chain's intermediate, and those are held to the rule by every test above)
