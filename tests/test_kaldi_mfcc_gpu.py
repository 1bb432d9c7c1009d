"""-m gpu: ``kaldi_mfcc`` / ``kaldi_spectrogram`` (layers, ``kaldi.mfcc`` / ``kaldi.spectrogram``) on the gfx950 kernel
(csrc/kaldi_fbank.hip, the MFCC and spectrogram epilogues of the fbank launch) — strict mode and poisoned outputs on, as in
tests/test_kaldi_gpu.py.

References and rules: tests/kaldi_mfcc_rules.py on top of tests/kaldi_rules.py.  That the signals meet the rules' conditions (99 %
of the bins held and the Nyquist bin held in half of the frames; 90 % of the frames with every band held or deep) is established
on the CPU (tests/test_kaldi_mfcc_cpu.py) on the same waveforms: 1 / 3 rows x 13 frames of ``kaldi_rules.waveform``, seed 5, which
is three whole units and a partial one at 4 frames per wave, one and a partial one at 8, six and a half at 2.  128 bins are outside
the MFCC rule and are covered by the exact equalities and the NaN test.

Worst ratios of error to allowance measured on the MI355X: DESIGN 3.16."""
import warnings

import numpy as np
import pytest
import torch

import kaldi_mfcc_rules as MR
import kaldi_rules as R

pytestmark = pytest.mark.gpu

MFCC, SPEC, FBANK = 'tac_kaldi_mfcc_f32', 'tac_kaldi_spectrogram_f32', 'tac_kaldi_fbank_f32'
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


def signal(kw, rows=3, frames=13, seed=5):
    o = R.options(**{k: v for k, v in kw.items() if k in R.DEFAULTS})
    w, s, n = R.sizes(o)
    return R.waveform(rows, R.length_for(frames, w, s, o['snip_edges']), seed=seed, kw=MR.waveform_kw(kw))


_references = {}


def reference(mode, x, kw, key):
    """the float64 reference of one (mode, options, waveform), computed once and shared by the tests that need it"""
    key = (mode, R.ident(kw)) + tuple(key)
    if key not in _references:
        if mode == 'mfcc':
            _references[key] = MR.mfcc_reference(x, MR.mfcc_options(**kw))
        else:
            _references[key] = MR.spectrogram_reference(x, MR.spectrogram_options(**kw))
    return _references[key]


def run_and_check(tac_, mode, x, kw, what, key, xdev=None):
    """one covered call on ``x`` (rows, n): exactly one launch, the result under the rule; returns (result, ratios)"""
    before = dict(tac_._hip.launches)
    fn = tac_.kaldi_mfcc if mode == 'mfcc' else tac_.kaldi_spectrogram
    got = fn(dev(x) if xdev is None else xdev, **kw)
    assert launched_since(tac_, before) == {MFCC if mode == 'mfcc' else SPEC: 1}, launched_since(tac_, before)
    ref = reference(mode, x, kw, key)
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (x.shape[0],) + ref.out.shape[1:]
    if mode == 'mfcc':
        res = MR.check_mfcc(got.cpu().numpy(), ref, MR.mfcc_options(**kw), what)
    else:
        res = MR.check_spectrogram(got.cpu().numpy(), ref, MR.spectrogram_options(**kw), what)
    print('%s %s: %r' % (mode, what, res))
    return got, res


# ----------------------------------------------------------------------------- geometries, rows
@pytest.mark.parametrize('rows', (1, 3))
@pytest.mark.parametrize('geo', R.GEOMETRIES, ids=R.ident)
@pytest.mark.parametrize('mode', ('mfcc', 'spectrogram'))
def test_every_geometry(tac, mode, geo, rows):
    """G = 8 / 4 / 2 frames per wave, odd W, odd S, W = N, and frames staged one by one (S = 2240)"""
    o = R.options(**geo)
    assert R.sizes(o) in ((400, 160, 512), (200, 80, 256), (551, 220, 1024), (400, 161, 512), (512, 160, 512), (400, 2240, 512))
    run_and_check(tac, mode, signal(geo, rows=rows), geo, '%s rows=%d' % (R.ident(geo), rows), (rows, 13))


@pytest.mark.parametrize('mode,kw', [('mfcc', dict(num_mel_bins=40, num_ceps=20)), ('spectrogram', dict())], ids=('mfcc', 'spectrogram'))
def test_more_units_than_the_grid_has_waves(tac, mode, kw):
    """96 rows of 120 frames: 2880 units of four frames, more than two workgroups of four waves on each of 256 compute units —
    every wave walks its loop more than once.  The rows repeat three checked ones and must repeat their bits."""
    fn = tac.kaldi_mfcc if mode == 'mfcc' else tac.kaldi_spectrogram
    base = R.waveform(3, R.length_for(120, 400, 160, True), seed=12)
    small = fn(dev(base), **kw)
    few = np.ascontiguousarray(base[:, :R.length_for(9, 400, 160, True)])
    got, _ = run_and_check(tac, mode, few, kw, 'three rows of the batch, nine frames', ('batch', 9))
    assert torch.equal(small[:, :9], got)                       # a frame depends on its own samples only
    big = fn(dev(np.tile(base, (32, 1))), **kw)
    cols = small.shape[-1]
    assert tuple(big.shape) == (96, 120, cols)
    assert torch.equal(big.reshape(32, 3, 120, cols), small[None].expand(32, 3, 120, cols))


@pytest.mark.parametrize('mode,kw', [('mfcc', dict(use_energy=True)), ('spectrogram', dict())], ids=('mfcc', 'spectrogram'))
def test_misaligned_rows_padded_stride_and_leading_dims(tac, mode, kw):
    fn = tac.kaldi_mfcc if mode == 'mfcc' else tac.kaldi_spectrogram
    x = signal(dict(), frames=6, seed=13)
    n = x.shape[1]
    store = torch.full((3, n + 6), float('nan'), device='cuda')
    store[:, 1:n + 1] = dev(x)
    view = store[:, 1:n + 1]                                    # rows start 4 bytes off a 16-byte line, stride n + 6
    assert view.stride() == (n + 6, 1) and view.data_ptr() % 8 == 4
    got, _ = run_and_check(tac, mode, x, kw, 'misaligned rows', (3, 6, 13), xdev=view)
    plain = fn(dev(x), **kw)
    assert torch.equal(plain, got)
    lead = fn(dev(x).reshape(3, 1, n).expand(3, 2, n)[:, :1], **kw)
    assert tuple(lead.shape) == (3, 1, 6, plain.shape[-1]) and torch.equal(lead[:, 0], plain)
    sliced = fn(dev(np.repeat(x, 2, axis=1))[:, ::2], **kw)       # a strided time axis is copied by the route
    assert torch.equal(sliced, plain)


# ----------------------------------------------------------------------------- options
@pytest.mark.parametrize('kw', MR.MFCC_OPTIONS, ids=R.ident)
def test_every_mfcc_option_against_the_defaults(tac, kw):
    run_and_check(tac, 'mfcc', signal(kw), kw, R.ident(kw), (3, 13))


def test_mfcc_80_bins_40_coefficients(tac):
    """three coefficients per lane: the chunks of two and of one; on the two rows without the offset row"""
    kw = MR.MFCC_TWO_ROWS
    _, res = run_and_check(tac, 'mfcc', signal(kw, rows=2), kw, '80 / 40', (2, 13))
    assert res['frames'] == 1.0


@pytest.mark.parametrize('kw', [dict(num_mel_bins=80, num_ceps=70, sample_frequency=8000.0), dict(num_mel_bins=40, num_ceps=33, sample_frequency=8000.0)],
                         ids=R.ident)
def test_mfcc_more_than_four_coefficients_per_lane(tac, kw):
    """8 lanes per frame at N = 256: 70 coefficients are two chunks of four and one of one, the last with lanes past the end;
    33 are one chunk of four and one of one"""
    run_and_check(tac, 'mfcc', signal(kw, rows=2), kw, R.ident(kw), (2, 13))


@pytest.mark.parametrize('kw', MR.SPECTROGRAM_OPTIONS, ids=R.ident)
def test_every_spectrogram_option_against_the_defaults(tac, kw):
    run_and_check(tac, 'spectrogram', signal(kw), kw, R.ident(kw), (3, 13))


def test_subtract_mean_is_a_reduction_after_the_launch(tac):
    x = dev(signal(dict(), frames=9, seed=16))
    for fn, entry, kw in ((tac.kaldi_mfcc, MFCC, dict(use_energy=True)), (tac.kaldi_spectrogram, SPEC, dict())):
        before = dict(tac._hip.launches)
        plain = fn(x, **kw)
        sub = fn(x, subtract_mean=True, **kw)
        assert launched_since(tac, before) == {entry: 2}
        R.check_subtracted(sub.cpu().numpy(), plain.cpu().numpy(), 'subtract_mean ' + entry)


# ----------------------------------------------------------------------------- exact equalities
@pytest.mark.parametrize('geo', R.GEOMETRIES[:3], ids=R.ident)
def test_energy_columns_are_the_fbank_energy_bit_for_bit(tac, geo):
    x = dev(signal(geo))
    for extra in (dict(), dict(raw_energy=False), dict(energy_floor=0.0), dict(snip_edges=False)):
        kw = dict(geo, **extra)
        energy = tac.kaldi_fbank(x, use_energy=True, **kw)[..., 0]
        assert torch.equal(tac.kaldi_mfcc(x, use_energy=True, **kw)[..., 0], energy)
        assert torch.equal(tac.kaldi_mfcc(x, use_energy=True, htk_compat=True, **kw)[..., -1], energy)
        assert torch.equal(tac.kaldi_mfcc(x, use_energy=True, num_mel_bins=128, num_ceps=40, **kw)[..., 0], energy)
        assert torch.equal(tac.kaldi_spectrogram(x, **kw)[..., 0], energy)


def test_options_move_columns_and_nothing_else(tac):
    """the energy replaces C0 and only C0; HTK rotates; the table carries the sqrt 2 — every other column keeps its bits"""
    x = dev(signal(dict()))
    for bins, ceps in ((23, 13), (128, 40)):
        kw = dict(num_mel_bins=bins, num_ceps=ceps)
        plain = tac.kaldi_mfcc(x, **kw)
        with_e = tac.kaldi_mfcc(x, use_energy=True, **kw)
        htk = tac.kaldi_mfcc(x, htk_compat=True, **kw)
        htk_e = tac.kaldi_mfcc(x, htk_compat=True, use_energy=True, **kw)
        assert torch.equal(with_e[..., 1:], plain[..., 1:]) and torch.equal(htk[..., :-1], plain[..., 1:])
        assert torch.equal(htk_e[..., :-1], plain[..., 1:]) and torch.equal(htk_e[..., -1], with_e[..., 0])
        # the same chain against a column rounded from sqrt 2 D: both within (M + 2) u of the sum of their terms' magnitudes
        logmel = tac.kaldi_fbank(x, num_mel_bins=bins).double()
        allow = 2.0 ** 0.5 * (2 * (bins + 2) * R.U * logmel.abs().sum(-1) / bins ** 0.5 + 2 * R.U * plain[..., 0].double().abs())
        assert bool(((htk[..., -1].double() - 2.0 ** 0.5 * plain[..., 0].double()).abs() <= allow).all())
        assert torch.equal(tac.kaldi_mfcc(x, num_mel_bins=bins, num_ceps=5), plain[..., :5])       # a chain per coefficient


@pytest.mark.parametrize('mode,kw', [('mfcc', dict(num_mel_bins=80, num_ceps=40, use_energy=True)), ('mfcc', dict(num_mel_bins=128, htk_compat=True)),
                                     ('spectrogram', dict())], ids=('mfcc-80-40', 'mfcc-128', 'spectrogram'))
def test_two_runs_are_bit_identical(tac, mode, kw):
    fn = tac.kaldi_mfcc if mode == 'mfcc' else tac.kaldi_spectrogram
    x = dev(R.waveform(3, R.length_for(33, 400, 160, True), seed=19))
    assert torch.equal(fn(x, **kw), fn(x.clone(), **kw))


def test_fbank_launch_is_untouched_by_the_new_modes(tac):
    """``tac_kaldi_fbank_f32`` before and after runs of the new modes in one process: the same bits; and the log-mel rows
    under the rule they were merged with"""
    x = signal(dict())
    xd = dev(x)
    before = dict(tac._hip.launches)
    first = tac.kaldi_fbank(xd)
    first_e = tac.kaldi_fbank(xd, num_mel_bins=80, use_energy=True)
    tac.kaldi_mfcc(xd, num_mel_bins=80, num_ceps=40)
    tac.kaldi_spectrogram(xd)
    tac.kaldi_mfcc(xd, use_energy=True, htk_compat=True)
    assert torch.equal(tac.kaldi_fbank(xd), first) and torch.equal(tac.kaldi_fbank(xd, num_mel_bins=80, use_energy=True), first_e)
    assert launched_since(tac, before) == {FBANK: 4, MFCC: 2, SPEC: 1}
    o = R.options()
    R.check(first.cpu().numpy(), R.reference(x, o), o, 'fbank beside the new modes')


# ----------------------------------------------------------------------------- signals
CASES_NAN = [('mfcc', dict()), ('mfcc', dict(num_mel_bins=128, num_ceps=40)), ('mfcc', dict(use_energy=True, htk_compat=True)),
             ('mfcc', dict(sample_frequency=8000.0, num_mel_bins=128, num_ceps=128 // 4)), ('spectrogram', dict()),
             ('spectrogram', dict(sample_frequency=22050.0))]


@pytest.mark.parametrize('mode,kw', CASES_NAN, ids=[m + '-' + R.ident(k) for m, k in CASES_NAN])
def test_nan_reaches_exactly_the_frames_that_read_it(tac, mode, kw):
    fn = tac.kaldi_mfcc if mode == 'mfcc' else tac.kaldi_spectrogram
    o = R.options(**{k: v for k, v in kw.items() if k in R.DEFAULTS})
    w, s, n = R.sizes(o)
    frames = 2 * (64 // (n // 32)) + 1
    length = R.length_for(frames, w, s, True)
    x = R.waveform(2, length, seed=18)
    clean = fn(dev(x), **kw)
    assert bool(torch.isfinite(clean).all())
    # the sample just before a frame's first; a frame's first and last; one past it; the row's first and last
    for sample in (3 * s - 1, 3 * s, 2 * s + w - 1, 2 * s + w, 0, length - 1):
        y = x.copy()
        y[1, sample] = np.nan
        got = fn(dev(y), **kw)
        hit = R.frames_reading(length, o, sample)
        bad = ~torch.isfinite(got)
        for t in range(frames):
            assert bool(bad[1, t].all()) == (t in hit) and bool(bad[1, t].any()) == (t in hit), (sample, t, hit)
        assert not bool(bad[0].any())
        keep = [t for t in range(frames) if t not in hit]
        assert torch.equal(got[:, keep], clean[:, keep]) and torch.equal(got[0], clean[0])
    y = x.copy()
    y[1, 0] = np.nan
    got = fn(dev(y), snip_edges=False, **kw)
    hit = R.frames_reading(length, dict(o, snip_edges=False), 0)
    bad = ~torch.isfinite(got)
    assert [t for t in range(got.shape[1]) if bool(bad[1, t].any())] == hit and not bool(bad[0].any())
    assert all(bool(bad[1, t].all()) for t in hit)


def test_zero_frame_and_tiny_frame(tac):
    """an all-zero frame and one at 1e-30 scale: log eps in every spectrogram bin and in the energy; a constant log-mel row
    log eps in the cepstrum — C0 = sqrt(M) log eps within the chain's roundings, zeros elsewhere within them"""
    x = signal(dict(), frames=9, seed=17)
    x[0, 320:720] = 0.0                                         # frame 2 of row 0 is all zeros
    x[1, 640:1040] *= np.float32(1e-30)                         # frame 4 of row 1 at 1e-30 scale
    spec = tac.kaldi_spectrogram(dev(x), energy_floor=0.0).cpu().numpy()
    assert (spec[0, 2] == R.LOG_EPS32).all() and (spec[1, 4] == R.LOG_EPS32).all()
    assert tac.kaldi_spectrogram(dev(x)).cpu().numpy()[0, 2, 0] == 0.0           # energy_floor = 1: log 1
    ceps = tac.kaldi_mfcc(dev(x), cepstral_lifter=0.0).cpu().numpy().astype(np.float64)
    for row, t in ((0, 2), (1, 4)):
        want = np.zeros(13)
        want[0] = np.sqrt(23.0) * float(R.LOG_EPS32)
        allow = (23 + 2) * R.U * np.abs(MR.dct64(23, 13) * float(R.LOG_EPS32)).sum(0) + 2 * R.U * np.abs(want)
        assert (np.abs(ceps[row, t] - want) <= allow).all(), (row, t, ceps[row, t])


# ----------------------------------------------------------------------------- routing
def test_wrappers_layers_and_half_precision_run_the_kernel(tac):
    x = dev(signal(dict(), frames=5, seed=20))
    before = dict(tac._hip.launches)
    full = tac.kaldi_mfcc(x, num_mel_bins=40, num_ceps=20)
    assert torch.equal(tac.kaldi.mfcc(x, num_mel_bins=40, num_ceps=20, channel=2), full[2])
    assert torch.equal(tac.KaldiMfcc(num_mel_bins=40, num_ceps=20)(x), full)
    half = tac.kaldi_mfcc(x.half(), num_mel_bins=40, num_ceps=20)
    assert half.dtype == torch.float16 and torch.equal(half, tac.kaldi_mfcc(x.half().float(), num_mel_bins=40, num_ceps=20).half())
    assert launched_since(tac, before) == {MFCC: 5}
    spec = tac.kaldi_spectrogram(x)
    assert torch.equal(tac.kaldi.spectrogram(x, channel=1), spec[1]) and torch.equal(tac.KaldiSpectrogram()(x), spec)
    assert launched_since(tac, before) == {MFCC: 5, SPEC: 3}
    assert tuple(tac.kaldi.mfcc(x, min_duration=1.0).shape) == (0, 13) and tuple(tac.kaldi_mfcc(x[:, :399]).shape) == (3, 0, 13)
    assert tuple(tac.kaldi.spectrogram(x, min_duration=1.0).shape) == (0, 257) and tuple(tac.kaldi_spectrogram(x[:, :399]).shape) == (3, 0, 257)
    assert launched_since(tac, before) == {MFCC: 5, SPEC: 3}    # empty results launch nothing


COMPOSITE = [('mfcc', 'float64', dict(), torch.float64, 1000), ('mfcc', 'N=2048', dict(sample_frequency=48000.0), torch.float32, 3000),
             ('mfcc', 'dither', dict(dither=0.5), torch.float32, 1000),
             ('mfcc', 'table 80 x 80', dict(num_mel_bins=80, num_ceps=80), torch.float32, 1000),
             ('mfcc', '200 bins', dict(num_mel_bins=200), torch.float32, 1000),
             ('spectrogram', 'float64', dict(), torch.float64, 1000), ('spectrogram', 'N=2048', dict(sample_frequency=48000.0), torch.float32, 3000),
             ('spectrogram', 'dither', dict(dither=0.5), torch.float32, 1000),
             ('spectrogram', 'short mirrored row', dict(snip_edges=False), torch.float32, 300)]


@pytest.mark.parametrize('mode,name,kw,dtype,length', COMPOSITE, ids=[c[0] + '-' + c[1] for c in COMPOSITE])
def test_composite_cases_warn_or_raise(tac, mode, name, kw, dtype, length):
    fn = tac.kaldi_mfcc if mode == 'mfcc' else tac.kaldi_spectrogram
    op = 'kaldi_' + mode
    x = R.waveform(2, length, seed=21)
    xd = dev(x).to(dtype)
    before = dict(tac._hip.launches)
    with pytest.raises(RuntimeError, match='strict mode'):
        fn(xd, **kw)
    tac.set_strict(False)
    try:
        for key in [k for k in tac._ops._warned if k[0] == op]:
            tac._ops._warned.discard(key)
        with pytest.warns(tac.CompositeRouteWarning):
            got = fn(xd, **kw)
    finally:
        tac.set_strict(True)
    assert launched_since(tac, before) == {}
    if mode == 'mfcc':
        o = MR.mfcc_options(**kw)
        ref = MR.mfcc_reference(x, o)
    else:
        o = MR.spectrogram_options(**kw)
        ref = MR.spectrogram_reference(x, o)
    assert got.dtype == xd.dtype and tuple(got.shape) == ref.out.shape
    if name == 'float64':
        assert np.abs(got.cpu().numpy() - ref.out).max() < 1e-9
    elif name == 'dither':
        assert bool(torch.isfinite(got).all())
    elif mode == 'mfcc':
        MR.check_mfcc(got.cpu().numpy(), ref, o, 'stock-torch route, ' + name)
    else:
        MR.check_spectrogram(got.cpu().numpy(), ref, o, 'stock-torch route, ' + name)


@pytest.mark.parametrize('mode,kw,cols', [('mfcc', dict(use_energy=True, htk_compat=True), 13), ('spectrogram', dict(), 257)],
                         ids=('mfcc', 'spectrogram'))
def test_backward_is_the_announced_composite_and_matches_float64(tac, mode, kw, cols):
    fn = tac.kaldi_mfcc if mode == 'mfcc' else tac.kaldi_spectrogram
    x = signal(dict(), rows=2, frames=5, seed=22)
    g = np.random.default_rng(3).standard_normal((2, 5, cols)).astype(np.float32)
    xd = dev(x).requires_grad_(True)
    before = dict(tac._hip.launches)
    out = fn(xd, **kw)
    assert launched_since(tac, before) == {MFCC if mode == 'mfcc' else SPEC: 1}
    with pytest.raises(RuntimeError, match='strict mode'):
        out.backward(dev(g), retain_graph=True)
    tac.set_strict(True, backward=False)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', tac.CompositeRouteWarning)
            out.backward(dev(g))
    finally:
        tac.set_strict(True)
    o = MR.mfcc_options(**kw) if mode == 'mfcc' else MR.spectrogram_options(**kw)
    want = MR.row_gradient(x, o, g, mode)
    got = xd.grad.cpu().numpy().astype(np.float64)
    ratio = np.abs(got - want).max(1) / np.abs(want).max(1)
    print('%s backward: worst row error / row maximum %.3e' % (mode, ratio.max()))
    assert (ratio <= GRAD_DB).all(), ratio
