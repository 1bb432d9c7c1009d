"""Not gpu: ``detect_pitch_frequency`` / ``PitchFrequency`` on the CPU route (``_composite.detect_pitch_frequency``: the definition in
torch operators), the argument checks, the routing decisions, the plan of the correlation launch and the C entries' refusals.

Reference: tests/pitch_rules.py — the literal restatement with its loop over the lags, which the CPU route has to equal bit for bit
in float32 and float64, and the decision-stability rule, whose share of unstable frames is held to its cap here for the restatement
alone (the GPU tests hold the kernel to the rule)."""
import ctypes
import os

import pytest
import torch

import pitch_rules as R


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    if not os.path.exists(t._native.LIB_PATH):
        t.build_native()
    return t


# ----------------------------------------------------------------------------- the CPU route against the restatement
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_cpu_route_equals_the_restatement(tac, dtype):
    for rate, kw in ((8000, {}), (16000, {}), (8000, dict(frame_time=0.01875, win_length=5, freq_low=85, freq_high=1000))):
        x = R.glide(rate, rows=4, seconds=0.3).to(dtype).reshape(2, 2, -1)
        got = tac.detect_pitch_frequency(x, rate, **kw)
        want = R.restatement(x, rate, **kw)
        geo = R.geometry(x.shape[-1], rate, **kw)
        assert got.dtype == torch.float32 and tuple(got.shape) == (2, 2, geo.n_out) and not got.requires_grad
        assert torch.equal(got, want), (rate, kw)
        one = tac.detect_pitch_frequency(x[0, 1], rate, **kw)
        assert tuple(one.shape) == (geo.n_out,) and torch.equal(one, want[0, 1])
    half = tac.detect_pitch_frequency(R.glide(8000, rows=2, seconds=0.3).half(), 8000)
    assert half.dtype == torch.float32


def test_known_answers(tac):
    for rate, freq in ((16000, 200.0), (8000, 250.0)):
        x = R.tone(rate, freq, rate // 2 + 13).reshape(1, -1)
        got = tac.detect_pitch_frequency(x, rate)
        geo = R.geometry(x.shape[-1], rate)
        lags = R.lags_of(R.nccf_of(x.double(), geo), geo)
        assert bool((lags[:, :-3] == int(rate / freq)).all())               # (the last frames run into the zero padding)
        assert tuple(got.shape) == (1, geo.N - 15) and bool((got == freq).all()), got


def test_output_length_and_lower_median(tac):
    rate = 8000
    x = R.glide(rate, rows=2, seconds=0.3)
    geo = R.geometry(x.shape[-1], rate)
    lags = R.lags_of(R.nccf_of(x, geo), geo)
    for win, n_out in ((1, geo.N), (2, geo.N - 1), (3, geo.N - 1), (30, geo.N - 15), (31, geo.N - 15)):
        got = tac.detect_pitch_frequency(x, rate, win_length=win)
        assert tuple(got.shape) == (2, n_out) == (2, R.geometry(x.shape[-1], rate, win_length=win).n_out)
        assert torch.equal(got, R.smooth(lags, win, rate))
    assert torch.equal(tac.detect_pitch_frequency(x, rate, win_length=1), torch.tensor(8000.0) / lags.float())
    # an even window takes the lower of its two middle lags: the larger of the two frequencies
    table = torch.tensor([[40, 20, 30, 10, 50]])
    assert torch.equal(tac._composite.pitch_smooth(table, 2, 1200), torch.tensor([[60.0, 60.0, 120.0, 120.0]]))
    assert torch.equal(tac._composite.pitch_smooth(table, 4, 1200), torch.tensor([[40.0, 60.0, 60.0]]))   # (40 40 20 30), (40 20 30 10), (20 30 10 50)
    assert torch.equal(R.smooth(table, 4, 1200), tac._composite.pitch_smooth(table, 4, 1200))


def test_argument_errors(tac):
    x = torch.zeros(2, 4000)
    f = tac.detect_pitch_frequency
    bad = (dict(freq_high=170), dict(win_length=0), dict(win_length=-3), dict(win_length=2.0), dict(frame_time=0.0), dict(frame_time=-1e-2),
           dict(freq_low=0), dict(freq_low=-85), dict(freq_high=0), dict(freq_high=float('inf')), dict(win_length=50))
    assert R.geometry(4000, 16000, freq_high=170).lag_min >= R.geometry(4000, 16000).half
    assert R.geometry(4000, 16000, win_length=50).n_out == 0 and R.geometry(4000, 16000, win_length=49).n_out == 1
    for kw in bad:
        with pytest.raises(ValueError):
            f(x, 16000, **kw)
        with pytest.raises(ValueError):
            tac._composite.detect_pitch_frequency(x, 16000, **kw)
        with pytest.raises(ValueError):
            tac._ops.pitch_reason(x, 16000, **kw)
        if kw != dict(win_length=50):
            with pytest.raises(ValueError):
                tac.PitchFrequency(16000, **kw)
    for rate in (0, -16000, 16000.5, True):
        with pytest.raises(ValueError):
            f(x, rate)
        with pytest.raises(ValueError):
            tac.PitchFrequency(rate)
    with pytest.raises(ValueError):
        f(torch.tensor(1.0), 16000)
    with pytest.raises(ValueError):
        f(torch.zeros(2, 0), 16000)
    with pytest.raises(ValueError):
        f(torch.zeros(2, 4000, dtype=torch.int16), 16000)
    with pytest.raises(TypeError):
        f([0.0] * 4000, 16000)
    assert tuple(f(x, 16000, win_length=49).shape) == (2, 1)
    assert tuple(f(torch.zeros(0, 4000), 16000).shape) == (0, 10)


def test_all_zero_frames_take_the_first_lag(tac):
    got = tac.detect_pitch_frequency(torch.zeros(1, 4000), 16000, win_length=3)
    assert bool((got == 16000.0 / (R.geometry(4000, 16000).lag_min + 1)).all())


def test_layer_fake_kernel_and_exports(tac):
    from torch._subclasses.fake_tensor import FakeTensorMode
    args = (8000, 0.01875, 5, 85.0, 1000.0)
    geo = R.geometry(3001, *args)
    with FakeTensorMode() as mode:
        fake = torch.ops.tac_amd.detect_pitch_frequency(mode.from_tensor(torch.zeros(2, 3, 3001, dtype=torch.float64)), *args)
    assert tuple(fake.shape) == (2, 3, geo.n_out) and fake.dtype == torch.float32
    x = R.glide(8000, rows=2, seconds=0.3)
    compiled = torch.compile(lambda w: tac.detect_pitch_frequency(w, *args), backend='eager')
    assert torch.equal(compiled(x), tac.detect_pitch_frequency(x, *args))
    m = tac.PitchFrequency(*args)
    assert m.state_dict() == {} and list(m.named_buffers()) == [] and list(m.parameters()) == []
    assert repr(m) == 'PitchFrequency(sample_rate=8000, frame_time=0.01875, win_length=5, freq_low=85.0, freq_high=1000.0)'
    assert torch.equal(m(x), tac.detect_pitch_frequency(x, *args))
    assert torch.equal(tac.PitchFrequency(8000)(x), tac.detect_pitch_frequency(x, 8000))
    assert 'detect_pitch_frequency' in tac.functional.__all__ and tac.detect_pitch_frequency is tac.functional.detect_pitch_frequency
    assert tac.PitchFrequency is tac.layers.PitchFrequency
    xg = x.clone().requires_grad_(True)
    assert not tac.detect_pitch_frequency(xg, 8000).requires_grad


def test_routing_decisions(tac):
    reason = tac._ops.pitch_reason
    x = torch.zeros(3, 2, 8000)
    for rate in R.RATES:
        assert reason(x, rate) is None
    for rate, ft, lo, hi in R.VARIANTS:
        assert reason(x, rate, ft, 30, lo, hi) is None
    assert reason(x.double(), 16000) == 'dtype float64'
    assert reason(x.half(), 16000) is None and reason(x.bfloat16(), 16000) is None
    assert reason(x[:1].expand(3, 2, 8000), 16000) == 'non-positive strides'
    assert reason(x[:, :1].expand(3, 2, 8000), 16000) == 'non-positive strides'
    assert reason(x.flip(-1), 16000) is None                    # (torch's flip copies: its strides are positive)
    assert reason(x[:, 1:, 3::2], 16000) is None
    assert reason(x, 16000, win_length=R.MAX_WIN) is None and tac._hip.PITCH_MAX_WIN == R.MAX_WIN
    assert reason(torch.zeros(1, 80000), 16000, win_length=R.MAX_WIN + 1) == 'a median window of 65 lags (the kernel takes 64 or fewer)'
    # one frame and its lags beyond 64 KB of LDS: F = 3840, L = 3200 at 192 kHz with 20 ms frames and a 60 Hz floor
    assert reason(torch.zeros(1, 400000), 192000, 0.02, 30, 60, 3400) == \
        'frames of 3840 samples and 3200 lags (beyond the LDS plan of the correlation launch)'
    assert reason(torch.zeros(1, 400000), 192000) is None      # F = 1920, L = 2259


def test_plan_of_the_correlation_launch(tac):
    with open(os.path.join(os.path.dirname(os.path.abspath(tac.__file__)), 'csrc', 'pitch.hip')) as f:
        text = f.read()
    for quote in ('constexpr int PT_THREADS = 256;', 'constexpr int PT_MAX_G = 32;', 'constexpr int PT_MAX_TASKS = 1024;',
                  'constexpr int PT_LDS_BYTES = 64 * 1024;', 'constexpr int PT_MAX_WIN = 64;',
                  'const long long bytes = 8 * span_p + 4 * ((span_x + 3) & ~3LL) + 16LL * G * NH + 8 * PT_WAVES;',
                  'long long per_cu = 160 * 1024 / pl.lds_bytes;', 'per_cu = per_cu > 8 ? 8 : per_cu;',
                  'persistent_blocks(A.units, 1, (long long)device_cu_count() * per_cu)',
                  'for (long long u = blockIdx.x; u < A.units; u += gridDim.x) {'):
        assert quote in text, 'csrc/pitch.hip no longer holds %r: tests/pitch_rules.py restates a launcher that has changed' % quote
    for n_frames in (1, 2, 7, 21, 22, 63, 1000):
        for F, L in list(R.RATES.values()) + [(150, 95), (120, 134), (99, 160), (1920, 2259), (3840, 3200), (1, 4)]:
            want = R.plan(n_frames, F, L)
            got = tac._hip.pitch_plan(n_frames, F, L)
            assert got == (None if want is None else (want[0], want[2])), (n_frames, F, L, got, want)
            if want is not None:
                assert 1 <= want[0] <= min(32, n_frames) and want[2] <= R.LDS_PLAN
    assert R.plan(1000, 160, 189)[:2] == (21, 24) and R.plan(1000, 480, 565)[:2] == (7, 71) and R.plan(1000, 3840, 3200) is None
    for cus in (256, 304):
        units, grid = R.lags_grid(cus, 256, 1000, 160, 189)
        assert units == 256 * 48 and grid == 3 * cus


def test_unstable_frames_stay_under_the_cap():
    """the rule of pitch_rules on the restatement alone: the GPU test's signals leave at most a tenth of their frames to the
    near-maximum check, and the float32 restatement — one more float32 evaluation — passes the rule itself"""
    for rate in sorted(R.RATES):
        x = R.glide(rate)
        verdict = R.judge(x, rate)
        assert (verdict.geo.F, verdict.geo.L) == R.RATES[rate] and x.shape[-1] % verdict.geo.F != 0
        silent = int(verdict.silent.sum())
        print('%d Hz: %d frames, %d silent, %.1f %% of the others unstable' % (rate, verdict.silent.numel(), silent, 100 * verdict.unstable_share))
        assert verdict.unstable_share <= R.UNSTABLE_CAP and silent >= 6 * (verdict.geo.N // 9 - 1)
        lags32 = R.lags_of(R.nccf_of(x, verdict.geo), verdict.geo)
        R.assert_lags(lags32, verdict, 'float32 restatement at %d Hz' % rate)
        for gain in (2.0 ** -12, 2.0 ** 12):
            scaled = R.judge(x * gain, rate)
            both = scaled.stable & verdict.stable
            assert scaled.unstable_share <= R.UNSTABLE_CAP and torch.equal(scaled.lags[both], verdict.lags[both])


def test_c_abi_surface(tac):
    h = tac._native.lib()
    assert h.tac_abi_version() == 5 and h.tac_pitch_max_win() == R.MAX_WIN
    names = ('tac_pitch_max_win', 'tac_pitch_plan', 'tac_pitch_lags_f32', 'tac_pitch_smooth_i32', 'tac_pitch_frequency_f32')
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tac_amd.h')) as f:
        header = f.read()
    for name in names:
        assert name in tac._native.EXPORTS and ' %s(' % name in header
    invalid, unsupported, short = tac._native.TAC_E_INVALID, tac._native.TAC_E_UNSUPPORTED, tac._native.TAC_E_SHORT_INPUT
    one = ctypes.c_void_p(16)
    # argument errors are refused before anything is launched (no device is touched)
    ok = (one, 3, 2, 8000, 16000, 8000, 1, 16000, 160, 189, 5, 30, one, one, None)
    keys = ('waveform', 'n0', 'n1', 'time', 'stride_0', 'stride_1', 'stride_t', 'sample_rate', 'frame', 'max_lag', 'lag_min', 'win_length',
            'lags', 'out', 'stream')

    def call(**change):
        return h.tac_pitch_frequency_f32(*[change.get(n, v) for n, v in zip(keys, ok)])

    for name in ('waveform', 'lags', 'out'):
        assert call(**{name: None}) == invalid, name
    for name in ('n0', 'n1', 'time', 'stride_0', 'stride_1', 'stride_t', 'sample_rate', 'frame', 'max_lag', 'lag_min', 'win_length'):
        assert call(**{name: 0}) == invalid, name
    assert call(stride_1=-8000) == invalid and call(lag_min=94) == invalid and call(lag_min=95) == invalid
    assert call(win_length=65) == unsupported
    assert call(frame=3840, max_lag=3200, time=400000, stride_1=400000, stride_0=800000) == unsupported
    assert call(time=160 * 15, win_length=30) == short and call(time=160 * 14, win_length=29) == short
    assert h.tac_pitch_smooth_i32(one, 3, 50, 65, 16000, one, None) == unsupported
    assert h.tac_pitch_smooth_i32(one, 3, 14, 30, 16000, one, None) == short
    assert h.tac_pitch_smooth_i32(None, 3, 50, 30, 16000, one, None) == invalid
    assert h.tac_pitch_lags_f32(one, 3, 2, 8000, 16000, 8000, 1, 160, 189, 94, one, None) == invalid
