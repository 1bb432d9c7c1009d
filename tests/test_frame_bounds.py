"""CPU: the per-frame comparison helpers of tests/frame_bounds.py catch the perturbations a per-tensor bound lets through,
and the poison fill / detection helpers of the HIP launchers work on CPU tensors."""
import math

import numpy as np
import pytest
import torch

import frame_bounds as fbnd
from conftest import rel_err

TIGHT = 2e-6        # STFT and |X|, per frame
MEL = 2e-5          # power and mel, per frame


@pytest.fixture(scope='module')
def H():
    import torchaudio_contrib_amd as t
    return t._hip


def _spec(seed=0, rows=6, n_bins=65, n_frames=40):
    """(rows, F, T) magnitudes with row gains 2^0 ... 2^-12 (row 3 is the 2^-12 one) and one silent frame in row 4."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(rows, n_bins, n_frames, generator=g, dtype=torch.float64) + 0.05
    gains = torch.tensor([1.0, 0.5, 2.0 ** -5, 2.0 ** -12, 0.25, 2.0 ** -7][:rows], dtype=torch.float64)
    x = x * gains[:, None, None]
    x[4, :, 17] = 0.0
    return x


def test_unperturbed_passes():
    ref = _spec()
    got = ref.float()
    assert fbnd.assert_linear(fbnd.frames_of(got, 'spec'), fbnd.frames_of(ref, 'spec'), TIGHT, 'same') < 1e-7


def test_quiet_row_frame_scaled_is_caught_per_frame_not_per_tensor():
    ref = _spec()
    got = ref.clone()
    got[3, :, 11] *= 1 + 1e-5
    assert rel_err(got.numpy(), ref.numpy()) < TIGHT            # what the per-tensor bound lets through
    with pytest.raises(AssertionError, match='row 3 frame 11'):
        fbnd.assert_linear(fbnd.frames_of(got, 'spec'), fbnd.frames_of(ref, 'spec'), TIGHT, 'scaled')


def test_middle_row_shifted_by_one_frame_is_caught():
    ref = _spec()
    got = ref.clone()
    got[2] = torch.roll(ref[2], 1, dims=-1)
    with pytest.raises(AssertionError, match='worst row 2'):
        fbnd.assert_linear(fbnd.frames_of(got, 'spec'), fbnd.frames_of(ref, 'spec'), MEL, 'shifted')


def test_poisoned_tile_is_caught(H):
    ref = _spec().float()
    got = ref.clone()
    H.poison_fill(got[1, 16:32, 8:16])
    assert int(H.poison_count(got)) == 16 * 8
    with pytest.raises(AssertionError, match='row 1 frame 8'):
        fbnd.assert_linear(fbnd.frames_of(got, 'spec'), fbnd.frames_of(ref, 'spec'), MEL, 'poisoned')


def test_complex_layout_and_nan():
    g = torch.Generator().manual_seed(1)
    ref = torch.randn(3, 33, 10, 2, generator=g, dtype=torch.float64)
    got = ref.clone()
    assert fbnd.assert_linear(fbnd.frames_of(got, 'complex'), fbnd.frames_of(ref, 'complex'), TIGHT) == 0.0
    got[2, 5, 7, 1] = float('nan')
    with pytest.raises(AssertionError, match='row 2 frame 7'):
        fbnd.assert_linear(fbnd.frames_of(got, 'complex'), fbnd.frames_of(ref, 'complex'), TIGHT, 'nan')


def test_silent_frame_must_be_exactly_zero():
    ref = _spec()
    got = ref.clone()
    assert fbnd.assert_linear(fbnd.frames_of(got, 'spec'), fbnd.frames_of(ref, 'spec'), MEL) < 1e-12
    got[4, 9, 17] = 1e-30
    with pytest.raises(AssertionError, match='row 4 frame 17'):
        fbnd.assert_linear(fbnd.frames_of(got, 'spec'), fbnd.frames_of(ref, 'spec'), MEL, 'silent')


def _db_case():
    """mel-like values of a white spectrum (flat within a frame, +-20 %), a few rows deep under the 1e-7 clamp of v^2."""
    g = torch.Generator().manual_seed(2)
    v = (0.8 + 0.4 * torch.rand(5, 30, 64, generator=g, dtype=torch.float64))
    v = v * torch.tensor([1.0, 1e-2, 2.0 ** -12, 1e-5, 1e-6], dtype=torch.float64)[:, None, None]
    return v                                                    # frames layout (rows, T, M)


def test_db_exact_passes_and_keeps_the_elements_above_the_clamp():
    v = _db_case()
    worst, kept, cdev = fbnd.assert_db(fbnd.db_of(v).float(), v, MEL, what='exact')
    assert worst < 1e-4 and kept >= 0.99 and cdev < 1e-5


def test_db_element_off_by_2e_3_is_caught():
    v = _db_case()
    got = fbnd.db_of(v)
    got[1, 7, 30] += 2e-3
    with pytest.raises(AssertionError, match='row 1 frame 7'):
        fbnd.assert_db(got, v, MEL, what='dB')


def test_db_clamp_value_and_poison_are_checked(H):
    v = _db_case()
    got = fbnd.db_of(v)
    got[4, 3, 3] += 1e-3                                        # row 4: v^2 ~ 1e-12, deep under the clamp
    with pytest.raises(AssertionError, match='clamp value; row 4 frame 3'):
        fbnd.assert_db(got, v, MEL, what='clamp')
    got = fbnd.db_of(v).float()
    H.poison_fill(got[0, 2])
    with pytest.raises(AssertionError, match='non-finite'):
        fbnd.assert_db(got, v, MEL, what='poison')


def test_db_mask_cannot_swallow_the_check():
    """Values spread over many decades inside a frame: most fall outside the derived mask, and the check says so."""
    g = torch.Generator().manual_seed(3)
    v = 10.0 ** (-3.0 * torch.rand(2, 8, 64, generator=g, dtype=torch.float64))
    with pytest.raises(AssertionError, match='keeps only'):
        fbnd.assert_db(fbnd.db_of(v), v, MEL, what='spread')


def test_row_bound_for_gradients():
    g = torch.Generator().manual_seed(4)
    ref = torch.randn(4, 1000, generator=g, dtype=torch.float64) * torch.tensor([1, 2.0 ** -12, 1, 1.0])[:, None]
    got = ref.clone()
    assert fbnd.assert_rows(got, ref, 1e-4) == 0.0
    got[1, 500] += 2e-4 * ref[1].abs().max()
    assert rel_err(got.numpy(), ref.numpy()) < 1e-4
    with pytest.raises(AssertionError, match='worst row 1'):
        fbnd.assert_rows(got, ref, 1e-4, 'grad')


def test_poison_patterns_on_cpu(H):
    for dtype, bits in ((torch.float32, 0x7FC0DEAD), (torch.float64, 0x7FF80000DEADBEEF)):
        t = H.poison_fill(torch.empty(7, 5, dtype=dtype))
        assert bool(torch.isnan(t).all())                       # a quiet NaN: any comparison that reads it fails
        iv = torch.int32 if dtype == torch.float32 else torch.int64
        assert bool((t.view(iv) == bits).all())
        assert int(H.poison_count(t)) == 35
        t[3, 1] = float('nan')                                  # the canonical NaN a kernel may produce is not the pattern
        t[0, 0] = 0.0
        assert int(H.poison_count(t)) == 33
    codes = H.poison_fill(torch.empty(100, dtype=torch.int64))
    assert bool((codes < 0).all()) and int(H.poison_count(codes)) == 100
    codes[:60] = torch.arange(60)
    assert int(H.poison_count(codes)) == 40
    assert int(H.poison_count(torch.empty(0))) == 0


def test_poisoned_allocation_and_write_check_on_cpu(H):
    assert not H.POISON_OUTPUTS
    try:
        H.set_poison_outputs(True)
        H.poison_report()
        out = H._empty((4, 6))
        assert int(H.poison_count(out)) == 24
        strided = H._empty_strided((3, 4), (1, 3))
        assert int(H.poison_count(strided)) == 12 and strided.stride() == (1, 3)
        out[:3] = 1.0                                           # a "launch" that leaves the last row
        H.check_written('cpu_selftest', out)
        H.check_written('cpu_selftest', out[:3])                # (a slice that was filled adds nothing)
        assert H.poison_report() == {'cpu_selftest': 6}
        assert H.poison_report() == {}                          # (read and reset)
    finally:
        H.set_poison_outputs(False)
    plain = H._empty((1000,))
    H.check_written('cpu_selftest', H.poison_fill(plain))       # switched off: nothing is counted
    assert H.poison_report() == {}
    assert math.isnan(float(H.poison_fill(torch.empty(1))[0]))
    assert np.isnan(H.poison_fill(torch.empty(3, dtype=torch.float64)).numpy()).all()


# ------------------------------------------------------------------ inputs and helpers of the route-diverse tests
from oracle import numpy_ref, signals                                           # noqa: E402


def test_gained_with_silence_is_reproducible_and_laid_out_as_documented():
    shape, n, hop = (2, 3, 5000), 256, 100
    x = signals.gained_with_silence(shape, 7, n, hop)
    assert x.dtype == np.float32 and x.shape == shape
    assert np.array_equal(x, signals.gained_with_silence(shape, 7, n, hop))
    assert not np.array_equal(x, signals.gained_with_silence(shape, 8, n, hop))
    rows, base = x.reshape(6, -1), signals.uniform(shape, 7).reshape(6, -1)
    assert not rows[1].any()                                                    # the silent row
    zero = np.zeros(rows.shape, dtype=bool)
    for r, lo, hi in signals.silent_spans(shape, n, hop):
        assert r % 3 == 0 and hi - lo == n + hop
        zero[r, lo:hi] = True
    spans = signals.silent_spans(shape, n, hop)
    assert sorted(lo for r, lo, _ in spans if r == 0) == [0, 2500 + 33, 5000 - 356]
    assert [r for r, _, _ in spans] == [0, 0, 0, 3, 3, 3]
    for r in (0, 2, 3, 4, 5):                                                   # exact gains elsewhere
        keep = ~zero[r]
        assert np.array_equal(rows[r][keep], base[r][keep] * np.float32(2.0 ** -r)) and not rows[r][zero[r]].any()
    g = signals.gained_with_silence((15, 40), 1, 4, 2).reshape(15, -1)          # gains wrap after 2^-12
    assert np.array_equal(g[13], signals.uniform((15, 40), 1).reshape(15, -1)[13])
    assert signals.silent_spans((1, 600), 256, 100) == [] and not signals.has_silence((1, 600), 256, 100)
    assert len(signals.silent_spans((1, 800), 256, 100)) == 2 and signals.has_silence((3, 10), 256, 100)


@pytest.mark.parametrize('center', [True, False])
@pytest.mark.parametrize('pad_mode', ['reflect', 'constant', 'replicate', 'circular'])
@pytest.mark.parametrize('n,hop', [(256, 64), (400, 160), (512, 500), (64, 7)])
def test_generated_spans_give_exactly_silent_frames(n, hop, pad_mode, center):
    """The premise of the silence checks: the oracle's STFT of a generated row is exactly zero on a frame inside each span,
    and on the first and last frames for every pad mode."""
    length = 3 * (n + hop) + 41
    x = signals.gained_with_silence((4, length), 2, n, hop)
    z = numpy_ref.stft(x, n, hop, center=center, pad_mode=pad_mode)            # (4, F, T)
    silent = ~np.abs(z).any(axis=1)
    assert silent[1].all() and not silent[2].any()
    for r in (0, 3):
        assert silent[r, 0] and silent[r, -1]
        for _, lo, hi in [s for s in signals.silent_spans(x.shape, n, hop) if s[0] == r]:
            off = n // 2 if center else 0
            inside = [t for t in range(z.shape[-1]) if lo <= t * hop - off and t * hop - off + n <= hi]
            assert inside and all(silent[r, t] for t in inside), (r, lo, hi)


def test_power_linear_bound_is_the_documented_bound():
    g = torch.Generator().manual_seed(5)
    mag = torch.rand(3, 7, 33, generator=g, dtype=torch.float64) * 2.0
    mag[0, 0, :5] = 0.0
    tol = 1e-3
    e = tol * mag.amax(-1, keepdim=True)
    for p in (1.0, 2.0, 0.7, 3.0):
        b = fbnd.power_linear_bound(mag, p, tol)
        assert bool(torch.isfinite(b).all()) and bool((b >= 0).all())
        for s in (-1.0, -0.5, 0.5, 1.0):                                        # |X| perturbed within e: |X|^p within b
            pert = (mag + s * e).clamp(min=0)
            assert bool(((pert ** p - mag ** p).abs() <= b * (1 + 1e-12)).all()), (p, s)
        first = p * mag.clamp(min=1e-300) ** (p - 1) * e                        # first order away from 0
        far = mag > 100 * e
        assert float(((b - first).abs() / first)[far].max()) < 0.02 * abs(p - 1) + 1e-12, p
        assert torch.allclose(b[0, 0, :5], e[0, 0, 0].expand(5) ** p)          # e^p at |X| = 0
    cplx = torch.complex(mag, torch.zeros_like(mag))
    assert torch.equal(fbnd.power_linear_bound(cplx, 2.0, tol), fbnd.power_linear_bound(mag, 2.0, tol))


def test_db_error_of_1e_3_in_a_quiet_bin_is_caught_with_the_power_bound():
    g = torch.Generator().manual_seed(6)
    mag = (0.5 + torch.rand(4, 20, 129, generator=g, dtype=torch.float64)) * torch.tensor([1.0, 2.0 ** -5, 2.0 ** -12, 0.1],
                                                                                          dtype=torch.float64)[:, None, None]
    for p in (1.0, 2.0, 0.7):
        v = mag ** p
        lin = fbnd.power_linear_bound(mag, p, TIGHT)
        got = fbnd.db_of(v, amin=1e-10)
        worst, kept, _ = fbnd.assert_db(got.float(), v, None, amin=1e-10, lin=lin, what='exact')
        assert worst < 1e-4 and kept >= 0.99
        got[2, 13, 77] += 1.05e-3                                              # the 2^-12 row: a quiet bin
        with pytest.raises(AssertionError, match='row 2 frame 13'):
            fbnd.assert_db(got, v, None, amin=1e-10, lin=lin, what='quiet')


def test_planted_error_in_the_quiet_row_passes_per_tensor_and_fails_per_frame():
    """The gap the route-diverse ports close: one frame of the 2^-12 row off by 1e-4 of that row's scale."""
    n, hop = 256, 64
    x = signals.gained_with_silence((13, 4000), 9, n, hop)
    ref = numpy_ref.stft(x, n, hop)                                             # complex128 (13, F, T)
    got = np.stack([ref.real, ref.imag], -1).astype(np.float32)
    got[12, :, 21, 0] += np.float32(1e-4 * np.abs(ref[12]).max())
    assert rel_err(got[..., 0] + 1j * got[..., 1], ref) < 5e-6
    with pytest.raises(AssertionError, match='row 12 frame 21'):
        fbnd.check_frames(got, ref, 'complex', TIGHT, 'planted', 0, n, silence=True)
    fbnd.check_frames(np.stack([ref.real, ref.imag], -1).astype(np.float32), ref, 'complex', TIGHT, 'clean', 0, n, silence=True)


def test_report_lines(tmp_path, monkeypatch):
    path = tmp_path / 'r.jsonl'
    monkeypatch.setenv('TAC_FUZZ_REPORT', str(path))
    ref = _spec()
    fbnd.check_frames(ref.float().numpy(), ref.numpy(), 'spec', MEL, 'unit', ('a', 1), 128, silence=True)
    v = _db_case().transpose(1, 2)                                              # (rows, M, T)
    fbnd.check_db(fbnd.db_of(v).numpy(), v.numpy(), 'unit', 'b', 128, tol=MEL, kind='db')
    fbnd.check_rows(ref[:, 0].numpy(), ref[:, 0], 1e-4, 'unit', 'c', 128)
    import json
    lines = [json.loads(s) for s in path.read_text().splitlines()]
    assert [l['kind'] for l in lines] == ['spec', 'db', 'grad'] and lines[0]['silent'] == 1
    assert lines[0]['test'] == 'unit' and lines[0]['fft_length'] == 128 and lines[1]['kept'] >= 0.99


def test_interior_frames_and_keep_floors():
    n, hop = 256, 64
    x = signals.gained_with_silence((4, 3000), 3, n, hop)
    inner = fbnd.interior_frames(x, n, hop, center=True)
    assert tuple(inner.shape) == (4, 1 + 3000 // hop)
    assert not bool(inner[1].any())                                             # the silent row
    assert not bool(inner[:, :2].any()) and not bool(inner[:, -2:].any())       # frames that read the padding
    starts = torch.arange(inner.shape[1]) * hop - n // 2
    for _, lo, hi in [s for s in signals.silent_spans(x.shape, n, hop) if s[0] == 0]:
        touching = (starts < hi) & (starts + n > lo)                            # reads a span (its border, or all silence)
        assert not bool(inner[0][touching].any())
    assert bool(inner[2, 2:-2].all())                                           # a row without spans: every unpadded frame
    assert bool(fbnd.interior_frames(x, n, hop, center=False)[2].all())
    assert fbnd.power_db_keep(1.0, 2e-6, 1025) == fbnd.KEEP_INTERIOR
    assert fbnd.power_db_keep(3.0, 5e-6, 1302) < fbnd.power_db_keep(2.0, 2e-6, 1025) < fbnd.KEEP_INTERIOR
    from oracle import torch_ref
    wide = torch_ref.create_mel_filter(1025, 40, 0.0, 8000.0, False)
    narrow = torch_ref.create_mel_filter(201, 160, 0.0, 22050.0, False)
    assert fbnd.mel_db_keep(wide) == fbnd.KEEP_INTERIOR
    assert 0.9 < fbnd.mel_db_keep(narrow) < fbnd.KEEP_INTERIOR
    assert fbnd.mel_db_keep(narrow, win_frac=0.25) < fbnd.mel_db_keep(narrow)
