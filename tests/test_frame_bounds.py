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
