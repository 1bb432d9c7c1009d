"""``cqt`` / ``CQT`` without a device: the composite against tests/cqt_rules.py in float64, the argument errors, known answers, and
the host arrangement of the kernel's bank."""
import numpy as np
import pytest
import torch

import cqt_rules as R
import torchaudio_contrib_amd as tac
from torchaudio_contrib_amd import _cqt

TINY = dict(hop_length=64, fmin=250.0, n_bins=9, bins_per_octave=4)


@pytest.mark.parametrize('extra', [{}, {'center': False}, {'pad_mode': 'constant'}, {'power': 1.0}, {'power': 2.0}, {'norm': 2},
                                   {'norm': None, 'scale': False}, {'gamma': 20.0, 'filter_scale': 0.5}, {'hop_length': 63},
                                   {'fmin': 251.0, 'hop_length': 85}])
def test_composite_is_the_definition_in_float64(extra):
    kw = dict(TINY, **extra)
    x = np.stack(R.signals(431, 4000.0, kw['hop_length'], 3)).astype(np.float64).reshape(2, 1, 431)
    got = tac.cqt(torch.from_numpy(x), 4000.0, **kw)
    value, bound = R.cqt(x, 4000.0, **kw)
    assert got.dtype == torch.float64 and got.is_contiguous()
    got = got.numpy()
    got = got if kw.get('power') else got[..., 0] + 1j * got[..., 1]
    assert got.shape == value.shape
    assert np.all(np.abs(got - value) <= 1e-7 * bound + 1e-300)         # (the float32 bound scaled to float64: 2^-53 / 2^-24 = 2e-9)
    layer = tac.CQT(4000.0, **kw)
    assert torch.equal(layer(torch.from_numpy(x)), torch.from_numpy(tac.cqt(torch.from_numpy(x), 4000.0, **kw).numpy()))
    assert repr(layer).startswith('CQT(sample_rate=4000.0, hop_length=%d' % kw['hop_length'])


@pytest.mark.parametrize('kw, error', [
    (dict(hop_length=0), ValueError), (dict(n_bins=0), ValueError), (dict(bins_per_octave=0), ValueError), (dict(fmin=0.0), ValueError),
    (dict(filter_scale=-1.0), ValueError), (dict(sample_rate=0.0), ValueError), (dict(gamma=-1.0), ValueError),
    (dict(n_bins=20), ValueError), (dict(norm=3), ValueError), (dict(pad_mode='edge'), ValueError), (dict(power=3.0), ValueError),
    (dict(length=42), RuntimeError), (dict(length=84, center=False), RuntimeError)])
def test_argument_errors(kw, error):
    kw = dict(TINY, **kw)
    x = torch.zeros(kw.pop('length', 400))
    sr = kw.pop('sample_rate', 4000.0)
    with pytest.raises(error, match='cqt'):
        tac.cqt(x, sr, **kw)
    with pytest.raises(TypeError):
        tac.cqt([0.0] * 400, 4000.0, **TINY)


def test_known_answers():
    sr, k = 4000.0, 5
    tone = torch.sin(2 * np.pi * 250.0 * 2.0 ** (k / 4) * torch.arange(2000, dtype=torch.float64) / sr)
    mag = tac.cqt(tone, sr, power=1.0, **TINY)
    assert mag.shape == (9, 1 + 2000 // 64) and int(mag[:, 10].argmax()) == k
    assert len(R.wavelets(sr, 250.0, 9, 4)[0]) == 85                    # N_0
    assert tac.cqt(tone[:85], sr, center=False, **TINY).shape == (9, 1, 2)
    assert tac.cqt(tone[:85 + 64], sr, center=False, **TINY).shape == (9, 2, 2)
    assert tac.cqt(tone[:43], sr, **TINY).shape == (9, 1, 2)
    assert tac.cqt(tone[:64], sr, **TINY).shape == (9, 2, 2)


@pytest.mark.parametrize('args', [(4000.0, 250.0, 9, 4, 1.0, 0.0, 1, True), (22050.0, 32.70, 84, 12, 1.0, 0.0, 1, True),
                                  (22050.0, 55.0, 30, 24, 0.5, 20.0, None, False)])
def test_bank_arrangement_is_the_conjugate_wavelets(args):
    """the 1 KiB blocks, de-permuted (lane ``(kk, i)``, component ``m`` = column ``i`` at tap ``16 s + 4 kk + m``), are ``conj(g_k)``
    rounded once, zero everywhere else; groups of 8 bins start on multiples of 16 taps and nest"""
    plan = _cqt.plan(*args)
    found, stray = _cqt.unpack(plan)
    wanted = R.wavelets(*args)
    assert stray == 0.0 and len(found) == len(wanted) == args[2]
    for got, c, g in zip(found, plan.wavelets, wanted):     # exactly the host's float64 wavelets rounded once; those are the rules'
        assert np.array_equal(got.real, c.real.astype(np.float32)) and np.array_equal(got.imag, c.imag.astype(np.float32))
        assert c.shape == g.shape and np.abs(c - np.conj(g)).max() <= 1e-13 * np.abs(g).max()
    groups = plan.groups.tolist()
    assert [g[3] for g in groups] == [8] * (args[2] // 8) + ([args[2] % 8] if args[2] % 8 else [])
    assert all(g[0] % 16 == 0 for g in groups) and plan.bank.shape == (sum(g[1] for g in groups), 64, 4)
    assert all(a[0] <= b[0] and b[0] + 16 * b[1] <= a[0] + 16 * a[1] for a, b in zip(groups, groups[1:]))
