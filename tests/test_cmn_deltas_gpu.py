"""-m gpu: ``sliding_window_cmn`` / ``compute_deltas`` on the gfx950 kernels (csrc/cmn_deltas.hip) — strict mode and poisoned
outputs on, as in tests/test_mfcc_gpu.py.

References and per-element rules: tests/cmn_rules.py (float64, every window summed directly; every element is checked).  The
shapes are the smallest at which the kernels can still go wrong: row lengths on every border of the window rules (1, 2, around
``min_cmn_window``, around ``cmn_window``) and of a thread's chunk (``tac_sliding_cmn_chunk``: one short chunk, one full chunk, one
frame more, two chunks and three frames), feature counts on both sides of the 16 / 32 / 64-lane feature blocks, 1 and 3 rows and
a 2-D lead, and every layout the kernels read in place (contiguous, a feature slice, a time slice, the transposed view); for the
deltas every window up to the cap, row lengths around the 64- and 256-frame tiles, both load forms and a strided time slice.
Gradients are held to the same rules on the adjoint, against the float64 autograd of the composite."""
import warnings

import numpy as np
import pytest
import torch

import cmn_rules as R

pytestmark = pytest.mark.gpu

CMN, DELTAS = 'tac_sliding_cmn_f32', 'tac_deltas_f32'
WINDOWS = ((7, 3), (3, 9), (600, 100))


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


# ---- layouts of a (…, A, B) array on the device, none of them a copy for the kernels
def last_slice(x):
    """[..., 1:] of a tensor one column wider (``fbank(use_energy=True)[:, 1:]``)"""
    wide = torch.full(tuple(x.shape[:-1]) + (x.shape[-1] + 1,), float('nan'), device='cuda')
    wide[..., 1:] = dev(x)
    return wide[..., 1:]


def second_slice(x):
    """[..., ::2, :] of a tensor twice as long on the second-to-last axis"""
    wide = torch.full(tuple(x.shape[:-2]) + (2 * x.shape[-2], x.shape[-1]), float('nan'), device='cuda')
    wide[..., ::2, :] = dev(x)
    return wide[..., ::2, :]


def last_strided(x):
    """[..., ::2] of a tensor twice as long on the last axis"""
    wide = torch.full(tuple(x.shape[:-1]) + (2 * x.shape[-1],), float('nan'), device='cuda')
    wide[..., ::2] = dev(x)
    return wide[..., ::2]


def transposed(x):
    """the transposed view of the array stored with its last two axes swapped"""
    return dev(np.swapaxes(x, -1, -2)).transpose(-1, -2)


CMN_LAYOUTS = (('contiguous', dev), ('feature slice', last_slice), ('time slice', second_slice), ('transposed', transposed))
DELTAS_LAYOUTS = (('contiguous', dev), ('transposed (T, F)', transposed), ('time slice', last_strided))


def run_cmn(tac_, xt, x, w, m, center, norm_vars, what, min_ratio=1e-4):
    before = dict(tac_._hip.launches)
    got = tac_.sliding_window_cmn(xt, w, m, center, norm_vars)
    assert launched_since(tac_, before) == {CMN: 1}, what
    assert got.dtype == torch.float32 and got.shape == xt.shape and got.is_contiguous()
    want, allow, nan = R.cmn_reference(x, w, m, center, norm_vars, min_ratio)
    return R.assert_within(got, want, allow, what, nan)


# ----------------------------------------------------------------------------- sliding_window_cmn
@pytest.mark.parametrize('norm_vars', (False, True))
@pytest.mark.parametrize('center', (False, True))
@pytest.mark.parametrize('w,m', WINDOWS)
def test_cmn_row_lengths(tac, w, m, center, norm_vars):
    chunk = tac._hip.sliding_cmn_chunk(1, 1, 13, w, m)
    lengths = sorted({1, 2, max(m - 1, 1), m, w, w + 1, w + 2, max(chunk - 1, 1), chunk, chunk + 1, 2 * chunk + 3})
    for n_frames in lengths:
        assert tac._hip.sliding_cmn_chunk(1, n_frames, 13, w, m) == chunk          # these lengths sit on the chunk's borders
        x = R.alternating((1, n_frames, 13), seed=n_frames + w, offset=3.0)
        run_cmn(tac, dev(x), x, w, m, center, norm_vars, 'W=%d min=%d T=%d' % (w, m, n_frames))


@pytest.mark.parametrize('name,layout', CMN_LAYOUTS)
@pytest.mark.parametrize('n_feats', (1, 13, 23, 64, 65, 80, 257))
def test_cmn_features_rows_and_layouts(tac, n_feats, name, layout):
    for lead in ((1,), (3,), (2, 2)):
        x = R.alternating(lead + (41, n_feats), seed=n_feats + len(lead), offset=-2.0)
        xt = layout(x)
        assert xt.shape == x.shape
        for center, norm_vars in ((False, False), (True, True)):
            run_cmn(tac, xt, x, 7, 3, center, norm_vars, '%s F=%d lead=%r' % (name, n_feats, lead))
    x = R.alternating((41, n_feats), seed=n_feats)                      # (T, F) without a batch: what kaldi.fbank returns
    run_cmn(tac, layout(x), x, 7, 3, False, False, '%s F=%d (T, F)' % (name, n_feats))


def test_cmn_many_chunks_per_row(tac):
    """a row long enough that the chunk is the share that fills the device, not the floor: several full chunks and a short one"""
    rows, n_frames, n_feats = 64, 1310, 80
    chunk = tac._hip.sliding_cmn_chunk(rows, n_frames, n_feats, 7, 3)
    assert 2 < chunk < n_frames and n_frames % chunk
    x = R.alternating((rows, n_frames, n_feats), seed=1310, offset=1.0)
    for center, norm_vars in ((False, True), (True, False)):
        run_cmn(tac, dev(x), x, 7, 3, center, norm_vars, 'chunk %d of %d' % (chunk, n_frames))


@pytest.mark.parametrize('norm_vars', (False, True))
@pytest.mark.parametrize('center', (False, True))
def test_cmn_does_not_drift(tac, center, norm_vars):
    """5000 frames x 8 features of 100 + N(0, 1) at the defaults: the float32 running-sum loop misses the CMN rule by three orders
    of magnitude here (tests/test_cmn_deltas_cpu.py, where the precondition's 0.5e-4 is explained)"""
    rng = np.random.default_rng(5000)
    x = (100.0 + rng.standard_normal((5000, 8))).astype(np.float32)
    run_cmn(tac, dev(x), x, 600, 100, center, norm_vars, 'drift', min_ratio=0.5e-4)


def test_cmn_nonfinite_reach_is_exact(tac):
    x = R.alternating((2, 700, 13), seed=700)
    x[0, 17, 1] = np.nan
    x[1, 400, 12] = np.inf
    x[1, 650, 0] = -np.inf
    for w, m in ((7, 3), (600, 100)):
        for center in (False, True):
            for norm_vars in (False, True):
                want, allow, nan = R.cmn_reference(x, w, m, center, norm_vars)
                assert 0 < nan.sum() < nan.size and not nan[0, :, 0].any()
                got = tac.sliding_window_cmn(dev(x), w, m, center, norm_vars)
                R.assert_within(got, want, allow, 'reach W=%d' % w, nan)


def test_cmn_reruns_are_bit_identical_and_other_routes_are_announced(tac):
    x = dev(R.alternating((3, 333, 80), seed=333))
    for norm_vars in (False, True):
        assert torch.equal(tac.sliding_window_cmn(x, 50, 10, False, norm_vars), tac.sliding_window_cmn(x, 50, 10, False, norm_vars))
    with pytest.raises(RuntimeError, match='strict'):
        tac.sliding_window_cmn(x.double())
    with pytest.raises(RuntimeError, match='strict'):
        tac.sliding_window_cmn(x[:, :1].expand(3, 333, 80))                     # a stride of zero
    tac.set_strict(False)
    try:
        key = ('sliding_window_cmn', 'dtype float64')
        counted = tac._ops.composite_calls.get(key, 0)
        tac._ops._warned.discard(key)                           # (warned once per reason: ask for it again)
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            got = tac.sliding_window_cmn(x.double(), 50, 10)
        assert any(issubclass(w.category, tac.CompositeRouteWarning) for w in seen)
        assert tac._ops.composite_calls.get(key, 0) == counted + 1
        assert got.dtype == torch.float64
        assert (got.float() - tac.sliding_window_cmn(x, 50, 10)).abs().max() < 1e-5
    finally:
        tac.set_strict(True)
    assert tuple(tac.sliding_window_cmn(x[:, :0]).shape) == (3, 0, 80)


@pytest.mark.parametrize('center', (False, True))
@pytest.mark.parametrize('w,m', WINDOWS)
def test_cmn_gradient_is_the_adjoint_mode(tac, w, m, center):
    chunk = tac._hip.sliding_cmn_chunk(1, 1, 13, w, m)
    for n_frames in sorted({1, 2, m, w + 1, w + 2, chunk, chunk + 1, 2 * chunk + 3}):
        rng = np.random.default_rng(n_frames)
        g = rng.standard_normal((2, n_frames, 13)).astype(np.float32)
        x = dev(R.alternating((2, n_frames, 13), seed=n_frames)).requires_grad_(True)
        before = dict(tac._hip.launches)
        out = tac.sliding_window_cmn(x, w, m, center)
        (gx,) = torch.autograd.grad((out * dev(g)).sum(), x)
        assert launched_since(tac, before) == {CMN: 2}
        x64 = x.detach().cpu().double().requires_grad_(True)
        (want,) = torch.autograd.grad(tac.sliding_window_cmn(x64, w, m, center), x64, torch.from_numpy(g).double())
        direct, allow = R.cmn_adjoint_reference(g, w, m, center)
        assert np.abs(want.numpy() - direct).max() <= 1e-12 * max(np.abs(g).max(), 1.0)
        R.assert_within(gx, want.numpy(), allow, 'adjoint W=%d min=%d T=%d' % (w, m, n_frames))


# ----------------------------------------------------------------------------- compute_deltas
def run_deltas(tac_, xt, ref, win_length, mode, what):
    """``ref``: (want, allow) of tests/cmn_rules.py for the values of ``xt``, computed once and shared by the layouts"""
    before = dict(tac_._hip.launches)
    got = tac_.compute_deltas(xt, win_length, mode)
    assert launched_since(tac_, before) == {DELTAS: 1}, what
    assert got.dtype == torch.float32 and got.shape == xt.shape and got.is_contiguous()
    return R.assert_within(got, ref[0], ref[1], what)


@pytest.mark.parametrize('mode', R.DELTAS_MODES)
@pytest.mark.parametrize('win_length', (3, 4, 5, 9, 65, 66))
def test_deltas_windows_lengths_and_load_forms(tac, win_length, mode):
    n = (win_length - 1) // 2
    rng = np.random.default_rng(win_length)
    for n_frames in sorted({1, 2, n, n + 1, 63, 64, 65, 257}):
        x = (rng.standard_normal((2, 13, n_frames)) + 0.5).astype(np.float32)
        short = (mode == 'reflect' and n >= n_frames) or (mode == 'circular' and n > n_frames)
        ref = None if short else R.deltas_reference(x, win_length, mode)
        for name, layout in DELTAS_LAYOUTS:
            if short:
                before = dict(tac._hip.launches)
                with pytest.raises(ValueError):
                    tac.compute_deltas(layout(x), win_length, mode)
                assert launched_since(tac, before) == {}
            else:
                run_deltas(tac, layout(x), ref, win_length, mode, '%s win=%d T=%d %s' % (mode, win_length, n_frames, name))


@pytest.mark.parametrize('name,layout', DELTAS_LAYOUTS)
@pytest.mark.parametrize('n_feats', (1, 13, 80, 257))
def test_deltas_features_rows_and_layouts(tac, n_feats, name, layout):
    rng = np.random.default_rng(n_feats)
    for lead in ((), (3,), (2, 2)):
        x = (rng.standard_normal(lead + (n_feats, 300)) - 0.25).astype(np.float32)
        for win_length, mode in ((5, 'replicate'), (9, 'reflect')):
            run_deltas(tac, layout(x), R.deltas_reference(x, win_length, mode), win_length, mode,
                       '%s F=%d lead=%r' % (name, n_feats, lead))


def test_deltas_wider_windows_take_the_composite_announced(tac):
    x = dev(np.random.default_rng(67).standard_normal((2, 13, 100)).astype(np.float32))
    with pytest.raises(RuntimeError, match='strict'):
        tac.compute_deltas(x, 67)
    tac.set_strict(False)
    try:
        before = dict(tac._hip.launches)
        (key,) = [k for k in tac._ops.composite_calls if k[0] == 'compute_deltas' and 'win_length 67' in k[1]]
        counted = tac._ops.composite_calls[key]                 # (the refused call above was counted before it raised)
        tac._ops._warned.discard(key)
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            got = tac.compute_deltas(x, 67)
        assert launched_since(tac, before) == {}
        assert any(issubclass(w.category, tac.CompositeRouteWarning) for w in seen)
        assert tac._ops.composite_calls[key] == counted + 1
        want, allow = R.deltas_reference(x.cpu().numpy(), 67, 'replicate')
        R.assert_within(got, want, allow, 'win_length 67, composite')
    finally:
        tac.set_strict(True)
    assert torch.equal(tac.compute_deltas(x, 66), tac.compute_deltas(x, 66))
    assert torch.equal(tac.compute_deltas(x.transpose(-1, -2), 5), tac.compute_deltas(x.transpose(-1, -2), 5))


@pytest.mark.parametrize('mode', ('replicate', 'constant'))
@pytest.mark.parametrize('win_length', (3, 5, 9, 65))
def test_deltas_gradient_is_the_adjoint_mode(tac, win_length, mode):
    n = (win_length - 1) // 2
    for n_frames in sorted({1, 2, n, n + 1, 64, 65, 257}):
        rng = np.random.default_rng(n_frames + win_length)
        g = rng.standard_normal((2, 13, n_frames)).astype(np.float32)
        for name, layout in DELTAS_LAYOUTS[:2]:
            x = layout(rng.standard_normal((2, 13, n_frames)).astype(np.float32)).requires_grad_(True)
            before = dict(tac._hip.launches)
            out = tac.compute_deltas(x, win_length, mode)
            (gx,) = torch.autograd.grad(out, x, layout(g))          # grad_out in the same layout: both load forms of the adjoint
            assert launched_since(tac, before) == {DELTAS: 2}
            x64 = x.detach().cpu().double().requires_grad_(True)
            (want,) = torch.autograd.grad(tac.compute_deltas(x64, win_length, mode), x64, torch.from_numpy(g).double())
            direct, allow = R.deltas_adjoint_reference(g, win_length, mode)
            assert np.abs(want.numpy() - direct).max() <= 1e-12 * max(np.abs(g).max(), 1.0) * n
            R.assert_within(gx, want.numpy(), allow, 'deltas adjoint %s win=%d T=%d %s' % (mode, win_length, n_frames, name))


# ----------------------------------------------------------------------------- the chain
def test_fbank_cmn_deltas_is_three_launches(tac):
    from torchaudio_contrib_amd import kaldi
    wave = dev(np.random.default_rng(16).standard_normal((1, 16000)).astype(np.float32))
    before = dict(tac._hip.launches)
    feats = kaldi.fbank(wave, num_mel_bins=80)
    normed = tac.SlidingWindowCmn()(feats)
    deltas = tac.ComputeDeltas()(normed.transpose(0, 1))
    assert launched_since(tac, before) == {'tac_kaldi_fbank_f32': 1, CMN: 1, DELTAS: 1}
    assert tuple(feats.shape) == tuple(normed.shape) == (98, 80) and tuple(deltas.shape) == (80, 98)
    assert bool(torch.isfinite(deltas).all()) and deltas.is_contiguous()
    want, allow, nan = R.cmn_reference(feats.cpu().numpy(), 600, 100, False, False)
    R.assert_within(normed, want, allow, 'chain: cmn', nan)
    want, allow = R.deltas_reference(normed.cpu().numpy().T, 5, 'replicate')
    R.assert_within(deltas, want, allow, 'chain: deltas')
    # energy in front: the column slice runs in place
    before = dict(tac._hip.launches)
    with_energy = kaldi.fbank(wave, num_mel_bins=80, use_energy=True)
    sliced = tac.sliding_window_cmn(with_energy[:, 1:])
    assert launched_since(tac, before) == {'tac_kaldi_fbank_f32': 1, CMN: 1}
    want, allow, nan = R.cmn_reference(with_energy[:, 1:].cpu().numpy(), 600, 100, False, False)
    R.assert_within(sliced, want, allow, 'chain: cmn of a column slice', nan)


@pytest.mark.parametrize('mode', ('replicate', 'constant'))
def test_chain_gradient_stays_on_the_kernels(tac, mode):
    rng = np.random.default_rng(7)
    feats = dev(R.alternating((2, 150, 23), seed=150)).requires_grad_(True)
    w = rng.standard_normal((2, 23, 150)).astype(np.float32)
    before = dict(tac._hip.launches)
    out = tac.compute_deltas(tac.sliding_window_cmn(feats, 50, 10).transpose(-1, -2), 5, mode)
    (gx,) = torch.autograd.grad((out * dev(w)).sum(), feats)
    assert launched_since(tac, before) == {CMN: 2, DELTAS: 2}
    # each stage's adjoint rule, applied to what it was given: float64 autograd of the composite, stage by stage
    mid, mid_allow = R.deltas_adjoint_reference(w, 5, mode)
    want, allow = R.cmn_adjoint_reference(np.swapaxes(mid, -1, -2), 50, 10, False)
    # what the first stage may be off by reaches the result through the second adjoint: d[s] + sum d[t] / n(t)
    d = np.swapaxes(mid_allow, -1, -2)
    carried, _ = R.cmn_adjoint_reference(d, 50, 10, False)                 # d[s] - sum d[t] / n(t), d >= 0
    through = d + np.abs(carried - d)
    f64 = feats.detach().cpu().double().requires_grad_(True)
    (auto,) = torch.autograd.grad(tac.compute_deltas(tac.sliding_window_cmn(f64, 50, 10).transpose(-1, -2), 5, mode), f64,
                                  torch.from_numpy(w).double())
    assert np.abs(auto.numpy() - want).max() < 1e-12
    R.assert_within(gx, auto.numpy(), allow + through, 'chain gradient %s' % mode)


def test_gradients_without_a_kernel_take_the_composite_announced(tac):
    feats = dev(R.alternating((2, 60, 13), seed=61)).requires_grad_(True)
    g = dev(np.random.default_rng(61).standard_normal((2, 60, 13)).astype(np.float32))
    f64 = feats.detach().cpu().double().requires_grad_(True)

    def grads(fn, x, gg):
        (r,) = torch.autograd.grad(fn(x), x, gg)
        return r

    cases = ((lambda a: tac.sliding_window_cmn(a, 7, 3, False, True), 'sliding_window_cmn'),
             (lambda a: tac.compute_deltas(a, 5, 'reflect'), 'compute_deltas'),
             (lambda a: tac.compute_deltas(a, 5, 'circular'), 'compute_deltas'))
    for fn, op in cases:
        with pytest.raises(RuntimeError, match='strict'):
            grads(fn, feats, g)
        tac.set_strict(True, backward=False)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', tac.CompositeRouteWarning)
                got = grads(fn, feats, g)
        finally:
            tac.set_strict(True)
        assert any(k[0] == op and k[1].startswith('backward: ') for k in tac._ops.composite_calls)
        want = grads(fn, f64, g.cpu().double())
        scale = float(want.abs().max())
        assert float((got.cpu().double() - want).abs().max()) <= 1e-5 * scale
