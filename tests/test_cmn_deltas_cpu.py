"""``sliding_window_cmn`` / ``SlidingWindowCmn`` / ``compute_deltas`` / ``ComputeDeltas`` without a device: the closed-form window
bounds against Kaldi's step-by-step procedure written out here, the torch-operator route (the CPU route) against the float64
references and per-element rules of tests/cmn_rules.py for every option, the reach of a non-finite sample, argument errors, empty
and batched shapes, the layers, fake kernels and tracing, the drift case, and the C ABI surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cmn_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_T = (1, 2, 3, 5, 8, 13, 40, 130)
GRID_W = (1, 2, 3, 4, 7, 12, 50)
GRID_M = (1, 2, 5, 9, 100)


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


# ----------------------------------------------------------------------------- the window
def step_by_step(n_frames, cmn_window, min_cmn_window, center):
    """Kaldi's SlidingWindowCmn (and torchaudio's loop): the window of every frame from the procedure, with the incremental
    add-one / drop-one bookkeeping on an integer ramp — returns [(ws, we, running sum)] per frame"""
    data = [3 * t * t + 1 for t in range(n_frames)]          # integers: the running sum is exact
    last_start, last_end, cur = 0, 0, 0
    res = []
    for t in range(n_frames):
        if center:
            window_start = t - cmn_window // 2
            window_end = window_start + cmn_window
        else:
            window_start = t - cmn_window
            window_end = t + 1
        if window_start < 0:
            window_end -= window_start
            window_start = 0
        if not center:
            if window_end > t:
                window_end = max(t + 1, min_cmn_window)
        if window_end > n_frames:
            window_start -= window_end - n_frames
            window_end = n_frames
            if window_start < 0:
                window_start = 0
        if last_start == 0 and last_end == 0:
            cur = sum(data[window_start:window_end])
        else:
            if window_start > last_start:
                assert window_start == last_start + 1
                cur -= data[last_start]
            if window_end > last_end:
                assert window_end == last_end + 1
                cur += data[last_end]
        last_start, last_end = window_start, window_end
        res.append((window_start, window_end, cur))
    return res, data


@pytest.mark.parametrize('center', (False, True))
def test_closed_form_bounds_are_the_procedure(tac, center):
    for n_frames in GRID_T:
        for w in GRID_W:
            for m in GRID_M:
                steps, data = step_by_step(n_frames, w, m, center)
                ws_t, we_t = tac._composite.cmn_bounds(n_frames, w, m, center)
                for t, (ws, we, cur) in enumerate(steps):
                    assert (ws, we) == R.bounds(t, n_frames, w, m, center), (n_frames, w, m, t)
                    assert (ws, we) == (int(ws_t[t]), int(we_t[t]))
                    assert cur == sum(data[ws:we])                  # the loop's running sum is the window's sum at every t
                assert all(a[0] <= b[0] and a[1] <= b[1] for a, b in zip(steps, steps[1:]))     # both bounds never move back


# ----------------------------------------------------------------------------- the composite on CPU tensors
CMN_CASES = [(7, 3), (3, 9), (600, 100), (1, 1), (4, 1)]


@pytest.mark.parametrize('norm_vars', (False, True))
@pytest.mark.parametrize('center', (False, True))
@pytest.mark.parametrize('w,m', CMN_CASES)
def test_cmn_cpu_float32_and_float64_follow_the_rules(tac, w, m, center, norm_vars):
    for n_frames in (1, 2, max(m - 1, 1), m, w, w + 1, w + 2, 41):
        x = R.alternating((2, n_frames, 5), seed=n_frames + w, offset=3.0)
        want, allow, nan = R.cmn_reference(x, w, m, center, norm_vars)
        got = tac.sliding_window_cmn(torch.from_numpy(x), w, m, center, norm_vars)
        assert got.dtype == torch.float32 and got.shape == x.shape and got.is_contiguous()
        R.assert_within(got, want, allow, 'cpu float32 T=%d' % n_frames, nan)
        got64 = tac.sliding_window_cmn(torch.from_numpy(x).double(), w, m, center, norm_vars)
        assert got64.dtype == torch.float64
        assert np.abs(got64.numpy() - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)


@pytest.mark.parametrize('norm_vars', (False, True))
@pytest.mark.parametrize('center', (False, True))
def test_drift_case_on_the_cpu_route(tac, center, norm_vars):
    """5000 frames of 100 + N(0, 1) at the defaults: the composite meets the rule; the float32 running-sum loop misses the CMN
    rule by orders of magnitude, so the rule tells the two apart.  The variance of a window of 100 .. 601 samples of N(0, 1) is
    between 0.7 and 1.3, its mean square 1e4, so this input sits ON the rule's precondition of 1e-4: it is evaluated at 0.5e-4
    here (the rule's terms do not depend on that ratio; it only keeps the cancellation in float64, 2^-53 mean square / variance,
    negligible: 2.2e-12 at 0.5e-4)."""
    rng = np.random.default_rng(5000)
    x = (100.0 + rng.standard_normal((5000, 8))).astype(np.float32)
    want, allow, nan = R.cmn_reference(x, 600, 100, center, norm_vars, min_ratio=0.5e-4)
    worst = R.assert_within(tac.sliding_window_cmn(torch.from_numpy(x), 600, 100, center, norm_vars), want, allow, 'drift, composite')
    assert worst < 1.0
    rounded_once = want.astype(np.float32)
    assert R.assert_within(rounded_once, want, allow, 'drift, float64 rounded once') <= 0.5       # one rounding: u |want| of 2 u |want|
    if not norm_vars:
        loop = R.float32_running_loop(x, 600, 100, center, norm_vars)
        miss = float((np.abs(loop.astype(np.float64) - want) / allow).max())
        print('float32 running-sum loop: error / allowance %.0f' % miss)
        assert miss > 100.0


def test_cmn_nonfinite_reach_is_exact(tac):
    x = R.alternating((2, 60, 3), seed=60)
    x[0, 17, 1] = np.nan
    x[1, 40, 2] = np.inf
    for center in (False, True):
        for norm_vars in (False, True):
            want, allow, nan = R.cmn_reference(x, 7, 3, center, norm_vars)
            assert nan.sum() == 2 * (8 if not center else 7) and not nan[0, :, 0].any()
            got = tac.sliding_window_cmn(torch.from_numpy(x), 7, 3, center, norm_vars)
            R.assert_within(got, want, allow, 'reach', nan)


def test_cmn_shapes_errors_and_layers(tac):
    for lead in ((), (3,), (2, 3)):
        x = torch.from_numpy(R.alternating(lead + (11, 4), seed=len(lead)))
        got = tac.sliding_window_cmn(x, 5, 2)
        assert got.shape == x.shape
        if lead:
            assert torch.equal(got[(0,) * len(lead)], tac.sliding_window_cmn(x[(0,) * len(lead)], 5, 2))
        assert torch.equal(tac.SlidingWindowCmn(5, 2)(x), got)
        assert torch.equal(tac.SlidingWindowCmn(5, 2, True, True)(x), tac.sliding_window_cmn(x, 5, 2, center=True, norm_vars=True))
    assert tuple(tac.sliding_window_cmn(torch.zeros(2, 0, 4)).shape) == (2, 0, 4)
    assert tuple(tac.sliding_window_cmn(torch.zeros(0, 5, 4)).shape) == (0, 5, 4)
    for bad in (dict(cmn_window=0), dict(min_cmn_window=0), dict(cmn_window=-3)):
        with pytest.raises(ValueError):
            tac.sliding_window_cmn(torch.zeros(4, 3), **bad)
        with pytest.raises(ValueError):
            tac.SlidingWindowCmn(**bad)
    with pytest.raises(ValueError):
        tac.sliding_window_cmn(torch.zeros(4))
    with pytest.raises(TypeError):
        tac.sliding_window_cmn(np.zeros((4, 3), dtype=np.float32))
    # windows of any size: beyond the row they are the whole row, up to the largest int64
    x = torch.from_numpy(R.alternating((2, 9, 3), seed=99))
    for center in (False, True):
        assert torch.equal(tac.sliding_window_cmn(x, 2 ** 63 - 1, 2 ** 63 - 1, center), tac.sliding_window_cmn(x, 9, 18, center))
        assert torch.equal(tac.sliding_window_cmn(x, 4, 2 ** 63 - 1, center), tac.sliding_window_cmn(x, 4, 18, center))
    assert repr(tac.SlidingWindowCmn()) == 'SlidingWindowCmn(cmn_window=600, min_cmn_window=100, center=False, norm_vars=False)'
    half = tac.sliding_window_cmn(torch.from_numpy(R.alternating((9, 2), seed=9)).half(), 3, 1)
    assert half.dtype == torch.float16


# ----------------------------------------------------------------------------- deltas on CPU tensors
@pytest.mark.parametrize('mode', R.DELTAS_MODES)
@pytest.mark.parametrize('win_length', (3, 4, 5, 9, 65, 66, 67))
def test_deltas_cpu_follows_the_rule(tac, win_length, mode):
    n = (win_length - 1) // 2
    rng = np.random.default_rng(win_length)
    for n_frames in (1, 2, n, n + 1, 65):
        x = (rng.standard_normal((2, 3, n_frames)) + 0.5).astype(np.float32)
        short = (mode == 'reflect' and n >= n_frames) or (mode == 'circular' and n > n_frames)
        if short:
            with pytest.raises(ValueError):
                tac.compute_deltas(torch.from_numpy(x), win_length, mode)
            continue
        want, allow = R.deltas_reference(x, win_length, mode)
        got = tac.compute_deltas(torch.from_numpy(x), win_length, mode)
        assert got.dtype == torch.float32 and got.is_contiguous()
        R.assert_within(got, want, allow, 'cpu deltas T=%d' % n_frames)
        got64 = tac.compute_deltas(torch.from_numpy(x).double(), win_length, mode)
        assert got64.dtype == torch.float64 and np.abs(got64.numpy() - want).max() <= 1e-13 * max(np.abs(x).max(), 1.0) * n


@pytest.mark.parametrize('mode', R.DELTAS_MODES)
def test_compute_deltas_layer_is_pad_and_conv1d(tac, mode):
    """torchaudio's own evaluation, written out: pad along time, then a grouped conv1d with the ramp -n .. n over denom"""
    x = torch.randn(2, 3, 7, 50, generator=torch.Generator().manual_seed(3))
    for win_length in (3, 5, 9):
        n = (win_length - 1) // 2
        rows = x.reshape(1, -1, 50)
        kernel = torch.arange(-n, n + 1, dtype=x.dtype).repeat(rows.shape[1], 1, 1)
        want = torch.nn.functional.conv1d(torch.nn.functional.pad(rows, (n, n), mode=mode), kernel, groups=rows.shape[1])
        want = (want / (n * (n + 1) * (2 * n + 1) / 3)).reshape(x.shape)
        got = tac.ComputeDeltas(win_length, mode)(x)
        assert got.shape == x.shape and torch.equal(got, tac.compute_deltas(x, win_length, mode))
        _, allow = R.deltas_reference(x.numpy(), win_length, mode)
        assert (np.abs(got.numpy().astype(np.float64) - want.numpy()) <= 2 * allow + 1e-30).all()     # both are within the rule


def test_deltas_shapes_errors_and_layouts(tac):
    x = torch.randn(4, 6, 20)
    assert torch.equal(tac.compute_deltas(x[0, 0]), tac.compute_deltas(x)[0, 0])
    assert torch.equal(tac.compute_deltas(x.transpose(-1, -2)), tac.compute_deltas(x.transpose(-1, -2).contiguous()))
    assert tac.compute_deltas(x.transpose(-1, -2)).is_contiguous()
    assert tuple(tac.compute_deltas(torch.zeros(0, 6, 20)).shape) == (0, 6, 20)
    assert tuple(tac.compute_deltas(torch.zeros(2, 6, 0)).shape) == (2, 6, 0)
    for bad in (dict(win_length=2), dict(win_length=0), dict(mode='edge'), dict(mode='zeros')):
        with pytest.raises(ValueError):
            tac.compute_deltas(x, **bad)
        with pytest.raises(ValueError):
            tac.ComputeDeltas(**bad)
    with pytest.raises(ValueError):
        tac.compute_deltas(x[..., :2], 5, 'reflect')
    with pytest.raises(ValueError):
        tac.compute_deltas(x[..., :1], 5, 'circular')
    with pytest.raises(ValueError):
        torch.ops.tac_amd.compute_deltas(x[..., :2], 5, 'reflect')          # the op itself refuses too, on every route
    with pytest.raises(TypeError):
        tac.compute_deltas(x.numpy())
    assert repr(tac.ComputeDeltas()) == "ComputeDeltas(win_length=5, mode='replicate')"


# ----------------------------------------------------------------------------- gradients, fake kernels, tracing
def test_gradients_cpu(tac):
    x = torch.randn(2, 12, 3, dtype=torch.float64, requires_grad=True)
    for center in (False, True):
        for norm_vars in (False, True):
            assert torch.autograd.gradcheck(lambda a: tac.sliding_window_cmn(a, 5, 3, center, norm_vars), (x,))
    # windows of ONE frame (min_cmn_window = 1 at the start of a row, a row of one frame): the output is exactly 0 there and so is
    # that frame's share of the gradient — finite, not the 0 * inf of a variance of zero
    for shape, w, m, center in (((6, 3), 3, 1, False), ((2, 6, 3), 1, 1, True), ((1, 3), 600, 100, False), ((2, 1, 3), 7, 3, True)):
        one = torch.randn(shape, dtype=torch.float64, requires_grad=True)
        out = tac.sliding_window_cmn(one, w, m, center, True)
        single = np.array([R.bounds(t, shape[-2], w, m, center) for t in range(shape[-2])])
        single = (single[:, 1] - single[:, 0]) == 1
        assert single.any() and not bool(out[..., torch.from_numpy(single), :].any())
        (grad,) = torch.autograd.grad(out, one, torch.ones_like(out))
        assert bool(torch.isfinite(grad).all()), grad
        assert torch.autograd.gradcheck(lambda a: tac.sliding_window_cmn(a, w, m, center, True), (one,))
        one32 = one.detach().float().requires_grad_(True)
        (grad32,) = torch.autograd.grad(tac.sliding_window_cmn(one32, w, m, center, True).sum(), one32)
        assert bool(torch.isfinite(grad32).all()) and float((grad32.double() - grad).abs().max()) <= 1e-5 * max(float(grad.abs().max()), 1.0)
    z = torch.randn(2, 3, 12, dtype=torch.float64, requires_grad=True)
    for mode in R.DELTAS_MODES:
        assert torch.autograd.gradcheck(lambda a: tac.compute_deltas(a, 5, mode), (z,))
    # the adjoint references of the rules are the float64 autograd of the composite
    g = np.random.default_rng(1).standard_normal((2, 12, 3))
    for center in (False, True):
        (gx,) = torch.autograd.grad(tac.sliding_window_cmn(x, 5, 3, center), x, torch.from_numpy(g))
        want, _ = R.cmn_adjoint_reference(g, 5, 3, center)
        assert np.abs(gx.numpy() - want).max() < 1e-13
    gz = np.random.default_rng(2).standard_normal((2, 3, 12))
    for mode in R.DELTAS_MODES:
        (gx,) = torch.autograd.grad(tac.compute_deltas(z, 9, mode), z, torch.from_numpy(gz))
        want, _ = R.deltas_adjoint_reference(gz, 9, mode)
        assert np.abs(gx.numpy() - want).max() < 1e-13


def test_traces_as_one_node_each(tac):
    seen = []

    def capture(gm, example_inputs):
        seen.extend(str(n.target) for n in gm.graph.nodes if n.op == 'call_function')
        return gm.forward

    torch._dynamo.reset()
    chain = torch.nn.Sequential(tac.SlidingWindowCmn(7, 3))
    x = torch.from_numpy(R.alternating((2, 30, 5), seed=30))
    out = torch.compile(chain, backend=capture, fullgraph=True)(x)
    assert sum('tac_amd.sliding_window_cmn' in n for n in seen) == 1 and len(seen) == 1, seen
    assert torch.equal(out, chain(x))
    del seen[:]
    torch._dynamo.reset()
    deltas = tac.ComputeDeltas()
    z = x.transpose(-1, -2)
    out = torch.compile(deltas, backend=capture, fullgraph=True)(z)
    assert sum('tac_amd.compute_deltas' in n for n in seen) == 1 and len(seen) == 1, seen
    assert torch.equal(out, deltas(z))
    from torch._subclasses.fake_tensor import FakeTensorMode
    sliced = x[:, ::2, 1:]
    with FakeTensorMode() as mode:
        f1 = torch.ops.tac_amd.sliding_window_cmn(mode.from_tensor(sliced), 7, 3, False, True)
        f2 = torch.ops.tac_amd.compute_deltas(mode.from_tensor(z), 5, 'replicate')
    assert tuple(f1.shape) == (2, 15, 4) and f1.dtype == torch.float32 and f1.is_contiguous()
    assert tuple(f2.shape) == (2, 5, 30) and f2.is_contiguous()


def test_names_are_exported(tac):
    for name in ('sliding_window_cmn', 'compute_deltas'):
        assert name in tac.functional.__all__ and getattr(tac, name) is getattr(tac.functional, name)
        assert name in tac._ops.cuda_kernels and hasattr(torch.ops.tac_amd, name) and name in tac._ops._HIP_BACKWARD
    for name in ('SlidingWindowCmn', 'ComputeDeltas'):
        assert getattr(tac, name) is getattr(tac.layers, name)


# ----------------------------------------------------------------------------- C ABI
def test_entry_points_are_declared_and_exported(tac):
    header = open(os.path.join(ROOT, 'include', 'tac_amd.h')).read()
    for name in ('tac_sliding_cmn_chunk', 'tac_sliding_cmn_f32', 'tac_deltas_supported', 'tac_deltas_f32'):
        assert re.search(r'\b%s\s*\(' % name, header) and name in tac._native.EXPORTS
    assert '(19)' in header and '(20)' in header
    if not os.path.exists(tac._native.LIB_PATH):
        tac.build_native()
    h = tac._native.lib()
    assert h.tac_abi_version() == 5
    cmn, deltas = h.tac_sliding_cmn_f32, h.tac_deltas_f32
    assert cmn.restype is ctypes.c_int and len(cmn.argtypes) == 14 and len(deltas.argtypes) == 12
    # refusals come before anything touches a device
    p = ctypes.c_void_p(4096)
    inv, uns = tac._native.TAC_E_INVALID, tac._native.TAC_E_UNSUPPORTED
    assert cmn(None, 1, 8, 4, 32, 4, 1, 600, 100, 0, 0, 0, p, None) == inv
    assert cmn(p, 0, 8, 4, 32, 4, 1, 600, 100, 0, 0, 0, p, None) == inv
    assert cmn(p, 1, 8, 4, 32, 4, 1, 0, 100, 0, 0, 0, p, None) == inv
    assert cmn(p, 1, 8, 4, 32, 4, 1, 600, 0, 0, 0, 0, p, None) == inv
    assert cmn(p, 2, 8, 4, 0, 4, 1, 600, 100, 0, 0, 0, p, None) == inv           # a row stride of zero over two rows
    assert cmn(p, 1, 8, 4, 32, -4, 1, 600, 100, 0, 0, 0, p, None) == inv
    assert cmn(p, 1, 8, 4, 32, 4, 1, 600, 100, 0, 1, 1, p, None) == uns          # no adjoint with norm_vars
    assert deltas(None, 1, 4, 8, 32, 8, 1, 5, 0, 0, p, None) == inv
    assert deltas(p, 1, 4, 8, 32, 8, 1, 2, 0, 0, p, None) == inv
    assert deltas(p, 1, 4, 8, 32, 8, 1, 5, 4, 0, p, None) == inv
    assert deltas(p, 1, 4, 2, 32, 8, 1, 5, 2, 0, p, None) == inv                 # 'reflect' needs n < T
    assert deltas(p, 1, 4, 8, 32, 8, 1, 67, 0, 0, p, None) == uns
    assert deltas(p, 1, 4, 8, 32, 8, 1, 5, 2, 1, p, None) == uns                 # no adjoint for 'reflect'
    assert h.tac_deltas_supported(8, 66, 0, 1) == 0 and h.tac_deltas_supported(8, 5, 3, 0) == 0
    # the chunk: never under a quarter of the first window, the same for every row length while the launch is short of threads,
    # the share of the row that fills the device beyond that
    chunk = tac._hip.sliding_cmn_chunk
    assert chunk(1, 1, 13, 600, 100) == chunk(1, 5000, 13, 600, 100) == 151
    assert chunk(1, 1000, 13, 2 ** 63 - 1, 2 ** 63 - 1) == (2 ** 40 + 1 + 3) // 4                 # capped, no overflow
    assert cmn(p, 1, 2 ** 40 + 1, 4, 32, 4, 1, 600, 100, 0, 0, 0, p, None) == uns
    assert chunk(1, 50, 13, 7, 3) == 2 and chunk(1, 50, 13, 3, 9) == 3
    assert chunk(4096, 100000, 80, 600, 100) == 16384 and chunk(4096, 2000, 80, 600, 100) == 2000
    assert chunk(256, 1000, 80, 600, 100) == 151
