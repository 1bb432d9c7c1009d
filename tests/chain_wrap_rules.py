"""Shared by tests/test_chain_grid_wrap_gpu.py and tests/test_chain_wrap_rules_cpu.py (a plain module: no tests in here): the body of
every STFT-chain case of ``grid_rules.chain_shapes``, written once and run on a device — on the GPU with the launch counters and
the recorded route asserted, on the CPU through the package's CPU route, which shows that inputs, references and bounds are sound
before a GPU sees them.

Two shapes per kernel:

* 'long rows': three rows of ``signals.gained_with_silence`` (audio, a silent row, a row at gain 2^-12), long enough for two rounds
  of the grid: a workgroup's frame slice starts and ends inside a row.  Every frame is held to the float64 oracle
  (``frame_bounds.ref64``) under the bound the kernel's own test holds it to; the silent row must come out exactly zero.
* 'short rows': ``rows`` rows drawn as ``arange(rows) % 5`` from five base rows of the fewest frames the launcher takes (no
  multiple of the frames a wave or workgroup takes at once: every row ends in a partial group).  The five base rows alone are held
  to the float64 oracle; the big launch must repeat them bit for bit where it ran the same instantiation, and is held to the
  float64 bound itself, on the device, where it did not (the generic kernel: five rows run its 4-wave form).

No tolerance is new: FRAME / FRAME_POW / frame_tol of tests/test_gpu_fuzz.py for the float32 kernels, FRAME_F64 (and DB_F64 behind
the dB epilogue, the mask shares from ``frame_bounds.power_db_keep``) for the float64 chain, GRAD / GRAD_DB per row for the waveform
gradients (against float64 autograd), and for ``istft`` the rules of tests/test_istft_gpu.py itself (``check_parity``: TIGHT per row
against float64 ``torch.istft``, blocks within 4 x what float32 ``torch.istft`` reaches on the same input).

On the GPU a case asserts the whole dict of launches its op made and the instantiation its launcher recorded; the route is kept
per thread, so the backward pass of a gradient case runs on the calling thread."""
import numpy as np
import torch

import frame_bounds as fbnd
import grid_rules as G
from oracle import signals, torch_ref
from test_gpu_fuzz import DB_F64, FRAME_F64, FRAME_POW, GRAD, GRAD_DB, frame_tol
from test_gpu_parity import F64_PHASE, F64_REL
from test_istft_gpu import check_parity as istft_parity

TEST = 'chain_grid_wrap'
QUIET = np.float32(2.0 ** -10)                   # on top of row 2's own 2^-2: the row at gain 2^-12


def on_gpu(device):
    return torch.device(device).type == 'cuda'


def launched_since(tac, before):
    now = tac._hip.launches
    return {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)}


def tolerance(c):
    if c['f64']:
        return FRAME_F64
    return frame_tol(c['n']) if c['power'] in (None, 1.0) else FRAME_POW


def window_of(c):
    """the periodic Hann window, built on the host (float64: raised by 0.1, as tests/test_gpu_parity.py's float64 cases)"""
    if c['f64']:
        return torch.hann_window(c['n'], dtype=torch.float64) + 0.1
    return torch.hann_window(c['n'])


def waveform(c, rows, seed):
    x = signals.gained_with_silence((rows, c['length']), seed, c['n'], c['hop'])
    x[2] *= QUIET
    assert not x[1].any() and x[0].any() and x[2].any()
    if c['f64']:                                  # bits below float32 (silence stays exact)
        x = x.astype(np.float64)
        x *= 1.0 + 1e-9 * np.random.default_rng(seed).standard_normal(x.shape)
    return x


def reference(c, x, w):
    """float64 oracle: complex rows (rows, F, T, 2) or |X|^power (rows, F, T), before the dB stage"""
    return fbnd.ref64(x, c['n'], c['hop'], w, c['power'], onesided=c['onesided'], center=c['center'], pad_mode=c['pad_mode'])


def run(tac, device, c, xt, wt):
    """one launch of the case's op on ``xt``; on the GPU exactly one launch of its entry point, on the instantiation named"""
    gpu = on_gpu(device)
    before = dict(tac._hip.launches) if gpu else None
    n, hop = c['n'], c['hop']
    if c['power'] is None:
        y = tac.stft(xt, n, hop_length=hop, window=wt, onesided=c['onesided'], center=c['center'], pad_mode=c['pad_mode'])
    else:
        y = torch.ops.tac_amd.spectrogram(xt, wt, n, hop, n, c['center'], c['pad_mode'], False, c['onesided'], c['power'], c['db'], 1.0, 1e-10)
    if gpu:
        ran = launched_since(tac, before)
        assert ran == {c['entry']: 1}, (c['entry'], ran)
    return y


def route_of(tac):
    return tac._native.lib().tac_last_route().decode()


AMIN_DB = 1e-10


def check(c, got, ref, x, w, name, silence):
    """every frame of ``got`` against the float64 oracle ``ref`` under the case's bound; returns the worst ratio — behind the dB
    epilogue the share of the interior elements the mask had to leave out (every element kept is within DB_F64; the worst
    |d dB| is in the report), beside the share it may leave out"""
    tol = tolerance(c)
    if c['db']:
        mag = ref ** (1.0 / c['power']) if c['power'] != 1.0 else ref
        keep = fbnd.power_db_keep(c['power'], tol, mag.shape[-2], db_tol=DB_F64)
        kept = fbnd.check_db(got, ref, TEST, name, c['n'], amin=AMIN_DB, db_tol=DB_F64, lin=fbnd.power_linear_bound(fbnd.frames_of(mag, 'spec'), c['power'], tol),
                             interior=fbnd.interior_frames(x, c['n'], c['hop']), keep_interior=keep)
        return 1.0 - kept, 1.0 - keep
    return fbnd.check_frames(got, ref, 'complex' if c['power'] is None else 'spec', tol, TEST, name, c['n'], silence), tol


def long_rows_body(tac, device, name, c):
    """returns (worst per-frame ratio, bound)"""
    assert c['form'] == 'long' and c['rows'] == 3
    x, w = waveform(c, 3, seed=c['n'] + c['hop']), window_of(c)
    ref = reference(c, x, w)
    got = run(tac, device, c, torch.from_numpy(x).to(device), w.to(device))
    if on_gpu(device):
        assert route_of(tac) == c['route'], (name, route_of(tac))
    assert tuple(got.shape) == tuple(ref.shape) and got.dtype == (torch.float64 if c['f64'] else torch.float32), name
    worst, bound = check(c, got, ref, x, w, name, True)
    if c['db']:                                    # the silent row sits on the clamp: one value, 10 log10(amin) to DB_F64
        floor = got[1].flatten()[0]
        assert bool((got[1] == floor).all()) and abs(float(floor) - 10.0 * np.log10(AMIN_DB)) <= DB_F64, (name, float(floor))
    else:
        assert not bool(got[1].any()), name + ': the silent row is exactly zero'
    return worst, bound


def short_rows_body(tac, device, name, c):
    """returns (worst per-frame ratio of the base rows, bound, whether the big launch repeated the base rows' bits)"""
    assert c['form'] == 'short' and (c['group'] == 1 or c['n_frames'] % c['group'] != 0)
    rows = c['rows']
    base, w = waveform(c, G.BASE_ROWS, seed=c['n'] + c['hop'] + 1), window_of(c)
    ref = reference(c, base, w)
    bt, wt = torch.from_numpy(base).to(device), w.to(device)
    small = run(tac, device, c, bt, wt)
    small_route = route_of(tac) if on_gpu(device) else None
    assert tuple(small.shape) == tuple(ref.shape), name
    worst, bound = check(c, small, ref, base, w, name + ': the base rows', True)
    index = torch.arange(rows, device=device) % G.BASE_ROWS
    big = run(tac, device, c, bt.index_select(0, index).contiguous(), wt)
    if on_gpu(device):
        assert route_of(tac) == c['route'], (name, route_of(tac))
        assert (small_route == c['route']) == c['same_kernel'], (name, small_route)
    want = small.index_select(0, index)
    bits = big.shape == want.shape and torch.equal(big.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8))
    if c['same_kernel']:
        assert bits, name + ': a row depends on where in the batch it stands'
    else:
        # another instantiation than the base rows' launch: the big output itself against the float64 oracle, on the device
        kind = 'complex' if c['power'] is None else 'spec'
        r = fbnd.frames_of(ref.to(device), kind).index_select(0, index)
        ratio = fbnd.linear_frame_errors(fbnd.frames_of(big, kind), r)
        big_worst = float(torch.nan_to_num(ratio, nan=float('inf')).max())
        fbnd.report(TEST, name + ': every row', c['n'], kind, big_worst, tolerance(c))
        assert big_worst <= tolerance(c), '%s: a frame of the big launch is %.3e of its maximum off (bound %.1e)' % (name, big_worst, tolerance(c))
        worst = max(worst, big_worst)
        assert not bool(big[1::G.BASE_ROWS].any()), name + ': the silent rows are exactly zero'
    return worst, bound, bits


def magphase_body(tac, device, name, c, spec_case):
    """``tac_magphase_f64`` on the complex rows of a long-rows float64 case: magnitude, |z|^0.7 and phase of every element"""
    x, w = waveform(spec_case, 3, seed=5), window_of(spec_case)
    z = run(tac, device, spec_case, torch.from_numpy(x).to(device), w.to(device))
    assert z.numel() // 2 == c['elements']
    gpu = on_gpu(device)
    before = dict(tac._hip.launches) if gpu else None
    mag, ph = tac.magphase(z, 1.0)
    p07 = tac.complex_norm(z, 0.7)
    if gpu:
        assert launched_since(tac, before) == {'tac_magphase_f64': 2}, launched_since(tac, before)
    zz = z.detach().cpu().numpy()                    # (the reference on the host, as tests/test_gpu_parity.py takes it)
    re, im = zz[..., 0], zz[..., 1]
    scale = float(np.abs(zz).max())
    errs = (float(np.abs(mag.cpu().numpy() - np.hypot(re, im)).max()) / scale,
            float(np.abs(p07.cpu().numpy() - np.hypot(re, im) ** 0.7).max()) / scale,
            float(np.abs(ph.cpu().numpy() - np.arctan2(im, re)).max()))
    for what, err, bound in zip(('|z|', '|z|^0.7', 'phase'), errs, (F64_REL, F64_REL, F64_PHASE)):
        fbnd.report(TEST, name + ' ' + what, spec_case['n'], 'elements', err, bound)
        assert err < bound, (name, what, err)
    assert not bool(mag[1].any()) and not bool(ph[1].any()), name + ': the silent row'
    return max(errs[:2]), F64_REL


# ----------------------------------------------------------------------------- the waveform gradients
def grad_tolerance(c):
    """GRAD per row; GRAD_DB through |X|, which is not differentiable at 0 (tests/test_gpu_fuzz.py's rule)"""
    return GRAD_DB if c['power'] == 1.0 else GRAD


def bank_of(tac, c):
    return tac.create_mel_filter(c['n'] // 2 + 1, c['mels'], 0.0, 8000.0, False) if c['gradient'] == 'mel' else None


def forward64(c, x64, w, fb):
    """the float64 oracle of the case's differentiable output"""
    kw = dict(center=c['center'], pad_mode=c['pad_mode'])
    if c['gradient'] == 'stft':
        return fbnd.ref64(x64, c['n'], c['hop'], w, **kw)
    return fbnd.ref64(x64, c['n'], c['hop'], w, c['power'], fb=fb, **kw)


def forward(tac, c, xt, wt, fbt):
    n, hop, geo = c['n'], c['hop'], (c['center'], c['pad_mode'], False, True)
    if c['gradient'] == 'stft':
        return tac.stft(xt, n, hop_length=hop, window=wt, center=c['center'], pad_mode=c['pad_mode'])
    if c['gradient'] == 'mel':
        return torch.ops.tac_amd.melspectrogram(xt, wt, fbt, n, hop, n, *geo, c['power'], False, 1.0, 1e-7)
    return torch.ops.tac_amd.spectrogram(xt, wt, n, hop, n, *geo, c['power'], False, 1.0, 1e-7)


def weights_and_reference(c, x, w, fb, seed):
    """(weights of the output, float64 gradient of sum(weights * output)): uniform weights, zero on the silent row of the linear
    output (whose gradient does not depend on the row) and, through |X|, on bins below 1e-3 of their row's maximum"""
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    y64 = forward64(c, x64, w, fb)
    wts = torch.from_numpy(signals.uniform(tuple(y64.shape), seed=seed).astype(np.float64))
    if c['gradient'] == 'stft':
        wts[1] = 0.0
    if c['power'] == 1.0 and c['gradient'] != 'mel':     # (a mel band of |X| is a sum over bins: no mask, GRAD_DB)
        rows = y64.detach().reshape(y64.shape[0], -1)
        wts = wts * (rows > 1e-3 * rows.amax(-1, keepdim=True)).reshape(y64.shape)
    (want,) = torch.autograd.grad((y64 * wts).sum(), x64)
    return wts.float(), want


def gradient(tac, device, c, xt, wt, fbt, weights):
    """the waveform gradient of sum(weights * output); on the GPU the launches of the backward pass are the case's"""
    gpu = on_gpu(device)
    x = xt.clone().requires_grad_(True)
    y = forward(tac, c, x, wt, fbt)
    before = dict(tac._hip.launches) if gpu else None
    with torch.autograd.set_multithreading_enabled(False):       # (on this thread: the route a launcher records is its thread's)
        (got,) = torch.autograd.grad(y, x, grad_outputs=weights.to(device))
    if gpu:
        ran = launched_since(tac, before)
        assert ran == c['launches'], (ran, c['launches'])
        assert route_of(tac) == c['route'], route_of(tac)
    assert got.shape == xt.shape
    return got


def gradient_long_rows_body(tac, device, name, c):
    assert c['form'] == 'long' and c['rows'] == 3
    x, w, fb = waveform(c, 3, seed=c['n'] + c['hop'] + 2), window_of(c), bank_of(tac, c)
    weights, want = weights_and_reference(c, x, w, fb, seed=c['n'] + 3)
    got = gradient(tac, device, c, torch.from_numpy(x).to(device), w.to(device), None if fb is None else fb.to(device), weights)
    worst = fbnd.check_rows(got, want, grad_tolerance(c), TEST, name, c['n'], silent_rows=(1,))
    assert not bool(got[1].any()), name + ': the silent row is exactly zero'
    return worst, grad_tolerance(c)


def gradient_short_rows_body(tac, device, name, c):
    assert c['form'] == 'short'
    rows, tol = c['rows'], grad_tolerance(c)
    base, w, fb = waveform(c, G.BASE_ROWS, seed=c['n'] + c['hop'] + 4), window_of(c), bank_of(tac, c)
    weights, want = weights_and_reference(c, base, w, fb, seed=c['n'] + 5)
    bt, wt, fbt = torch.from_numpy(base).to(device), w.to(device), None if fb is None else fb.to(device)
    small = gradient(tac, device, c, bt, wt, fbt, weights)
    worst = fbnd.check_rows(small, want, tol, TEST, name + ': the base rows', c['n'], silent_rows=(1,))
    assert not bool(small[1].any()), name + ': the silent row is exactly zero'
    index = torch.arange(rows, device=device) % G.BASE_ROWS
    big = gradient(tac, device, c, bt.index_select(0, index).contiguous(), wt, fbt, weights.to(device).index_select(0, index).contiguous())
    expect = small.index_select(0, index)
    bits = big.shape == expect.shape and torch.equal(big.contiguous().view(torch.int32), expect.contiguous().view(torch.int32))
    if c['same_kernel']:
        assert bits, name + ': a row of the gradient depends on where in the batch it stands'
    else:
        # the rows are cut into other segments than the base rows alone: the big gradient itself against float64, on the device
        ratio = fbnd.row_errors(big, want.to(device).index_select(0, index))
        big_worst = float(torch.nan_to_num(ratio, nan=float('inf')).max())
        fbnd.report(TEST, name + ': every row', c['n'], 'grad', big_worst, tol)
        assert big_worst <= tol, '%s: a row of the big gradient is %.3e of its maximum off (bound %.1e)' % (name, big_worst, tol)
        worst = max(worst, big_worst)
        assert not bool(big[1::G.BASE_ROWS].any()), name + ': the silent rows are exactly zero'
    return worst, tol, bits


# ----------------------------------------------------------------------------- istft
def istft_inputs(c, rows, seed):
    """(Hann window, float32 spectrogram (rows, F, T, 2)): the CPU stft of ``rows`` rows of ``signals.gained_with_silence`` (row 1
    silent, row 2 at gain 2^-12), which ``istft`` takes back to ``hop (T - 1)`` samples a row"""
    n, hop, full = c['n'], c['hop'], c['hop'] * (c['n_frames'] - 1)
    assert c['length'] == full - c['trim'] and c['center']
    x = signals.gained_with_silence((rows, full), seed, n, hop)
    x[2] *= QUIET
    assert not x[1].any() and x[0].any() and x[2].any()
    w = torch.hann_window(n)
    mode = 'reflect' if full > n // 2 else 'constant'                 # (a row of one or two hops is too short to reflect)
    z = torch_ref.stft(torch.from_numpy(x), n, hop, window=w, center=True, pad_mode=mode).float()
    assert tuple(z.shape) == (rows, n // 2 + 1, c['n_frames'], 2)
    return w, z


def run_istft(tac, device, c, z, wt):
    """one ``istft`` of the frame-major rows ``z`` (read in place); on the GPU one launch of ``tac_istft_f32`` (the envelope of a
    window and geometry is built once, by a launch of its own) on the route named"""
    gpu = on_gpu(device)
    zt = z.to(device).transpose(-3, -2).contiguous().transpose(-3, -2)
    before = dict(tac._hip.launches) if gpu else None
    y = tac.istft(zt, c['n'], c['hop'], window=wt, length=c['length'] if c['trim'] else None)
    if gpu:
        ran = launched_since(tac, before)
        ran.pop('tac_istft_envelope_f32', None)
        assert ran == c['launches'], (ran, c['launches'])
        assert route_of(tac) == c['route'], route_of(tac)
    assert tuple(y.shape) == (z.shape[0], c['length'])
    return y


def check_istft(tac, c, got, z, w, name):
    """tests/test_istft_gpu.py's rules: every row within TIGHT of its own maximum of ``torch.istft`` in float64 on the same
    spectrogram, silent rows exactly zero, every block of a hop within 4 x the worst block ratio float32 ``torch.istft`` reaches on
    the same input.  Returns (worst block ratio, its bound)."""
    mine, theirs = istft_parity(tac, got, z, c['n'], c['hop'], w, False, c['length'] if c['trim'] else None, TEST, name)
    bound = 4.0 * theirs
    fbnd.report(TEST, name, c['n'], 'blocks', mine, bound)
    assert bound > 0.0 and mine <= bound, '%s: a block is %.3e of its neighbourhood off (4 x the float32 reference: %.3e)' % (name, mine, bound)
    return mine, bound


def istft_long_rows_body(tac, device, name, c):
    assert c['form'] == 'long' and c['rows'] == 3 and c['inverse']
    w, z = istft_inputs(c, 3, seed=c['n'] + c['hop'])
    got = run_istft(tac, device, c, z, w.to(device))
    return check_istft(tac, c, got, z, w, name)


def istft_short_rows_body(tac, device, name, c):
    """returns (worst block ratio of the base rows, bound, whether the big launch repeated the base rows' bits — required: both
    launches run one instantiation, the frames of a row in one segment)"""
    assert c['form'] == 'short' and c['inverse'] and c['same_kernel']
    w, z = istft_inputs(c, G.BASE_ROWS, seed=c['n'] + c['hop'] + 1)
    wt = w.to(device)
    small = run_istft(tac, device, c, z, wt)
    worst, bound = check_istft(tac, c, small, z, w, name + ': the base rows')
    index = torch.arange(c['rows']) % G.BASE_ROWS
    big = run_istft(tac, device, c, z.index_select(0, index), wt)
    want = small.index_select(0, index.to(device))
    bits = big.shape == want.shape and torch.equal(big.contiguous().view(torch.int32), want.contiguous().view(torch.int32))
    assert bits, name + ': a row depends on where in the batch it stands'
    return worst, bound, bits
