"""-m gpu: ``griffinlim`` / ``GriffinLim`` on the gfx950 kernels (csrc/griffinlim.hip around ``tac_stft_f32`` / ``tac_istft_f32``) —
strict mode and poisoned outputs on, as in tests/test_istft_gpu.py.

What is held tightly is one step (``tac_griffinlim_update_f32`` against the float64 formula within ``update_bound``), the prepare
launch (within the bound of its one operation) and the driver's bookkeeping (``griffinlim`` equals, to the bit, the same steps
called one by one, with exactly the launches the route promises).  Against the float64 definition the waveform is held
to 4 x what the float32 CPU run of the same definition reaches on the same inputs at the same ``n_iter`` — the 4 x rule of
tests/test_istft_gpu.py — per row and in the measure ``E`` that bounds how far the spectral convergence can differ
(tests/griffinlim_rules.py).  Both worst values are computed here, never hard-coded."""
import math

import pytest
import torch

import frame_bounds as fbnd
import grid_rules as G
import griffinlim_rules as R

pytestmark = pytest.mark.gpu

UPDATE, PREPARE = 'tac_griffinlim_update_f32', 'tac_griffinlim_prepare_f32'
STFT, ISTFT = 'tac_stft_f32', 'tac_istft_f32'


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


@pytest.fixture(scope='module')
def cus(tac):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def launched_since(tac_, before):
    now = tac_._hip.launches
    return {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)}


def m_of(momentum):
    return float(R.momentum_m(momentum))


# ----------------------------------------------------------------------------- 1. one step
def step_operands(rows, frames, bins, m, seed):
    """frame-major ``(rows, T, F, 2)`` float32 R and Rprev from the stft of two waveforms and a magnitude from a third, with
    planted bins — R == m Rprev exactly, both zero, either zero — and rows at gains 2^-70 (first), 2^70 (last), 2^-12 (middle)"""
    n_fft = 2 * (bins - 1)
    hop = n_fft // 4
    w = torch.hann_window(n_fft)
    keep = [0, 3, 4][:rows]                                                      # (the chirp and two noise rows: none silent)
    z = [torch.view_as_real(R.torch_stft(R.waves(5, hop * (frames - 1), seed + i)[keep], n_fft, hop, w).transpose(1, 2)).contiguous()
         for i in range(3)]
    r, p = z[0].clone(), z[1].clone()
    mag = z[2].pow(2).sum(-1).sqrt() + 0.125
    r[:, 1, 3::7] = p[:, 1, 3::7] * torch.tensor(m, dtype=torch.float32)         # R == fl(m Rprev): A is the rounding residual
    r[:, 2, 5::11] = 0.0
    p[:, 2, 5::11] = 0.0                                                         # both zero: exactly 0
    r[:, 3, 1::13] = 0.0                                                         # R zero alone
    p[:, 3, 2::13] = 0.0                                                         # Rprev zero alone
    mag[:, 4, ::5] = 0.0
    gains = {0: 2.0 ** -70, rows - 1: 2.0 ** 70}
    if rows >= 3:
        gains[1] = 2.0 ** -12
    for row, gain in gains.items():
        r[row] *= gain
        p[row] *= gain
    return r, p, mag


def odd_offset(t):
    """the same values one float past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device='cuda')
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 8 == 4
    return v


@pytest.mark.parametrize('shape', [(3, 37, 129), (2, 5, 1025)])
def test_one_step_within_its_bound(tac, shape):
    H = tac._hip
    rows, frames, bins = shape
    for momentum in (0.0, 0.5, 0.99):
        m = m_of(momentum)
        r, p, mag = step_operands(rows, frames, bins, m, 40 + bins)
        rd, pd, md = r.cuda(), p.cuda(), mag.cuda()
        for prev in (None, p):
            want = R.update_reference(r, prev, mag, m)
            bound = R.update_bound(r, prev, mag, m)
            before = dict(H.launches)
            got = H.griffinlim_update(rd, None if prev is None else pd, md, m)
            assert launched_since(tac, before) == {UPDATE: 1}
            assert H.last_route() == 'gl_update_kernel<vec=1>'
            frac = R.fractions(got, want, bound)
            worst = float(frac.max())
            print('update %r momentum %g prev %s: worst error %.3f of its bound' % (shape, momentum, prev is not None, worst))
            fbnd.report('griffinlim_update', '%r m=%g prev=%s' % (shape, momentum, prev is not None), 2 * (bins - 1), 'update', worst, 1.0)
            assert worst <= 1.0, (shape, momentum, prev is not None, worst, int(frac.argmax()))
            both_zero = (r.abs().sum(-1) == 0) if prev is None or m == 0.0 else ((r.abs().sum(-1) == 0) & (p.abs().sum(-1) == 0))
            assert bool(both_zero.any()) and not bool(got.cpu()[both_zero].any()), 'an all-zero bin is not exactly 0'
            # the dword path: every operand one float off its alignment, the same bits
            odd = H.griffinlim_update(odd_offset(rd), None if prev is None else odd_offset(pd), odd_offset(md), m)
            assert H.last_route() == 'gl_update_kernel<vec=0>'
            assert torch.equal(odd.view(torch.int32), got.view(torch.int32))


def test_one_step_beyond_two_rounds_of_the_grid(tac, cus):
    H = tac._hip
    rows, frames, bins = 5, 257, 1025
    n = rows * frames * bins
    work, cap = R.update_launch(cus, n)
    assert G.persistent_blocks((n + 1) // 2, R.UPDATE_THREADS, cap) == cap and work > 2 * cap, (work, cap)
    assert n % 2 == 1                                       # (the last pair is half a pair)
    m = m_of(0.99)
    r, p, mag = step_operands(3, 37, 129, m, 77)
    idx = torch.arange(n) % (r.numel() // 2)
    rb, pb, mb = r.reshape(-1, 2)[idx], p.reshape(-1, 2)[idx], mag.reshape(-1)[idx]
    want, bound = R.update_reference(rb, pb, mb, m), R.update_bound(rb, pb, mb, m)
    got = H.griffinlim_update(rb.cuda().reshape(rows, frames, bins, 2), pb.cuda().reshape(rows, frames, bins, 2),
                              mb.cuda().reshape(rows, frames, bins), m)
    worst = float(R.fractions(got.reshape(-1, 2), want, bound).max())
    print('update %d bins, %d workgroups of work on a grid of %d: worst error %.3f of its bound' % (n, work, cap, worst))
    assert worst <= 1.0


# ----------------------------------------------------------------------------- 2. prepare
def prepare_layouts(tac, rows, bins, frames, seed):
    """(name, device tensor (rows, F, T), dense frame-major) for the three layouts, all of the same values"""
    n_fft, hop = 2 * (bins - 1), (bins - 1) // 2
    w = torch.hann_window(n_fft)
    x = R.waves(rows, hop * (frames - 1), seed)
    view = tac.complex_norm(tac.stft(x.cuda(), n_fft, hop, n_fft, w.cuda()), 1.0)            # the frame-major view
    assert view.shape == (rows, bins, frames) and view.transpose(1, 2).is_contiguous()
    values = view.cpu().contiguous()
    padded = torch.full((rows, 2, bins, frames + 5), float('nan'), device='cuda')
    padded[:, 1, :, :frames] = values.cuda()
    return values, [('time-contiguous', values.cuda(), False), ('frame-major view', view, True),
                    ('channel slice of a padded tensor', padded[:, 1, :, :frames], False)]


@pytest.mark.parametrize('power', [1.0, 2.0, 0.7])
def test_prepare_within_the_bound_of_its_operation(tac, power):
    H = tac._hip
    rows, bins, frames = 3, 129, 37
    values, layouts = prepare_layouts(tac, rows, bins, frames, 61)
    assert not bool(values[1].any()) and bool((values >= 0).all())
    angles = R.seeded_angles((rows, bins, frames), 5)
    for name, spec, dense_fm in layouts:
        for ang in (None, angles):
            mag64, x064 = R.prepare_reference(values, ang, power)
            b_mag, b_x0 = R.prepare_bounds(mag64, x064, power, ang is not None)
            before = dict(H.launches)
            mag, x0 = H.griffinlim_prepare(spec, None if ang is None else ang.cuda(), power)
            assert launched_since(tac, before) == {PREPARE: 1}, (name, launched_since(tac, before))
            assert mag.shape == (rows, frames, bins) and x0.shape == (rows, frames, bins, 2) and mag.is_contiguous() and x0.is_contiguous()
            kept = dense_fm and power == 1.0
            assert (mag.data_ptr() == spec.data_ptr()) == kept, (name, power)          # one launch and the input's own storage: M was not copied
            worst_m = float(R.fractions(mag, mag64, b_mag).max())
            worst_x = float(R.fractions(x0, x064, b_x0).max())
            print('prepare power %g, %s, angles %s: M %.3f, X0 %.3f of their bounds' % (power, name, ang is not None, worst_m, worst_x))
            assert worst_m <= 1.0 and worst_x <= 1.0, (name, power, ang is not None, worst_m, worst_x)
            assert not bool(x0[1].any()) and not bool(mag[1].any())


# ----------------------------------------------------------------------------- 3. bookkeeping, to the bit
def hand_chain(tac, spec, w, case, n_iter, momentum, length, angles0):
    """the steps of ``griffinlim`` called one by one through the package's own entry points, ``Rprev`` rotated by hand"""
    H = tac._hip
    n_fft, hop, wl, user, rows, frames, power = case
    m = m_of(momentum)
    mag, x = H.griffinlim_prepare(spec, angles0, power)
    y = H.istft(x.transpose(1, 2), w, n_fft, hop, wl, True, False, length)
    prev = None
    for _ in range(n_iter):
        r = H.stft(y, w, n_fft, hop, wl, True, 'reflect', False, True).transpose(1, 2)
        x = H.griffinlim_update(r, prev, mag, m)
        y = H.istft(x.transpose(1, 2), w, n_fft, hop, wl, True, False, length)
        prev = r
    return y


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('tag', sorted(R.CASES))
def test_driver_equals_the_steps_called_one_by_one(tac, tag):
    """(at fft_length 2048 the inverse of every step is the fused one-launch route of ``istft``, or — a length that leaves the rows
    off a 16-byte stride — its general route: the same entry point, one launch counted either way)"""
    case = R.CASES[tag]
    n_fft, hop, wl, user, rows, frames, power = case
    w, spec = R.case_input(tag)
    wd, sd = w.cuda(), spec.cuda()
    tac.griffinlim(sd, wd, n_fft, hop, wl, power, 0, 0.99, None, False)         # (the window's envelope table: built once, not counted)
    for n_iter in (0, 1, 2, 5):
        for momentum in (0.0, 0.99):
            for length in (None, hop * (frames - 1) + 3):
                before = dict(tac._hip.launches)
                got = tac.griffinlim(sd, wd, n_fft, hop, wl, power, n_iter, momentum, length, False)
                since = launched_since(tac, before)
                want_launches = {PREPARE: 1, ISTFT: n_iter + 1}
                if n_iter:
                    want_launches.update({UPDATE: n_iter, STFT: n_iter})
                assert since == want_launches, (tag, n_iter, since)
                want = hand_chain(tac, sd, wd, case, n_iter, momentum, length, None)
                assert same_bits(got, want), (tag, n_iter, momentum, length)
    torch.manual_seed(23)
    got = tac.griffinlim(sd, wd, n_fft, hop, wl, power, 5, 0.99, None, True)
    torch.manual_seed(23)
    angles0 = torch.rand(sd.shape, dtype=torch.complex64, device='cuda')
    assert same_bits(got, hand_chain(tac, sd, wd, case, 5, 0.99, None, angles0))
    assert not same_bits(got, tac.griffinlim(sd, wd, n_fft, hop, wl, power, 5, 0.99, None, False))


# ----------------------------------------------------------------------------- 4. against the reference
def test_against_the_float64_definition(tac):
    """every geometry, n_iter 1 / 4 / 32, momentum 0.99, without and with a seeded ``angles0`` handed identically to both sides"""
    runs = {1: [], 4: [], 32: []}
    for tag in sorted(R.CASES):
        n_fft, hop, wl, user, rows, frames, power = R.CASES[tag]
        w, spec = R.case_input(tag)
        wd, sd = w.cuda(), spec.cuda()
        s_lin = R.linear_magnitude(spec, power)
        for init, ang in (('ones', None), ('seeded', R.seeded_angles(spec.shape, 31 + n_fft))):
            for n_iter in runs:
                y64 = R.reference(spec, w, n_fft, hop, wl, power, n_iter, 0.99, None, ang, torch.float64)
                y32 = R.reference(spec, w, n_fft, hop, wl, power, n_iter, 0.99, None, ang, torch.float32)
                got = torch.ops.tac_amd.griffinlim(sd, wd, None if ang is None else ang.cuda(), n_fft, hop, wl, power, n_iter,
                                                   m_of(0.99), None).cpu()
                assert got.shape == y64.shape and bool(torch.isfinite(got).all())
                for row in range(rows):
                    if not bool(spec[row].any()):
                        assert not bool(got[row].any()), '%s: silent row %d is not exactly zero' % (tag, row)
                args = (s_lin, n_fft, hop, w)
                runs[n_iter].append(dict(
                    case='%s %s' % (tag, init), n_fft=n_fft,
                    rel=R.row_max_rel(got, y64), rel32=R.row_max_rel(y32, y64), E=R.E(got, y64, *args), E32=R.E(y32, y64, *args),
                    conv=(R.conv(got, *args), R.conv(y32, *args), R.conv(y64, *args))))
    bad = []
    for n_iter, results in runs.items():
        rel_bound = 4.0 * max(float(r['rel32'].max()) for r in results)
        e_bound = 4.0 * max(float(r['E32'].max()) for r in results)
        assert rel_bound > 0.0 and e_bound > 0.0
        for r in results:
            rel, e = float(torch.nan_to_num(r['rel'], nan=math.inf).max()), float(torch.nan_to_num(r['E'], nan=math.inf).max())
            fbnd.report('griffinlim_reference', '%s n_iter=%d' % (r['case'], n_iter), r['n_fft'], 'rows', rel, rel_bound)
            fbnd.report('griffinlim_reference', '%s n_iter=%d' % (r['case'], n_iter), r['n_fft'], 'E', e, e_bound)
            for name, c in zip(('kernels', 'float32 CPU', 'float64 CPU'), r['conv']):
                fbnd.report('griffinlim_reference', '%s n_iter=%d conv %s' % (r['case'], n_iter, name), r['n_fft'], 'conv', float(c.max()), None)
            print('%-28s n_iter %2d: rows %.3g (float32 CPU %.3g, bound %.3g), E %.3g (float32 CPU %.3g, bound %.3g), conv %s / %s / %s'
                  % (r['case'], n_iter, rel, float(r['rel32'].max()), rel_bound, e, float(r['E32'].max()), e_bound,
                     *('%.4g' % float(c.max()) for c in r['conv'])))
            if not (rel <= rel_bound and e <= e_bound):
                bad.append((r['case'], n_iter, rel, rel_bound, e, e_bound))
    assert not bad, bad


# ----------------------------------------------------------------------------- 5. housekeeping
@pytest.mark.parametrize('tag', ['256/64', '2048/512'])
def test_memory_does_not_grow_with_the_iterations_and_runs_repeat(tac, tag):
    n_fft, hop, wl, user, rows, frames, power = R.CASES[tag]
    w, spec = R.case_input(tag)
    wd, sd = w.cuda(), spec.cuda()

    def peak(n_iter):
        """(peak bytes of one call, its result on the host: nothing of a call stays allocated while the next one is measured)"""
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        out = tac.griffinlim(sd, wd, n_fft, hop, wl, power, n_iter, 0.99, None, False)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(), out.cpu()

    peak(4)
    p4, y4 = peak(4)
    p32, y32 = peak(32)
    assert p32 == p4, (p4, p32)
    assert same_bits(y4, peak(4)[1]) and same_bits(y32, peak(32)[1])


def test_float64_takes_the_announced_route(tac):
    n_fft, hop, wl, user, rows, frames, power = R.CASES['256/64']
    w, spec = R.case_input('256/64')
    wd, sd = w.cuda().double(), spec.cuda().double()
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.griffinlim(sd, wd, n_fft, hop, wl, power, 2, 0.99, None, False)
    tac.set_strict(False)
    try:
        tac._ops._warned.discard(('griffinlim', 'dtype float64'))
        with pytest.warns(tac.CompositeRouteWarning, match='griffinlim'):
            got = tac.griffinlim(sd, wd, n_fft, hop, wl, power, 2, 0.99, None, False)
    finally:
        tac.set_strict(True)
    want = R.reference(spec, w, n_fft, hop, wl, power, 2, 0.99, None, None, torch.float64)
    assert got.dtype == torch.float64 and float(R.row_max_rel(got.cpu(), want).max()) < 1e-9


def test_layer_after_spectrogram_round_trips_a_tone(tac):
    n_fft, hop, rate = 400, 200, 16000
    t = torch.arange(rate, dtype=torch.float64) / rate
    x = (0.5 * torch.sin(2.0 * math.pi * 440.0 * t)).float()[None]
    spec = tac.Spectrogram(fft_length=n_fft, hop_length=hop, power=2.0).to('cuda')(x.cuda())
    assert spec.shape == (1, n_fft // 2 + 1, rate // hop + 1)
    layer = tac.GriffinLim(n_fft=n_fft, hop_length=hop, power=2.0).to('cuda')
    torch.manual_seed(3)
    y = layer(spec)
    assert y.shape == (1, rate)
    s_lin = R.linear_magnitude(spec, 2.0)
    w = layer.window.cpu()
    y0 = tac.GriffinLim(n_fft=n_fft, n_iter=0, hop_length=hop, power=2.0, rand_init=False).to('cuda')(spec)
    c32, c0 = float(R.conv(y, s_lin, n_fft, hop, w)), float(R.conv(y0, s_lin, n_fft, hop, w))
    print('a 440 Hz tone through Spectrogram(power=2) and GriffinLim: conv %.4g after 32 iterations, %.4g after none' % (c32, c0))
    assert c32 < c0
