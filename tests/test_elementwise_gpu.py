"""-m gpu: the elementwise kernels (csrc/elementwise.hip, the float64 forms of csrc/chain_f64.hip) and their gradient kernels
(csrc/backward.hip) held element by element — strict mode and poisoned outputs on, launches counted.

References, bounds, generators and the list of intended deviations: tests/elementwise_rules.py.  Every test prints its worst error
as a fraction of the element's own bound.  Sections: the core sweep (float32 forward and backward through the public functional,
float64 forward against a ``longdouble`` reference), the edge table, placement (16-byte body, dword kernel and scalar tail give the
same bits; nothing written beyond n), layouts, and the second trip of every grid."""
import itertools
import os

import numpy as np
import pytest
import torch

import elementwise_rules as R

pytestmark = pytest.mark.gpu

NORM, MAGPHASE, TO_DB, FROM_DB = 'tac_complex_norm_f32', 'tac_magphase_f32', 'tac_amplitude_to_db_f32', 'tac_db_to_amplitude_f32'
NORM_BW, MAGPHASE_BW = 'tac_complex_norm_backward_f32', 'tac_magphase_backward_f32'
TO_DB_BW, FROM_DB_BW = 'tac_amplitude_to_db_backward_f32', 'tac_db_to_amplitude_backward_f32'
MAGPHASE64, TO_DB64, FROM_DB64 = 'tac_magphase_f64', 'tac_amplitude_to_db_f64', 'tac_db_to_amplitude_f64'
#: blocks per CU of each family's grid (csrc/elementwise.hip: EW_COMPLEX_NORM, EW_MAGPHASE, EW_DEFAULT; csrc/backward.hip: bw_blocks;
#: csrc/chain_f64.hip: launch_ew) and the elements a thread takes per trip (4 in the 16-byte forms, 1 in the scalar kernels)
PER_CU = {NORM: (2, 4), MAGPHASE: (3, 4), TO_DB: (8, 4), FROM_DB: (8, 4), NORM_BW: (16, 1), MAGPHASE_BW: (16, 1), FROM_DB_BW: (16, 1),
          TO_DB_BW: (16, 4), FROM_DB64: (16, 1)}
ALL_DB_CASES = R.DB_CASES + (R.DB_EQUALITY_CASE,)


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


def counted(tac_, expect, fn):
    """``fn()`` with exactly the launches ``expect``"""
    before = dict(tac_._hip.launches)
    out = fn()
    assert launched_since(tac_, before) == expect, (launched_since(tac_, before), expect)
    return out


def leaf(t):
    return t.detach().cuda().requires_grad_(True)


def grad_of(tac_, expect, outs, x, weights):
    (g,) = counted(tac_, expect, lambda: torch.autograd.grad(outs, x, weights, retain_graph=True, allow_unused=False))
    assert g.dtype == x.dtype and g.shape == x.shape and g.stride() == x.stride()
    return g


def pair_case():
    return R.pair_sweep(), R.grad_weights(R.N_PAIRS, 1), R.grad_weights(R.N_PAIRS, 2)


# ----------------------------------------------------------------------------- 1. core sweep, float32
@pytest.mark.parametrize('p', R.POWERS)
def test_complex_norm_sweep(tac, p):
    z, w, _ = pair_case()
    x = leaf(z)
    out = counted(tac, {NORM: 1}, lambda: tac.complex_norm(x, p))
    R.assert_forward('norm', out, z, p, what='complex_norm, power %g' % p, key=('norm', p))
    g = grad_of(tac, {NORM_BW: 1}, out, x, w.cuda())
    R.assert_grad('norm', g, z, w, p, what='complex_norm backward, power %g' % p, key=('d norm', p))


def test_angle_sweep(tac):
    z, _, w2 = pair_case()
    x = leaf(z)
    out = counted(tac, {MAGPHASE: 1}, lambda: tac.angle(x))
    R.assert_forward('angle', out, z, what='angle', key=('angle',))
    g = grad_of(tac, {MAGPHASE_BW: 1}, out, x, w2.cuda())
    R.assert_grad('magphase', g, z, None, 1.0, second=w2, what='angle backward', key=('d angle',))


@pytest.mark.parametrize('p', R.POWERS)
def test_magphase_sweep(tac, p):
    """both outputs from one launch, and the gradient with both, only the magnitude's and only the phase's arriving"""
    z, w, w2 = pair_case()
    x = leaf(z)
    mag, phase = counted(tac, {MAGPHASE: 1}, lambda: tac.magphase(x, p))
    R.assert_forward('norm', mag, z, p, what='magphase magnitude, power %g' % p, key=('norm', p))
    R.assert_forward('angle', phase, z, what='magphase phase', key=('angle',))
    both = grad_of(tac, {MAGPHASE_BW: 1}, (mag, phase), x, (w.cuda(), w2.cuda()))
    R.assert_grad('magphase', both, z, w, p, second=w2, what='magphase backward, power %g' % p, key=('d magphase', p))
    only_mag = grad_of(tac, {MAGPHASE_BW: 1}, (mag,), x, (w.cuda(),))
    R.assert_grad('norm', only_mag, z, w, p, what='magphase backward, phase unused, power %g' % p, key=('d norm', p))
    only_phase = grad_of(tac, {MAGPHASE_BW: 1}, (phase,), x, (w2.cuda(),))
    R.assert_grad('magphase', only_phase, z, None, 1.0, second=w2, what='magphase backward, magnitude unused', key=('d angle',))


@pytest.mark.parametrize('ref,amin', ALL_DB_CASES)
def test_amplitude_to_db_sweep(tac, ref, amin):
    xs = R.db_sweep(amin)
    below, equal, above = R.clamp_sides(xs, amin)
    assert below >= 2 and above >= 2 and ((ref, amin) != R.DB_EQUALITY_CASE or equal >= 2), (below, equal, above)
    w = R.grad_weights(xs.numel(), 3)
    x = leaf(xs)
    out = counted(tac, {TO_DB: 1}, lambda: tac.amplitude_to_db(x, ref, amin))
    R.assert_forward('to_db', out, xs, ref, amin, what='amplitude_to_db %r (%d below the clamp, %d on it)' % ((ref, amin), below, equal),
                     key=('to_db', ref, amin))
    g = grad_of(tac, {TO_DB_BW: 1}, out, x, w.cuda())
    R.assert_grad('to_db', g, xs, w, ref, amin, what='amplitude_to_db backward %r' % ((ref, amin),), key=('d to_db', ref, amin))
    gv = g.cpu().numpy()
    passes = R.t_passes(xs, amin).numpy()
    assert (gv[~passes] == 0).all() and (gv[passes] != 0).all()


@pytest.mark.parametrize('ref', R.UNDB_REFS)
def test_db_to_amplitude_sweep(tac, ref):
    xs = R.undb_sweep()
    w = R.grad_weights(xs.numel(), 4)
    x = leaf(xs)
    out = counted(tac, {FROM_DB: 1}, lambda: tac.db_to_amplitude(x, ref))
    R.assert_forward('from_db', out, xs, ref, what='db_to_amplitude, ref %g' % ref, key=('from_db', ref))
    g = grad_of(tac, {FROM_DB_BW: 1}, out, x, w.cuda())
    R.assert_grad('from_db', g, xs, w, ref, what='db_to_amplitude backward, ref %g' % ref, key=('d from_db', ref))


# ----------------------------------------------------------------------------- 2. core sweep, float64
needs_longdouble = pytest.mark.skipif(not R.longdouble_ok(), reason='numpy.longdouble has no more mantissa bits than float64 here: '
                                      'nothing on this host can judge a float64 kernel')


@needs_longdouble
@pytest.mark.parametrize('p', R.POWERS)
def test_float64_magphase_sweep(tac, p):
    assert np.finfo(np.longdouble).nmant >= 63
    z = R.pair_sweep(np.float64)
    mag, phase = counted(tac, {MAGPHASE64: 1}, lambda: tac.magphase(z.cuda(), p))
    assert mag.dtype == torch.float64 and phase.dtype == torch.float64
    R.assert_forward('norm', mag, z, p, what='float64 magphase magnitude, power %g' % p, key=('norm64', p))
    R.assert_forward('angle', phase, z, what='float64 magphase phase', key=('angle64',))
    alone = counted(tac, {MAGPHASE64: 1}, lambda: tac.complex_norm(z.cuda(), p))
    assert torch.equal(alone, mag)
    alone = counted(tac, {MAGPHASE64: 1}, lambda: tac.angle(z.cuda()))
    assert torch.equal(alone, phase)


@needs_longdouble
@pytest.mark.parametrize('ref,amin', R.DB_CASES)
def test_float64_amplitude_to_db_sweep(tac, ref, amin):
    xs = R.db_sweep(amin, np.float64)
    below, equal, above = R.clamp_sides(xs, amin)
    assert below >= 2 and above >= 2
    out = counted(tac, {TO_DB64: 1}, lambda: tac.amplitude_to_db(xs.cuda(), ref, amin))
    assert out.dtype == torch.float64
    R.assert_forward('to_db', out, xs, ref, amin, what='float64 amplitude_to_db %r' % ((ref, amin),), key=('to_db64', ref, amin))


@needs_longdouble
@pytest.mark.parametrize('ref', R.UNDB_REFS)
def test_float64_db_to_amplitude_sweep(tac, ref):
    xs = R.undb_sweep(np.float64)
    out = counted(tac, {FROM_DB64: 1}, lambda: tac.db_to_amplitude(xs.cuda(), ref))
    assert out.dtype == torch.float64
    R.assert_forward('from_db', out, xs, ref, what='float64 db_to_amplitude, ref %g' % ref, key=('from_db64', ref))


# ----------------------------------------------------------------------------- 3. the edge table
def test_pair_edges(tac):
    ze = R.pair_edges()
    w = R.grad_weights(ze.shape[0], 6)
    used = set()
    for p in R.POWERS:
        x = leaf(ze)
        mag, phase = counted(tac, {MAGPHASE: 1}, lambda: tac.magphase(x, p))
        out = counted(tac, {NORM: 1}, lambda: tac.complex_norm(x, p))
        assert torch.equal(out.view(torch.int32), mag.detach().view(torch.int32))
        R.assert_edges('norm', out, ze, p, what='complex_norm edges')
        g = grad_of(tac, {NORM_BW: 1}, out, x, w.cuda())
        used |= set(R.assert_edges('norm', g, ze, p, g=w, what='complex_norm backward edges'))
        # the phase unused: its gradient is absent, not a tensor of zeros (0 * inf would be NaN): the magnitude's gradient alone
        g2 = grad_of(tac, {MAGPHASE_BW: 1}, (mag,), x, (w.cuda(),))
        assert np.array_equal(g2.cpu().numpy(), g.cpu().numpy(), equal_nan=True)
    x = leaf(ze)
    out = counted(tac, {MAGPHASE: 1}, lambda: tac.angle(x))
    assert torch.equal(out.view(torch.int32), phase.detach().view(torch.int32))
    R.assert_edges('angle', out, ze, what='angle edges')
    g = grad_of(tac, {MAGPHASE_BW: 1}, out, x, w.cuda())
    used |= set(R.assert_edges('angle', g, ze, g=w, what='angle backward edges'))
    assert used <= set(R.DEVIATIONS), used
    print('deviations met on the pair edges: %r' % sorted(used))


def test_db_edges(tac):
    xe = torch.tensor(R.DB_EDGE_X, dtype=torch.float32)
    w = R.grad_weights(xe.numel(), 7)
    used = set()
    for ref in R.DB_EDGE_REF:
        for amin in R.DB_EDGE_AMIN:
            x = leaf(xe)
            out = counted(tac, {TO_DB: 1}, lambda: tac.amplitude_to_db(x, ref, amin))
            R.assert_edges('to_db', out, xe, ref, amin, what='amplitude_to_db edges')
            g = grad_of(tac, {TO_DB_BW: 1}, out, x, w.cuda())
            used |= set(R.assert_edges('to_db', g, xe, ref, amin, g=w, what='amplitude_to_db backward edges'))
    ue = torch.tensor(R.UNDB_EDGE_X, dtype=torch.float32)
    w = R.grad_weights(ue.numel(), 8)
    for ref in R.UNDB_EDGE_REF:
        x = leaf(ue)
        out = counted(tac, {FROM_DB: 1}, lambda: tac.db_to_amplitude(x, ref))
        used |= set(R.assert_edges('from_db', out, ue, ref, what='db_to_amplitude edges'))
        g = grad_of(tac, {FROM_DB_BW: 1}, out, x, w.cuda())
        used |= set(R.assert_edges('from_db', g, ue, ref, g=w, what='db_to_amplitude backward edges'))
    assert used <= set(R.DEVIATIONS), used
    print('deviations met on the dB edges: %r' % sorted(used))


# ----------------------------------------------------------------------------- 4. placement
LENGTHS = (4096, 1, 2, 3, 4, 5, 7, 8, 1021)
GUARD = 8


def place(values, offset, n, width):
    """``n`` entries (``width`` floats each) of ``values`` at float offset ``offset`` of a fresh 16-byte aligned buffer"""
    buf = torch.zeros(n * width + GUARD, device='cuda')
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + n * width]
    view.copy_(values[:n * width])
    return view


def placement(tac_, name, ins, outs, combos, args_of):
    """Launch entry point ``name`` through the checked launch helper for every length of LENGTHS and every combination of float
    offsets in ``combos`` (one offset per input, then one per output).  ``ins``: ``(flat values on the device, floats per entry)``
    per input (None: the pointer is absent); ``outs``: floats per entry of each output.  The first combination at the first length
    is the base: every other launch must give its bits entry for entry, leave no poison inside its ``n`` entries and touch nothing
    outside them.  ``args_of(in_ptrs, n, out_ptrs)`` orders the arguments."""
    H, ptr = tac_._hip, tac_._native.ptr
    base, flags, labels = None, [], []
    for n in LENGTHS:
        for combo in combos:
            offs_in, offs_out = combo[:len(ins)], combo[len(ins):]
            views = [None if spec is None else place(spec[0], o, n, spec[1]) for spec, o in zip(ins, offs_in)]
            bufs = [H.poison_fill(torch.empty(n * wd + GUARD, device='cuda')) for wd in outs]
            filled = [b[o:o + n * wd] for b, o, wd in zip(bufs, offs_out, outs)]
            before = dict(H.launches)
            H._launch(name, filled[0].device, tuple(filled), *args_of([None if v is None else ptr(v) for v in views], n,
                                                                      [ptr(f) for f in filled]))
            assert launched_since(tac_, before) == {name: 1}
            if base is None:
                base = [f.clone() for f in filled]
            for k, (f, b, buf, wd) in enumerate(zip(filled, base, bufs, outs)):
                same = (f.view(torch.int32) == b[:n * wd].view(torch.int32)).all()
                untouched = H.poison_count(buf) == GUARD
                flags.append(same & untouched)
                labels.append((n, combo, 'output %d' % k))
    flags = torch.stack(flags).cpu().numpy()
    wrong = [labels[i] for i in np.flatnonzero(~flags)]
    assert not wrong, '%s: (n, offsets, output) whose bits differ from the aligned launch or that wrote outside n: %r' % (name, wrong[:12])
    return len(flags)


def test_placement_forward(tac):
    z = R.pair_sweep()[:4096].reshape(-1).cuda()
    ref, amin = R.DB_CASES[1]
    xdb = torch.cat([torch.from_numpy(R.clamp_neighbours(amin)), R.db_sweep(amin)[:4096 - 18]]).cuda()
    xun = R.undb_sweep()[:4096].cuda()
    pair_in_out = list(itertools.product((0, 2), (0, 1, 2, 3)))
    n = 0
    for p in (1.0, 0.7):
        n += placement(tac, NORM, [(z, 2)], [1], pair_in_out, lambda i, n, o: (i[0], n, p, o[0]))
        n += placement(tac, MAGPHASE, [(z, 2)], [1, 1], [(a, m, ph) for a in (0, 2) for m, ph in ((0, 0), (1, 0), (0, 3), (2, 2), (3, 1))],
                       lambda i, n, o: (i[0], n, p, o[0], o[1]))
    n += placement(tac, MAGPHASE, [(z, 2)], [1], pair_in_out, lambda i, n, o: (i[0], n, 1.0, None, o[0]))
    every = list(itertools.product(range(4), range(4)))
    n += placement(tac, TO_DB, [(xdb, 1)], [1], every, lambda i, n, o: (i[0], n, ref, amin, o[0]))
    n += placement(tac, FROM_DB, [(xun, 1)], [1], every, lambda i, n, o: (i[0], n, 3.5, o[0]))
    print('%d placed outputs gave the bits of the aligned launch' % n)


def test_placement_backward(tac):
    z = R.pair_sweep()[:4096].reshape(-1).cuda()
    w, w2 = R.grad_weights(4096, 1).cuda(), R.grad_weights(4096, 2).cuda()
    ref, amin = R.DB_CASES[1]
    xdb = torch.cat([torch.from_numpy(R.clamp_neighbours(amin)), R.db_sweep(amin)[:4096 - 18]]).cuda()
    xun = R.undb_sweep()[:4096].cuda()
    n = 0
    # the pair kernels move (re, im) as one 8-byte access: pairs sit at even float offsets
    pairs = list(itertools.product((0, 2), (0, 1, 3), (0, 2)))
    for p in (1.0, 0.7):
        n += placement(tac, NORM_BW, [(z, 2), (w, 1)], [2], pairs, lambda i, n, o: (i[0], i[1], n, p, o[0]))
        n += placement(tac, MAGPHASE_BW, [(z, 2), (w, 1), (w2, 1)], [2],
                       [(a, b, c, d) for a in (0, 2) for b, c in ((0, 0), (1, 2), (3, 1)) for d in (0, 2)],
                       lambda i, n, o: (i[0], i[1], i[2], n, p, o[0]))
    n += placement(tac, MAGPHASE_BW, [(z, 2), None, (w2, 1)], [2], [(a, 0, c, d) for a in (0, 2) for c in (0, 1, 3) for d in (0, 2)],
                   lambda i, n, o: (i[0], None, i[2], n, 1.0, o[0]))
    three = [(0, 0, 0), (1, 0, 0), (0, 2, 0), (0, 0, 3), (1, 2, 3), (1, 1, 1), (3, 3, 3), (2, 0, 2)]
    n += placement(tac, TO_DB_BW, [(xdb, 1), (w, 1)], [1], three, lambda i, n, o: (i[0], i[1], n, amin, o[0]))
    n += placement(tac, FROM_DB_BW, [(xun, 1), (w, 1)], [1], three, lambda i, n, o: (i[0], i[1], n, 3.5, o[0]))
    print('%d placed outputs gave the bits of the aligned launch' % n)


# ----------------------------------------------------------------------------- 5. layouts
def relaid(t, order):
    """the values of ``t`` in the same logical order, stored with the dimensions in ``order`` (dense, not contiguous)"""
    inverse = [order.index(d) for d in range(t.dim())]
    out = t.permute(*order).contiguous().permute(*inverse)
    assert out.shape == t.shape and not out.is_contiguous()
    return out


@pytest.mark.parametrize('layout', ['permuted', 'frame-major'])
def test_pair_layouts(tac, layout):
    """a dense permuted tensor keeps its layout; the (..., F, T, 2) view of frame-major storage is what the STFT kernels return.
    Gradients arrive once in the output's own layout (no copy) and once contiguous (the copy branch of ``*_backward``)."""
    z, w, w2 = pair_case()
    p = 0.7
    zz = relaid(z.view(*R.PAIR_SHAPE, 2), (1, 0, 2, 3) if layout == 'permuted' else (0, 2, 1, 3))
    x = leaf(zz)
    assert x.stride() == zz.stride()
    want_stride = tuple(s // 2 for s in zz.stride()[:-1])
    out = counted(tac, {NORM: 1}, lambda: tac.complex_norm(x, p))
    mag, phase = counted(tac, {MAGPHASE: 1}, lambda: tac.magphase(x, p))
    assert out.stride() == want_stride and mag.stride() == want_stride and phase.stride() == want_stride
    R.assert_forward('norm', out, z, p, what='complex_norm, %s' % layout, key=('norm', p))
    assert torch.equal(mag, out)
    R.assert_forward('angle', phase, z, what='magphase phase, %s' % layout, key=('angle',))
    wl, wl2 = w.view(R.PAIR_SHAPE).cuda(), w2.view(R.PAIR_SHAPE).cuda()
    assert wl.is_contiguous() and wl.stride() != out.stride()
    for how, (a, b) in (('copied', (wl, wl2)), ('in place', (torch.empty_like(out).copy_(wl), torch.empty_like(out).copy_(wl2)))):
        assert (a.stride() == out.stride()) == (how == 'in place')
        g = grad_of(tac, {NORM_BW: 1}, out, x, a)
        R.assert_grad('norm', g, z, w, p, what='complex_norm backward, %s, gradient %s' % (layout, how), key=('d norm', p))
        g = grad_of(tac, {MAGPHASE_BW: 1}, (mag, phase), x, (a, b))
        R.assert_grad('magphase', g, z, w, p, second=w2, what='magphase backward, %s, gradient %s' % (layout, how), key=('d magphase', p))


def test_unary_layouts(tac):
    ref, amin = R.DB_CASES[0]
    xs = R.db_sweep(amin)[:R.N_DB]
    us = R.undb_sweep()
    w = R.grad_weights(R.N_DB, 5)
    wl = w.view(R.DB_SHAPE).cuda()
    for name, op, bw, src, call, params in (('amplitude_to_db', TO_DB, TO_DB_BW, xs, lambda t: tac.amplitude_to_db(t, ref, amin), (ref, amin)),
                                            ('db_to_amplitude', FROM_DB, FROM_DB_BW, us, lambda t: tac.db_to_amplitude(t, 3.5), (3.5,))):
        rules_op = 'to_db' if op == TO_DB else 'from_db'
        xx = relaid(src.view(R.DB_SHAPE), (2, 0, 1))
        x = leaf(xx)
        out = counted(tac, {op: 1}, lambda: call(x))
        assert out.stride() == xx.stride()
        R.assert_forward(rules_op, out, src, *params, what='%s, permuted' % name, key=('layout', rules_op))
        for how, a in (('copied', wl), ('in place', torch.empty_like(out).copy_(wl))):
            assert (a.stride() == out.stride()) == (how == 'in place')
            g = grad_of(tac, {bw: 1}, out, x, a)
            R.assert_grad(rules_op, g, src, w, *params, what='%s backward, permuted, gradient %s' % (name, how), key=('layout d', rules_op))


# ----------------------------------------------------------------------------- 6. the second trip of the grid
def one_trip(name):
    assert not os.environ.get('TAC_EW_BLOCKS_PER_CU'), 'the grids under test are the kernels\' own, not an A/B override'
    per_cu, per_thread = PER_CU[name]
    return torch.cuda.get_device_properties(0).multi_processor_count * per_cu * 256 * per_thread


def repeated(t, n):
    return t[torch.arange(n) % t.shape[0]]


def test_second_trip_pairs(tac):
    """complex_norm, magphase and their gradient kernels with more pairs than one trip of the largest of their grids: every pair is
    checked, the input is the core sweep repeated"""
    n = max(one_trip(k) for k in (NORM, MAGPHASE, NORM_BW, MAGPHASE_BW)) + 1021
    assert all(n > one_trip(k) for k in (NORM, MAGPHASE, NORM_BW, MAGPHASE_BW)) and n * 8 <= 16 * 2 ** 20
    z, w, w2 = pair_case()
    p = 0.7
    x = leaf(repeated(z, n))
    wn, wn2 = repeated(w, n).cuda(), repeated(w2, n).cuda()
    out = counted(tac, {NORM: 1}, lambda: tac.complex_norm(x, p))
    R.assert_held(out.detach().cpu().numpy(), *R.tiled(R.forward_reference('norm', z, p, key=('norm', p)), n), 'complex_norm, %d pairs' % n)
    mag, phase = counted(tac, {MAGPHASE: 1}, lambda: tac.magphase(x, p))
    assert torch.equal(mag, out)
    R.assert_held(phase.detach().cpu().numpy(), *R.tiled(R.forward_reference('angle', z, key=('angle',)), n), 'magphase phase, %d pairs' % n)
    g = grad_of(tac, {NORM_BW: 1}, out, x, wn)
    ref = R.cached(('d norm', p), lambda: R.grad_reference('norm', z, w, p))
    R.assert_held(g.cpu().numpy(), *R.tiled(ref, n), 'complex_norm backward, %d pairs' % n)
    g = grad_of(tac, {MAGPHASE_BW: 1}, (mag, phase), x, (wn, wn2))
    ref = R.cached(('d magphase', p), lambda: R.grad_reference('magphase', z, w, p, second=w2))
    R.assert_held(g.cpu().numpy(), *R.tiled(ref, n), 'magphase backward, %d pairs' % n)


def test_second_trip_unary(tac):
    ref, amin = R.DB_CASES[0]
    xs = R.db_sweep(amin)
    w = R.grad_weights(xs.numel(), 3)
    n = max(one_trip(TO_DB), one_trip(TO_DB_BW)) + 1021
    assert n > one_trip(TO_DB) and n > one_trip(TO_DB_BW) and n * 4 <= 17 * 2 ** 20
    x = leaf(repeated(xs, n))
    out = counted(tac, {TO_DB: 1}, lambda: tac.amplitude_to_db(x, ref, amin))
    R.assert_held(out.detach().cpu().numpy(), *R.tiled(R.forward_reference('to_db', xs, ref, amin, key=('to_db', ref, amin)), n),
                  'amplitude_to_db, %d elements' % n)
    g = grad_of(tac, {TO_DB_BW: 1}, out, x, repeated(w, n).cuda())
    pair = R.cached(('d to_db', ref, amin), lambda: R.grad_reference('to_db', xs, w, ref, amin))
    R.assert_held(g.cpu().numpy(), *R.tiled(pair, n), 'amplitude_to_db backward, %d elements' % n)
    del x, out, g

    us = R.undb_sweep()
    w = R.grad_weights(us.numel(), 4)
    n = max(one_trip(FROM_DB), one_trip(FROM_DB_BW)) + 1021
    assert n > one_trip(FROM_DB) and n > one_trip(FROM_DB_BW)
    x = leaf(repeated(us, n))
    out = counted(tac, {FROM_DB: 1}, lambda: tac.db_to_amplitude(x, 3.5))
    R.assert_held(out.detach().cpu().numpy(), *R.tiled(R.forward_reference('from_db', us, 3.5, key=('from_db', 3.5)), n),
                  'db_to_amplitude, %d elements' % n)
    g = grad_of(tac, {FROM_DB_BW: 1}, out, x, repeated(w, n).cuda())
    pair = R.cached(('d from_db', 3.5), lambda: R.grad_reference('from_db', us, w, 3.5))
    R.assert_held(g.cpu().numpy(), *R.tiled(pair, n), 'db_to_amplitude backward, %d elements' % n)


@needs_longdouble
def test_second_trip_float64(tac):
    us = R.undb_sweep(np.float64)
    n = one_trip(FROM_DB64) + 1021
    assert n > one_trip(FROM_DB64) and n * 8 <= 16 * 2 ** 20
    out = counted(tac, {FROM_DB64: 1}, lambda: tac.db_to_amplitude(repeated(us, n).cuda(), 3.5))
    R.assert_held(out.cpu().numpy(), *R.tiled(R.forward_reference('from_db', us, 3.5, key=('from_db64', 3.5)), n),
                  'float64 db_to_amplitude, %d elements' % n)
