"""-m gpu: ``soft_dtw`` / ``SoftDTW`` on the gfx950 kernels (csrc/soft_dtw.hip) — strict mode and poisoned outputs on.

Reference and bounds: tests/soft_dtw_rules.py — the float64 recursion fed the SAME float32 inputs and the derived bounds of the
value, the alignment and the gradients.  Every bound test prints its worst error as a fraction of the bound.  Shapes are
``(B, N, M, D)``."""
import pytest
import torch

import soft_dtw_rules as R

pytestmark = pytest.mark.gpu

FORWARD, GRAD, ALIGN = 'tac_soft_dtw_f32', 'tac_soft_dtw_grad_f32', 'tac_soft_dtw_alignment_f32'
SMALL = [(2, 1, 1, 1), (3, 5, 7, 3), (2, 7, 5, 4), (1, 1, 9, 2), (1, 9, 1, 2)]
SEAMS = [(1, n, 70, 2) for n in (63, 64, 65)] + [(1, 70, m, 2) for m in (63, 64, 65)]
FEATURES = [(2, 40, 40, d) for d in (1, 3, 4, 5, 33, 130, 256)]     # (above 128 a gradient wave has a second column block)
TILES = [(2, 130, 97, 80)]                      # several gradient tiles each way, three column blocks


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


@pytest.fixture(autouse=True)
def every_output_written(tac):
    tac._hip.poison_report()
    yield
    left = tac._hip.poison_report()
    assert not left, 'kernel outputs left unwritten (poisoned elements per entry point): %r' % left


def launched_since(tac_, before):
    now = tac_._hip.launches
    return {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)}


def weights_for(B):                             # a non-uniform incoming gradient, both signs, never zero
    return 0.5 - 0.7 * torch.arange(B, dtype=torch.float32)


def run(tac_, x, y, gamma, xl=None, yl=None, w=None):
    """``(value, grad_x, grad_y)`` through the public functional, the launches counted: one forward, one backward"""
    xg, yg = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
    before = dict(tac_._hip.launches)
    value = tac_.soft_dtw(xg, yg, gamma, xl, yl)
    assert launched_since(tac_, before) == {FORWARD: 1}, launched_since(tac_, before)
    assert value.dtype == torch.float32 and tuple(value.shape) == (x.shape[0],)
    before = dict(tac_._hip.launches)
    gx, gy = torch.autograd.grad(value, (xg, yg), torch.ones_like(value) if w is None else w.to(value.device))
    assert launched_since(tac_, before) == {GRAD: 1}, launched_since(tac_, before)
    return value.detach(), gx, gy


VIEWS = {
    'contiguous': lambda t: t.cuda(),
    'misaligned': lambda t: torch.cat([t[..., :1], t], -1).cuda()[..., 1:],
    'transposed': lambda t: t.transpose(1, 2).contiguous().cuda().transpose(1, 2),
    'slice': lambda t: torch.nn.functional.pad(t, (0, 3, 0, 2), value=-1.0).cuda()[:, :t.shape[1], :t.shape[2]],
}


def held(tac_, shape, gamma=1.0, view='contiguous', xl=None, yl=None, gradients=True):
    x, y = R.make_case(*shape)
    w = weights_for(shape[0])
    ref = R.reference((shape, gamma, str(xl), str(yl)), x, y, gamma, xl, yl, w)
    xv, yv = VIEWS[view](x), VIEWS[view](y)
    what = '(B, N, M, D) = %r, gamma %g, %s' % (shape, gamma, view)
    if not gradients:
        with torch.no_grad():
            value = tac_.soft_dtw(xv, yv, gamma, xl, yl)
        R.assert_within(value, ref.value, ref.value_bound, what + ' value')
        return value, None, None
    value, gx, gy = run(tac_, xv, yv, gamma, xl, yl, w)
    if view in ('contiguous', 'transposed'):
        assert gx.stride() == xv.stride() and gy.stride() == yv.stride()    # the gradients in the layout of dense inputs
    R.assert_within(value, ref.value, ref.value_bound, what + ' value')
    R.assert_within(gx, ref.gx, ref.gx_bound, what + ' grad_x'), R.assert_within(gy, ref.gy, ref.gy_bound, what + ' grad_y')
    return value, gx, gy


@pytest.mark.parametrize('shape', SMALL + SEAMS + FEATURES + TILES)
@pytest.mark.parametrize('gamma', [0.1, 1.0])
def test_value_and_gradients(tac, shape, gamma):
    held(tac, shape, gamma)


@pytest.mark.parametrize('gamma', [0.01, 100.0])
def test_value_at_extreme_gamma(tac, gamma):
    before = dict(tac._hip.launches)
    held(tac, (3, 5, 7, 3), gamma, gradients=False), held(tac, (2, 40, 40, 33), gamma, gradients=False)
    assert launched_since(tac, before) == {FORWARD: 2}                 # a forward without grad: one entry point and nothing else


def test_rows_per_lane_boundaries_and_longest_row(tac):
    lib = tac._native.lib()
    lanes, longest = lib.tac_soft_dtw_lanes(), lib.tac_soft_dtw_max_len()
    edges = [n for n in range(lanes, longest, lanes) if lib.tac_soft_dtw_rows_per_lane(n) != lib.tac_soft_dtw_rows_per_lane(n + 1)]
    assert edges, 'the plan has no rows-per-lane boundary below its longest row'
    for n in [v for e in edges for v in (e, e + 1)] + [longest]:
        held(tac, (1, n, 8, 2))
    held(tac, (1, 8, longest, 2), gradients=False)


def test_ragged_batch_and_an_invalid_entry(tac):
    B, N, M, D = 4, 37, 70, 5
    xl, yl = [N, 1, N, (N + 1) // 2], [M, M, 1, (M + 2) // 3]
    value, gx, gy = held(tac, (B, N, M, D), xl=xl, yl=yl)
    for b in range(B):
        assert not gx[b, xl[b]:].any() and not gy[b, yl[b]:].any()   # exactly zero on the padding
    x, y = R.make_case(B, N, M, D)
    for bad_xl, bad_yl in (([N, 0, N, 19], yl), (xl, [M, M, M + 1, 24])):
        v2, gx2, gy2 = run(tac, x.cuda(), y.cuda(), 1.0, bad_xl, bad_yl, weights_for(B))
        bad = [b for b in range(B) if (bad_xl[b], bad_yl[b]) != (xl[b], yl[b])]
        good = [b for b in range(B) if b not in bad]
        assert v2[bad].isnan().all() and gx2[bad].isnan().all() and gy2[bad].isnan().all()
        assert torch.equal(v2[good], value[good]) and torch.equal(gx2[good], gx[good]) and torch.equal(gy2[good], gy[good])


def test_identical_sequences(tac):
    x, _ = R.make_case(2, 45, 45, 7)
    ref = R.reference('identical', x, x, 1.0)
    with torch.no_grad():
        R.assert_within(tac.soft_dtw(x.cuda(), x.cuda(), 1.0), ref.value, ref.value_bound, 'x against x')
    delta = tac._hip.soft_dtw_forward(x.cuda(), x.cuda(), torch.tensor([45, 45]), torch.tensor([45, 45]), 1.0, False)[1]
    assert not delta[:, 0::2][:, torch.arange(45), torch.arange(45)].any()      # cost (i, i): row 2 i, position i — exactly zero
    assert torch.equal(tac.soft_dtw(x.cuda(), x.cuda(), 1.0, normalize=True), torch.zeros(2, device='cuda'))


@pytest.mark.parametrize('view', ['misaligned', 'transposed', 'slice'])
def test_views_give_the_same_bits(tac, view):
    shape = (2, 40, 33, 8)
    plain, other = held(tac, shape), held(tac, shape, view=view)
    for a, b in zip(plain, other):
        assert torch.equal(a, b)                                    # the 16-byte and the dword form round alike


def test_alignment(tac):
    shape, xl, yl = (3, 37, 70, 5), [37, 20, 1], [70, 33, 70]
    x, y = R.make_case(*shape)
    ref = R.reference((shape, 'E'), x, y, 1.0, xl, yl)
    before = dict(tac._hip.launches)
    value, E = tac.soft_dtw(x.cuda(), y.cuda(), 1.0, xl, yl, return_alignment=True)
    assert launched_since(tac, before) == {FORWARD: 1, ALIGN: 1}
    assert E.dtype == torch.float32 and tuple(E.shape) == (3, 37, 70) and float(E.max()) <= 1.0
    R.assert_within(E, ref.E, ref.E_bound, 'alignment')
    rows = E.double().sum(2).cpu().numpy()
    for b in range(3):                                              # every path crosses every row of the entry
        assert (rows[b, :xl[b]] >= 1.0 - ref.E_bound[b].sum(1)[:xl[b]]).all() and not rows[b, xl[b]:].any()


def test_reproducible_and_independent_of_the_batch(tac):
    x, y = (t.cuda() for t in R.make_case(3, 65, 70, 5))
    w = weights_for(3)
    first, again, alone = run(tac, x, y, 1.0, w=w), run(tac, x, y, 1.0, w=w), run(tac, x[:1], y[:1], 1.0, w=w[:1])
    for a, b, c in zip(first, again, alone):
        assert torch.equal(a, b) and torch.equal(a[:1], c)


def test_layer_and_refusals(tac):
    x, y = (t.cuda() for t in R.make_case(2, 9, 7, 3))
    assert torch.equal(tac.SoftDTW(0.5, reduction='sum')(x, y), tac.soft_dtw(x, y, 0.5).sum())
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.soft_dtw(x.double(), y.double())
    xg = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match='double backward'):
        torch.autograd.grad(tac.soft_dtw(xg, y).sum(), xg, create_graph=True)
