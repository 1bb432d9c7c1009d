"""-m gpu: ``rnnt_loss`` / ``RNNTLoss`` on the gfx950 kernels (csrc/rnnt.hip) — strict mode and poisoned outputs on.

Reference and bounds: tests/rnnt_rules.py — the float64 recursion fed the SAME float32 logits, its autograd gradient, and the
derived bounds ``E_b`` (cost) and ``4 E_b + 2^-23`` (gradient element, before the ``grad_costs`` scale).  Every test prints its worst
error as a fraction of the bound.  Shapes are the smallest at which each mechanism of the kernels can go wrong."""
import pytest
import torch

import rnnt_rules as R

pytestmark = pytest.mark.gpu

ROWS, LATTICE, GRAD = 'tac_rnnt_rows_f32', 'tac_rnnt_lattice_f32', 'tac_rnnt_grad_f32'
FORWARD = {ROWS: 1, LATTICE: 1}


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


def run(tac_, logits, targets, tl, ul, grad_costs=None, **kw):
    """``(costs, grad)`` of device tensors through the public functional, the launches counted: two forward, one backward"""
    x = logits.detach().requires_grad_(True)
    before = dict(tac_._hip.launches)
    costs = tac_.rnnt_loss(x, targets, tl, ul, reduction='none', **kw)
    assert launched_since(tac_, before) == FORWARD, launched_since(tac_, before)
    assert costs.dtype == torch.float32 and tuple(costs.shape) == (logits.shape[0],)
    before = dict(tac_._hip.launches)
    weights = torch.ones_like(costs) if grad_costs is None else grad_costs
    (grad,) = torch.autograd.grad(costs, x, weights)
    assert launched_since(tac_, before) == {GRAD: 1}, launched_since(tac_, before)
    assert grad.is_contiguous() and tuple(grad.shape) == tuple(logits.shape)
    return costs.detach(), grad


def on_device(case):
    return tuple(t.cuda() for t in case)


def weights_for(B):
    """a non-uniform incoming gradient, both signs"""
    return torch.linspace(0.5, -1.5, B)


def held(tac_, shape, blank=-1, seed=1, what=None, **kw):
    case = R.make_case(*shape, blank=blank, seed=seed)
    ref = R.reference(('gpu', shape, blank, seed), *case, blank=blank)
    w = weights_for(shape[0])
    costs, grad = run(tac_, *on_device(case), grad_costs=w.cuda(), blank=blank, **kw)
    what = what or '(B, T, U, V) = %r, blank %d' % (shape, blank)
    return R.assert_costs(costs, ref, what), R.assert_grad(grad, ref, what, grad_costs=w)


# ----------------------------------------------------------------------------- 1. bounds
@pytest.mark.parametrize('shape', [(3, 7, 4, 6), (2, 5, 0, 3), (2, 1, 3, 5)])
@pytest.mark.parametrize('blank_at', ['first', 'last', 'middle'])
def test_small_lattices(tac, shape, blank_at):
    """ragged lengths, empty targets, a single frame; blank first, last (-1) and in the middle"""
    held(tac, shape, blank={'first': 0, 'last': -1, 'middle': shape[3] // 2}[blank_at])


@pytest.mark.parametrize('U1', [63, 64, 65, 129])
def test_wave_edge_and_lds_hand_over(tac, U1):
    """one wave up to 64 columns, the boundary value through the LDS above"""
    held(tac, (2, 9, U1 - 1, 8), blank=3)


def test_long_lattice_of_characters(tac):
    held(tac, (2, 70, 66, 29), blank=0)


@pytest.mark.parametrize('V', [2, 3, 4, 5, 16, 17, 20, 63, 64, 68, 256, 257, 260, 1024, 1025, 1028])
def test_class_axis(tac, V):
    """dword and 16-byte loads, several rows per wave (V <= 16: a lane per row; 17 .. 32: two lanes; …; above 512: a wave), the row
    in one batch of registers (V <= 1024) and the online reduction over batches (1025, 1028)"""
    held(tac, (2, 4, 3, V), blank=-1 if V % 2 else 0)


# ----------------------------------------------------------------------------- 2. clamp, the unfused form, -inf logits
def test_clamp_bites(tac):
    shape, clamp = (3, 7, 4, 6), 0.05
    case = R.make_case(*shape, seed=1)
    ref = R.reference(('gpu', shape, -1, 1), *case)
    share = float((ref.grad.abs() > clamp).double().mean())
    assert 0.0 < share < 1.0
    w = weights_for(3)
    costs, grad = run(tac, *on_device(case), grad_costs=w.cuda(), clamp=clamp)
    R.assert_costs(costs, ref, 'clamp')
    R.assert_grad(grad, ref, 'clamp %.2f (%.0f %% of the elements clipped)' % (clamp, 100 * share), grad_costs=w, clamp=clamp)
    assert float((grad.cpu().abs() / w.abs()[:, None, None, None]).max()) <= clamp * (1 + 2.0 ** -23)


@pytest.mark.parametrize('V', [6, 29, 1025])
def test_unfused_on_log_probabilities(tac, V):
    shape = (3, 7, 4, V)
    logits, targets, tl, ul = R.make_case(*shape, blank=1, seed=2)
    lp = torch.log_softmax(logits, -1)
    ref = R.Reference(lp, targets, tl, ul, blank=1, fused=False)
    w = weights_for(3)
    costs, grad = run(tac, lp.cuda(), targets.cuda(), tl.cuda(), ul.cuda(), grad_costs=w.cuda(), blank=1, fused_log_softmax=False)
    R.assert_costs(costs, ref, 'unfused, V %d' % V)
    R.assert_grad(grad, ref, 'unfused, V %d' % V, grad_costs=w)


def test_minus_infinity_logits(tac):
    """a class masked out everywhere and one label impossible at one cell: cost and gradient stay finite and inside the bounds"""
    shape = (3, 7, 4, 6)
    logits, targets, tl, ul = R.make_case(*shape, blank=0, seed=4)
    targets = targets.clamp(max=4)                                 # class 5 is used by no target
    logits[..., 5] = float('-inf')
    logits[0, 2, 1, int(targets[0, 1])] = float('-inf')            # (t = 2, u = 1): the paths around that cell remain
    ref = R.Reference(logits, targets, tl, ul, blank=0)
    assert torch.isfinite(ref.costs).all() and torch.isfinite(ref.grad).all()
    w = weights_for(3)
    costs, grad = run(tac, logits.cuda(), targets.cuda(), tl.cuda(), ul.cuda(), grad_costs=w.cuda(), blank=0)
    assert torch.isfinite(costs).all() and torch.isfinite(grad).all()
    R.assert_costs(costs, ref, '-inf logits')
    R.assert_grad(grad, ref, '-inf logits', grad_costs=w)
    assert float(grad[..., 5].abs().max()) == 0.0


# ----------------------------------------------------------------------------- 3. invalid entries
@pytest.mark.parametrize('fault', ['Tb = 0', 'Tb = T + 1', 'Ub = U + 1', 'target = V'])
@pytest.mark.parametrize('where', [0, 1, 2])
def test_invalid_entry_is_nan_and_alone(tac, fault, where):
    """Every index the kernels form is checked against the tensor's own extents before it is used (csrc/rnnt.hip: ``entry_ok``, the
    label range), so an entry outside its ranges reads and writes nothing outside the tensors."""
    shape = (3, 7, 4, 6)
    B, T, U, V = shape
    logits, targets, tl, ul = R.make_case(*shape, seed=5, full=True)
    clean = run(tac, *on_device((logits, targets, tl, ul)), grad_costs=weights_for(3).cuda())
    targets, tl, ul = targets.clone(), tl.clone(), ul.clone()
    if fault == 'Tb = 0':
        tl[where] = 0
    elif fault == 'Tb = T + 1':
        tl[where] = T + 1
    elif fault == 'Ub = U + 1':
        ul[where] = U + 1
    else:
        targets[where, 2] = V
    costs, grad = run(tac, *on_device((logits, targets, tl, ul)), grad_costs=weights_for(3).cuda())
    others = [b for b in range(B) if b != where]
    assert bool(costs[where].isnan()) and bool(grad[where].isnan().all())
    assert torch.equal(costs[others], clean[0][others]) and torch.equal(grad[others], clean[1][others])


# ----------------------------------------------------------------------------- 4. layouts, batch independence, repeatability
def test_layouts_give_the_bits_of_the_contiguous_copy(tac):
    B, T, U, V = 3, 7, 4, 8
    logits, targets, tl, ul = on_device(R.make_case(B, T, U, V, seed=6))
    w = weights_for(B).cuda()
    want = run(tac, logits, targets, tl, ul, grad_costs=w)
    again = run(tac, logits, targets, tl, ul, grad_costs=w)
    assert torch.equal(want[0], again[0]) and torch.equal(want[1], again[1])            # two runs of the same call

    big = torch.randn((B, T + 3, U + 3, V), device='cuda')
    big[:, :T, :U + 1] = logits
    view = big[:, :T, :U + 1]
    assert not view.is_contiguous()
    got = run(tac, view, targets, tl, ul, grad_costs=w)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])

    stack = torch.randn((B + 2, T, U + 1, V), device='cuda')
    stack[1:1 + B] = logits
    got = run(tac, stack[1:1 + B], targets, tl, ul, grad_costs=w)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])

    flat = torch.zeros(logits.numel() + 1, device='cuda')
    shifted = flat[1:].view(B, T, U + 1, V)
    shifted.copy_(logits)
    assert shifted.data_ptr() % 16 == 4                                                 # dword loads; V % 4 == 0 took 16-byte ones
    got = run(tac, shifted, targets, tl, ul, grad_costs=w)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])

    wide = torch.randn((B, T, U + 1, V + 3), device='cuda')                             # a slice of the class axis: unit stride, dwords
    wide[..., :V] = logits
    got = run(tac, wide[..., :V], targets, tl, ul, grad_costs=w)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize('shape', [(3, 7, 4, 6), (2, 9, 64, 8), (2, 4, 3, 1025)])
def test_an_entry_does_not_depend_on_its_batch(tac, shape):
    logits, targets, tl, ul = on_device(R.make_case(*shape, seed=7))
    w = weights_for(shape[0]).cuda()
    costs, grad = run(tac, logits, targets, tl, ul, grad_costs=w)
    for b in range(shape[0]):
        Tb, Ub = int(tl[b]), int(ul[b])
        alone = run(tac, logits[b:b + 1, :Tb, :Ub + 1], targets[b:b + 1, :Ub].contiguous(), tl[b:b + 1], ul[b:b + 1],
                    grad_costs=w[b:b + 1])
        assert torch.equal(alone[0], costs[b:b + 1]), (shape, b)
        assert torch.equal(alone[1], grad[b:b + 1, :Tb, :Ub + 1]), (shape, b)
        assert float(grad[b, Tb:].abs().sum()) == 0.0 and float(grad[b, :, Ub + 1:].abs().sum()) == 0.0


# ----------------------------------------------------------------------------- 5. announced routes
def test_announced_routes(tac):
    shape = (3, 7, 4, 6)
    case = R.make_case(*shape, seed=8)
    ref = R.reference(('gpu', shape, -1, 8), *case)
    logits, targets, tl, ul = on_device(case)
    limit = tac._hip.rnnt_max_targets()
    assert limit >= 256
    long_case = R.make_case(1, 2, limit, 3, seed=8)
    long_ref = R.reference(('gpu long', limit), *long_case)
    one = (logits[:1].expand(3, -1, -1, -1), targets[:1].expand(3, -1).contiguous(), tl[:1].expand(3).contiguous(),
           ul[:1].expand(3).contiguous())
    cases = [('dtype float64', (logits.double(), targets, tl, ul), ref.costs, 1e-9),
             ('dtype float16', (logits.half(), targets, tl, ul), ref.costs, 2e-2),
             ('expanded or non-positive strides', one, ref.costs[:1].expand(3), 1e-4),
             ('a target axis of %d' % (limit + 1), on_device(long_case), long_ref.costs, 1e-4)]
    before = dict(tac._hip.launches)
    for reason, args, want, tol in cases:
        with pytest.raises(RuntimeError, match=reason):
            tac.rnnt_loss(*args, reduction='none')
    x = logits.clone().requires_grad_(True)
    total = tac.rnnt_loss(x, targets, tl, ul, reduction='sum')
    with pytest.raises(RuntimeError, match='double backward'):                          # a backward pass that is itself recorded
        torch.autograd.grad(total, x, create_graph=True)
    assert set(launched_since(tac, before)) <= {ROWS, LATTICE, GRAD}
    tac.set_strict(False)
    try:
        for key in [k for k in tac._ops._warned if k[0] == 'rnnt_loss']:
            tac._ops._warned.discard(key)
        for reason, args, want, tol in cases:
            before = dict(tac._hip.launches)
            with pytest.warns(tac.CompositeRouteWarning):
                got = tac.rnnt_loss(*args, reduction='none')
            assert launched_since(tac, before) == {}, reason
            assert got.dtype == args[0].dtype
            err = float((got.cpu().double() - want).abs().max())
            assert err <= tol * float(want.abs().max()), (reason, err)
        # the gradient of an announced route is announced too and agrees with the reference
        x64 = logits.double().requires_grad_(True)
        with pytest.warns(tac.CompositeRouteWarning):
            (g64,) = torch.autograd.grad(tac.rnnt_loss(x64, targets, tl, ul, reduction='sum'), x64)
        assert float((g64.cpu() - ref.grad).abs().max()) < 1e-9
        total = tac.rnnt_loss(x, targets, tl, ul, reduction='sum')
        with pytest.warns(tac.CompositeRouteWarning):
            (first,) = torch.autograd.grad(total, x, create_graph=True)
        assert float((first.detach().cpu().double() - ref.grad).abs().max()) <= float(ref.grad_bound.max())
        (second,) = torch.autograd.grad(first.square().sum(), x)
        assert bool(torch.isfinite(second).all()) and float(second.abs().max()) > 0.0
    finally:
        tac.set_strict(True)


# ----------------------------------------------------------------------------- 6. 64-bit offsets
def test_offsets_beyond_two_to_the_31(tac):
    """logits of 2 x 264 x 64 x 64000 = 2.16e9 elements: entry 1 starts beyond 2^32 bytes and ends beyond 2^31 elements.  Its cost
    and gradient block must be the bits of the same call on ``logits[1:2]`` alone; the values are held by the small cases."""
    B, T, U1, V = 2, 264, 64, 64000
    assert B * T * U1 * V > 2 ** 31
    gen = torch.Generator(device='cuda').manual_seed(9)
    logits = torch.randn((B, T, U1, V), device='cuda', generator=gen)
    targets = torch.randint(1, V, (B, U1 - 1), device='cuda', generator=gen).to(torch.int32)
    tl = torch.tensor([T, T - 3], dtype=torch.int32, device='cuda')
    ul = torch.tensor([U1 - 1, U1 - 2], dtype=torch.int32, device='cuda')
    w = torch.tensor([1.0, -0.5], device='cuda')
    costs, grad = run(tac, logits, targets, tl, ul, grad_costs=w, blank=0)
    block = grad[1:2].clone()
    del grad
    assert bool(torch.isfinite(costs).all())
    alone = run(tac, logits[1:2], targets[1:2], tl[1:2], ul[1:2], grad_costs=w[1:2], blank=0)
    assert torch.equal(alone[0], costs[1:2])
    assert torch.equal(alone[1], block)
    assert float(block[0, T - 3:].abs().max()) == 0.0 and float(block[0, :T - 3, :U1 - 1].abs().max()) > 0.0
    del logits, block, alone
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- 7. training
def test_training_chain_stays_on_the_kernels(tac):
    """waveform -> KaldiFbank -> a small linear joint -> RNNTLoss under strict mode: forward and backward without a stock-torch route"""
    torch.manual_seed(10)
    B, U, V = 2, 5, 12
    wave = torch.randn((B, 16000), device='cuda') * 0.1
    feats = tac.KaldiFbank(num_mel_bins=23).cuda()(wave)                       # (B, T, 23)
    T = feats.shape[1]
    enc = torch.nn.Linear(23, V).cuda()
    pred = torch.nn.Embedding(U + 1, V).cuda()
    logits = enc(feats[:, ::8])[:, :, None, :] + pred(torch.arange(U + 1, device='cuda'))[None, None]
    Tj = logits.shape[1]
    targets = torch.randint(0, V - 1, (B, U), device='cuda').to(torch.int32)
    tl = torch.tensor([Tj, Tj - 2], dtype=torch.int32, device='cuda')
    ul = torch.tensor([U, U - 1], dtype=torch.int32, device='cuda')
    before = dict(tac._hip.launches)
    calls = dict(tac._ops.composite_calls)
    loss = tac.RNNTLoss()(logits, targets, tl, ul)
    grads = torch.autograd.grad(loss, list(enc.parameters()) + list(pred.parameters()))
    since = launched_since(tac, before)
    assert since.get(ROWS) == 1 and since.get(LATTICE) == 1 and since.get(GRAD) == 1, since
    assert tac._ops.composite_calls == calls
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)
    ref = R.Reference(logits.detach().cpu(), targets.cpu(), tl.cpu(), ul.cpu())
    assert abs(float(loss.detach()) - float(ref.costs.mean())) <= float(ref.cost_bound.max())
