"""-m gpu: SpecAugment's masks on the gfx950 kernel (csrc/specaug.hip) — strict mode and poisoned outputs on, as in
tests/test_kaldi_gpu.py.

The reference is the slicing loop of tests/specaug_rules.py and, for the functionals and layers, the definition applied mask by mask
under the same seed on the same device.  The kernel computes nothing, so every comparison is bit for bit, NaN positions outside the
masks included.  Shapes: one element, odd sizes under one unit, rows that are no multiple of the 16-byte chunk, several A-blocks
and B-chunks, every width of the line segments (16 / 32 / 64 lanes), both load widths and the turned load on tiles that are and are
not full; span counts 0 .. 64 on either axis, shared and per-row tables, immediate and device fills."""
import warnings

import numpy as np
import pytest
import torch

import specaug_rules as R

pytestmark = pytest.mark.gpu

ENTRY = 'tac_mask_spans_f32'


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


def run(tac_, xt, spans, k_a, fill, want, what):
    """one call of the op on ``xt``: exactly one launch, a fresh dense tensor, ``want`` bit for bit"""
    value_t, value = (fill, 0.0) if torch.is_tensor(fill) else (None, fill)
    before = dict(tac_._hip.launches)
    got = torch.ops.tac_amd.mask_spans(xt, dev(spans), k_a, value_t, value)
    assert launched_since(tac_, before) == {ENTRY: 1}, what
    assert got.dtype == xt.dtype and got.shape == xt.shape and got.is_contiguous(), what
    R.assert_same(got, want, what)
    return got


# ----------------------------------------------------------------------------- 1. the op against the slicing reference
@pytest.mark.parametrize('shape', R.SHAPES)
def test_op_equals_the_reference(tac, shape):
    x = R.values(shape, seed=shape[2])
    xt = dev(x)
    fill_t = torch.tensor(-3.25, device='cuda')
    for i, (name, spans, k_a) in enumerate(R.span_sets(*shape, seed=shape[1])):
        fill = (0.0, fill_t, 7.5)[i % 3]
        want = R.reference(x, spans, k_a, float(fill))
        run(tac, xt, spans, k_a, fill, want, '%s %r' % (name, shape))
    assert torch.equal(torch.ops.tac_amd.mask_spans(xt, dev(spans), k_a, None, 1.0), torch.ops.tac_amd.mask_spans(xt, dev(spans), k_a, None, 1.0))


# ----------------------------------------------------------------------------- 2. layouts
def offset_by_one(x):
    """a view that starts one element into its allocation: no 16-byte alignment"""
    flat = torch.full((x.size + 1,), float('nan'), device='cuda')
    flat[1:] = dev(x).reshape(-1)
    return flat[1:].view(x.shape)


def b_slice(x):
    wide = torch.full(x.shape[:-1] + (x.shape[-1] + 3,), float('nan'), device='cuda')
    wide[..., 2:-1] = dev(x)
    return wide[..., 2:-1]


def a_slice(x):
    wide = torch.full(x.shape[:-2] + (x.shape[-2] + 2, x.shape[-1]), float('nan'), device='cuda')
    wide[..., 1:-1, :] = dev(x)
    return wide[..., 1:-1, :]


def a_slice_aligned(x):
    """lines 4 .. of a taller tensor: a row stride beyond A B that keeps the 16-byte chunks"""
    wide = torch.full(x.shape[:-2] + (x.shape[-2] + 4, x.shape[-1]), float('nan'), device='cuda')
    wide[..., 4:, :] = dev(x)
    return wide[..., 4:, :]


def every_second_row(x):
    wide = torch.full((2 * x.shape[0],) + x.shape[1:], float('nan'), device='cuda')
    wide[::2] = dev(x)
    return wide[::2]


def transposed(x):
    """the transposed view of a contiguous (rows, B, A) tensor"""
    return dev(np.swapaxes(x, -1, -2)).transpose(-1, -2)


LAYOUTS = (('offset by one element', offset_by_one), ('slice along B', b_slice), ('slice along A', a_slice),
           ('aligned slice along A', a_slice_aligned), ('every second row', every_second_row), ('transposed', transposed))


@pytest.mark.parametrize('name,layout', LAYOUTS)
@pytest.mark.parametrize('shape', ((3, 23, 68), (2, 70, 131), (3, 5, 7), (2, 64, 64), (2, 80, 1000)))
def test_layouts(tac, shape, name, layout):
    x = R.values(shape, seed=shape[1])
    xt = layout(x)
    assert tuple(xt.shape) == shape and (xt.cpu().numpy() == x).all()
    for what, spans, k_a in R.span_sets(*shape, seed=7)[4:10]:
        run(tac, xt, spans, k_a, -1.0, R.reference(x, spans, k_a, -1.0), '%s, %s %r' % (name, what, shape))


@pytest.mark.parametrize('dtype', (torch.float16, torch.bfloat16))
def test_half_inputs_are_widened(tac, dtype):
    shape = (3, 23, 68)
    xt = dev(R.values(shape, seed=16)).to(dtype)
    x = xt.float().cpu().numpy()
    for what, spans, k_a in R.span_sets(*shape, seed=16)[4:8]:
        for fill in (-2.5, torch.tensor(0.75, device='cuda', dtype=dtype)):          # representable in both formats
            value_t, value = (fill, 0.0) if torch.is_tensor(fill) else (None, fill)
            before = dict(tac._hip.launches)
            got = torch.ops.tac_amd.mask_spans(xt, dev(spans), k_a, value_t, value)
            assert launched_since(tac, before) == {ENTRY: 1} and got.dtype == dtype
            R.assert_same(got.float(), R.reference(x, spans, k_a, float(fill)), '%s %s' % (dtype, what))


# ----------------------------------------------------------------------------- 3. what lies under a mask does not matter
@pytest.mark.parametrize('name,layout', (('contiguous', dev),) + LAYOUTS[:1] + LAYOUTS[-1:])
def test_nan_under_the_masks_does_not_reach_the_output(tac, name, layout):
    shape = (3, 70, 132)
    for what, spans, k_a in R.span_sets(*shape, seed=3)[4:12]:
        hit = R.masked(shape, spans, k_a)
        x = R.values(shape, seed=9)
        x[hit] = np.nan
        x[0, 0, 0] = x[0, 0, 0] if hit[0, 0, 0] else np.float32(np.nan)              # and one NaN outside: it is copied, bit for bit
        for fill in (0.0, torch.tensor(4.0, device='cuda')):
            got = run(tac, layout(x), spans, k_a, fill, R.reference(x, spans, k_a, float(fill)), '%s, %s' % (name, what))
            assert bool(torch.isfinite(got[torch.from_numpy(hit).to('cuda')]).all())


# ----------------------------------------------------------------------------- 4. functional and layers against the definition
SHAPE = (2, 2, 80, 300)


@pytest.mark.parametrize('seed', (0, 1))
def test_functional_equals_the_definition(tac, seed):
    x = dev(R.values(SHAPE, seed))
    for axis in (2, 3):
        for kind, fn in (('iid', tac.mask_along_axis_iid), ('shared', tac.mask_along_axis)):
            for p, fill in ((1.0, 0.0), (0.2, -1.5), (1.0, torch.tensor(0.25, device='cuda'))):
                torch.manual_seed(seed)
                before = dict(tac._hip.launches)
                got = fn(x, 27, fill, axis, p)
                assert launched_since(tac, before) == {ENTRY: 1}
                R.assert_same(got, R.sequential(x, [(kind, 27, fill, axis, p)], seed), '%s axis %d p %g' % (kind, axis, p))
    before = dict(tac._hip.launches)
    assert tac.mask_along_axis_iid(x, 0, 0.0, 2) is x and tac.mask_along_axis(x, 27, 0.0, 3, p=0.001) is x
    assert tuple(tac.mask_along_axis_iid(x[..., :0], 5, 0.0, 2).shape) == (2, 2, 80, 0)
    assert launched_since(tac, before) == {}
    torch.manual_seed(seed)                      # a (freq, time) matrix and the (time, freq) view of a Kaldi matrix
    plane = x[0, 0]
    R.assert_same(tac.mask_along_axis(plane, 27, 0.0, 1), R.sequential(plane, [('shared', 27, 0.0, 1, 1.0)], seed), '2-D')
    kaldi = x[0].transpose(-1, -2)
    torch.manual_seed(seed)
    before = dict(tac._hip.launches)
    got = tac.mask_along_axis_iid(kaldi, 27, 0.0, 1)
    assert launched_since(tac, before) == {ENTRY: 1}
    R.assert_same(got, R.sequential(kaldi, [('iid', 27, 0.0, 1, 1.0)], seed), 'the transposed view')


@pytest.mark.parametrize('iid', (False, True))
@pytest.mark.parametrize('seed', (0, 5))
def test_layers_equal_the_definition(tac, seed, iid):
    x = dev(R.values(SHAPE, seed + 20))
    kind = 'iid' if iid else 'shared'
    for layer, calls in ((tac.TimeMasking(100, iid, p=0.2), [(kind, 100, 0.0, 3, 0.2)]),
                         (tac.FrequencyMasking(27, iid), [(kind, 27, 0.0, 2, 1.0)])):
        torch.manual_seed(seed)
        before = dict(tac._hip.launches)
        got = layer(x)
        assert launched_since(tac, before) == {ENTRY: 1}
        R.assert_same(got, R.sequential(x, calls, seed), repr(layer))
    for zero in (False, True):
        for p in (1.0, 0.2):
            layer = tac.SpecAugment(2, 100, 2, 27, iid_masks=iid, p=p, zero_masking=zero)
            torch.manual_seed(seed)
            before = dict(tac._hip.launches)
            got = layer(x)
            assert launched_since(tac, before) == {ENTRY: 1}, repr(layer)
            fill = 0.0 if zero else x.mean()
            want = R.sequential(x, R.spec_augment_calls(4, 2, 100, 2, 27, iid, p, fill), seed)
            R.assert_same(got, want, repr(layer))
            assert bool((got != x).any())


# ----------------------------------------------------------------------------- 5. gradients
def test_gradients_are_the_same_kernel(tac):
    shape = (3, 70, 132)
    rng = np.random.default_rng(70)
    g = rng.standard_normal(shape).astype(np.float32)
    for what, spans, k_a in R.span_sets(*shape, seed=5)[5:12]:
        hit = R.masked(shape, spans, k_a)
        for name, layout in (('contiguous', dev),) + LAYOUTS[-1:]:
            x = layout(R.values(shape, seed=1)).requires_grad_(True)
            fill = torch.tensor(0.5, device='cuda', requires_grad=True)
            before = dict(tac._hip.launches)
            out = torch.ops.tac_amd.mask_spans(x, dev(spans), k_a, fill, 0.0)
            gx, gv = torch.autograd.grad(out, (x, fill), layout(g))                 # grad_out in the same layout
            assert launched_since(tac, before) == {ENTRY: 2}, what
            R.assert_same(gx, np.where(hit, np.float32(0.0), g), 'grad_x, %s, %s' % (what, name))
            n_masked = int(hit.sum())
            want = float(g.astype(np.float64)[hit].sum())
            bound = n_masked * 2.0 ** -24 * float(np.abs(g).max())
            print('%s, %s: %d masked, fill gradient %.9g, float64 sum %.9g, bound %.3g' % (what, name, n_masked, float(gv), want, bound))
            assert abs(float(gv) - want) <= bound, (what, name, float(gv), want, bound)


def test_fbank_then_specaugment_trains_on_the_kernels(tac):
    wave = dev(np.random.default_rng(16).standard_normal((4, 16000)).astype(np.float32)).requires_grad_(True)
    fbank, augment = tac.KaldiFbank(num_mel_bins=80), tac.SpecAugment(2, 30, 2, 27, zero_masking=True)
    torch.manual_seed(1)
    before = dict(tac._hip.launches)
    feats = fbank(wave)                                     # (4, 98, 80): time second to last, as Kaldi lays it out
    out = augment(feats.transpose(-1, -2))                  # (…, freq, time): the turned load
    assert launched_since(tac, before) == {'tac_kaldi_fbank_f32': 1, ENTRY: 1}
    assert tuple(out.shape) == (4, 80, 98) and out.is_contiguous()
    R.assert_same(out, R.sequential(feats.detach().transpose(-1, -2), R.spec_augment_calls(3, 2, 30, 2, 27, True, 1.0, 0.0), 1), 'chain')
    # the mean as the fill: torch's mean beside the one launch, and its gradient flows on into the features
    feats = feats.detach().requires_grad_(True)
    torch.manual_seed(2)
    before = dict(tac._hip.launches)
    out = tac.SpecAugment(2, 30, 2, 27)(feats.transpose(-1, -2))
    (gf,) = torch.autograd.grad(out.sum(), feats)
    assert launched_since(tac, before) == {ENTRY: 2}
    n_masked = int((out == feats.mean()).sum())
    want = (out != feats.mean()).transpose(-1, -2).double() + n_masked / feats.numel()
    assert n_masked > 0 and float((gf.double() - want).abs().max()) <= n_masked * 2.0 ** -24


# ----------------------------------------------------------------------------- 6. announced routes
def test_other_routes_are_announced(tac):
    shape = (3, 23, 68)
    x = R.values(shape, seed=6)
    xt = dev(x)
    few = np.array([[[1, 3], [2, 40]]], np.int32)
    many = np.concatenate([few] * 33, axis=1)[:, :65]
    # (torch has no negative strides — ``flip`` copies, and the copy takes the kernel like any dense tensor: the non-positive stride
    # a tensor can have is the zero of an expanded view)
    flipped = xt.flip(-1)
    assert all(st > 0 for st in flipped.stride())
    run(tac, flipped, few, 1, 0.0, R.reference(x[..., ::-1], few, 1, 0.0), 'flipped')
    cases = (('dtype float64', xt.double(), few, 1), ('non-positive strides', xt[..., :1].expand(shape), few, 1), ('65 spans', xt, many, 30))
    for reason, t, spans, k_a in cases:
        with pytest.raises(RuntimeError, match='strict'):
            torch.ops.tac_amd.mask_spans(t, dev(spans), k_a, None, 0.0)
    tac.set_strict(False)
    try:
        for reason, t, spans, k_a in cases:
            (key,) = [k for k in tac._ops.composite_calls if k[0] == 'mask_spans' and reason in k[1]]
            counted = tac._ops.composite_calls[key]
            tac._ops._warned.discard(key)
            before = dict(tac._hip.launches)
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter('always')
                got = torch.ops.tac_amd.mask_spans(t, dev(spans), k_a, None, 0.0)
            assert launched_since(tac, before) == {}, reason
            assert any(issubclass(w.category, tac.CompositeRouteWarning) for w in seen), reason
            assert tac._ops.composite_calls[key] == counted + 1
            assert got.is_contiguous() and got.dtype == t.dtype
            R.assert_same(got, R.reference(t.cpu().numpy(), spans, k_a, 0.0), reason)
    finally:
        tac.set_strict(True)
    before = dict(tac._hip.launches)                        # an integer dtype through the functional: announced, too
    with pytest.raises(RuntimeError, match='strict'):
        tac.mask_along_axis_iid((xt * 100).to(torch.int32), 9, 0, 2)
    assert launched_since(tac, before) == {}


# ----------------------------------------------------------------------------- 7. past the grid
@pytest.mark.parametrize('name,n_a,n_b,turn', R.WRAP_FORMS)
def test_grid_wrap(tac, name, n_a, n_b, turn):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus in R.CU_COUNTS:
        R.assert_wraps(cus)
    rows = R.wrap_rows(cus)
    units, grid = R.launch(cus, rows, n_a, n_b, turn)
    assert units == rows > 2 * grid and (units - 2 * grid) % 2 == 1
    base = R.values((R.BASE_ROWS, n_a, n_b), seed=n_a)
    base_spans = np.array([[[0, 1], [1, 3]], [[2, 9], [0, 0]], [[1, 2], [0, 2]], [[0, 0], [-1, 1]], [[-1, 1], [3, 4]]], np.int32)
    small = run(tac, transposed(base) if turn else dev(base), base_spans, 1, -1.0, R.reference(base, base_spans, 1, -1.0), name)
    pick = torch.arange(rows) % R.BASE_ROWS
    big_x = torch.from_numpy(base)[pick].contiguous()
    big_spans = torch.from_numpy(base_spans)[pick].contiguous()
    xt = transposed(big_x.numpy()) if turn else dev(big_x)
    before = dict(tac._hip.launches)
    big = torch.ops.tac_amd.mask_spans(xt, dev(big_spans), 1, None, -1.0)
    assert launched_since(tac, before) == {ENTRY: 1}
    assert torch.equal(big.view(torch.int32), small[pick.to('cuda')].view(torch.int32)), name
