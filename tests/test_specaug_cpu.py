"""``mask_along_axis`` / ``mask_along_axis_iid`` / ``TimeMasking`` / ``FrequencyMasking`` / ``SpecAugment`` without a device: every
``ValueError`` of the definitions, the input returned as it is where nothing can be masked, the torch-operator route (the CPU route)
against the definition applied mask by mask under the same seed (tests/specaug_rules.py), the one-call ``SpecAugment`` against the
sequential functional calls, the op against the slicing reference, gradients, fake kernels and tracing, the launcher expressions
the grid rule restates, and the C ABI surface."""
import ctypes
import os

import numpy as np
import pytest
import torch

import specaug_rules as R


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


def spec(shape, seed):
    return torch.from_numpy(R.values(shape, seed))


# ----------------------------------------------------------------------------- arguments
def test_value_errors(tac):
    x = spec((2, 3, 8, 20), 1)
    for fn in (tac.mask_along_axis, tac.mask_along_axis_iid):
        for axis in (0, 1, 4, -1):
            with pytest.raises(ValueError):
                fn(x, 5, 0.0, axis)
        for p in (-0.1, 1.5):
            with pytest.raises(ValueError):
                fn(x, 5, 0.0, 2, p=p)
    with pytest.raises(ValueError):
        tac.mask_along_axis_iid(x[0, 0], 5, 0.0, 1)                 # iid needs a leading index
    with pytest.raises(ValueError):
        tac.mask_along_axis(x[0, 0, 0], 5, 0.0, 0)                  # one dimension
    assert tac.mask_along_axis(x[0, 0], 5, 0.0, 1).shape == (8, 20)
    for p in (-0.1, 1.5):
        with pytest.raises(ValueError):
            tac.TimeMasking(5, p=p)
        with pytest.raises(ValueError):
            tac.SpecAugment(1, 5, 1, 3, p=p)
    with pytest.raises(ValueError):
        tac.mask_along_axis(x, 5, torch.zeros(2), 2)                # a fill of two elements


def test_a_shared_span_as_wide_as_mask_param_is_refused(tac, monkeypatch):
    """``end - start >= mask_param`` cannot come out of float32 draws below one: hand the rule the draw that rounds up"""
    draws = iter((torch.tensor([1.0]), torch.tensor([0.0])))
    monkeypatch.setattr(torch, 'rand', lambda *a, **k: next(draws))
    with pytest.raises(ValueError):
        tac.mask_along_axis(spec((3, 8, 20), 2), 5, 0.0, 2)


def test_nothing_to_mask_returns_the_input_itself(tac):
    x = spec((2, 8, 20), 3)
    assert tac.mask_along_axis(x, 0, 0.0, 1) is x and tac.mask_along_axis_iid(x, 0, 0.0, 2) is x
    assert tac.mask_along_axis(x, 7, 0.0, 2, p=0.04) is x           # int(20 * 0.04) = 0
    assert tac.mask_along_axis_iid(x, 7, 0.0, 1, p=0.1) is x        # int(8 * 0.1) = 0
    assert tac.TimeMasking(9, p=0.01)(x) is x and tac.FrequencyMasking(0)(x) is x
    assert tac.SpecAugment(2, 0, 2, 0)(x) is x and tac.SpecAugment(0, 5, 0, 5)(x) is x
    state = torch.get_rng_state()
    tac.mask_along_axis_iid(x, 0, 0.0, 2)
    assert torch.equal(state, torch.get_rng_state())                # and nothing was drawn
    empty = tac.mask_along_axis_iid(x[:, :, :0], 5, 0.0, 1)
    assert tuple(empty.shape) == (2, 8, 0)


# ----------------------------------------------------------------------------- the op against the slicing reference
@pytest.mark.parametrize('shape', R.SHAPES[:2] + ((5, 40, 3),))
def test_op_equals_the_reference_on_the_cpu_route(tac, shape):
    x = R.values(shape, seed=shape[1])
    for name, spans, k_a in R.span_sets(*shape, seed=shape[2]):
        for fill in (0.0, torch.tensor(-7.5)):
            value_t, value = (fill, 0.0) if torch.is_tensor(fill) else (None, fill)
            got = torch.ops.tac_amd.mask_spans(torch.from_numpy(x), torch.from_numpy(spans), k_a, value_t, value)
            assert got.is_contiguous() and got.data_ptr() != torch.from_numpy(x).data_ptr()
            R.assert_same(got, R.reference(x, spans, k_a, float(fill)), '%s %r' % (name, shape))
    # four dimensions, a transposed view, float64 and an integer dtype
    spans, k_a = np.array([[[1, 3], [2, 9]]], np.int32), 1
    want = R.reference(x, spans, k_a, 2.0)
    lead = torch.from_numpy(x).reshape((1, shape[0]) + shape[1:])
    R.assert_same(torch.ops.tac_amd.mask_spans(lead, torch.from_numpy(spans), k_a, None, 2.0)[0], want, 'lead')
    turned = torch.from_numpy(np.ascontiguousarray(np.swapaxes(x, -1, -2))).transpose(-1, -2)
    out = torch.ops.tac_amd.mask_spans(turned, torch.from_numpy(spans), k_a, None, 2.0)
    assert out.is_contiguous()
    R.assert_same(out, want, 'transposed')
    R.assert_same(torch.ops.tac_amd.mask_spans(torch.from_numpy(x).double(), torch.from_numpy(spans), k_a, None, 2.0),
                  want.astype(np.float64), 'float64')
    ints = (torch.from_numpy(x) * 100).to(torch.int16)
    R.assert_same(torch.ops.tac_amd.mask_spans(ints, torch.from_numpy(spans), k_a, None, 2.0),
                  R.reference(ints.numpy(), spans, k_a, 2), 'int16')
    with pytest.raises(ValueError):
        torch.ops.tac_amd.mask_spans(torch.from_numpy(x), torch.zeros((shape[0] + 1, 2, 2), dtype=torch.int32), 1, None, 0.0)
    with pytest.raises(ValueError):
        torch.ops.tac_amd.mask_spans(torch.from_numpy(x), torch.from_numpy(spans), 3, None, 0.0)


# ----------------------------------------------------------------------------- functional and layers against the definition
SHAPE = (2, 2, 20, 60)


@pytest.mark.parametrize('seed', (0, 1, 2))
def test_functional_equals_the_definition(tac, seed):
    x = spec(SHAPE, seed)
    for axis in (2, 3):
        for p in (1.0, 0.3):
            for fill in (0.0, -1.5, torch.tensor(0.25)):
                torch.manual_seed(seed)
                got = tac.mask_along_axis_iid(x, 9, fill, axis, p)
                R.assert_same(got, R.sequential(x, [('iid', 9, fill, axis, p)], seed), 'iid axis %d p %g' % (axis, p))
                torch.manual_seed(seed)
                got = tac.mask_along_axis(x, 9, fill, axis, p)
                R.assert_same(got, R.sequential(x, [('shared', 9, fill, axis, p)], seed), 'shared axis %d p %g' % (axis, p))
                assert got.is_contiguous() and got.dtype == x.dtype and bool((got != x).any())
    plane = x[0, 0]
    for axis in (0, 1):
        torch.manual_seed(seed)
        R.assert_same(tac.mask_along_axis(plane, 9, 0.0, axis), R.sequential(plane, [('shared', 9, 0.0, axis, 1.0)], seed), '2-D')


@pytest.mark.parametrize('seed', (0, 3))
def test_layers_equal_the_definition(tac, seed):
    x = spec(SHAPE, seed + 10)
    for iid in (False, True):
        kind = 'iid' if iid else 'shared'
        torch.manual_seed(seed)
        R.assert_same(tac.TimeMasking(15, iid, p=0.2)(x), R.sequential(x, [(kind, 15, 0.0, 3, 0.2)], seed), 'TimeMasking')
        torch.manual_seed(seed)
        R.assert_same(tac.FrequencyMasking(7, iid)(x, 3.0), R.sequential(x, [(kind, 7, 3.0, 2, 1.0)], seed), 'FrequencyMasking')
        torch.manual_seed(seed)                  # iid applies from three dimensions on
        R.assert_same(tac.TimeMasking(15, iid)(x[0, 0]), R.sequential(x[0, 0], [('shared', 15, 0.0, 1, 1.0)], seed), 'TimeMasking 2-D')
        for zero in (False, True):
            for p in (1.0, 0.2):
                fill = 0.0 if zero else x.mean()
                layer = tac.SpecAugment(2, 30, 2, 7, iid_masks=iid, p=p, zero_masking=zero)
                torch.manual_seed(seed)
                got = layer(x)
                calls = R.spec_augment_calls(4, 2, 30, 2, 7, iid, p, fill)
                R.assert_same(got, R.sequential(x, calls, seed), 'SpecAugment iid %r zero %r p %g' % (iid, zero, p))
                # and the one call equals the package's own functionals called one after the other
                torch.manual_seed(seed)
                step = x
                for _ in range(2):
                    step = (tac.mask_along_axis_iid if iid else tac.mask_along_axis)(step, 30, fill, 3, p)
                for _ in range(2):
                    step = (tac.mask_along_axis_iid if iid else tac.mask_along_axis)(step, 7, fill, 2)
                R.assert_same(got, step, 'SpecAugment against the functionals')
    assert 'SpecAugment(n_time_masks=2' in repr(tac.SpecAugment(2, 30, 2, 7)) and not list(tac.SpecAugment(2, 30, 2, 7).state_dict())
    assert 'TimeMasking(mask_param=15' in repr(tac.TimeMasking(15))


# ----------------------------------------------------------------------------- gradients, fake kernels, tracing
def test_gradients_cpu(tac):
    x = torch.randn(2, 5, 7, dtype=torch.float64, requires_grad=True)
    fill = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
    spans = torch.tensor([[[1, 3], [0, 2], [4, 9]], [[0, 0], [3, 4], [-2, 1]]], dtype=torch.int32)
    assert torch.autograd.gradcheck(lambda a: torch.ops.tac_amd.mask_spans(a, spans, 1, None, 0.5), (x,))
    assert torch.autograd.gradcheck(lambda a, v: torch.ops.tac_amd.mask_spans(a, spans, 1, v, 0.0), (x, fill))
    assert torch.autograd.gradgradcheck(lambda a, v: torch.ops.tac_amd.mask_spans(a, spans[:1], 2, v, 0.0), (x, fill))
    g = torch.randn(2, 5, 7, dtype=torch.float64)
    gx, gv = torch.autograd.grad(torch.ops.tac_amd.mask_spans(x, spans, 1, fill, 0.0), (x, fill), g)
    hit = R.masked((2, 5, 7), spans.numpy(), 1)
    assert np.array_equal(gx.numpy(), np.where(hit, 0.0, g.numpy())) and abs(float(gv) - g.numpy()[hit].sum()) < 1e-12
    # through the layer: the mean's gradient flows on into the input
    y = torch.randn(2, 6, 9, dtype=torch.float64, requires_grad=True)
    torch.manual_seed(4)
    out = tac.SpecAugment(1, 4, 1, 3)(y)
    (gy,) = torch.autograd.grad(out.sum(), y)
    n_masked = int((out == y.mean()).sum())
    assert n_masked > 0 and torch.allclose(gy, (out != y.mean()).double() + n_masked / y.numel())


def test_fake_kernels_and_tracing(tac):
    seen = []

    def capture(gm, example_inputs):
        seen.extend(str(n.target) for n in gm.graph.nodes if n.op == 'call_function')
        return gm.forward

    x = spec((3, 8, 20), 5)
    spans = torch.tensor([[[1, 3], [2, 9]]], dtype=torch.int32)
    torch._dynamo.reset()
    fn = torch.compile(lambda a, s: torch.ops.tac_amd.mask_spans(a, s, 1, None, 0.0), backend=capture, fullgraph=True)
    out = fn(x, spans)
    assert sum('tac_amd.mask_spans' in n for n in seen) == 1 and len(seen) == 1, seen
    R.assert_same(out, R.reference(x.numpy(), spans.numpy(), 1, 0.0), 'compiled')
    del seen[:]
    torch._dynamo.reset()
    layer = tac.SpecAugment(2, 6, 1, 3, zero_masking=True)
    compiled = torch.compile(layer, backend=capture, fullgraph=True)
    torch.manual_seed(6)
    out = compiled(x)
    assert sum('tac_amd.mask_spans' in n for n in seen) == 1, seen
    assert out.shape == x.shape and bool((out == 0).any())
    from torch._subclasses.fake_tensor import FakeTensorMode
    sliced = x[:, ::2, 1:]
    with FakeTensorMode() as mode:
        fake = torch.ops.tac_amd.mask_spans(mode.from_tensor(sliced), mode.from_tensor(spans), 1, None, 0.0)
    real = torch.ops.tac_amd.mask_spans(sliced, spans, 1, None, 0.0)
    assert tuple(fake.shape) == tuple(real.shape) and fake.stride() == real.stride() and fake.dtype == real.dtype
    torch.library.opcheck(torch.ops.tac_amd.mask_spans.default, (x, spans, 1, None, 0.0),
                          test_utils=('test_schema', 'test_faketensor'))


# ----------------------------------------------------------------------------- the grid rule and the C ABI
@pytest.mark.parametrize('cus', R.CU_COUNTS)
def test_wrap_rows_wrap_the_grid(cus):
    rows = R.assert_wraps(cus)
    assert rows == 2 * 32 * cus + 5
    assert R.launch(cus, 256, 80, 1000) == (256 * 5 * 4, 32 * cus)                  # 16 lines x 256 columns a unit
    assert R.launch(cus, 256, 1000, 80) == (256 * 32 * 1, 32 * cus)                 # 80 columns: 32 lanes, 32 lines a unit
    assert R.launch(cus, 256, 80, 1000, turn=True) == (256 * 2 * 16, 32 * cus)
    with pytest.raises(AssertionError):                                             # the rule has teeth
        assert R.launch(cus, 3, 3, 5)[0] > 2 * R.launch(cus, 3, 3, 5)[1]
    assert [R.lpl_log(b) for b in (1, 3, 80, 1000, 1001, 3000, 64, 65)] == [4, 4, 5, 6, 6, 6, 4, 5]


def test_quoted_launcher_expressions_are_in_the_source(tac):
    name, quotes = R.QUOTED
    with open(os.path.join(os.path.dirname(os.path.abspath(tac.__file__)), 'csrc', name)) as f:
        text = f.read()
    for q in quotes:
        assert q in text, '%s no longer holds %r: tests/specaug_rules.py restates a launcher that has changed' % (name, q)


def test_c_abi_surface(tac):
    h = tac._native.lib()
    assert h.tac_abi_version() == 5
    assert 'tac_mask_spans_f32' in tac._native.EXPORTS and 'tac_mask_spans_supported' in tac._native.EXPORTS
    assert h.tac_mask_spans_supported(0, 0) == 0 and h.tac_mask_spans_supported(64, 0) == 0 and h.tac_mask_spans_supported(31, 33) == 0
    assert h.tac_mask_spans_supported(64, 1) == tac._native.TAC_E_UNSUPPORTED
    assert h.tac_mask_spans_supported(-1, 1) == tac._native.TAC_E_INVALID
    assert tac._hip.mask_spans_supported(10, 2) and not tac._hip.mask_spans_supported(33, 32)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tac_amd.h')) as f:
        header = f.read()
    assert '#define TAC_MASK_MAX_SPANS %d' % R.MAX_SPANS in header and 'int tac_mask_spans_f32(' in header
    # argument errors are refused before anything is launched (no device is touched)
    one = ctypes.c_void_p(16)
    assert h.tac_mask_spans_f32(None, 1, 1, 1, 1, 1, 1, None, 1, 0, 0, None, 0.0, one, None) == tac._native.TAC_E_INVALID
    assert h.tac_mask_spans_f32(one, 2, 2, 2, -4, 2, 1, None, 1, 0, 0, None, 0.0, one, None) == tac._native.TAC_E_INVALID
    assert h.tac_mask_spans_f32(one, 2, 2, 2, 4, 2, 1, None, 1, 1, 0, None, 0.0, one, None) == tac._native.TAC_E_INVALID      # no table
    assert h.tac_mask_spans_f32(one, 2, 2, 2, 4, 2, 1, one, 3, 1, 0, None, 0.0, one, None) == tac._native.TAC_E_INVALID      # 3 tables, 2 rows
    assert h.tac_mask_spans_f32(one, 2, 2, 2, 4, 2, 1, one, 1, 40, 25, None, 0.0, one, None) == tac._native.TAC_E_UNSUPPORTED
