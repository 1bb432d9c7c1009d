"""``add_noise`` / ``AddNoise`` / ``speed`` / ``Speed`` / ``SpeedPerturbation`` without a device: the torch-operator route (the CPU route)
against the definition restated in tests/augment_rules.py, bit for bit; every ``ValueError``; broadcasting, the length mask and the
special-value rows; gradients (``gradcheck`` of the op and the rules' gradient formulas against autograd of the float64 definition);
``speed`` against ``resample`` at the reduced pair, its lengths and its draw; fake kernels and tracing; the launcher expressions the
grid rule restates, and the C ABI surface."""
import ctypes
import os

import pytest
import torch

import augment_rules as R


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    view = {4: torch.int32, 8: torch.int64}[got.element_size()]
    assert torch.equal(got.contiguous().view(view), want.contiguous().view(view)), what


# ----------------------------------------------------------------------------- add_noise: the CPU route
@pytest.mark.parametrize('dtype', (torch.float32, torch.float64))
def test_cpu_route_equals_the_definition(tac, dtype):
    for length in (1, 5, 130):
        w, n = R.normal((2, 3, length), length).to(dtype), R.normal((2, 3, length), length + 1).to(dtype)
        for snr in (torch.tensor([[10.0], [-5.0]], dtype=dtype), torch.zeros((2, 3), dtype=dtype) + 40.0):
            for lengths in (None, torch.tensor([[length], [1]]), torch.tensor([[length + 5, 1, length], [length, length, 2]], dtype=torch.int32)):
                got = tac.add_noise(w, n, snr, lengths)
                assert got.is_contiguous()
                same_bits(got, R.definition(w, n, snr, lengths), 'L %d' % length)
                same_bits(tac.AddNoise()(w, n, snr, lengths), got, 'layer')
    assert tuple(tac.add_noise(w[..., :0], n[..., :0], snr).shape) == (2, 3, 0)


def test_value_errors(tac):
    w, n, snr = R.normal((2, 3, 9), 0), R.normal((2, 3, 9), 1), torch.zeros(2, 3)
    for bad in ((w, n[0], snr, None), (w, n, snr[0], None), (w, n, snr, torch.tensor([9, 9])), (w, n[..., :8], snr, None),
                (w, n, torch.zeros(2, 3, 1), None), (w, torch.zeros(2, 2, 9), snr, None)):
        with pytest.raises(ValueError):
            tac.add_noise(*bad)
        with pytest.raises(ValueError):
            tac.AddNoise()(*bad)
    with pytest.raises(ValueError):                                      # the op checks for itself too
        torch.ops.tac_amd.add_noise(w, n[0], snr, None)
    with pytest.raises(TypeError):
        tac.add_noise(w, n, 10.0)


def test_broadcasting(tac):
    w, n, snr = R.normal((4, 3, 50), 2), R.normal((4, 1, 50), 3), torch.tensor([[0.0], [10.0], [-5.0], [40.0]])
    lengths = torch.tensor([[50], [20], [1], [49]])
    got = tac.add_noise(w, n, snr, lengths)
    assert tuple(got.shape) == (4, 3, 50)
    same_bits(got, R.definition(w, n, snr, lengths), 'noise (B, 1, L), snr (B, 1)')
    for b in range(4):
        for c in range(3):                                              # and row by row: one noise row serves every channel
            same_bits(got[b, c], R.definition(w[b, c], n[b, 0], snr[b, 0], lengths[b, 0]), 'row %d %d' % (b, c))
    wide = tac.add_noise(w[:, :1], n.expand(4, 3, 50), snr.expand(4, 3), None)
    assert tuple(wide.shape) == (4, 3, 50)
    same_bits(wide, R.definition(w[:, :1], n.expand(4, 3, 50), snr.expand(4, 3)), 'a waveform row for every noise row')


def test_lengths(tac):
    length = 12
    w, n, snr = R.normal((5, length), 4), R.normal((5, length), 5), torch.full((5,), 10.0)
    lengths = torch.tensor([0, 1, length, length + 5, -1])
    got = tac.add_noise(w, n, snr, lengths)
    same_bits(got[1:4], R.definition(w[1:4], n[1:4], snr[1:4], lengths[1:4]), 'lengths 1, L, L + 5')
    same_bits(got[2:4], R.definition(w[2:4], n[2:4], snr[2:4]), 'L and beyond: the whole row')
    assert bool(torch.isnan(got[0]).all()) and bool(torch.isnan(got[4]).all())          # nothing inside the mask: 0 / 0
    one = R.definition(w[1, :1], n[1, :1], snr[1])                                      # one sample sets the scale of the row
    scale = (w[1, 0].abs() / n[1, 0].abs()).double() * 10 ** -0.5
    assert abs(float(one[0] - w[1, 0]) / float(n[1, 0]) - float(scale)) < 1e-5 * float(scale)
    assert torch.allclose(got[1], w[1] + (float(scale) * n[1].double()).float(), rtol=1e-5, atol=1e-6)
    # what lies behind a length does not reach the scale, yet is mixed at its own position
    w2, n2 = w.clone(), n.clone()
    w2[1, 5], n2[1, 7] = float('nan'), float('inf')
    poisoned = tac.add_noise(w2, n2, snr, lengths)
    keep = torch.ones(length, dtype=torch.bool)
    keep[5] = keep[7] = False
    same_bits(poisoned[1, keep], got[1, keep], 'behind the length')
    assert bool(torch.isnan(poisoned[1, 5])) and bool(torch.isinf(poisoned[1, 7]))


def test_special_rows(tac):
    length = 9
    w, n, snr = R.normal((3, length), 6), R.normal((3, length), 7), torch.zeros(3)
    w[0] = 0.0                      # E_s = 0: scale 0
    n[1] = 0.0                      # E_n = 0: scale inf
    w[2], n[2] = 0.0, 0.0           # both: NaN
    got = tac.add_noise(w, n, snr)
    same_bits(got, R.definition(w, n, snr), 'special rows')
    assert bool((got[0] == 0).all())                                      # scale 0 on a silent waveform
    assert bool(torch.isnan(got[1]).all())                                # inf * 0
    assert bool(torch.isnan(got[2]).all())
    n[1, 3] = 1e-30                                                       # E_n underflows in float32, the sample itself does not vanish
    t = R.terms(w, n, snr)
    assert float(t['e_n'][1]) > 0 and bool(torch.isinf(tac.add_noise(w, n, snr)[1, 3]))


# ----------------------------------------------------------------------------- gradients
def test_gradcheck_of_the_op(tac):
    torch.manual_seed(0)
    w = torch.randn(2, 3, 7, dtype=torch.float64, requires_grad=True)
    n = torch.randn(2, 1, 7, dtype=torch.float64, requires_grad=True)
    snr = torch.tensor([[3.0], [-2.0]], dtype=torch.float64, requires_grad=True)
    for lengths in (None, torch.tensor([[7], [4]]), torch.tensor([[9, 2, 7], [1, 7, 3]], dtype=torch.int32)):
        assert torch.autograd.gradcheck(lambda a, b, c: torch.ops.tac_amd.add_noise(a, b, c, lengths), (w, n, snr))
    assert torch.autograd.gradgradcheck(lambda a, b, c: torch.ops.tac_amd.add_noise(a, b, c, None), (w, n, snr))


def test_gradient_formulas_equal_autograd(tac):
    torch.manual_seed(1)
    for shape_n, shape_s, lengths in (((2, 3, 11), (2, 3), None), ((2, 1, 11), (2, 1), torch.tensor([[11], [4]])),
                                      ((1, 3, 11), (1, 1), torch.tensor([[14, 1, 6], [11, 3, 10]]))):
        w = torch.randn(2, 3, 11, dtype=torch.float64, requires_grad=True)
        n = torch.randn(shape_n, dtype=torch.float64, requires_grad=True)
        snr = (torch.randn(shape_s, dtype=torch.float64) * 5).requires_grad_(True)
        g = torch.randn(2, 3, 11, dtype=torch.float64)
        want = torch.autograd.grad(R.definition(w, n, snr, lengths), (w, n, snr), g)
        r = R.gradients(g, w, n, snr, lengths)
        for key, ref, t in zip(('g_wave', 'g_noise', 'g_snr'), want, (w, n, snr)):
            got = R.sum_to(r[key], t.shape)
            assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), key
        got = torch.autograd.grad(tac.add_noise(w, n, snr, lengths), (w, n, snr), g)           # and the op's own backward
        for a, b in zip(got, want):
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


# ----------------------------------------------------------------------------- speed
FACTORS = ((0.9, 9, 10), (1.1, 11, 10), (0.95, 19, 20), (1.05, 21, 20), (1.0, 1, 1))


@pytest.mark.parametrize('factor,source,target', FACTORS)
def test_speed_is_resample_at_the_reduced_pair(tac, factor, source, target):
    x = R.normal((2, 3, 1601), 8)
    assert tac._augment.speed_rates(16000, factor) == (source, target)
    out, out_lengths = tac.speed(x, 16000, factor)
    assert out_lengths is None
    same_bits(out, tac.resample(x, source, target), 'functional')
    layer = tac.Speed(16000, factor)
    same_bits(layer(x)[0], out, 'layer')
    assert (layer.source_sample_rate, layer.target_sample_rate) == (source, target)
    assert isinstance(layer.resampler, tac.Resample) and layer.state_dict() == {}
    for lengths in (torch.tensor([1601, 800, 1], dtype=torch.int32), torch.tensor([[1601], [7]], dtype=torch.int64),
                    torch.tensor([1601.0, 0.0, 12.5])):
        want = torch.ceil(lengths * target / source).to(lengths.dtype)
        for got in (tac.speed(x, 16000, factor, lengths)[1], layer(x, lengths)[1]):
            assert got.dtype == lengths.dtype and torch.equal(got, want)
    assert int(tac.speed(x, 16000, factor, torch.tensor([1601]))[1]) == out.shape[-1]


def test_speed_one_returns_the_input(tac):
    x = R.normal((2, 160), 9)
    assert tac.Speed(16000, 1.0)(x)[0] is x and tac.speed(x, 16000, 1.0)[0] is x
    assert tac.speed(x, 8000, 1.0, torch.tensor([160, 3]))[1].tolist() == [160, 3]


def test_speed_value_errors(tac):
    x = R.normal((2, 160), 10)
    for factor in (0.0, -1.0, 1e-9):
        with pytest.raises(ValueError):
            tac.speed(x, 16000, factor)
        with pytest.raises(ValueError):
            tac.Speed(16000, factor)
        with pytest.raises(ValueError):
            tac.SpeedPerturbation(16000, [1.0, factor])
    with pytest.raises(ValueError):
        tac.SpeedPerturbation(16000, [])


def test_speed_perturbation_draws_as_the_definition(tac):
    x = R.normal((2, 1600), 11)
    factors = [0.9, 1.0, 1.1]
    layer = tac.SpeedPerturbation(16000, factors)
    lengths = torch.tensor([1600, 801], dtype=torch.int32)
    picked = set()
    for seed in range(8):
        torch.manual_seed(seed)
        index = int(torch.randint(3, ()))
        after = torch.get_rng_state()
        picked.add(index)
        torch.manual_seed(seed)
        out, out_lengths = layer(x, lengths)
        assert torch.equal(torch.get_rng_state(), after)                # exactly one draw, also where the factor drawn is 1.0
        want, want_lengths = tac.speed(x, 16000, factors[index], lengths)
        same_bits(out, want, 'seed %d' % seed)
        assert torch.equal(out_lengths, want_lengths) and (out is x) == (index == 1)
    assert picked == {0, 1, 2}


# ----------------------------------------------------------------------------- fake kernels and tracing
def test_fake_kernels_and_tracing(tac):
    seen = []

    def capture(gm, example_inputs):
        seen.extend(str(n.target) for n in gm.graph.nodes if n.op == 'call_function')
        return gm.forward

    w, n, snr, lengths = R.normal((2, 3, 40), 12), R.normal((2, 1, 40), 13), torch.tensor([[10.0], [0.0]]), torch.tensor([[40], [7]])
    torch._dynamo.reset()
    fn = torch.compile(lambda a, b, c, d: torch.ops.tac_amd.add_noise(a, b, c, d), backend=capture, fullgraph=True)
    out = fn(w, n, snr, lengths)
    assert sum('tac_amd.add_noise' in t for t in seen) == 1 and len(seen) == 1, seen
    same_bits(out, R.definition(w, n, snr, lengths), 'compiled')
    from torch._subclasses.fake_tensor import FakeTensorMode
    ws, ns = w[..., ::2], n[..., ::2]
    with FakeTensorMode() as mode:
        fake = torch.ops.tac_amd.add_noise(mode.from_tensor(ws), mode.from_tensor(ns), mode.from_tensor(snr), None)
    real = torch.ops.tac_amd.add_noise(ws, ns, snr, None)
    assert tuple(fake.shape) == tuple(real.shape) and fake.stride() == real.stride() and fake.dtype == real.dtype
    for args in ((w, n, snr, lengths), (w, n, snr, None)):
        torch.library.opcheck(torch.ops.tac_amd.add_noise.default, args, test_utils=('test_schema', 'test_faketensor'))
    w64, n64, s64 = (t.double().requires_grad_(True) for t in (w, n, snr))
    torch.library.opcheck(torch.ops.tac_amd.add_noise.default, (w64, n64, s64, lengths),
                          test_utils=('test_schema', 'test_faketensor', 'test_autograd_registration'))


def test_result_dtype_is_that_of_the_operands(tac):
    """``snr`` is converted inside the op: every route, the fake one included, returns ``result_type(waveform, noise)``"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    w, n = R.normal((2, 9), 14), R.normal((2, 9), 15)
    for snr in (torch.tensor([10.0, 0.0], dtype=torch.float64), torch.tensor([10, 0])):
        real = torch.ops.tac_amd.add_noise(w, n, snr, None)
        with FakeTensorMode() as mode:
            fake = torch.ops.tac_amd.add_noise(mode.from_tensor(w), mode.from_tensor(n), mode.from_tensor(snr), None)
        assert real.dtype == fake.dtype == tac.add_noise(w, n, snr).dtype == torch.float32
        same_bits(real, R.definition(w, n, snr.float()), str(snr.dtype))
    assert tac.add_noise(w, n.double(), torch.zeros(2)).dtype == torch.float64                  # the operands promote as torch's do


# ----------------------------------------------------------------------------- the grid rule and the C ABI
@pytest.mark.parametrize('cus', R.CU_COUNTS)
def test_wrap_rows_wrap_the_grid(tac, cus):
    assert R.assert_wraps(cus) == 32 * cus + 5 and R.wrap_rows(cus, 1) == 64 * cus + 5
    assert R.TILE == tac._hip.ADD_NOISE_TILE == 4096
    assert R.launch(cus, 256, 160000) == (256 * 40, 32 * cus)
    assert R.launch(cus, 64, 2880000) == (64 * 704, 32 * cus)
    assert R.launch(cus, 3, R.TILE) == (3, 32 * cus) and R.launch(cus, 3, R.TILE + 1) == (6, 32 * cus)
    with pytest.raises(AssertionError):                                             # the rule has teeth
        assert R.launch(cus, 5, R.TILE + 1)[0] > 2 * R.launch(cus, 5, R.TILE + 1)[1]


def test_quoted_launcher_expressions_are_in_the_source(tac):
    name, quotes = R.QUOTED
    with open(os.path.join(os.path.dirname(os.path.abspath(tac.__file__)), 'csrc', name)) as f:
        text = f.read()
    for q in quotes:
        assert q in text, '%s no longer holds %r: tests/augment_rules.py restates a launcher that has changed' % (name, q)


def test_c_abi_surface(tac):
    h = tac._native.lib()
    assert h.tac_abi_version() == 5
    for name in ('tac_add_noise_tile', 'tac_add_noise_work_bytes', 'tac_add_noise_f32', 'tac_add_noise_grad_f32'):
        assert name in tac._native.EXPORTS
    assert h.tac_add_noise_tile() == R.TILE
    assert h.tac_add_noise_work_bytes(3, 2 * R.TILE + 5) == 8 * (3 * 3 * 3 + 3 * 4)
    assert h.tac_add_noise_work_bytes(256, 160000) == 8 * (256 * 40 * 3 + 256 * 4)
    assert h.tac_add_noise_work_bytes(0, 5) == 0 and h.tac_add_noise_work_bytes(2 ** 31, R.TILE + 1) == 0
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tac_amd.h')) as f:
        header = f.read()
    assert 'int tac_add_noise_f32(' in header and 'int tac_add_noise_grad_f32(' in header
    # argument errors are refused before anything is launched (no device is touched)
    one = ctypes.c_void_p(16)
    invalid, unsupported = tac._native.TAC_E_INVALID, tac._native.TAC_E_UNSUPPORTED
    w4, z4 = (one, 0, 4, 1), (None, 0, 4, 1)
    tail = (one, 1, None, 1, 0, one, one, None)                                   # snr, its rows, no lengths, scratch, out, stream
    assert h.tac_add_noise_f32(*z4, *w4, 2, 2, 4, *tail) == invalid
    assert h.tac_add_noise_f32(*w4, *w4, 2, 2, 4, one, 1, None, 1, 0, None, one, None) == invalid          # no workspace
    assert h.tac_add_noise_f32(*w4, *w4, 2, 2, 4, one, 3, None, 1, 0, one, one, None) == invalid           # 3 ratios, 2 rows
    assert h.tac_add_noise_f32(*w4, *w4, 2, 2, 4, one, 1, one, 3, 1, one, one, None) == invalid            # 3 lengths, 2 rows
    assert h.tac_add_noise_f32(one, 0, 4, 0, *w4, 2, 2, 4, *tail) == invalid                              # a zero time stride
    assert h.tac_add_noise_f32(*w4, one, 0, -4, 1, 2, 2, 4, *tail) == invalid
    assert h.tac_add_noise_f32(*w4, *w4, 6, 4, 4, *tail) == invalid                                       # 4 channels do not divide 6 rows
    assert h.tac_add_noise_f32(one, 0, 0, 1, one, 0, 0, 1, 2 ** 31, 2 ** 31, R.TILE + 1, *tail) == unsupported
    assert h.tac_add_noise_grad_f32(*z4, *w4, *w4, 2, 2, 4, one, 1, None, 1, 0, one, one, one, one, None) == invalid
    assert h.tac_add_noise_grad_f32(*w4, *w4, *w4, 2, 2, 4, one, 1, None, 1, 0, one, None, None, None, None) == invalid
    reason, plan = tac._hip.add_noise_reason, tac._hip._add_noise_plan
    assert plan((2, 3), (torch.zeros(2, 3, 8), torch.zeros(8).expand(2, 3, 8))) == (6, [(0, 8, 1), (0, 0, 1)])          # one noise row for all
    assert plan((2, 3), (torch.zeros(2, 3, 8), torch.zeros(2, 1, 8))) == (3, [(24, 8, 1), (8, 0, 1)])                   # one per batch entry
    assert plan((2, 3), (torch.zeros(2, 4, 8)[:, :3], torch.zeros(2, 3, 8))) == (3, [(32, 8, 1), (24, 8, 1)])           # padded channels
    assert plan((2, 3), (torch.zeros(2, 3, 16)[..., ::2], torch.zeros(1, 1, 8))) == (6, [(0, 16, 2), (0, 0, 1)])
    assert reason((2, 3), torch.zeros(2, 3, 1).expand(2, 3, 8)) == 'non-positive time strides'
    assert reason((2, 3, 3), torch.zeros(2, 4, 4, 8)[:, :3, :3]) == 'leading dimensions that do not collapse to two strides'
    assert reason((2, 3, 3), torch.zeros(2, 3, 3, 8), torch.zeros(2, 1, 3, 8)) == 'leading dimensions that do not collapse to two strides'
    assert reason((2 ** 31,), torch.zeros(R.TILE + 1).expand(2 ** 31, R.TILE + 1)).startswith('more tiles')
